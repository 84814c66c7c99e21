"""GPU tests of muxgl_fmx_alpha_fit (fmx_alpha_fit.hip): the per-droplet maximum-likelihood mixing share of a pair of
clusters with its observed information.  Against the restatement (tests/fmx_alpha_fit_ref.py) evaluated at the device's own
alpha_hat, against the restatement's Newton-free maximiser, against the oracle's E-step (the slot of (j, k) at alpha = 0.5) and
the singlet table (alpha = 0 and 1), the bounds and the statuses, the mirror, bit identity across calls, budgets, device
groups, slabbed ranks, the sharded driver, orders and groupings of slots and subsets of outputs, the state the call must
leave alone, and the refusals.

The posteriors of the shape tests are handed in: the clusters are set from the truth (muxgl_fmx_set_clusters), held to the
panel's genotypes (muxgl_fmx_set_anchors), and one E-step runs; the restatement reads the posteriors that E-step read
(muxgl_fmx_get_cluster_gp).

Bars: check_fit, tests/fit_check.py, as CALL describes this call: with ll_top, and ll_hat on a bound is ll_zero resp. ll_top
bit for bit on every slot; status 6 and no NaN.  A pair with an element within 1e-6 relative of the 1e-6 floor at the
estimate would skip the two derivative bars only; the seeds are such that there is none, at the device's estimate or at the
restatement's, and the count is asserted to be 0.  The bodies shared with the other three fits: tests/fit_suite.py."""
import functools

import numpy as np
import pytest

import fmx_alpha_fit_ref as far
import fit_check
import fit_suite as suite
import parity
from popscle_amd import freemuxlet, muxgl, synth
from test_fmx_alpha_fit import check_clean, check_mixed, oracle_case
from test_fmx_ambient_fit_gpu import ready, small_case
from test_fmx_singlets_gpu import prepared, spread_init

pytestmark = pytest.mark.gpu

XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
FIELDS = muxgl.Engine.ALPHA_FIT_FIELDS
CALL = fit_check.Call(
    name="fmx alpha fit", share="alpha", fields=FIELDS, width=2, top=True, fit=far.fit,
    closing="{on_kink} on a kink, mean n_steps {mean:.2f}", nearest=True, kink_at_ref=True, kink_frac=0.0, no_nan=True,
    bounds_everywhere=True,
    method="fmx_alpha_fit", x_name="alpha_max", slot_name="pair", extra=("pair", "alpha_max"),
    subsets=(("alpha_hat",), ("status", "n_steps"), ("info", "ll_zero"), ("ll_top",), ("ll_hat", "n_steps", "alpha_hat")),
    x_identity=0.87)
same = functools.partial(suite.same, CALL)


def check_fit(p, q, pair, alpha_max, got, what, pairs=None, ll_tol=parity.LL_TOL):
    """every bar of fit_check.check_fit on the (droplet, slot) pairs of `pairs` (None: all); returns the number of interior
    fits and of those with restated info >= 1"""
    return fit_check.check_fit(CALL, (p, q), pair, alpha_max, got, what, pairs, ll_tol)


# ---- 1. parity and optimality over the shapes, and the mirror -----------------------------------------------------------------

@pytest.mark.parametrize("K,V,seed,flags", [c + (0,) for c in far.SHAPE_CASES] + [(40, 40, 41, XE)])
def test_shapes_vs_restatement_and_the_mirror(K, V, seed, flags):
    """droplets of 0, 1, 2, 63, 64, 65, 130, 300 and 2049 entries; K = 17, 70 and 300 run the wave, the oct and the streamed
    E-step, K = 40 the streamed one by its flag.  K > 1: cluster j is held to donor j and the slots are the droplet's own pair
    and the pair reversed, on [0, 1].  K = 1: one cluster learned from all droplets of six donors, the pair (0, 0)"""
    p, first, second = far.shaped(V, seed)
    if K == 1:
        init, anchors, pair = np.zeros(p.C, np.int32), None, np.zeros((p.C, 1, 2), np.int32)
    else:
        init, anchors = first, list(range(K))
        pair = np.stack([np.stack([first, second], axis=1), np.stack([second, first], axis=1)], axis=1).astype(np.int32)
    with ready(p, K, init, flags=flags, anchors=anchors) as e:
        q = e.fmx_cluster_gp()
        got = e.fmx_alpha_fit(pair, 1.0)
    assert got["kernel_ms"] > 0.0 and got["alpha_max"] == 1.0 and np.array_equal(got["pair"], pair)
    fitted, strong = check_fit(p, q, pair, 1.0, got, f"shapes K={K}")
    assert got["status"][0].tolist() == [5] * pair.shape[1]                              # the droplet without entries
    if K == 1:
        return
    assert fitted >= 8 and strong >= 0.5 * fitted, (fitted, strong)
    d = np.abs(got["ll_hat"][:, 0] - got["ll_hat"][:, 1])
    ok = (got["status"] == 0).all(axis=1) & (got["info"] >= 1.0).all(axis=1)
    s = got["alpha_hat"][:, 0] + got["alpha_hat"][:, 1]
    print(f"fmx alpha fit mirror K={K}: |ll_hat(j, k) - ll_hat(k, j)| {d.max():.3e}; alpha_hat sums to 1 within "
          f"{np.abs(s[ok] - 1.0).max():.3e} on {int(ok.sum())} droplets, exactly on {int((s[ok] == 1.0).sum())}")
    assert d.max() <= 1e-9 and ok.sum() >= 4 and np.abs(s[ok] - 1.0).max() <= 1e-6
    assert np.abs(got["ll_zero"][:, 0] - got["ll_top"][:, 1]).max() <= 1e-9              # j alone, from either side


def drawn_pairs(rng, C, K, n):
    """[C][n][2]: drawn pairs, j == k among them, a tenth of the slots skipped"""
    pair = rng.integers(0, K, size=(C, n, 2)).astype(np.int32)
    pair[rng.random((C, n)) < 0.1] = -1
    return pair


def test_sixteen_slots_with_skips_repeats_wrong_pairs_and_a_cap():
    K = 17
    p, first, second = far.shaped(K, 77, entries=(0, 1, 65, 300, 2, 130), S=900)
    pair = drawn_pairs(np.random.default_rng(5), p.C, K, 16)
    pair[:, 0] = np.stack([first, second], axis=1)
    pair[:, 3] = pair[:, 0]                                                              # a repeated pair
    pair[:, 5] = np.stack([first, first], axis=1)                                        # j == k
    pair[:, 6] = np.stack([(first + 3) % K, (second + 5) % K], axis=1)                   # a wrong pair
    pair[:, 7] = -1
    with ready(p, K, first, anchors=list(range(K))) as e:
        q = e.fmx_cluster_gp()
        got = e.fmx_alpha_fit(pair, 0.8)
        one = e.fmx_alpha_fit(np.ascontiguousarray(pair[:, :1]), 0.8)                    # n_cand = 1
        two = e.fmx_alpha_fit(np.ascontiguousarray(pair[:, 5:7]), 0.8)                   # n_cand = 2
    suite.sixteen_slots(CALL, (p, q), pair, 0.8, got, "16 slots")
    assert all(one[k].tobytes() == np.ascontiguousarray(got[k][:, :1]).tobytes() for k in FIELDS)
    assert all(two[k].tobytes() == np.ascontiguousarray(got[k][:, 5:7]).tobytes() for k in FIELDS)
    assert (got["status"][0] >= 4).all()                                                 # the empty droplet
    assert (got["alpha_hat"] <= 0.8).all() and (got["status"][1:, 5] <= 2).all()


# ---- 2. the reference's E-step and the singlet table -----------------------------------------------------------------------

@pytest.mark.parametrize("K,seed", [(3, 7), (5, 8)])
def test_the_oracle_slot_at_one_half_and_the_singlet_table_at_the_ends(K, seed):
    p, _q, _sng, full = oracle_case(K, seed)
    init = (np.arange(p.C) % K).astype(np.int32)
    jk = [(j, k) for j in range(K) for k in range(j)]
    pair = np.ascontiguousarray(np.broadcast_to(np.array(jk, np.int32), (p.C, len(jk), 2)))
    with prepared(p) as e:
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1)
        half = e.fmx_alpha_fit(pair, 0.5)
        whole = e.fmx_alpha_fit(pair, 1.0)
        sng = e.fmx_singlets()
    slot = np.array([j * (j + 1) // 2 + k for j, k in jk])
    d_half = np.abs(half["ll_top"] - full[:, slot]).max()
    d_zero = np.abs(half["ll_zero"] - sng[:, [j for j, _ in jk]]).max()
    d_top = np.abs(whole["ll_top"] - sng[:, [k for _, k in jk]]).max()
    print(f"fmx alpha fit K={K}: |ll_top(alpha_max = 0.5) - oracle full_ll slot| {d_half:.3e} over {pair.shape[0] * pair.shape[1]} "
          f"pairs, |ll_zero - singlets[j]| {d_zero:.3e}, |ll_top(alpha_max = 1) - singlets[k]| {d_top:.3e}")
    assert d_half <= 1e-5 and d_zero <= 1e-5 and d_top <= 1e-5
    assert half["ll_zero"].tobytes() == whole["ll_zero"].tobytes()


# ---- 3. statuses 5 and 6, C == 0 -------------------------------------------------------------------------------------------

def test_a_zeroed_posterior_row_gives_status_6_and_no_nan():
    import torch

    K = 5
    p, who, _pool = small_case(K, seed=78)
    pair = np.stack([np.stack([who, (who + 1) % K], axis=1), np.stack([(who + 1) % K, who], axis=1),
                     np.stack([who, (who + 2) % K], axis=1)], axis=1).astype(np.int32)
    with ready(p, K, who) as e:
        clean = e.fmx_alpha_fit(pair, 1.0)
        c = 3                                                                            # the droplet of 300 entries
        s, j = int(p.entry_snp[int(p.cell_ptr[c]) + 17]), int(pair[c, 0, 1])
        t = freemuxlet.engine_exchange_tensor(e, freemuxlet.UNIT_CGP)
        t[s, j * 3:j * 3 + 3] = 0.0                                                      # cluster j at one of the droplet's markers
        torch.cuda.synchronize()
        q = e.fmx_cluster_gp()
        assert not q[s, j].any()
        got = e.fmx_alpha_fit(pair, 1.0)
    hit = np.array([[s in p.entry_snp[p.cell_ptr[d]:p.cell_ptr[d + 1]] and j in pair[d, k] for k in range(3)] for d in range(p.C)])
    assert hit[c, 0] and hit[c, 1] and (got["status"][hit] == 6).all() and not (got["status"][~hit] == 6).any()
    for n in ("ll_hat", "ll_zero", "ll_top"):
        assert (got[n][hit] == -np.inf).all()
    assert (got["alpha_hat"][hit] == 0).all() and (got["info"][hit] == 0).all() and (got["n_steps"][hit] == 0).all()
    assert not any(np.isnan(got[k]).any() for k in FIELDS)
    assert all(got[k][~hit].tobytes() == clean[k][~hit].tobytes() for k in FIELDS)       # every other pair as before
    check_fit(p, q, pair, 1.0, got, "zeroed row")
    sm = freemuxlet.alpha_fit_summary(got)
    assert np.isnan(sm["se"][hit]).all() and np.isnan(sm["lrt"][hit]).all()


def test_droplets_without_entries_and_zero_cells():
    K = 4
    p, who, _pool = small_case(K, seed=9, entries=(3, 0, 70, 0))
    with ready(p, K, who) as e:
        got = e.fmx_alpha_fit(np.array([[[0, 1], [-1, -1]], [[1, 2], [2, 2]], [[3, 0], [3, 3]], [[-1, -1], [0, 2]]], dtype=np.int32))
    assert got["status"][[1, 3]].tolist() == [[5, 5], [4, 5]] and got["status"][0, 1] == 4
    assert all(not got[k][[1, 3]].any() for k in FIELDS if k != "status")
    suite.fmx_zero_cells(CALL, p, K, ())


# ---- 4. what the feature is for --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def doublet_fit(which, alpha_max):
    """the sanity pileups of tests/test_fmx_alpha_fit.py with the clusters held to the donors' genotypes, one E-step at
    geno_error 0, every droplet's own pair as the slot"""
    p, first, second = far.doublet_pileup(**(far.MIXED if which == "mixed" else far.CLEAN))
    V = far.MIXED["V"]
    pair = np.stack([first, second], axis=1).astype(np.int32)
    with ready(p, V, first.astype(np.int32), anchors=list(range(V)), ge=0.0) as e:
        q = e.fmx_cluster_gp()
        got = e.fmx_alpha_fit(pair, alpha_max)
    return p, pair, q, got


def test_the_device_meets_the_sanity_checks_and_sits_on_the_bounds_bit_for_bit():
    p, pair, q, got = doublet_fit("mixed", 1.0)
    g = lambda n: got[n][:, 0]
    check_mixed(g("alpha_hat"), g("info"), g("status"), g("ll_hat"), g("ll_zero"), g("ll_top"), np.array(far.MIXED["shares"]))
    check_fit(p, q, pair, 1.0, got, "mixed", pairs=[(c, 0) for c in range(0, p.C, 4)])
    p, pair, q, got = doublet_fit("clean", 1.0)
    at0 = check_clean(got["status"][:, 0], got["ll_hat"][:, 0], got["ll_zero"][:, 0])
    b = got["status"][:, 0] == 1
    assert got["ll_hat"][b].tobytes() == got["ll_zero"][b].tobytes() and (got["n_steps"][b] == 0).all() and at0 == b.sum()
    check_fit(p, q, pair, 1.0, got, "clean", pairs=[(c, 0) for c in range(0, p.C, 4)])
    p, pair, q, got = doublet_fit("mixed", 0.05)                                         # a small cap: the upper bound
    b = got["status"][:, 0] == 2
    print(f"mixed, alpha_max = 0.05: {int(b.sum())} of {p.C} droplets at the upper bound")
    assert b.sum() > p.C / 2 and got["alpha_hat"][b].tobytes() == np.full(int(b.sum()), 0.05).tobytes()
    assert got["ll_hat"][b].tobytes() == got["ll_top"][b].tobytes() and (got["n_steps"][b] == 0).all()
    check_fit(p, q, pair, 0.05, got, "upper bound", pairs=[(c, 0) for c in range(0, p.C, 4)])


# ---- 5. bit identity ---------------------------------------------------------------------------------------------------

def _long_cells_pileup(seed, C=30):
    p = synth.make_pileup(C, 9000, 8, seed=seed, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000, with_gp=False)
    assert np.diff(p.cell_ptr).max() > 2048
    return p


@functools.lru_cache(maxsize=None)
def identity_case(K, C=30):
    p = _long_cells_pileup(11000 + K, C)
    pair = drawn_pairs(np.random.default_rng(K), p.C, K, 16)
    init = spread_init(p.C, K)
    with prepared(p) as e:
        e.fmx_set_clusters(K, init)
        for _ in range(2):
            cells, st = e.fmx_iterate(0.5, 0.1)
        want = e.fmx_alpha_fit(pair, 0.87)
    return p, pair, init, want, cells


def test_call_to_call_budget_permutation_split_and_null_outputs(monkeypatch):
    K = 24
    p, pair, init, want, _cells = identity_case(K)
    monkeypatch.delenv("MUXGL_FMX_SLAB_MB", raising=False)
    with suite.fmx_iterated(p, K, init) as e:
        suite.identity(CALL, e, (), pair, want)
        for mb in ("1", "64"):
            monkeypatch.setenv("MUXGL_FMX_SLAB_MB", mb)                                   # (not read by the call)
            assert same(e.fmx_alpha_fit(pair, 0.87), want)
        monkeypatch.delenv("MUXGL_FMX_SLAB_MB")


@pytest.mark.parametrize("K", [24, 300])
def test_device_groups(K):
    p, pair, init, want, cells = identity_case(K)
    suite.device_groups(CALL, lambda devs, flags: suite.fmx_iterated(p, K, init, devs, flags, cells), (), pair, want)


@pytest.mark.parametrize("K,world,flags", [(20, 2, 0), (300, 3, 0)])
def test_slabbed_ranks_and_the_sharded_driver(K, world, flags):
    """suite.fmx_slabbed_ranks: the ranks' outputs, concatenated, are the one-handle outputs bit for bit; and
    run_em(want_alpha_fit=...) returns them for the pairs of call_pairs()."""
    p, pair, init, want, cells = identity_case(K, C=36)
    suite.fmx_slabbed_ranks(CALL, p, K, world, flags, init, (), pair, want)
    slots = freemuxlet.call_pairs(cells)
    with suite.fmx_iterated(p, K, init) as e:
        direct = e.fmx_alpha_fit(slots, 0.87)
    with prepared(p) as e:
        out, hist, got = freemuxlet.run_em(e, K, init, max_iter=2, early_stop=False, want_alpha_fit=(0.87,))
    assert out.tobytes() == cells.tobytes() and np.array_equal(got["pair"], slots) and same(got, direct)
    assert got["alpha_max"] == 0.87 and (slots >= 0).any()


# ---- 6. state ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anchored", [None, "held", "prior"])
def test_records_tables_pileups_and_timing_slots_stay(anchored):
    K = 6
    p, who, pool = small_case(K, seed=10200, entries=(40, 0, 90, 300, 7, 130, 64, 33, 2100, 12), S=2500)
    pair = drawn_pairs(np.random.default_rng(3), p.C, K, 3)
    def tables(e):
        amb = e.fmx_ambient_fit(pool, np.ascontiguousarray(pair[:, :, 0]), 0.5)
        return e.fmx_ambient(pool, (0.0, 0.1, 0.5))["ll"].tobytes(), tuple(amb[n].tobytes() for n in muxgl.Engine.AMBIENT_FIT_FIELDS)

    suite.fmx_state_stays(CALL, p, K, who, anchored, (), pair, 1.0, tables)


@pytest.mark.parametrize("K,devs,flags", [(6, 0, 0), (40, 0, XE), (300, 0, 0), (24, [0, 0], 0)])
def test_the_call_leaves_the_em_alone(K, devs, flags):
    p = synth.make_pileup(300, 500, 4, seed=10300 + K, mean_entries=10, min_entries=2, reads_lambda=0.3, with_gp=False)
    init = (np.arange(p.C) % 3).astype(np.int32)
    pair = drawn_pairs(np.random.default_rng(K), p.C, K, 2)
    suite.fmx_em_alone(CALL, p, K, devs, flags, init, (), pair, 1.0)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals_leave_the_handle_usable(devs):
    K = 5
    p, who, _pool = small_case(K, seed=612, entries=(5, 0, 130, 64), S=400)
    pair = np.stack([np.stack([who, (who + 3) % K], axis=1), np.stack([who, who], axis=1)], axis=1).astype(np.int32)
    with ready(p, K, who, devs) as e:
        fresh = e.fmx_alpha_fit(pair, 1.0)
    with muxgl.Engine(devs) as e:
        refused, still_good = suite.refusal_frame(CALL, e, (), pair, 1.0, fresh, named=True)
        refused(b"no pileup")
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        refused(b"muxgl_fmx_prepare")
        e.fmx_prepare(p.af)
        refused(b"E-step")
        e.fmx_set_clusters(K, who)
        refused(b"no E-step since muxgl_fmx_set_clusters")
        e.fmx_iterate(0.5, 0.1)
        still_good()
        suite.common_refusals(CALL, refused, still_good, pair, K)
        for t in (0, 1):
            c2 = pair.copy()
            c2[3, 0, t] = -1
            refused(b"pair[3][0] ", slots=c2)
            refused(b"exactly one negative index", slots=c2)
        still_good()
        with pytest.raises(ValueError):
            e.fmx_alpha_fit(pair[:-1])
        with pytest.raises(ValueError):
            e.fmx_alpha_fit(pair[:, :, :1])
        if devs == 0:                    # (the phases run on a one-device handle)
            e.fmx_iter_gp(0.5, 0.1)      # the posteriors of the NEXT iteration
            refused(b"the cluster posteriors were rewritten")
        e.fmx_set_clusters(K, who)       # fresh clusters: the fit of the old ones is gone
        refused(b"no E-step since muxgl_fmx_set_clusters")
        e.fmx_iterate(0.5, 0.1)
        still_good()
