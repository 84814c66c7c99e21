"""GPU tests of muxgl_fmx_ambient_fit (fmx_ambient_fit.hip): the per-droplet maximum-likelihood ambient share of a candidate
cluster with its observed information.  Against the restatement (tests/fmx_ambient_fit_ref.py) evaluated at the device's own
rho_hat, against the restatement's Newton-free maximiser, against the existing calls (singlet table, ambient table), the
bounds and the statuses, bit identity across calls, budgets, device groups, slabbed ranks, the sharded driver, orders and
groupings of candidates and subsets of outputs, the state the call must leave alone, and the refusals.

The posteriors of the shape tests are handed in: the clusters are set from the truth (muxgl_fmx_set_clusters), held to the
panel's genotypes (muxgl_fmx_set_anchors), and one E-step runs; the restatement reads the posteriors that E-step read
(muxgl_fmx_get_cluster_gp).

Bars: check_fit, tests/fit_check.py, as CALL describes this call: no ll_top; status 6 and no NaN; a pair with an element
within 1e-6 relative of the 1e-6 floor at the device's rho_hat skips the two derivative bars only, and such pairs may be at
most 1 % of the checked ones.  The bodies shared with the other three fits: tests/fit_suite.py."""
import functools

import numpy as np
import pytest

import ambient_ref as ar
import fmx_ambient_fit_ref as ffr
import fit_check
import fit_suite as suite
import fmx_ambient_ref as fr
import parity
from popscle_amd import freemuxlet, muxgl, synth
from test_fmx_ambient_fit import check_soup_fits
from test_fmx_singlets_gpu import prepared, spread_init

pytestmark = pytest.mark.gpu

XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
DEFAULT_RHOS = fr.DEFAULT_RHOS
FIELDS = muxgl.Engine.AMBIENT_FIT_FIELDS
CALL = fit_check.Call(
    name="fmx ambient fit", share="rho", fields=FIELDS, width=1, top=False, fit=ffr.fit,
    closing="{on_kink} on a kink, mean n_steps {mean:.2f}", nearest=True, kink_frac=0.01, no_nan=True,
    method="fmx_ambient_fit", amb_af=True, x_name="rho_max", slot_name="cand",
    subsets=(("rho_hat",), ("status", "n_steps"), ("info", "ll_zero"), ("ll_hat", "n_steps", "rho_hat")), x_identity=0.37)
same = functools.partial(suite.same, CALL)


def check_fit(p, q, f, cand, rho_max, got, what, pairs=None, ll_tol=parity.LL_TOL):
    """every bar of fit_check.check_fit on the (droplet, slot) pairs of `pairs` (None: all); returns the number of interior
    fits and of those with restated info >= 1"""
    return fit_check.check_fit(CALL, (p, q, f), cand, rho_max, got, what, pairs, ll_tol)


def ready(p, K, init, devs=0, flags=0, anchors=None, modes=None, ge=0.1):
    """an engine after one E-step on the clusters `init`; anchors: the donors clusters 0 .. are held to"""
    e = prepared(p, devs, flags)
    if anchors is not None:
        e.demux_set_gp(p.gp, p.has_gp)
    e.fmx_set_clusters(K, init)
    if anchors is not None:
        e.fmx_set_anchors(anchors, modes)
    e.fmx_iterate(0.5, ge)
    return e


# ---- 1. parity and optimality over the shapes ----------------------------------------------------------------------------

@pytest.mark.parametrize("K,V,seed", [(1, 6, 7), (6, 6, 46), (17, 17, 57), (70, 70, 110), (300, 300, 340)])
def test_shapes_vs_restatement(K, V, seed):
    """droplets of 0, 1, 2, 63, 64, 65, 2048, 2049 and 5003 entries; K = 17, 70 and 300 run the wave, the oct and the streamed
    E-step.  K > 1: cluster j is held to donor j and the candidates are the droplet's own cluster and the next one.  K = 1:
    one cluster learned from all droplets of six donors"""
    p, who, pool = ffr.shaped(V, seed)
    if K == 1:
        init, anchors, cand = np.zeros(p.C, np.int32), None, np.zeros((p.C, 1), np.int32)
    else:
        init, anchors = who.astype(np.int32), list(range(K))
        cand = np.stack([who, (who + 1) % K], axis=1).astype(np.int32)
    with ready(p, K, init, anchors=anchors) as e:
        q = e.fmx_cluster_gp()
        got = e.fmx_ambient_fit(pool, cand, 0.5)
    assert got["kernel_ms"] > 0.0
    fitted, strong = check_fit(p, q, pool, cand, 0.5, got, f"shapes K={K}")
    assert got["status"][0].tolist() == [5] * cand.shape[1]                              # the droplet without entries
    assert K == 1 or (fitted >= 5 and strong >= 0.8 * fitted), (fitted, strong)


def small_case(K=17, seed=77, entries=(0, 1, 65, 300, 2, 130), S=900):
    p, who, pool = ffr.shaped_pileup(list(entries), S, K, seed, missing_gp_frac=0.0)
    return p, who.astype(np.int32), pool


def test_sixteen_candidates_with_skips_and_repeats():
    K = 17
    p, who, pool = small_case(K)
    rng = np.random.default_rng(5)
    cand = rng.integers(-1, K, size=(p.C, 16)).astype(np.int32)
    cand[:, 0] = who
    cand[:, 3] = who                                                                     # a repeated candidate
    cand[:, 7] = -1
    with ready(p, K, who, anchors=list(range(K))) as e:
        q = e.fmx_cluster_gp()
        got = e.fmx_ambient_fit(pool, cand, 0.4)
    suite.sixteen_slots(CALL, (p, q, pool), cand, 0.4, got, "16 candidates")
    assert (got["status"][0] >= 4).all()                                                 # the empty droplet


def test_a_zeroed_posterior_row_gives_status_6_and_no_nan():
    import torch

    K = 5
    p, who, pool = small_case(K, seed=78)
    cand = np.stack([who, (who + 1) % K, (who + 2) % K], axis=1).astype(np.int32)
    with ready(p, K, who) as e:
        clean = e.fmx_ambient_fit(pool, cand, 0.5)
        c = 3                                                                            # the droplet of 300 entries
        s, j = int(p.entry_snp[int(p.cell_ptr[c]) + 17]), int(cand[c, 1])
        t = freemuxlet.engine_exchange_tensor(e, freemuxlet.UNIT_CGP)
        t[s, j * 3:j * 3 + 3] = 0.0                                                      # cluster j at one of the droplet's markers
        torch.cuda.synchronize()
        q = e.fmx_cluster_gp()
        assert not q[s, j].any()
        got = e.fmx_ambient_fit(pool, cand, 0.5)
    hit = np.array([[s in p.entry_snp[p.cell_ptr[d]:p.cell_ptr[d + 1]] and cand[d, k] == j for k in range(3)] for d in range(p.C)])
    assert hit[c, 1] and (got["status"][hit] == 6).all() and not (got["status"][~hit] == 6).any()
    assert (got["rho_hat"][hit] == 0).all() and (got["ll_hat"][hit] == -np.inf).all() and (got["ll_zero"][hit] == -np.inf).all()
    assert (got["info"][hit] == 0).all() and (got["n_steps"][hit] == 0).all()
    assert not any(np.isnan(got[k]).any() for k in FIELDS)
    assert all(got[k][~hit].tobytes() == clean[k][~hit].tobytes() for k in FIELDS)       # every other pair as before
    check_fit(p, q, pool, cand, 0.5, got, "zeroed row")
    sm = freemuxlet.ambient_fit_summary(got)
    assert np.isnan(sm["se"][hit]).all() and np.isnan(sm["lrt"][hit]).all()


def test_droplets_without_entries():
    K = 4
    p, who, pool = small_case(K, seed=9, entries=(3, 0, 70, 0))
    with ready(p, K, who) as e:
        got = e.fmx_ambient_fit(pool, np.array([[0, -1], [1, 2], [3, 3], [-1, 0]], dtype=np.int32))
    assert got["status"][[1, 3]].tolist() == [[5, 5], [4, 5]] and got["status"][0, 1] == 4
    assert all(not got[k][[1, 3]].any() for k in FIELDS if k != "status")


def test_zero_cells():
    """C == 0: the call succeeds and writes nothing"""
    K = 4
    p, who, pool = small_case(K, seed=9, entries=(3, 0, 70, 0))
    suite.fmx_zero_cells(CALL, p, K, (pool,))


# ---- 2. consistency with the existing calls ------------------------------------------------------------------------------

@pytest.mark.parametrize("K,flags", [(6, 0), (40, 0), (40, XE)])
def test_consistent_with_the_singlet_and_the_ambient_tables(K, flags):
    p, who, pool = small_case(K, seed=300 + K, entries=(0, 5, 64, 200, 700, 2100, 90, 33), S=2500)
    with ready(p, K, who, flags=flags, anchors=list(range(K))) as e:
        sng = e.fmx_singlets()
        cand = freemuxlet.top_clusters(sng, 2)
        got = e.fmx_ambient_fit(pool, cand, 0.5)
        table = e.fmx_ambient(pool, DEFAULT_RHOS)["ll"]
        at_hat = np.zeros(cand.shape)
        for c in range(p.C):                       # the table at the droplet's own estimates: one rho per call and slot
            for k in range(2):
                at_hat[c, k] = e.fmx_ambient(pool, [got["rho_hat"][c, k]])["ll"][c, cand[c, k], 0]
        coarse = e.fmx_ambient(pool, ffr.coarse_points(0.5))["ll"]
    rows = np.arange(p.C)[:, None]
    d0 = np.abs(got["ll_zero"] - sng[rows, cand]).max()
    d1 = np.abs(got["ll_hat"] - at_hat).max()
    print(f"fmx ambient fit K={K} flags={flags}: |ll_zero - singlet table| {d0:.3e}, |ll_hat - ambient table at rho_hat| {d1:.3e}")
    assert d0 <= parity.LL_TOL and d1 <= parity.LL_TOL
    assert (got["status"][1:] <= 2).all() and (got["status"] == 0).any()
    xs = ffr.coarse_points(0.5)
    for c in range(1, p.C):                        # no point of the default grid inside the bracket is better
        for k in range(2):
            i = int(np.argmax(coarse[c, cand[c, k]]))
            lo, hi = xs[max(i - 1, 0)], xs[min(i + 1, 8)]
            assert lo <= got["rho_hat"][c, k] <= hi, (c, k, lo, hi, got["rho_hat"][c, k])
            inside = [r for r, rho in enumerate(DEFAULT_RHOS) if lo <= rho <= hi]
            assert inside and (got["ll_hat"][c, k] >= table[c, cand[c, k], inside] - 1e-9).all(), (c, k)


# ---- 3. bounds, and what the feature is for ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def soup_fit(soup, rho_max):
    """the SOUP pileup of fmx_ambient_ref.py with the clusters handed in from the truth, one E-step, every droplet's own
    cluster as the candidate"""
    p, who, _pool = ar.soup_pileup(soup=soup, **fr.SOUP)
    who = who.astype(np.int32)
    with ready(p, fr.SOUP["V"], who) as e:
        f = muxgl.ambient_profile(*e.pileup_allele_counts(), p.af)
        q = e.fmx_cluster_gp()
        got = e.fmx_ambient_fit(f, who, rho_max)
        table = e.fmx_ambient(f, DEFAULT_RHOS)["ll"]
    return p, who, f, q, got, table


def test_no_soup_sits_on_the_lower_bound_and_a_small_cap_on_the_upper():
    p, who, f, q, got, table = soup_fit(0.0, 0.5)
    at0 = got["status"][:, 0] == 1
    print(f"soup = 0: {int(at0.sum())} of {p.C} droplets at the lower bound")
    assert at0.sum() > p.C / 2 and (got["rho_hat"][at0] == 0.0).all() and (got["n_steps"][at0] == 0).all()
    assert np.abs(got["ll_hat"][at0] - got["ll_zero"][at0]).max() <= 1e-9      # (both are LL(0))
    p, who, f, q, got, table = soup_fit(0.2, 0.05)
    at_cap = got["status"][:, 0] == 2
    print(f"soup = 0.2, rho_max = 0.05: {int(at_cap.sum())} of {p.C} droplets at the upper bound")
    assert at_cap.sum() > p.C / 2 and got["rho_hat"][at_cap].tobytes() == np.full(int(at_cap.sum()), 0.05).tobytes()
    assert (got["n_steps"][at_cap] == 0).all()
    check_fit(p, q, f, who, 0.05, got, "upper bound", pairs=[(c, 0) for c in range(0, p.C, 96)])


@pytest.mark.parametrize("soup", [0.2, 0.0])
def test_the_device_meets_the_soup_sanity_check(soup):
    """tests/test_fmx_ambient_fit.py holds the restatement to the same check on every eighth droplet of the same pileup"""
    p, who, f, q, got, table = soup_fit(soup, 0.5)
    check_soup_fits(got["rho_hat"][:, 0], got["status"][:, 0], table, who, soup)
    check_fit(p, q, f, who, 0.5, got, f"soup {soup}", pairs=[(c, 0) for c in range(0, p.C, 96)])


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------

def _long_cells_pileup(seed, C=30):
    p = synth.make_pileup(C, 9000, 8, seed=seed, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000, with_gp=False)
    assert np.diff(p.cell_ptr).max() > 2048
    return p


@functools.lru_cache(maxsize=None)
def identity_case(K, C=30):
    p = _long_cells_pileup(11000 + K, C)
    f = ar.draw_af(p.S, seed=K)
    cand = np.random.default_rng(K).integers(-1, K, size=(p.C, 16)).astype(np.int32)
    init = spread_init(p.C, K)
    with prepared(p) as e:
        e.fmx_set_clusters(K, init)
        for _ in range(2):
            cells, st = e.fmx_iterate(0.5, 0.1)
        want = e.fmx_ambient_fit(f, cand, 0.37)
    return p, f, cand, init, want, cells


def test_call_to_call_budget_permutation_split_and_null_outputs(monkeypatch):
    K = 24
    p, f, cand, init, want, _cells = identity_case(K)
    monkeypatch.delenv("MUXGL_FMX_SLAB_MB", raising=False)
    with suite.fmx_iterated(p, K, init) as e:
        suite.identity(CALL, e, (f,), cand, want)
        for mb in ("1", "64"):
            monkeypatch.setenv("MUXGL_FMX_SLAB_MB", mb)                                   # (not read by the call)
            assert same(e.fmx_ambient_fit(f, cand, 0.37), want)
        monkeypatch.delenv("MUXGL_FMX_SLAB_MB")


@pytest.mark.parametrize("K", [24, 300])
def test_device_groups(K):
    p, f, cand, init, want, cells = identity_case(K)
    suite.device_groups(CALL, lambda devs, flags: suite.fmx_iterated(p, K, init, devs, flags, cells), (f,), cand, want)


@pytest.mark.parametrize("K,world,flags", [(20, 2, 0), (300, 3, 0)])
def test_slabbed_ranks_and_the_sharded_driver(K, world, flags):
    """suite.fmx_slabbed_ranks: the ranks' outputs, concatenated, are the one-handle outputs bit for bit; and
    run_em(want_ambient_fit=...) returns them for the best clusters of the singlet table."""
    p, f, cand, init, want, cells = identity_case(K, C=36)
    suite.fmx_slabbed_ranks(CALL, p, K, world, flags, init, (f,), cand, want)
    with suite.fmx_iterated(p, K, init) as e:
        top = freemuxlet.top_clusters(e.fmx_singlets(), 3)
        direct = e.fmx_ambient_fit(f, top, 0.37)
    with prepared(p) as e:
        out, hist, got = freemuxlet.run_em(e, K, init, max_iter=2, early_stop=False, want_ambient_fit=(f, 0.37, 3))
    assert out.tobytes() == cells.tobytes() and np.array_equal(got["cand"], top) and same(got, direct)


# ---- 5. state ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("anchored", [None, "held", "prior"])
def test_records_tables_pileups_and_timing_slots_stay(anchored):
    K = 6
    p, who, pool = small_case(K, seed=10200, entries=(40, 0, 90, 300, 7, 130, 64, 33, 2100, 12), S=2500)
    cand = np.random.default_rng(3).integers(-1, K, size=(p.C, 3)).astype(np.int32)
    suite.fmx_state_stays(CALL, p, K, who, anchored, (pool,), cand, 0.5, lambda e: e.fmx_ambient(pool, DEFAULT_RHOS)["ll"].tobytes())


@pytest.mark.parametrize("K,devs,flags", [(6, 0, 0), (40, 0, XE), (300, 0, 0), (24, [0, 0], 0)])
def test_the_call_leaves_the_em_alone(K, devs, flags):
    p = synth.make_pileup(300, 500, 4, seed=10300 + K, mean_entries=10, min_entries=2, reads_lambda=0.3, with_gp=False)
    init = (np.arange(p.C) % 3).astype(np.int32)
    f = ar.draw_af(p.S, seed=K)
    cand = np.random.default_rng(K).integers(-1, K, size=(p.C, 2)).astype(np.int32)
    suite.fmx_em_alone(CALL, p, K, devs, flags, init, (f,), cand, 0.5)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals_leave_the_handle_usable(devs):
    K = 5
    p, who, pool = small_case(K, seed=612, entries=(5, 0, 130, 64), S=400)
    f = pool
    cand = np.stack([who, (who + 3) % K], axis=1).astype(np.int32)
    with ready(p, K, who, devs) as e:
        fresh = e.fmx_ambient_fit(f, cand, 0.5)
    with muxgl.Engine(devs) as e:
        refused, still_good = suite.refusal_frame(CALL, e, (f,), cand, 0.5, fresh, named=True)
        refused(b"no pileup")
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        refused(b"muxgl_fmx_prepare")
        e.fmx_prepare(p.af)
        refused(b"E-step")
        e.fmx_set_clusters(K, who)
        refused(b"no E-step since muxgl_fmx_set_clusters")
        e.fmx_iterate(0.5, 0.1)
        still_good()
        suite.common_refusals(CALL, refused, still_good, cand, K)
        for bad in (-0.01, 1.5, float("nan"), float("inf")):
            for s in (0, 17, p.S - 1):
                g = f.copy()
                g[s] = bad
                g[min(s + 3, p.S - 1)] = bad                                             # (the first offending marker is named)
                refused(f"amb_af of marker {s} ".encode(), af=g)
            still_good()
        with pytest.raises(ValueError):
            e.fmx_ambient_fit(f[:-1], cand)
        with pytest.raises(ValueError):
            e.fmx_ambient_fit(f, cand[:-1])
        if devs == 0:                    # (the phases run on a one-device handle)
            e.fmx_iter_gp(0.5, 0.1)      # the posteriors of the NEXT iteration
            refused(b"the cluster posteriors were rewritten")
        e.fmx_set_clusters(K, who)       # fresh clusters: the fit of the old ones is gone
        refused(b"no E-step since muxgl_fmx_set_clusters")
        e.fmx_iterate(0.5, 0.1)
        still_good()
