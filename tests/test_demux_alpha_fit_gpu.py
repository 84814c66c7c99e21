"""GPU tests of muxgl_demux_alpha_fit (demux_alpha_fit.hip): the per-droplet maximum-likelihood mixing share of a pair of
samples with its observed information.  Against the restatement (tests/alpha_fit_ref.py, itself the reference's llksAB bit
for bit at every alpha of the grid: tests/test_demux_alpha_fit.py) evaluated at the device's own alpha_hat, against the
restatement's Newton-free maximiser, against the reference's own slots (the oracle's full_ll) and the singlet table, the
mirror (j, k) <-> (k, j), the two sanity pileups, bit identity across calls, budgets, device groups, the sharded driver,
orders and groupings of slots and subsets of outputs, the state the call must leave alone, and the refusals.

Bars: check_fit, tests/fit_check.py, as CALL describes this call: with ll_top, so ll_hat on a bound is ll_zero resp. ll_top
bit for bit on the checked slots; no floor, hence no kink and no slot that skips a derivative bar.  The bodies shared with
the other three fits: tests/fit_suite.py."""
import functools

import numpy as np
import pytest

import alpha_fit_ref as alr
import fit_check
import fit_suite as suite
import many_samples
import parity
import unknown_ref as ur
from popscle_amd import demuxlet, muxgl

pytestmark = pytest.mark.gpu

G2 = (0.0, 0.5)
G6 = (0.0, 0.13, 0.37, 0.5, 0.71, 1.0)
FIELDS = muxgl.Engine.ALPHA_FIT_FIELDS
CALL = fit_check.Call(
    name="alpha fit", share="alpha", fields=FIELDS, width=2, top=True, fit=alr.fit,
    closing="n_steps mean {mean:.2f} max {max}", guard_info_note=True,
    method="demux_alpha_fit", grid=True, x_name="alpha_max", slot_name="pair", extra=("pair", "alpha_max"),
    subsets=(("alpha_hat",), ("status", "n_steps"), ("info", "ll_zero"), ("ll_top",), ("ll_hat", "n_steps", "alpha_hat")),
    x_identity=0.87)
load = suite.demux_load
same = functools.partial(suite.same, CALL)


def fit(p, alphas, pairs, alpha_max=1.0, **kw):
    return suite.demux_fit(CALL, p, (alphas,), pairs, alpha_max, **kw)


def check_fit(p, alphas, pairs, alpha_max, got, what, slots=None):
    """every bar of fit_check.check_fit on the (droplet, slot) pairs of `slots` (None: all); returns the number of fitted
    cases and of those with restated info >= 1"""
    return fit_check.check_fit(CALL, (p, alphas), pairs, alpha_max, got, what, slots, parity.LL_TOL)


# ---- 1. parity and optimality over the shapes ----------------------------------------------------------------------------

SHAPES = [0, 1, 2, 63, 64, 65, 2048, 2049, 5003]


@functools.lru_cache(maxsize=None)
def shaped(V, seed, missing=0.03):
    """droplets of exactly 0, 1, 2, 63, 64, 65, 2048, 2049 and 5003 entries of 1, 2, 33 and 60 reads at base qualities 2..93,
    READ_OTHER bytes, 3 % of the markers without genotypes, three reads in ten from the second cell"""
    p, first, second = alr.shaped_pileup(SHAPES, 6000, V, seed, missing_gp_frac=missing)
    assert (p.reads == alr.READ_OTHER).any() and set(np.diff(p.entry_rptr).tolist()) == {1, 2, 33, 60}
    assert (p.has_gp == 0).any()
    return p, first, second


def shape_pairs(V, first, second, kinds):
    """[C][len(kinds)][2]: "own" the droplet's own two samples, "rev" the same reversed, "wrong" two other samples"""
    cols = {"own": (first, second), "rev": (second, first), "wrong": ((first + 2) % V, (second + 3) % V)}
    return np.ascontiguousarray(np.stack([np.stack(cols[k], axis=1) for k in kinds], axis=1), dtype=np.int32)


@pytest.mark.parametrize("V,alphas,kinds,alpha_max", [(1, G2, ("own",), 1.0), (2, G6, ("own", "rev"), 1.0),
                                                      (17, G6, ("own", "wrong"), 1.0), (70, G2, ("rev", "wrong"), 0.8),
                                                      (300, G2, ("own",), 1.0)])
def test_shapes_vs_restatement(V, alphas, kinds, alpha_max):
    p, first, second = shaped(V, 40 + V)
    pairs = shape_pairs(V, first, second, kinds)
    got = fit(p, alphas, pairs, alpha_max)
    assert got["kernel_ms"] > 0.0
    # the first slot on every droplet; the second on the small ones and on one of more than 2048 entries
    slots = [(c, 0) for c in range(p.C)] + [(c, 1) for c in (0, 1, 2, 3, 4, 5, 7) if len(kinds) > 1]
    fitted, strong = check_fit(p, alphas, pairs, alpha_max, got, f"shapes V={V}", slots)
    assert (got["status"][0] == 5).all()                                                # the droplet without entries
    assert V == 1 or (fitted >= 5 and strong >= 0.8 * fitted), (fitted, strong)


def test_sixteen_slots_with_skips_and_repeats():
    V = 17
    p, first, second = alr.shaped_pileup([0, 1, 65, 300, 2, 130], 900, V, seed=77)
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, V, size=(p.C, 16, 2)).astype(np.int32)
    pairs[rng.random((p.C, 16)) < 0.2] = -1
    pairs[:, 0] = np.stack([first, second], axis=1)
    pairs[:, 3] = pairs[:, 0]                                                            # a repeated pair
    pairs[:, 5, 1] = pairs[:, 5, 0] = np.abs(pairs[:, 5, 0])                             # j == k
    pairs[:, 7] = -1
    got = fit(p, G6, pairs, 0.9)
    suite.sixteen_slots(CALL, (p, G6), pairs, 0.9, got, "16 slots")


def test_no_marker_has_genotypes():
    p, first, second = alr.shaped_pileup([3, 0, 70], 200, 4, seed=9, missing_gp_frac=1.0)
    assert not p.has_gp.any()
    got = fit(p, G2, np.array([[[0, 1], [-1, -1]], [[1, 2], [2, 2]], [[3, 0], [3, 3]]], dtype=np.int32))
    assert got["status"].tolist() == [[5, 4], [5, 5], [5, 5]]
    assert all(not got[k].any() for k in FIELDS if k != "status")


def test_zero_cells():
    p, first, second = alr.shaped_pileup([3, 4], 50, 3, seed=8)
    with muxgl.Engine(0) as e:
        suite.empty_pileup(e, p)
        e.demux_set_gp(p.gp, p.has_gp)
        suite.zero_cells(CALL, e, (G2,))


# ---- 2. the reference's own slots ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,alphas", [(3, G2), (5, G6)])
def test_ll_top_and_ll_zero_are_the_reference_slots(V, alphas):
    """a call with alpha_max = alpha[n] has ll_top = llksAB[j][k][n] and ll_zero = the alpha = 0 slot, fitted or not; with
    alpha_max = 1 on a grid that holds 1.0, ll_top is the singlet table's entry of k"""
    p, first, second = alr.shaped_pileup([0, 1, 2, 63, 64, 65, 130, 700], 900, V, seed=500 + V)
    full = ur.full_ll(p, alphas)                                                         # [C][V][V][A]
    allp = np.array([(j, k) for j in range(V) for k in range(V)], dtype=np.int32)        # every ordered pair, j == k too
    rows = np.arange(p.C)[:, None]
    worst = 0.0
    with muxgl.Engine(0) as e:
        load(e, p)
        sng = e.demux_singlets(alphas)
        for b in range(0, len(allp), 16):
            pairs = np.ascontiguousarray(np.broadcast_to(allp[b:b + 16], (p.C,) + allp[b:b + 16].shape))
            j, k = pairs[..., 0], pairs[..., 1]
            for n in range(1, len(alphas)):
                got = e.demux_alpha_fit(alphas, pairs, alphas[n])
                d_top = np.abs(got["ll_top"] - full[rows, j, k, n])[1:].max()
                d_zero = np.abs(got["ll_zero"] - full[rows, j, k, 0])[1:].max()
                worst = max(worst, d_top, d_zero)
                assert d_top <= parity.LL_TOL and d_zero <= parity.LL_TOL, (b, n, d_top, d_zero)
                assert (got["status"][0] == 5).all() and not got["ll_top"][0].any()
                up = got["status"] == 2
                assert got["ll_hat"][up].tobytes() == got["ll_top"][up].tobytes()
                assert not (got["status"] == 3).any()
            if alphas[-1] == 1.0:
                assert np.abs(got["ll_top"] - sng[rows, k])[1:].max() <= parity.LL_TOL
                assert np.abs(got["ll_zero"] - sng[rows, j])[1:].max() <= parity.LL_TOL
    print(f"alpha fit V={V}: ll_top, ll_zero against the reference's slots: worst {worst:.3e}")


# ---- 3. mirror -----------------------------------------------------------------------------------------------------------

def test_mirror_on_the_device():
    V = 6
    p, first, second = alr.shaped_pileup([1, 64, 65, 300, 2100, 130, 33, 700], 2500, V, seed=321)
    pairs = shape_pairs(V, first, second, ("own", "rev", "wrong"))
    pairs = np.concatenate([pairs, pairs[:, 2:3, ::-1]], axis=1)                         # ... and the wrong pair reversed
    got = fit(p, G6, np.ascontiguousarray(pairs), 1.0)
    for a, b in ((0, 1), (2, 3)):
        d = np.abs(got["ll_hat"][:, a] - got["ll_hat"][:, b]).max()
        assert d <= 1e-9, d
        assert np.abs(got["ll_zero"][:, a] - got["ll_top"][:, b]).max() <= 1e-9
        strong = (got["info"][:, a] >= 1.0) & (got["status"][:, a] == 0)
        assert (got["status"][strong, b] == 0).all()
        s = np.abs(got["alpha_hat"][strong, a] + got["alpha_hat"][strong, b] - 1.0)
        print(f"alpha fit mirror slots {a}, {b}: |ll_hat difference| {d:.3e}, |alpha sum - 1| {s.max() if s.size else 0.0:.3e} "
              f"on {int(strong.sum())} droplets")
        assert (a > 0 or strong.sum() >= 4) and (s <= 1e-6).all()


# ---- 4. the model on the device -----------------------------------------------------------------------------------------

def test_the_device_finds_the_mixing_share():
    """tests/test_demux_alpha_fit.py holds the restatement to the same checks on the same pileup"""
    p, first, second = alr.doublet_pileup(**alr.MIXED)
    pairs = np.stack([first, second], axis=1).astype(np.int32)
    got = fit(p, G2, pairs, 1.0)
    sm = muxgl.alpha_fit_summary(got)
    assert (got["status"] == 0).all() and (sm["lrt"] > 10.0).all()
    assert (np.abs(got["alpha_hat"][:, 0] - np.array(alr.MIXED_SHARES)) <= 4.0 * sm["se"][:, 0]).mean() >= 0.9
    small = got["alpha_hat"][:, 0] < 0.4                                                 # shares 0.15 and 0.3: the first sample
    assert (sm["major"][small, 0] == first[small]).all()
    check_fit(p, G2, pairs, 1.0, got, "mixed", slots=[(c, 0) for c in range(0, p.C, 4)])


def test_clean_singlets_sit_on_the_lower_bound():
    p, first, second = alr.doublet_pileup(**alr.CLEAN)
    pairs = np.stack([first, second], axis=1).astype(np.int32)
    got = fit(p, G2, pairs, 1.0)
    at0 = got["status"][:, 0] == 1
    lrt0 = 2.0 * (got["ll_hat"] - got["ll_zero"])                                        # against j alone
    print(f"clean: {int(at0.sum())} of {p.C} droplets at the lower bound; largest LRT against the first alone {lrt0.max():.2f}")
    assert at0.sum() > p.C / 2 and (got["alpha_hat"][at0] == 0.0).all() and (got["n_steps"][at0] == 0).all()
    assert lrt0.max() <= 10.0
    assert got["ll_hat"][at0].tobytes() == got["ll_zero"][at0].tobytes()                 # (both are LL(0))
    check_fit(p, G2, pairs, 1.0, got, "clean", slots=[(c, 0) for c in range(0, p.C, 6)])


# ---- 5. bit identity ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def identity_case(V):
    p = many_samples.pileup(60, 4000, V, seed=900 + V, mean_entries=300, sigma=1.0, min_entries=0, max_entries=3000)
    rng = np.random.default_rng(V)
    pairs = rng.integers(0, V, size=(p.C, 16, 2)).astype(np.int32)
    pairs[rng.random((p.C, 16)) < 0.15] = -1
    pairs[:, 9] = pairs[:, 2]                                                            # a repeated pair in two slots
    return p, pairs, fit(p, G6, pairs, 0.87)


def test_call_to_call_budget_permutation_split_and_null_outputs(monkeypatch):
    p, pairs, want = identity_case(24)
    assert all(want[k][:, 9].tobytes() == want[k][:, 2].tobytes() for k in FIELDS)
    with suite.demux_open(p) as e:
        suite.identity(CALL, e, (G6,), pairs, want)
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
    assert same(fit(p, G6, pairs, 0.87), want)


@pytest.mark.parametrize("V", [24, 300])
def test_device_group_and_sharded_driver(V):
    p, pairs, want = identity_case(V)
    suite.device_groups(CALL, functools.partial(suite.demux_open, p), (G6,), pairs, want, flags=muxgl.FLAG_DEMUX_ONLY)
    with muxgl.Engine(0) as e:
        load(e, p)
        records = e.demux_run(G6, 0.5)
        called = demuxlet.call_pairs(records)
        direct = e.demux_alpha_fit(G6, called, 0.87)
    rec, got = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, G6, 0.5, want_alpha_fit=(0.87,))
    assert rec.tobytes() == records.tobytes() and np.array_equal(got["pair"], called) and same(got, direct)
    assert got["alpha_max"] == 0.87 and (called[records["valid"] != 0, 0] >= 0).all()


# ---- 6. state ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,flags", [(12, 0), (40, 0), (40, muxgl.FLAG_FORCE_STREAMED_CALL)])
def test_the_call_leaves_the_demuxlet_state_alone(V, flags):
    p = many_samples.pileup(30, 2000, V, seed=800 + V, mean_entries=80)
    pairs = np.random.default_rng(V).integers(0, V, size=(p.C, 2, 2)).astype(np.int32)
    pairs[::7, 1] = -1
    suite.demux_state_alone(CALL, p, flags, pairs, (G6,), (G2,), 1.0, G6)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals_leave_the_handle_usable(devs):
    p, first, second = alr.shaped_pileup([5, 0, 130, 64], 400, 8, seed=612)
    pairs = shape_pairs(8, first, second, ("own", "wrong"))
    fresh = fit(p, G2, pairs, 1.0, flags=muxgl.FLAG_DEMUX_ONLY, devs=devs)
    with muxgl.Engine(devs, muxgl.FLAG_DEMUX_ONLY) as e:
        refused, still_good = suite.refusal_frame(CALL, e, (G2,), pairs, 1.0, fresh, named=False)
        refused(b"pileup")
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        refused(b"GP tensor")
        e.demux_set_gp(p.gp, p.has_gp)
        still_good()
        suite.common_refusals(CALL, refused, still_good, pairs, 8)
        for n_alpha in (0, muxgl.MAX_ALPHA + 1):
            refused(b"n_alpha", n_alpha=n_alpha)
        still_good()
        for t in (0, 1):
            q = pairs.copy()
            q[3, 0, t] = -1
            refused(b"exactly one negative index", slots=q)
            still_good()
        with pytest.raises(ValueError):
            e.demux_alpha_fit(G2, pairs[:-1])
        with pytest.raises(ValueError):
            e.demux_alpha_fit(G2, pairs[:, :, :1])
        with pytest.raises(ValueError):
            e.demux_alpha_fit(G2, pairs, want=("rho_hat",))
