"""GPU tests of muxgl_demux_ambient_fit (demux_ambient_fit.hip): the per-droplet maximum-likelihood ambient share with its
observed information.  Against the restatement (tests/ambient_fit_ref.py) evaluated at the device's own rho_hat, against the
restatement's Newton-free maximiser, against the existing calls (singlet table, ambient table), the bounds, bit identity
across calls, budgets, device groups, the sharded driver, orders and groupings of candidates and subsets of outputs, the
state the call must leave alone, and the refusals.

Bars (check_fit): ll_hat, ll_zero within parity.LL_TOL; info and the implied LL' (0 at an interior estimate) within 1000 x
the float64-to-longdouble disagreement of the restatement on the case, floored at 1e-9 x the sum of absolute per-entry
terms; the restated LL at the device's estimate within 1e-9 of the LL at the restatement's; where the restated info is
>= 1 the two estimates within 1e-6.  One special case: where that tolerance is exactly 0 -- every per-entry term of the
restatement is exactly 0 in both precisions, which happens where the three genotype classes of a one-read entry cancel
(gp[0] == gp[2] at f == 0.5; droplet 1 of test_sixteen_candidates_with_skips_and_repeats is one) while the device's fused
dot leaves 1e-19 -- the floor is 1e-9 x the same sum over absolute summands (ambient_fit_ref.Cell.eval)."""
import ctypes
import functools

import numpy as np
import pytest

import ambient_fit_ref as afr
import ambient_ref as ar
import many_samples
import parity
from popscle_amd import demuxlet, muxgl

pytestmark = pytest.mark.gpu

G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
DEFAULT_RHOS = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)
FIELDS = muxgl.Engine.AMBIENT_FIT_FIELDS
WORST = {}   # what -> worst figure seen, printed by every check


def load(e, p):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)


def fit(p, alphas, f, cand, rho_max=0.5, flags=0, devs=0, want=FIELDS):
    with muxgl.Engine(devs, flags) as e:
        load(e, p)
        return e.demux_ambient_fit(alphas, f, cand, rho_max, want=want)


def same(a, b, fields=FIELDS):
    return all(a[k].tobytes() == b[k].tobytes() for k in fields)


def note(what, v):
    WORST[what] = max(WORST.get(what, 0.0), float(v))


def check_fit(p, alphas, f, cand, rho_max, got, what, pairs=None):
    """every bar of the module's docstring on the (droplet, slot) pairs of `pairs` (None: all); returns the number of fitted
    cases and of those with restated info >= 1"""
    ld = np.longdouble
    cand = np.asarray(cand).reshape(p.C, -1)
    assert all(got[k].shape == cand.shape for k in FIELDS)
    assert (got["n_steps"] <= 48).all() and (got["n_steps"] >= 0).all() and not (got["status"] == 3).any()
    fitted = strong = 0
    seen = {}
    for c, k in (pairs if pairs is not None else [(c, k) for c in range(p.C) for k in range(cand.shape[1])]):
        j = int(cand[c, k])
        g = {n: got[n][c, k] for n in FIELDS}
        if j < 0:
            assert g["status"] == 4 and all(g[n] == 0 for n in FIELDS if n != "status"), (c, k, g)
            continue
        if (c, j) not in seen:
            seen[(c, j)] = afr.fit(p, alphas, f, c, j, rho_max)
        r = seen[(c, j)]
        cell = r["cell"]
        if cell.n == 0:
            assert g["status"] == 5 and all(g[n] == 0 for n in FIELDS if n != "status"), (c, k, g)
            continue
        x = float(g["rho_hat"])
        assert g["status"] in (0, 1, 2) and 0.0 <= x <= rho_max, (c, k, g)
        L, d1, d2, aL, a1, a2, s1, s2 = [float(v[0]) for v in cell.eval([x], ld)]
        L64, d164, d264 = [float(v[0]) for v in cell.eval([x], np.float64)[:3]]
        tol1 = max(1000.0 * abs(d164 - d1), 1e-9 * a1)
        tol2 = max(1000.0 * abs(d264 - d2), 1e-9 * a2)
        if tol1 == 0.0 or tol2 == 0.0:   # every term exactly 0 in both precisions: the floor over absolute summands
            tol1, tol2 = max(tol1, 1e-9 * s1), max(tol2, 1e-9 * s2)
        note(f"{what}: |ll_hat - ref|", abs(g["ll_hat"] - L))
        note(f"{what}: |ll_zero - ref|", abs(g["ll_zero"] - r["ll_zero"]))
        note(f"{what}: |info - ref| / tol", abs(g["info"] + d2) / tol2)
        assert abs(g["ll_hat"] - L) <= parity.LL_TOL and abs(g["ll_zero"] - r["ll_zero"]) <= parity.LL_TOL, (c, k, g, L)
        assert abs(g["info"] + d2) <= tol2, (c, k, g, d2, tol2)
        if g["status"] == 1:
            assert x == 0.0 and d1 <= tol1, (c, k, g, d1)
        elif g["status"] == 2:
            assert x == rho_max and d1 >= -tol1, (c, k, g, d1)
        else:
            note(f"{what}: |LL'(rho_hat)| / tol", abs(d1) / tol1)
            assert abs(d1) <= tol1, (c, k, g, d1, tol1)
            fitted += 1
        note(f"{what}: LL(ref rho) - LL(device rho)", r["ll_hat"] - L)
        assert L >= r["ll_hat"] - 1e-9, (c, k, g, r["rho_hat"], r["ll_hat"], L)
        if r["info"] >= 1.0:
            strong += g["status"] == 0
            note(f"{what}: |rho_hat - ref|", abs(x - r["rho_hat"]))
            assert abs(x - r["rho_hat"]) <= 1e-6, (c, k, g, r["rho_hat"], r["info"])
            assert g["status"] == r["status"], (c, k, g, r["status"])
    for key in sorted(WORST):
        if key.startswith(what + ":"):
            print(f"ambient fit {key} {WORST[key]:.3e}")
    print(f"ambient fit {what}: {fitted} interior fits, {strong} with info >= 1, mean n_steps "
          f"{float(got['n_steps'][got['status'] == 0].mean()) if (got['status'] == 0).any() else 0.0:.2f}")
    return fitted, strong


# ---- 1. parity and optimality over the shapes ----------------------------------------------------------------------------

SHAPES = [0, 1, 2, 63, 64, 65, 2048, 2049, 5003]


@functools.lru_cache(maxsize=None)
def shaped(V, seed, missing=0.03):
    """droplets of exactly 0, 1, 2, 63, 64, 65, 2048, 2049 and 5003 entries of 1, 2, 33 and 60 reads at base qualities 2..93,
    READ_OTHER bytes, 3 % of the markers without genotypes, a fifth of the reads from the pool"""
    p, who, pool = afr.shaped_pileup(SHAPES, 6000, V, seed, missing_gp_frac=missing)
    assert (p.reads == ar.READ_OTHER).any() and set(np.diff(p.entry_rptr).tolist()) == {1, 2, 33, 60}
    assert missing in (0.0, 1.0) or (p.has_gp == 0).any()
    return p, who, pool


@pytest.mark.parametrize("V,alphas,n_cand", [(1, G2, 1), (17, G6, 2), (70, G2, 2), (300, G2, 1)])
def test_shapes_vs_restatement(V, alphas, n_cand):
    p, who, pool = shaped(V, 40 + V)
    # (one sample: the pool IS the sample and LL is flat in rho, so the profile is a drawn one there and most droplets
    # sit on the lower bound)
    f = pool if V > 1 else ar.draw_af(p.S, seed=3)
    cand = np.stack([(who + k) % V for k in range(n_cand)], axis=1).astype(np.int32)   # the droplet's own sample first
    got = fit(p, alphas, f, cand, 0.5)
    assert got["kernel_ms"] > 0.0
    fitted, strong = check_fit(p, alphas, f, cand, 0.5, got, f"shapes V={V}")
    assert got["status"][0].tolist() == [5] * n_cand                                    # the droplet without entries
    assert V == 1 or (fitted >= 5 and strong >= 0.8 * fitted), (fitted, strong)


def test_sixteen_candidates_with_skips_and_repeats():
    V = 17
    p, who, pool = afr.shaped_pileup([0, 1, 65, 300, 2, 130], 900, V, seed=77)
    rng = np.random.default_rng(5)
    cand = rng.integers(-1, V, size=(p.C, 16)).astype(np.int32)
    cand[:, 0] = who
    cand[:, 3] = who                                                                     # a repeated candidate
    cand[:, 7] = -1
    got = fit(p, G6, pool, cand, 0.4)
    check_fit(p, G6, pool, cand, 0.4, got, "16 candidates")
    assert all(got[k][:, 3].tobytes() == got[k][:, 0].tobytes() for k in FIELDS)
    assert (got["status"][:, 7] == 4).all()


def test_no_marker_has_genotypes():
    p, who, pool = afr.shaped_pileup([3, 0, 70], 200, 4, seed=9, missing_gp_frac=1.0)
    assert not p.has_gp.any()
    got = fit(p, G2, np.full(p.S, np.nan), np.array([[0, -1], [1, 2], [3, 3]], dtype=np.int32))   # (such f do not matter)
    assert got["status"].tolist() == [[5, 4], [5, 5], [5, 5]]
    assert all(not got[k].any() for k in FIELDS if k != "status")


def test_zero_cells():
    p, who, pool = afr.shaped_pileup([3, 4], 50, 3, seed=8)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8))
        e.demux_set_gp(p.gp, p.has_gp)
        got = e.demux_ambient_fit(G2, pool, np.zeros((0, 2), np.int32))
    assert got["rho_hat"].shape == (0, 2) and got["kernel_ms"] == 0.0


# ---- 2. consistency with the existing calls ------------------------------------------------------------------------------

@pytest.mark.parametrize("V,alphas", [(6, G2), (40, G6)])
def test_consistent_with_the_singlet_and_the_ambient_tables(V, alphas):
    p, who, pool = afr.shaped_pileup([0, 5, 64, 200, 700, 2100, 90, 33], 2500, V, seed=300 + V)
    with muxgl.Engine(0) as e:
        load(e, p)
        sng = e.demux_singlets(alphas)
        cand = demuxlet.top_samples(sng, 2)
        got = e.demux_ambient_fit(alphas, pool, cand, 0.5)
        table = e.demux_ambient(alphas, pool, DEFAULT_RHOS)["ll"]
        at_hat = np.zeros(cand.shape)
        for c in range(p.C):                       # the table at the droplet's own estimates: one rho per call and slot
            for k in range(2):
                at_hat[c, k] = e.demux_ambient(alphas, pool, [got["rho_hat"][c, k]])["ll"][c, cand[c, k], 0]
        coarse = e.demux_ambient(alphas, pool, afr.coarse_points(0.5))["ll"]
    rows = np.arange(p.C)[:, None]
    d0 = np.abs(got["ll_zero"] - sng[rows, cand]).max()
    d1 = np.abs(got["ll_hat"] - at_hat).max()
    print(f"ambient fit V={V}: |ll_zero - singlet table| {d0:.3e}, |ll_hat - ambient table at rho_hat| {d1:.3e}")
    assert d0 <= parity.LL_TOL and d1 <= parity.LL_TOL
    xs = afr.coarse_points(0.5)
    for c in range(p.C):                           # no point of the default grid inside the bracket is better
        for k in range(2):
            if got["status"][c, k] in (4, 5):
                continue
            i = int(np.argmax(coarse[c, cand[c, k]]))
            lo, hi = xs[max(i - 1, 0)], xs[min(i + 1, 8)]
            assert lo <= got["rho_hat"][c, k] <= hi, (c, k, lo, hi, got["rho_hat"][c, k])
            inside = [r for r, rho in enumerate(DEFAULT_RHOS) if lo <= rho <= hi]
            assert inside and (got["ll_hat"][c, k] >= table[c, cand[c, k], inside] - 1e-9).all(), (c, k)


# ---- 3. bounds ---------------------------------------------------------------------------------------------------------

def test_no_soup_sits_on_the_lower_bound_and_a_small_cap_on_the_upper():
    clean, who, pool = ar.soup_pileup(**dict(ar.SOUP, soup=0.0))
    got = fit(clean, G2, pool, who.astype(np.int32), 0.5)
    at0 = got["status"][:, 0] == 1
    print(f"soup = 0: {int(at0.sum())} of {clean.C} droplets at the lower bound; others {got['rho_hat'][~at0, 0].tolist()}")
    assert at0.sum() > clean.C / 2 and (got["rho_hat"][at0] == 0.0).all() and (got["n_steps"][at0] == 0).all()
    assert np.abs(got["ll_hat"][at0] - got["ll_zero"][at0]).max() <= 1e-9      # (both are LL(0))
    soup, who, pool = ar.soup_pileup(**ar.SOUP)
    got = fit(soup, G2, pool, who.astype(np.int32), 0.05)
    assert (got["status"] == 2).all() and got["rho_hat"].tobytes() == np.full((soup.C, 1), 0.05).tobytes()
    check_fit(soup, G2, pool, who.astype(np.int32), 0.05, got, "upper bound", pairs=[(c, 0) for c in range(0, soup.C, 6)])


def test_the_device_finds_the_soup_share():
    """tests/test_demux_ambient_fit.py holds the restatement to the same checks on the same pileup"""
    p, who, pool = ar.soup_pileup(**ar.SOUP)
    got = fit(p, G2, pool, who.astype(np.int32), 0.5)
    sm = muxgl.ambient_fit_summary(got)
    assert (got["status"] == 0).all() and (sm["lrt"] > 10.0).all()
    assert (np.abs(got["rho_hat"] - 0.2) <= 4.0 * sm["se"]).mean() >= 0.9
    check_fit(p, G2, pool, who.astype(np.int32), 0.5, got, "soup", pairs=[(c, 0) for c in range(0, p.C, 4)])


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def identity_case(V):
    p = many_samples.pileup(60, 4000, V, seed=900 + V, mean_entries=300, sigma=1.0, min_entries=0, max_entries=3000)
    f = ar.draw_af(p.S, seed=V)
    cand = np.random.default_rng(V).integers(-1, V, size=(p.C, 16)).astype(np.int32)
    return p, f, cand, fit(p, G6, f, cand, 0.37)


def test_call_to_call_budget_permutation_split_and_null_outputs(monkeypatch):
    p, f, cand, want = identity_case(24)
    assert (want["status"] == 0).any() and (want["status"] == 4).any()
    with muxgl.Engine(0) as e:
        load(e, p)
        assert same(e.demux_ambient_fit(G6, f, cand, 0.37), want) and same(e.demux_ambient_fit(G6, f, cand, 0.37), want)
        perm = np.random.default_rng(1).permutation(16)
        got = e.demux_ambient_fit(G6, f, np.ascontiguousarray(cand[:, perm]), 0.37)
        assert same(got, {k: np.ascontiguousarray(want[k][:, perm]) for k in FIELDS})
        lo = e.demux_ambient_fit(G6, f, np.ascontiguousarray(cand[:, :8]), 0.37)
        hi = e.demux_ambient_fit(G6, f, np.ascontiguousarray(cand[:, 8:]), 0.37)
        assert same({k: np.concatenate([lo[k], hi[k]], axis=1) for k in FIELDS}, want)
        for sub in (("rho_hat",), ("status", "n_steps"), ("info", "ll_zero"), ("ll_hat", "n_steps", "rho_hat")):
            got = e.demux_ambient_fit(G6, f, cand, 0.37, want=sub)
            assert set(got) == set(sub) | {"kernel_ms"} and same(got, want, sub)
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
    assert same(fit(p, G6, f, cand, 0.37), want)


@pytest.mark.parametrize("V", [24, 300])
def test_device_group_and_sharded_driver(V):
    p, f, cand, want = identity_case(V)
    for devs in ([0, 0], [0, 0, 0]):
        got = fit(p, G6, f, cand, 0.37, flags=muxgl.FLAG_DEMUX_ONLY, devs=devs)
        assert same(got, want) and got["kernel_ms"] > 0.0
    with muxgl.Engine(0) as e:
        load(e, p)
        records = e.demux_run(G6, 0.5)
        top = demuxlet.top_samples(e.demux_singlets(G6), 3)
        direct = e.demux_ambient_fit(G6, f, top, 0.37)
    rec, got = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, G6, 0.5, want_ambient_fit=(f, 0.37, 3))
    assert rec.tobytes() == records.tobytes() and np.array_equal(got["cand"], top) and same(got, direct)


# ---- 5. state ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,flags", [(12, 0), (40, 0), (40, muxgl.FLAG_FORCE_STREAMED_CALL)])
def test_the_call_leaves_the_demuxlet_state_alone(V, flags):
    p = many_samples.pileup(30, 2000, V, seed=800 + V, mean_entries=80)
    f = ar.draw_af(p.S, seed=V)
    cand = np.random.default_rng(V).integers(-1, V, size=(p.C, 2)).astype(np.int32)
    with muxgl.Engine(0, flags) as e:
        load(e, p)
        full = flags == 0                                    # (the streamed call keeps no LL tensor)
        run = lambda: e.demux_run(G6, 0.5, want_full_ll=True) if full else (e.demux_run(G6, 0.5), np.zeros(0))
        r0, full0 = run()
        view, t0, pg0 = e.demux_results_view().tobytes(), e.timing().copy(), e.demux_entry_pg().tobytes()
        a0 = e.demux_ambient_fit(G6, f, cand, 0.5)
        assert e.demux_results_view().tobytes() == view and np.array_equal(e.timing(), t0)
        e.demux_ambient_fit(G2, f, cand, 0.25)               # another grid between two runs
        assert e.demux_results_view().tobytes() == view and np.array_equal(e.timing(), t0)
        assert e.demux_entry_pg().tobytes() == pg0           # the cached grid is still the run's
        r1, full1 = run()
        a1 = e.demux_ambient_fit(G6, f, cand, 0.5)
    assert r0.tobytes() == r1.tobytes() == view and full0.tobytes() == full1.tobytes() and same(a0, a1)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals_leave_the_handle_usable(devs):
    p, who, pool = afr.shaped_pileup([5, 0, 130, 64], 400, 8, seed=612)
    f = pool
    with_gp = int(np.flatnonzero(p.has_gp != 0)[3])
    cand = np.stack([who, (who + 3) % 8], axis=1).astype(np.int32)
    fresh = fit(p, G2, f, cand, 0.5, flags=muxgl.FLAG_DEMUX_ONLY, devs=devs)
    VP = ctypes.c_void_p

    def raw(e, n_alpha=2, n_cand=2, cnd=cand, rho_max=0.5, outs=True, af=f):
        dp = muxgl._DemuxParams()
        dp.n_alpha = n_alpha
        dp.alpha[1] = 0.5
        dp.doublet_prior = 0.5
        bufs = [np.zeros(cand.shape), np.zeros(cand.shape), np.zeros(cand.shape), np.zeros(cand.shape),
                np.zeros(cand.shape, np.int32), np.zeros(cand.shape, np.int32)]
        rc = e.lib.muxgl_demux_ambient_fit(e.h, ctypes.byref(dp), None if af is None else af.ctypes.data_as(VP), n_cand,
                                           None if cnd is None else cnd.ctypes.data_as(VP), ctypes.c_double(rho_max),
                                           *[b.ctypes.data_as(VP) if outs else None for b in bufs], None)
        return rc, e.lib.muxgl_last_error(e.h)

    def refused(e, word, **kw):
        rc, why = raw(e, **kw)
        assert rc != 0 and word in why, (kw, why)

    with muxgl.Engine(devs, muxgl.FLAG_DEMUX_ONLY) as e:
        def still_good():
            assert same(e.demux_ambient_fit(G2, f, cand, 0.5), fresh)

        refused(e, b"pileup")
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        refused(e, b"GP tensor")
        e.demux_set_gp(p.gp, p.has_gp)
        still_good()
        refused(e, b"every output is NULL", outs=False)
        still_good()
        refused(e, b"cand is NULL", cnd=None)
        refused(e, b"amb_af is NULL", af=None)
        still_good()
        for n_cand in (0, 17, -1):
            refused(e, b"n_cand", n_cand=n_cand)
        for n_alpha in (0, muxgl.MAX_ALPHA + 1):
            refused(e, b"n_alpha", n_alpha=n_alpha)
        still_good()
        for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
            refused(e, b"rho_max", rho_max=bad)
        still_good()
        for bad in (-2, 8, 1 << 20):
            c2 = cand.copy()
            c2[2, 1] = bad
            refused(e, b"cand[2][1]", cnd=c2)
            still_good()
        for bad in (-0.01, 1.5, float("nan"), float("inf")):
            g = f.copy()
            g[with_gp] = bad
            refused(e, f"amb_af of marker {with_gp} ".encode(), af=g)
            still_good()
        with pytest.raises(ValueError):
            e.demux_ambient_fit(G2, f[:-1], cand)
        with pytest.raises(ValueError):
            e.demux_ambient_fit(G2, f, cand[:-1])
