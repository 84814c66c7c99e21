"""GPU tests of muxgl_pileup_read_hist and muxgl_demux_soup_mix (soup_mix.hip): the histogram against numpy, exactly; the fit
against the longdouble restatement of tests/soup_mix_ref.py (every ll[i] within LL_TOL, pi, grad and amb_af within 1e-6);
the evaluation mode; bit identity across calls, for the own pileup against its histogram passed in, for permuted droplets,
on a group and through the sharded driver; the identities; the refusals and the state the call must leave alone; and the
planted pool of tests/test_soup_mix.py on the device's output.

Shapes: at most 400 droplets and 3 000 markers; M in {1, 2, 3, 6, 63, 64, 65, 130, 300} (the packed forms, the wave boundary,
several lanes' worth of columns); an active-marker count the update block does not divide and one that gives a single
block; markers without genotypes and without reads; a marker with 40 records, 0xFF reads, qualities 0, 1, 2 and 93."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import soup_mix_ref as sr
from popscle_amd import demuxlet, muxgl, synth

pytestmark = pytest.mark.gpu

UPDATE_BLOCK = 256          # soup_mix_plan::UPDATE_BLOCK (tests/test_soup_mix.py holds the header to it)
OUT = ("pi", "grad", "ll", "amb_af")


def load(e, p):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)


@functools.lru_cache(maxsize=None)
def case(V, S, C, ment, seed=0):
    """a random pileup with markers without genotypes, 0xFF reads, markers nobody covers, and one more droplet whose single
    entry puts 40 distinct read bytes (both alleles at qualities 0, 1, 2, 93 and others), some twice, and 0xFF on a marker
    with genotypes"""
    p = synth.make_pileup(C, S, V, seed=4000 + 13 * V + seed, mean_entries=ment, min_entries=0, reads_lambda=1.0, other=0.1,
                          missing_gp_frac=0.05, max_bq=60, cap_bq=60)
    s0 = int(np.flatnonzero(p.has_gp != 0)[1])
    bqs = [0, 1, 2, 93] + list(range(10, 26))
    extra = np.array([(a << 7) | q for a in (0, 1) for q in bqs] + [0xFF, 93, 0x80 | 2, 0xFF, 17], dtype=np.uint8)
    q = synth.Pileup(p.C + 1, p.S, np.append(p.cell_ptr, p.nnz + 1), np.append(p.entry_snp, np.int32(s0)),
                     np.append(p.entry_rptr, p.R + extra.size), np.concatenate([p.reads, extra]), p.af, p.gp, p.has_gp)
    k, _ = sr.read_hist(q)
    assert np.sum(k >> 8 == s0) >= 40 and (q.has_gp == 0).any() and (q.reads == synth.READ_OTHER).any()
    assert np.unique(k >> 8).size < q.S                                   # markers without reads
    return q


def same(a, b, what=""):
    for k in OUT:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert (a["n_iter"], a["n_reads"], a["status"]) == (b["n_iter"], b["n_reads"], b["status"]), what


def against(got, want, what, strict=True):
    """the issue's bars; prints and returns the worst deviations (ll, pi, grad, amb_af).  strict: the two stopped at the
    same step (with one component a step is 0 or one rounding, so tol = 0 may stop either of them early)"""
    n = min(int((~np.isnan(want["ll"])).sum()), int((~np.isnan(got["ll"])).sum()))
    assert n >= 1 and (not strict or np.array_equal(np.isnan(got["ll"]), np.isnan(np.asarray(want["ll"], dtype=np.float64)))), what
    d = [float(np.max(np.abs(got["ll"][:n] - want["ll"][:n])))] + \
        [float(np.max(np.abs(got[k] - want[k]))) for k in ("pi", "grad", "amb_af")]
    print(f"soup mix {what}: max |dLL| {d[0]:.3e}, |dpi| {d[1]:.3e}, |dgrad| {d[2]:.3e}, |daf| {d[3]:.3e}")
    assert d[0] <= sr.LL_TOL and max(d[1:]) <= 1e-6, (what, d)
    assert got["n_reads"] == want["n_reads"] and (not strict or (got["n_iter"], got["status"]) == (want["n_iter"], want["status"])), what
    return d


# ---- 1. the histogram ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_read_hist_equals_numpy(devs):
    p = case(6, 3000, 200, 40)
    rng = np.random.default_rng(5)
    reads_of_cell = np.diff(p.entry_rptr[p.cell_ptr])
    with muxgl.Engine(devs, muxgl.FLAG_DEMUX_ONLY) as e:
        with pytest.raises(muxgl.MuxglError, match="pileup"):
            e.pileup_read_hist()
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)   # (needs no genotypes)
        for mask in (None, rng.random(p.C) < 0.5, np.zeros(p.C, bool), np.ones(p.C, bool), reads_of_cell <= np.median(reads_of_cell)):
            k, c = e.pileup_read_hist(mask)
            wk, wc = sr.read_hist(p, mask)
            assert k.dtype == np.int64 and np.array_equal(k, wk) and np.array_equal(c, wc)
            n_ref, n_alt = e.pileup_allele_counts(mask)                      # summed per (marker, allele)
            alt = (k & 0x80) != 0
            assert np.array_equal(np.bincount(k[~alt] >> 8, weights=c[~alt], minlength=p.S).astype(np.int64), n_ref)
            assert np.array_equal(np.bincount(k[alt] >> 8, weights=c[alt], minlength=p.S).astype(np.int64), n_alt)
        n = ctypes.c_int64(0)
        small = np.zeros(3, dtype=np.int64)
        VP = ctypes.c_void_p
        assert e.lib.muxgl_pileup_read_hist(e.h, None, small.ctypes.data_as(VP), small.ctypes.data_as(VP), 3, ctypes.byref(n)) != 0
        assert b"room for 3" in e.lib.muxgl_last_error(e.h) and n.value == sr.read_hist(p)[0].size
        assert np.array_equal(e.pileup_read_hist()[0], sr.read_hist(p)[0])    # the handle is still usable


# ---- 2. against the restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,S,C,ment,unknown", [
    (1, 200, 30, 20, False),          # 64 markers side by side; a single update block
    (2, 200, 30, 20, False),
    (3, 700, 60, 40, False),
    (6, 3000, 200, 40, False),        # eight markers side by side; several blocks, the last one short
    (5, 3000, 200, 40, "hwe"),        # M = 6 with the unknown component from a caller's prior
    (63, 1500, 80, 40, False),
    (63, 1500, 80, 40, "mean"),       # M = 64: the wave boundary through the extra column
    (64, 1500, 80, 40, False),
    (64, 1500, 80, 40, "mean"),       # M = 65: one component in a lane's second round
    (65, 1500, 80, 40, False),
    (130, 3000, 100, 60, False),      # three rounds per lane, three column groups of the update
    (300, 2000, 60, 60, False),
])
def test_twenty_steps_against_the_restatement(V, S, C, ment, unknown):
    p = case(V, S, C, ment)
    gp0 = sr.hwe_prior(p.af) if unknown == "hwe" else None
    reads_of_cell = np.diff(p.entry_rptr[p.cell_ptr])
    mask = reads_of_cell <= np.quantile(reads_of_cell, 0.7)
    mask[-1] = True                                                       # (the droplet with the 40 records)
    keys, counts = sr.read_hist(p, mask)
    want = sr.fit(keys, counts, p.gp, p.has_gp, with_unknown=bool(unknown), gp0=gp0, n_iter_max=20, tol=0.0)
    n_act = want["model"].markers.size
    if S == 200:
        assert 0 < n_act <= UPDATE_BLOCK                                  # a single block
    if S == 3000:
        assert n_act > UPDATE_BLOCK and n_act % UPDATE_BLOCK != 0         # the block does not divide it
    with muxgl.Engine(0) as e:
        load(e, p)
        got = e.demux_soup_mix(mask, with_unknown=bool(unknown), gp0=gp0, n_iter_max=20, tol=0.0)
    assert got["kernel_ms"] > 0.0 and (V == 1 or (got["status"] == 1 and got["n_iter"] == 20))
    against(got, want, f"V={V} M={V + bool(unknown)} active={n_act}", strict=V > 1)


# ---- 3. the evaluation mode -----------------------------------------------------------------------------------------------

def test_evaluation_mode():
    p = case(6, 3000, 200, 40)
    keys, counts = sr.read_hist(p)
    conv = sr.fit(keys, counts, p.gp, p.has_gp, n_iter_max=3000, tol=1e-13)
    assert conv["status"] == 0
    pi_hat = np.asarray(conv["pi"], dtype=np.float64)
    rng = np.random.default_rng(2)
    pi0 = rng.random(6) * 3.0                                              # (not normalised: the call divides by the sum)
    with muxgl.Engine(0) as e:
        load(e, p)
        got = e.demux_soup_mix(pi0=pi0, n_iter_max=0)
        against(got, sr.fit(keys, counts, p.gp, p.has_gp, pi0=pi0, n_iter_max=0), "evaluation at a given pi0")
        assert got["ll"].shape == (1,) and got["n_iter"] == 0 and got["status"] == 1
        one = e.demux_soup_mix(pi0=pi_hat, n_iter_max=5, tol=1e-8)
    ref = sr.fit(keys, counts, p.gp, p.has_gp, pi0=pi_hat, n_iter_max=5, tol=1e-8)
    assert one["status"] == 0 and one["n_iter"] == 1 and np.isnan(one["ll"][2:]).all() and not np.isnan(one["ll"][:2]).any()
    on = one["pi"] > 0
    dev = np.abs(one["grad"][on] - 1.0)
    assert np.max(np.abs(dev - np.abs(np.asarray(ref["grad"], dtype=np.float64)[on] - 1.0))) <= 1e-6
    assert muxgl.soup_mix_summary(one)["max_grad_dev"] == float(dev.max())
    against(one, ref, "one step from the converged pi")


# ---- 4. determinism -------------------------------------------------------------------------------------------------------

class ThreadExchange:
    """two ranks of demuxlet.run_sharded as two threads of this process"""

    def __init__(self, rank, world, shared):
        self.rank, self.world, self.device_ordered, self.shared = rank, world, False, shared

    def gather_objects(self, obj):
        box, barrier = self.shared
        box[self.rank] = obj
        barrier.wait()
        out = list(box)
        barrier.wait()
        return out


@pytest.mark.parametrize("V,unknown", [(6, True), (65, False)])
def test_bit_identity(V, unknown):
    p = case(V, 3000 if V == 6 else 1500, 200 if V == 6 else 80, 40)
    kw = dict(with_unknown=unknown, n_iter_max=12, tol=1e-3)
    with muxgl.Engine(0) as e:
        load(e, p)
        a = e.demux_soup_mix(**kw)
        same(a, e.demux_soup_mix(**kw), "two calls")
        hist = e.pileup_read_hist()
        same(a, e.demux_soup_mix(hist=hist, **kw), "the own pileup against its histogram")
        sub = e.demux_soup_mix(want=("pi",), **kw)
        assert set(sub) & set(OUT) == {"pi"} and np.array_equal(sub["pi"], a["pi"])
    perm = np.random.default_rng(3).permutation(p.C)
    q = p.subset_cells(perm)
    with muxgl.Engine(0) as e:
        load(e, q)
        same(a, e.demux_soup_mix(**kw), "droplets permuted")
    with muxgl.Engine([0, 0], muxgl.FLAG_DEMUX_ONLY) as e:
        load(e, p)
        same(a, e.demux_soup_mix(**kw), "a [0, 0] group")
        assert np.array_equal(e.pileup_read_hist()[0], hist[0])
    got = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, want_soup_mix=(None, unknown, 12, 1e-3))[-1]
    same(a, got, "run_sharded, world 1")
    assert np.array_equal(got["hist"][0], hist[0]) and np.array_equal(got["hist"][1], hist[1])
    shared = ([None, None], threading.Barrier(2))
    res = [None, None]

    def rank(r):
        res[r] = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, exchange=ThreadExchange(r, 2, shared),
                                      want_soup_mix=(None, unknown, 12, 1e-3))[-1]

    th = [threading.Thread(target=rank, args=(r,)) for r in (0, 1)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert res[0] is not None and res[1] is not None
    same(a, res[0], "run_sharded, rank 0 of 2")
    same(a, res[1], "run_sharded, rank 1 of 2")


def test_masked_group_equals_one_device():
    p = case(6, 3000, 200, 40)
    mask = np.random.default_rng(9).random(p.C) < 0.4
    with muxgl.Engine(0) as e:
        load(e, p)
        a = e.demux_soup_mix(mask, n_iter_max=8, tol=0.0)
    with muxgl.Engine([0, 0, 0], muxgl.FLAG_DEMUX_ONLY) as e:
        load(e, p)
        same(a, e.demux_soup_mix(mask, n_iter_max=8, tol=0.0), "a masked [0, 0, 0] group")


# ---- 5. identities --------------------------------------------------------------------------------------------------------

def test_identities():
    p1 = case(1, 200, 30, 20)
    with muxgl.Engine(0) as e:
        load(e, p1)
        one = e.demux_soup_mix(n_iter_max=3, tol=0.0)
    # M = 1: grad = (1 / N) sum n (pR r + pA a) / D with D = pR r + pA a, N terms of value n within a few roundings each
    assert np.array_equal(one["pi"], [1.0]) or abs(one["pi"][0] - 1.0) <= 64 * 2.0 ** -52
    assert abs(one["grad"][0] - 1.0) <= 64 * 2.0 ** -52 and one["n_reads"] > 0
    p = case(6, 3000, 200, 40)
    gp = p.gp.copy()
    gp[:, 4, :] = gp[:, 1, :]                                              # two identical panel columns
    twin = synth.Pileup(p.C, p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads, p.af, gp, p.has_gp)
    pi0 = np.array([0.3, 0.0, 0.2, 0.1, 0.4, 0.0])
    with muxgl.Engine(0) as e:
        load(e, twin)
        t = e.demux_soup_mix(n_iter_max=25, tol=0.0)
        z = e.demux_soup_mix(pi0=pi0, n_iter_max=25, tol=0.0)
    assert t["pi"][1] == t["pi"][4] and t["grad"][1] == t["grad"][4] and t["pi"][1] > 0       # bitwise
    assert z["pi"][1] == 0.0 and z["pi"][5] == 0.0 and np.all(z["pi"][[0, 2, 3, 4]] > 0)      # a share of 0 stays 0
    assert abs(t["pi"].sum() - 1.0) < 1e-12 and np.all(np.diff(t["ll"]) >= -sr.LL_TOL)


def test_no_record_takes_part():
    p = case(3, 700, 60, 40)
    with muxgl.Engine(0) as e:
        load(e, p)
        got = e.demux_soup_mix(np.zeros(p.C, bool), pi0=[1.0, 2.0, 1.0], n_iter_max=4)
        empty = e.demux_soup_mix(hist=(np.zeros(0, np.int64), np.zeros(0, np.int64)), pi0=[1.0, 2.0, 1.0], n_iter_max=4)
    for g in (got, empty):
        assert g["status"] == 2 and g["n_reads"] == 0 and g["n_iter"] == 0 and np.array_equal(g["pi"], [0.25, 0.5, 0.25])
        assert g["ll"][0] == 0.0 and np.isnan(g["ll"][1:]).all() and not g["grad"].any()
        want = sr.fit(np.zeros(0, np.int64), np.zeros(0, np.int64), p.gp, p.has_gp, pi0=[1.0, 2.0, 1.0], n_iter_max=4)
        assert np.max(np.abs(g["amb_af"] - want["amb_af"])) <= 1e-6 and np.all(g["amb_af"][p.has_gp == 0] == 0.5)


# ---- 6. refusals and state ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals_leave_the_handle_usable(devs):
    p = case(6, 3000, 200, 40)
    keys, counts = sr.read_hist(p)
    G2 = (0.0, 0.5)
    with muxgl.Engine(0) as e:
        load(e, p)
        fresh = e.demux_run(G2, 0.5)
    bad_hists = [
        (keys[::-1].copy(), counts, "ascending"), (np.append(keys, keys[-1]), np.append(counts, 1), "ascending"),
        (np.append(keys, p.S * 256 + 3), np.append(counts, 1), "names no marker"), (np.array([-5]), np.array([1]), "names no marker"),
        (np.array([256 * 7 + 255]), np.array([2]), "0xFF"), (keys, np.where(np.arange(keys.size) == 4, 0, counts), "not above 0"),
        (keys, np.where(np.arange(keys.size) == 4, -3, counts), "not above 0")]
    inf, nan = float("inf"), float("nan")
    gp0 = sr.hwe_prior(p.af)
    with muxgl.Engine(devs, muxgl.FLAG_DEMUX_ONLY) as e:
        with pytest.raises(muxgl.MuxglError, match="pileup"):
            e.V = 6
            e.S = p.S
            e.demux_soup_mix(hist=(keys, counts))
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        with pytest.raises(muxgl.MuxglError, match="GP tensor"):
            e.V = 6
            e.demux_soup_mix()
        e.demux_set_gp(p.gp, p.has_gp)

        def still_good():
            assert e.demux_run(G2, 0.5).tobytes() == fresh.tobytes()

        still_good()
        for k, c, why in bad_hists:
            with pytest.raises(muxgl.MuxglError, match=why):
                e.demux_soup_mix(hist=(k, c))
            still_good()
        for bad in ([0.5, -0.1, 0.2, 0.2, 0.1, 0.1], [0.5, nan, 0.2, 0.2, 0.1, 0.1], [0.5, inf, 0.2, 0.2, 0.1, 0.1]):
            with pytest.raises(muxgl.MuxglError, match=r"pi0\[1\]"):
                e.demux_soup_mix(pi0=bad)
        with pytest.raises(muxgl.MuxglError, match="pi0 sums to"):
            e.demux_soup_mix(pi0=np.zeros(6))
        still_good()
        for bad in (-0.5, nan, inf):
            g = gp0.copy()
            g[11, 2] = bad
            with pytest.raises(muxgl.MuxglError, match="gp0 of marker 11 "):
                e.demux_soup_mix(with_unknown=True, gp0=g)
        still_good()
        with pytest.raises(muxgl.MuxglError, match="n_iter_max"):
            e.demux_soup_mix(n_iter_max=-1)
        for bad in (-1e-9, nan, inf):
            with pytest.raises(muxgl.MuxglError, match="tol"):
                e.demux_soup_mix(tol=bad)
        with pytest.raises(muxgl.MuxglError, match="every output is NULL"):
            e._check(e.lib.muxgl_demux_soup_mix(e.h, None, 0, None, None, 0, None, None, 3, 0.0, *([None] * 8)))
        m = np.ones(p.C, dtype=np.uint8)
        VP = ctypes.c_void_p
        pi = np.zeros(6)
        assert e.lib.muxgl_demux_soup_mix(e.h, m.ctypes.data_as(VP), keys.size, keys.ctypes.data_as(VP), counts.ctypes.data_as(VP), 0,
                                          None, None, 3, 0.0, pi.ctypes.data_as(VP), *([None] * 7)) != 0
        assert b"cell_mask must be NULL" in e.lib.muxgl_last_error(e.h)
        still_good()
        with pytest.raises(ValueError):
            e.demux_soup_mix(pi0=np.ones(5))
        assert e.demux_soup_mix(n_iter_max=2)["n_iter"] == 2               # and the call itself still runs


def test_the_call_changes_no_state():
    p = case(6, 3000, 200, 40)
    G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
    with muxgl.Engine(0) as e:
        load(e, p)
        r0 = e.demux_run(G6, 0.5)
        view, t0 = e.demux_results_view().tobytes(), e.timing().copy()
        a0 = e.demux_soup_mix(with_unknown=True, n_iter_max=6, tol=0.0)
        e.pileup_read_hist()
        assert e.demux_results_view().tobytes() == view and np.array_equal(e.timing(), t0)
        assert e.demux_entry_pg().size == p.nnz * len(G6) * 9             # the cached grid is still the run's
        r1 = e.demux_run(G6, 0.5)
        same(a0, e.demux_soup_mix(with_unknown=True, n_iter_max=6, tol=0.0), "after another run")
    assert r0.tobytes() == r1.tobytes() == view


# ---- 7. the feature does what it is for -----------------------------------------------------------------------------------

def test_the_device_recovers_the_planted_shares():
    """tests/test_soup_mix.py holds the restatement to the same checks on the same pileups"""
    p, mask, pool, w = sr.planted_pool(**sr.POOL)
    with muxgl.Engine(0) as e:
        load(e, p)
        got = e.demux_soup_mix(mask, n_iter_max=500, tol=1e-8)
        counts_profile = muxgl.ambient_profile(*e.pileup_allele_counts(mask), p.af)
        keys, counts = e.pileup_read_hist(mask)
    model = sr.Model(keys, counts, p.gp, p.has_gp, np.full(6, 1.0 / 6.0), dtype=np.float64)
    sr.check_planted(got, model, w, pool, counts_profile, "device")
    sm = muxgl.soup_mix_summary(got, names=[f"S{i}" for i in range(6)])
    assert sm["names"][0] == "S0" and sm["ll_gain"] > 0 and sm["max_grad_dev"] < 1e-3
    p, mask, pool, w = sr.planted_pool(**sr.POOL_OUTSIDE)
    gp0 = sr.hwe_prior(p.af)
    with muxgl.Engine(0) as e:
        load(e, p)
        got = e.demux_soup_mix(mask, with_unknown=True, gp0=gp0, n_iter_max=500, tol=1e-8)
        without = e.demux_soup_mix(mask, n_iter_max=500, tol=1e-8)
        counts_profile = muxgl.ambient_profile(*e.pileup_allele_counts(mask), p.af)
        keys, counts = e.pileup_read_hist(mask)
    model = sr.Model(keys, counts, p.gp, p.has_gp, np.full(7, 1.0 / 7.0), with_unknown=True, gp0=gp0, dtype=np.float64)
    z = sr.check_planted(got, model, w, pool, counts_profile, "device, outside donor")
    assert abs(z[-1]) <= 4.0
    assert np.any(np.abs(without["grad"][without["pi"] > 0] - 1.0) < 1e-6) and np.nanmax(without["ll"]) < np.nanmax(got["ll"]) - 2.0
