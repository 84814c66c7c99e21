"""GPU tests of muxgl_fmx_inclusion (fmx_incl.hip): per droplet and cluster the evidence that the cluster is in the droplet
and the cluster it pairs best with, as the last E-step formed the pair triangle -- against `restate_fmx`
(tests/test_fmx_inclusion.py) of the reference's full_ll of the same iteration (its own loop where oracle/_ref is built,
else the oracle), against full_ll and the records of the same handle on the E-step paths that have it, exact ties across
blocks, bit for bit across calls, budgets, device groups and slabbed ranks, that the call changes nothing, its refusals,
and `popscle-amd freemuxlet --write-inclusion`.

Bar: parity.LL_TOL (1e-5 absolute) on every element of incl, tot and dbl.  `partner`: the reference's value of the named
hypothesis lies within LL_TOL of the reference's maximum over H_s, and where the reference's best and runner-up are more
than 2e-5 apart it is the reference's.  No cell or cluster is masked out.  The streamed-path fuzz cases are held to the
fuzz's own TABLE_TOL (1e-7).  Every test prints the worst deviation it saw.
"""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
import ref_binding as rb
from popscle_amd import freemuxlet, muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup
from test_demux_gpu import _truncate_cells, _with_empty_cells
from test_fmx_inclusion import SLAB1_KS, reference_run, restate_fmx
from test_fmx_singlets_gpu import _clust_buffer, _local_allgather, _long_cells_pileup, _read, prepared, spread_init

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
TOL = parity.LL_TOL
FIELDS = ("incl", "tot", "dbl", "partner")


def pair_value(full, s, partner):
    hi, lo = np.maximum(s, partner), np.minimum(s, partner)
    return full[np.arange(full.shape[0]), hi * (hi + 1) // 2 + lo]


def compare_tables(got, full, want, what, tol=TOL):
    """the four tables against want = restate_fmx(full, ...): incl, tot, dbl within tol on every element; partner names
    a hypothesis at the reference's maximum (within tol) and is the reference's where the gap exceeds 2e-5"""
    worst = {}
    for k in ("incl", "tot", "dbl"):
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, k
        assert not np.isnan(got[k]).any(), k
        with np.errstate(invalid="ignore"):
            d = np.abs(got[k] - want[k])
        d = d[np.isfinite(d)]   # (-inf on both sides is equal below)
        worst[k] = float(d.max()) if d.size else 0.0
    print(f"fmx inclusion {what}: max |d incl| = {worst['incl']:.3e}, |d tot| = {worst['tot']:.3e}, |d dbl| = {worst['dbl']:.3e}")
    for k in ("incl", "tot", "dbl"):
        assert np.all(parity._close(got[k], want[k], tol)), (k, worst[k])
    none = want["partner"] < 0
    assert got["partner"].dtype == np.int32 and np.array_equal(got["partner"] < 0, none)
    decided = 0
    for s in range(want["incl"].shape[1]):
        m = ~none[:, s]
        if not m.any():
            continue
        assert np.all(got["partner"][m, s] != s)
        v = pair_value(full, s, np.where(m, got["partner"][:, s], 0))
        assert np.all(np.abs(v - want["dbl"][:, s])[m] <= tol), s
        clear = m & (want["gap"][:, s] > 2e-5)
        decided += int(clear.sum())
        assert np.array_equal(got["partner"][clear, s], want["partner"][clear, s]), s
    worst["decided"] = decided
    return worst


def check_vs_reference(p, K, init, geno_error=0.1, dp=0.5, flags=0, what="", tol=TOL):
    """same init on both sides; after iterations 1 and 2: the assignments are equal (no cell is masked) and the tables
    equal restate_fmx of the reference's full_ll of that iteration"""
    ref = reference_run(p, K, init, geno_error, dp)
    n = ref["n_iter"]
    worst = {}
    with prepared(p, 0, flags) as e:
        e.fmx_set_clusters(K, init)
        for it in range(min(n, 2)):
            cells, st = e.fmx_iterate(dp, geno_error)
            assert tuple(st) == tuple(ref["counters"][it]), (it, st, ref["counters"][it])
            parity.compare_fmx(cells, ref["cells"][it], resolved=True)
            assert np.array_equal(cells["clust"], ref["cells"][it]["clust"])   # zero cells left out
            got = e.fmx_inclusion(dp)
            w = compare_tables(got, ref["full"][it], restate_fmx(ref["full"][it], K, dp),
                               f"{what} K={K} ge={geno_error} dp={dp} flags={flags} iter {it + 1}/{n}", tol)
            worst = {k: max(v, worst.get(k, 0)) for k, v in w.items()}
    return worst


# ---- 1. against the reference ------------------------------------------------------------------------------------------

def _random_pileup(K, seed_base=7000):
    C = 48 if K <= 33 else (24 if K < 256 else 16)
    base = synth.make_pileup(C, 1200 if K < 64 else 2000, min(K, 12), seed=seed_base + K, mean_entries=60, min_entries=15,
                             reads_lambda=0.6, doublet_frac=0.25, with_gp=False)
    return _with_empty_cells(base, [1, C - 1])   # empty droplets among the others


@pytest.mark.parametrize("dp", [0.5, 0.1])
@pytest.mark.parametrize("geno_error", [0.1, 0.0])
@pytest.mark.parametrize("K", [1, 2, 3, 16, 17, 33, 64, 65, 130, 200, 256, 300])
def test_random_vs_reference(K, geno_error, dp):
    p = _random_pileup(K)
    check_vs_reference(p, K, spread_init(p.C, K), geno_error, dp, 0, "random")   # (spread_init: a cluster without cells)


@pytest.mark.parametrize("K", [33, 65, 130, 200])
def test_forced_streamed_estep_vs_reference(K):
    p = _random_pileup(K, 7400)
    check_vs_reference(p, K, spread_init(p.C, K), 0.1, 0.5, XE, "forced stream")


@pytest.mark.parametrize("K", [5, 70])
def test_long_short_and_empty_cells(K):
    base = synth.make_pileup(20, 9000, min(K, 10), seed=7500 + K, mean_entries=500, sigma=1.2, min_entries=1,
                             max_entries=6000, with_gp=False)
    p = _with_empty_cells(_truncate_cells(base, {3: 1, 11: 2}), [0, 7, 19])
    lens = np.diff(p.cell_ptr)
    assert (lens == 0).sum() == 3 and lens.max() > 2048
    check_vs_reference(p, K, spread_init(p.C, K), 0.1, 0.5, 0, "ragged")


def test_a_cluster_without_cells_and_cells_without_a_cluster():
    K = 20
    p = _random_pileup(K, 7600)
    init = spread_init(p.C, K)
    init[init == 3] = -1          # cells that start without a cluster; clusters 3 and K - 1 start without cells
    assert not np.any(init == K - 1) and not np.any(init == 3)
    check_vs_reference(p, K, init, 0.1, 0.5, 0, "empty cluster")


# ---- 2. against the handle's own full_ll and records ---------------------------------------------------------------------

@pytest.mark.parametrize("K,flags", [
    (8, 0), (8, muxgl.FLAG_FORCE_ROW_KERNEL), (16, muxgl.FLAG_FORCE_TILE_SWEEP), (24, 0),
    (24, muxgl.FLAG_FORCE_WAVE_KERNEL), (24, muxgl.FLAG_FORCE_TILE_SWEEP), (40, 0), (40, muxgl.FLAG_NO_LINEAR_ENTRIES),
    (40, muxgl.FLAG_NO_PIVOT_SUMS), (100, 0)])
def test_consistent_with_the_handles_own_numbers(K, flags):
    dp = 0.3
    p = synth.make_pileup(40, 2000, min(K, 16), seed=7700 + K, mean_entries=100, min_entries=20, max_entries=3000,
                          reads_lambda=0.6, doublet_frac=0.2, with_gp=False)
    with prepared(p, 0, flags) as e:
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        e.fmx_set_clusters(K, e.fmx_greedy_init(K, llk2 - llk0))
        for it in range(2):
            cells, _, full = e.fmx_iterate(dp, 0.1, want_full_ll=True)
            got = e.fmx_inclusion(dp)
            compare_tables(got, full, restate_fmx(full, K, dp), f"own full_ll K={K} flags={flags} iter {it + 1}")
            d1 = np.abs(got["dbl"].max(axis=1) - cells["dblBestLLK"])
            d2 = np.abs(got["tot"] - cells["sumLLK"])
            print(f"K={K} flags={flags}: max |max dbl - dblBestLLK| = {d1.max():.3e}, |tot - sumLLK| = {d2.max():.3e}")
            assert np.all(d1 <= TOL) and np.all(d2 <= TOL)


# ---- 3. exact ties: empty droplets among normal ones ---------------------------------------------------------------------

@pytest.mark.parametrize("slab_mb", [None, "1"])
@pytest.mark.parametrize("K", SLAB1_KS)
def test_ties_of_empty_droplets(K, slab_mb):
    from test_fuzz_gpu import slab_env

    assert tuple(SLAB1_KS) == (65, 130, 300)
    C = 64
    base = synth.make_pileup(C, 800, 8, seed=7800 + K, mean_entries=60, min_entries=15, with_gp=False)
    empty = [0, 5, 31, 32, C - 1]
    p = _with_empty_cells(base, empty)
    with slab_env("MUXGL_FMX_SLAB_MB", slab_mb), prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K))
        e.fmx_iterate(0.5, 0.1)
        got = e.fmx_inclusion(0.5)
    # every LL of an empty droplet is exactly 0: the earliest position wins, across blocks, roles and rotations
    assert np.all(got["dbl"][empty] == 0.0)
    assert np.all(got["partner"][empty, 0] == 1) and np.all(got["partner"][empty, 1:] == 0)
    assert np.all(np.abs(got["tot"][empty]) <= 1e-12), np.abs(got["tot"][empty]).max()
    for k in FIELDS:
        for c in empty[1:]:
            assert got[k][c].tobytes() == got[k][empty[0]].tobytes(), (k, c)
    others = np.setdiff1d(np.arange(C), empty)
    assert np.all(got["dbl"][others] < 0.0)
    # sum_s exp(incl - tot) = 1 + P(doublet), on the flat rows: P(doublet) = doublet_prior exactly
    assert np.allclose(np.exp(got["incl"][empty] - got["tot"][empty][:, None]).sum(axis=1), 1.5, rtol=0, atol=1e-9)


# ---- 4. bit-identical ----------------------------------------------------------------------------------------------------

def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in FIELDS)


def _tables(p, K, init, devs=0, flags=0, iters=2):
    with prepared(p, devs, flags) as e:
        e.fmx_set_clusters(K, init)
        for _ in range(iters):
            cells, st = e.fmx_iterate(0.5, 0.1)
        return e.fmx_inclusion(0.5), cells, st


def test_two_calls_on_one_handle_and_null_outputs():
    p = _long_cells_pileup(8100, C=24)
    K = 70
    with prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K))
        e.fmx_iterate(0.5, 0.1)
        a = e.fmx_inclusion(0.5)
        t = e.timing()
        assert t[muxgl.T_FMX_INCLUSION] > 0.0 and t[muxgl.T_FMX_ESTEP] > 0.0   # the iteration's slots keep their values
        b = e.fmx_inclusion(0.5)
        assert _same(a, b)
        for k in FIELDS:   # any subset of the outputs
            one = e.fmx_inclusion(0.5, want=(k,))
            assert list(one) == [k] and one[k].tobytes() == a[k].tobytes()
        p_ = muxgl._FmxParams(0.5, 0.1)
        import ctypes
        assert e.lib.muxgl_fmx_inclusion(e.h, ctypes.byref(p_), None, None, None, None) == 0   # nothing to write


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from popscle_amd import muxgl, synth
K = 300
p = synth.make_pileup(64, 9000, 8, seed=8211, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000, with_gp=False)
assert np.diff(p.cell_ptr).max() > 2048
with muxgl.Engine(0) as e:
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.fmx_prepare(p.af)
    e.fmx_set_clusters(K, ((np.arange(p.C) * 7) % K).astype(np.int32))
    e.fmx_iterate(0.5, 0.1)
    r = e.fmx_inclusion(0.5)
    np.savez(sys.argv[2], **r)
"""


def test_budget_does_not_matter(tmp_path):
    """64 cells at K = 300 under 1 MB: four batches of 21 cells, one block of the fifteen at a time"""
    outs = []
    for mb in (0, 1):
        env = dict(os.environ)
        env.pop("MUXGL_FMX_SLAB_MB", None)
        if mb:
            env["MUXGL_FMX_SLAB_MB"] = str(mb)
        out = str(tmp_path / f"mb{mb}.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(dict(np.load(out)))
    assert outs[0]["incl"].shape == (64, 300) and _same(outs[0], outs[1])


@pytest.mark.parametrize("K", [20, 300])
def test_device_groups(K):
    p = _long_cells_pileup(8200 + K, C=24)
    init = spread_init(p.C, K)
    want, cells, st = _tables(p, K, init)
    for devs, flags in (([0, 0], 0), ([0, 0, 0], 0), ([0, 0], muxgl.FLAG_ASYNC_PHASES), ([0, 0, 0], muxgl.FLAG_ASYNC_PHASES)):
        got, gcells, gst = _tables(p, K, init, devs, flags)
        assert tuple(gst) == tuple(st)
        parity.same_records(gcells, cells)
        assert _same(got, want), (devs, flags)


@pytest.mark.parametrize("K,world,flags", [(20, 2, 0), (300, 3, 0), (70, 2, muxgl.FLAG_ASYNC_PHASES)])
def test_slabbed_ranks_and_the_sharded_driver(K, world, flags):
    """every rank holds its two slabs (freemuxlet.load_rank) and folds its own cells; the ranks' tables, concatenated, are
    the one-handle tables bit for bit; and run_em(want_inclusion=True) returns them"""
    p = _long_cells_pileup(8310 + K, C=24)   # (seeds whose 24 cells hold one beyond 2 048 entries)
    init = spread_init(p.C, K)
    want, cells, st = _tables(p, K, init, iters=2)
    (c_ranges, per_c), (s_ranges, per_s) = freemuxlet.plan_ranges(p.C, p.S, world)
    import torch

    def drain():   # (the copies below cross the handles' streams; under MUXGL_FLAG_ASYNC_PHASES nothing else waits)
        torch.cuda.synchronize()

    engs = [muxgl.Engine(0, flags) for _ in range(world)]
    for r, e in enumerate(engs):
        freemuxlet.load_rank(e, p, c_ranges[r], s_ranges[r])
        e.fmx_set_clusters(K, init)
    for it in range(2):
        for e in engs:
            e.fmx_iter_gp(0.5, 0.1)
        drain()
        _local_allgather(engs, muxgl.BUF_CGP, per_s, p.S, K * 3 * 8)
        drain()
        for e in engs:
            e.fmx_iter_estep(0.5, 0.1)
        for e in engs:
            e.fmx_iter_fetch()
        if sum(e.fmx_exact_pending() for e in engs) > 0:
            freemuxlet.settle_near_ties(engs, lambda obj: [obj], 0.5, 0.1)
        drain()
        _local_allgather(engs, muxgl.BUF_CLUST, per_c, p.C, 4)
        drain()
        for e in engs:
            e.fmx_iter_mstep()
    parts = [e.fmx_inclusion(0.5) for e in engs]
    recs = np.concatenate([e.fmx_iter_fetch()[0] for e in engs])
    for e in engs:
        e.close()
    parity.same_records(recs, cells)
    got = {k: np.concatenate([x[k] for x in parts]) for k in FIELDS}
    assert _same(got, want)
    with prepared(p) as e:
        out, hist, sng, inc = freemuxlet.run_em(e, K, init, max_iter=2, early_stop=False, want_singlets=True,
                                                want_inclusion=True)
        assert sng.shape == (p.C, K)
    with prepared(p) as e:
        out2, hist2, inc2 = freemuxlet.run_em(e, K, init, max_iter=2, early_stop=False, want_inclusion=True)
    assert out.tobytes() == cells.tobytes() and out2.tobytes() == cells.tobytes()
    assert _same(inc, want) and _same(inc2, want)


# ---- 5. the call changes nothing -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,flags", [(6, 0), (24, 0), (40, XE), (300, 0)])
def test_the_call_leaves_the_em_alone(K, flags):
    # few reads per droplet and fewer used clusters than K: near-tie cells, so the exact path's bookkeeping is in play
    p = synth.make_pileup(200, 500, 4, seed=7900 + K, mean_entries=10, min_entries=2, reads_lambda=0.3, with_gp=False)
    init = (np.arange(p.C) % 3).astype(np.int32)

    def run(with_call):
        out = []
        with prepared(p, 0, flags) as e:
            e.fmx_set_clusters(K, init)
            for _ in range(4):
                cells, st = e.fmx_iterate(0.5, 0.1)
                if with_call:
                    e.fmx_inclusion(0.5)
                    e.fmx_inclusion(0.2)
                out.append((cells.tobytes(), tuple(st), _clust_buffer(e).tobytes(),
                            tuple(x.tobytes() for x in e.fmx_cluster_pileup()), e.fmx_exact_stats()))
        return out

    a, b = run(False), run(True)
    assert a == b
    print(f"K={K} flags={flags}: near-tie cells settled = {a[-1][4][0]}")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals(devs):
    import ctypes

    K = 5
    p = synth.make_pileup(24, 300, K, seed=1, mean_entries=40, min_entries=5, with_gp=False)
    init = spread_init(p.C, K, empty_cluster=False)
    with muxgl.Engine(devs) as e:
        e.C, e.K = p.C, K   # (the binding sizes its output from these)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_inclusion: no pileup"):
            e.fmx_inclusion()
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.K = K
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_inclusion: call muxgl_fmx_prepare"):
            e.fmx_inclusion()
        e.fmx_prepare(p.af)
        with pytest.raises(muxgl.MuxglError, match="E-step"):
            e.fmx_inclusion()
        e.fmx_set_clusters(K, init)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_inclusion: no E-step since muxgl_fmx_set_clusters"):
            e.fmx_inclusion()
        e.fmx_iterate(0.5, 0.1)
        first = e.fmx_inclusion()
        buf = np.zeros((p.C, K))
        assert e.lib.muxgl_fmx_inclusion(e.h, None, muxgl._ptr(buf), None, None, None) != 0
        assert b"muxgl_fmx_inclusion" in e.lib.muxgl_last_error(e.h) and b"NULL" in e.lib.muxgl_last_error(e.h)
        assert not buf.any()
        pp = muxgl._FmxParams(0.5, 0.1)
        assert e.lib.muxgl_fmx_inclusion(e.h, ctypes.byref(pp), None, None, None, None) == 0
        again = e.fmx_inclusion()   # the handle is still usable
        assert _same(first, again)
        e.fmx_set_clusters(K, init)   # fresh clusters: the tables of the old ones are gone
        with pytest.raises(muxgl.MuxglError, match="no E-step since muxgl_fmx_set_clusters"):
            e.fmx_inclusion()
        e.fmx_iterate(0.5, 0.1)
        assert _same(first, e.fmx_inclusion())   # the same start gives the same tables
        ref = reference_run(p, K, init)
        compare_tables(first, ref["full"][0], restate_fmx(ref["full"][0], K, 0.5), "after the refusals")


def test_posterior_phase_without_its_estep_is_refused():
    K = 4
    p = synth.make_pileup(24, 300, K, seed=2, mean_entries=40, min_entries=5, with_gp=False)
    with prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K, False))
        e.fmx_iter_gp(0.5, 0.1)
        e.fmx_iter_estep(0.5, 0.1)
        e.fmx_iter_mstep()
        a = e.fmx_inclusion()
        e.fmx_iter_gp(0.5, 0.1)   # the posteriors of the NEXT iteration: the tables of the last E-step are gone
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_inclusion: the cluster posteriors were rewritten"):
            e.fmx_inclusion()
        e.fmx_iter_estep(0.5, 0.1)
        b = e.fmx_inclusion()
        assert a["incl"].shape == b["incl"].shape == (p.C, K) and not np.array_equal(a["incl"], b["incl"])


# ---- 7. front end --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,devices", [(4, None), (300, None), (4, "0,0")])
def test_freemuxlet_cli_write_inclusion(tmp_path, K, devices):
    import pyplp

    if K == 300:
        p = synth.make_pileup(24, 1200, 24, seed=18, mean_entries=80, min_entries=20, max_entries=300, reads_lambda=0.8,
                              with_gp=False)
    else:
        p = synth.make_pileup(80, 1200, K, seed=18, mean_entries=150, min_entries=30, with_gp=False)
    prefix = str(tmp_path / "plp")
    plpio.write_plp(prefix, p, seed=18)
    d = pyplp.load(prefix)
    q = as_pileup(d)
    init = spread_init(q.C, K)
    initf = str(tmp_path / "init.txt")
    with open(initf, "w") as f:
        for i, bc in enumerate(d["bcs"]):
            f.write(f"{bc}\t{int(init[i])}\n")
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = [BIN, "freemuxlet", "--plp", prefix, "--nsample", str(K), "--init-cluster", initf] + \
           (["--devices", devices] if devices else [])
    for cmd in (base + ["--out", plain], base + ["--out", out, "--write-inclusion"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
    assert not os.path.exists(plain + ".clust1.incl.gz")
    for suffix in (".lmix", ".clust1.samples.gz", ".clust1.vcf.gz"):   # every other output: byte-equal
        assert _read(out + suffix) == _read(plain + suffix), suffix

    # the engine's tables of the last iteration, from the same start
    with prepared(q) as e:
        e.fmx_set_clusters(K, init)
        for _ in range(10):
            _, st = e.fmx_iterate(0.5, 0.1)
            if st[2] == 0:
                break
        want = e.fmx_inclusion(0.5)
    post = np.exp(want["incl"] - want["tot"][:, None])
    with gzip.open(out + ".clust1.samples.gz", "rt") as f:
        srows = [ln.rstrip("\n").split("\t") for ln in f.readlines()[1:]]
    lines = gzip.open(out + ".clust1.incl.gz", "rt").read().splitlines()
    assert lines[0] == "BARCODE\tCLUST\tNUM.SNPS\tNUM.READS\tLLK.INCL\tPOSTPRB.INCL\tDBL.PARTNER\tDBL.LLK"
    assert len(srows) == q.C and len(lines) == 1 + q.C * K
    worst = 0.0
    for i, srow in enumerate(srows):       # droplets in the order of .clust1.samples.gz
        assert srow[1] == d["bcs"][i]
        for j in range(K):                 # clusters 0 .. K-1
            f = lines[1 + i * K + j].split("\t")
            assert len(f) == 8 and f[:4] == [srow[1], str(j), srow[2], srow[3]], (f, srow[:4])
            worst = max(worst, abs(float(f[4]) - want["incl"][i, j]))
            assert abs(float(f[4]) - want["incl"][i, j]) <= 5e-5, (f, want["incl"][i, j])
            assert abs(float(f[5]) - post[i, j]) <= max(6e-3 * post[i, j], 1e-300), (f, post[i, j])
            if want["partner"][i, j] < 0:
                assert f[6:] == ["NA", "NA"]
            else:
                assert "NA" not in f[6:] and int(f[6]) == want["partner"][i, j]
                assert abs(float(f[7]) - want["dbl"][i, j]) <= 5e-5, (f, want["dbl"][i, j])
    print(f"CLI K={K} devices={devices}: max |LLK.INCL - engine| = {worst:.3e}")


# ---- 8. the streamed-path fuzz cases, at the fuzz's own bar ----------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5])
def test_fuzz_cases_of_the_streamed_estep(seed):
    """the freemuxlet cases of tests/test_fuzz_gpu.py's streamed-path fuzz (hard pileups, K = 33 .. 320, the sweep's four
    flag combinations), on one handle from the reference's own start: the four tables against restate_fmx of the
    reference's full_ll at TABLE_TOL = 1e-7.  Observed on the device: see DESIGN.md 4.2d."""
    import test_fuzz_gpu as fz

    if not rb.available():
        pytest.skip("reference library not built")
    info, p = fz.stream_fmx_case(seed)
    K, dp, ge = info["K"], info["dp"], info["ge"]
    ref = fz.fmx_reference(info, p)
    tol = fz.TABLE_TOL["incl"]
    assert tol == 1e-7 and fz.TABLE_TOL["tot"] == tol and fz.TABLE_TOL["dbl"] == tol
    step = max(1, int(fz.RESTATE_BYTES // (8 * K * K)))
    with fz.slab_env("MUXGL_FMX_SLAB_MB", info["run_slab"]), prepared(p, 0, info["flags"]) as e:
        e.fmx_set_clusters(K, ref["clust0"] if info["init"] is None else info["init"])
        worst = {}
        for it in range(min(2, ref["n_iter"])):
            cells, st = e.fmx_iterate(dp, ge)
            fz._check_iteration(it, ref, cells, st, K)
            assert np.array_equal(cells["clust"], ref["cells"][it]["clust"])
            got = e.fmx_inclusion(dp)
            full = ref["full_ll"][it]
            for c0 in range(0, p.C, step):
                sl = slice(c0, c0 + step)
                w = compare_tables({k: got[k][sl] for k in FIELDS}, full[sl], restate_fmx(full[sl], K, dp),
                                   f"fuzz seed {seed} K={K} cells {c0}.. iter {it + 1}", tol)
                worst = {k: max(v, worst.get(k, 0)) for k, v in w.items()}
    print(f"fuzz seed {seed}: K={K} C={p.C} flags={info['flags']} slab={info['run_slab']}: worst {worst}")
