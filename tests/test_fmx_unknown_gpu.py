"""GPU tests of muxgl_fmx_unknown (fmx_unknown.hip): every droplet against a donor that no cluster holds -- ll_ju [C][K],
ll_u [C], ll_uu [C] from the posteriors the last E-step read.

The yardstick is the oracle's one E-step on its own cluster pileups of that iteration with two EMPTY pileups appended
(tests/fmx_unknown_ref.py; tests/test_fmx_unknown.py shows on the CPU that this leaves the K-cluster triangle alone and
holds the three formulas of include/muxgl.h in the slots (K, j), (K, K), (K + 1, K), for the oracle and the reference).
Bar: parity.LL_TOL (1e-5 absolute) on every element of every table; every test prints the worst deviation it saw
(DESIGN.md 4.2g).  Beside that: a caller's prior, bit-identity across calls, budgets, subsets of outputs, device groups,
slabbed ranks and the sharded driver, that the call changes nothing, its refusals, and an end-to-end pool with a donor
no cluster was given to.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fmx_unknown_ref as fur
import oracle_binding as ob
import parity
from popscle_amd import freemuxlet, muxgl, synth
from test_demux_gpu import _truncate_cells, _with_empty_cells
from test_fmx_singlets import cluster_posteriors
from test_fmx_singlets_gpu import _clust_buffer, _local_allgather, prepared, spread_init

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
FIELDS = muxgl.FMX_UNKNOWN_FIELDS


def oracle_run(p, K, init, geno_error=0.1, max_iter=10, nthreads=16):
    """the oracle's EM from `init`; per iteration its records and counters, and for the iterations 1, 2 and the last the
    three tables of its E-step on the pileups of that iteration with two empty ones appended"""
    e = ob.fmx_entry_pileup(p)
    cplp = ob.fmx_build_cluster_pileup(p, e, K, init)
    cells = ob.fmx_init_cells(init)
    before, recs, cnt = [], [], []
    for _ in range(max_iter):
        before.append((cplp.copy(), cells.copy()))
        ns, na, nch = ob.fmx_iterate(p, e, K, cplp, cells, 0.5, geno_error, nthreads=nthreads)
        recs.append(cells.copy())
        cnt.append((ns, na, nch))
        if nch == 0:
            break
    n = len(recs)
    tables = {it: fur.oracle_tables(p, e, K, before[it][0], before[it][1], geno_error, nthreads=nthreads)
              for it in sorted({0, min(1, n - 1), n - 1})}
    return dict(n_iter=n, cells=recs, counters=cnt, tables=tables, eplp=e)


def assert_tables(got, want, what=""):
    """got: the dict of Engine.fmx_unknown; want: (ll_ju, ll_u, ll_uu)"""
    worst = 0.0
    for name, w in zip(FIELDS, want):
        worst = max(worst, parity.compare_singlet_table(got[name], w, parity.LL_TOL))
    print(f"fmx unknown {what}: {want[0].shape[0]} x {want[0].shape[1]}, max |dLL| = {worst:.3e}")
    return worst


def check_vs_oracle(p, K, init, geno_error=0.1, what="", flags=0, max_iter=10, empty_cluster=None):
    """same init on both sides; after iterations 1, 2 and the last the assignments are equal (no cell is masked) and the
    three tables equal the oracle's.  empty_cluster: a cluster without cells in `init` -- in iteration 1 its column of
    ll_ju is ll_uu and its singlet column is ll_u"""
    ref = oracle_run(p, K, init, geno_error, max_iter)
    lens = np.diff(p.cell_ptr)
    worst = 0.0
    with prepared(p, 0, flags) as e:
        e.fmx_set_clusters(K, init)
        for it in range(ref["n_iter"]):
            cells, st = e.fmx_iterate(0.5, geno_error)
            if it not in ref["tables"]:
                continue
            assert tuple(st) == tuple(ref["counters"][it]), (it, st, ref["counters"][it])
            assert np.array_equal(cells["clust"], ref["cells"][it]["clust"])   # zero cells left out
            got = e.fmx_unknown()
            worst = max(worst, assert_tables(got, ref["tables"][it], f"{what} K={K} ge={geno_error} flags={flags} iter {it + 1}"))
            for name in FIELDS:
                assert np.all(got[name][lens == 0] == 0.0), name
            if it == 0 and empty_cluster is not None:
                tol = parity.LL_TOL
                assert np.all(parity._close(got["ll_ju"][:, empty_cluster], got["ll_uu"], tol))
                assert np.all(parity._close(e.fmx_singlets()[:, empty_cluster], got["ll_u"], tol))
    return worst


# ---- 1. against the oracle: every lane width, one, two and three cluster blocks ------------------------------------------

@pytest.mark.parametrize("geno_error", [0.1, 0.0])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8, 16, 17, 32, 33, 64, 65, 130])
def test_shapes_vs_oracle(K, geno_error):
    base = synth.make_pileup(40, 500, min(K, 12), seed=7000 + K, mean_entries=100, min_entries=10, reads_lambda=0.6,
                             doublet_frac=0.2, with_gp=False)
    p = _with_empty_cells(base, [1, 39])   # two empty droplets
    init = spread_init(p.C, K)             # one empty cluster (K > 2)
    check_vs_oracle(p, K, init, geno_error, "shapes", empty_cluster=K - 1 if K > 2 else None)


@pytest.mark.parametrize("K", [6, 70])
def test_cells_of_two_and_three_parts(K):
    base = synth.make_pileup(12, 9000, 4, seed=7200, mean_entries=6000, sigma=0.1, min_entries=5500, max_entries=7000,
                             with_gp=False)
    keep = {c: 40 + 13 * c for c in range(12)}
    keep.update({0: 2100, 1: 4200, 2: 2048, 3: 2049, 4: 1})
    p = _with_empty_cells(_truncate_cells(base, keep), [7])
    lens = np.diff(p.cell_ptr)
    assert lens[0] == 2100 and lens[1] == 4200 and lens[7] == 0
    check_vs_oracle(p, K, spread_init(p.C, K, empty_cluster=False), 0.1, "long cells", max_iter=3)


@pytest.mark.parametrize("K", [256, 300])
def test_many_clusters_on_the_streamed_estep(K):
    p = synth.make_pileup(K + 20, 600, 24, seed=7300 + K, mean_entries=15, min_entries=5, max_entries=60,
                          reads_lambda=0.8, doublet_frac=0.25, with_gp=False)   # (the oracle's time goes with entries x K^2)
    init = ((K - 1 - np.arange(p.C) * 7) % K).astype(np.int32)
    check_vs_oracle(p, K, init, 0.1, "many clusters", max_iter=2)


@pytest.mark.parametrize("K,flags", [
    (16, 0), (16, muxgl.FLAG_FORCE_ROW_KERNEL), (16, muxgl.FLAG_FORCE_TILE_SWEEP), (16, muxgl.FLAG_NO_LINEAR_ENTRIES),
    (16, muxgl.FLAG_NO_PIVOT_SUMS), (40, 0), (40, muxgl.FLAG_FORCE_WAVE_KERNEL), (40, muxgl.FLAG_FORCE_TILE_SWEEP),
    (40, XE), (40, muxgl.FLAG_NO_LINEAR_ENTRIES)])
def test_every_estep_path(K, flags):
    p = synth.make_pileup(48, 800, 8, seed=7400 + K, mean_entries=100, min_entries=10, reads_lambda=0.6, doublet_frac=0.2,
                          with_gp=False)
    check_vs_oracle(p, K, spread_init(p.C, K), 0.1, "paths", flags=flags, max_iter=3)


# ---- 2. a caller's prior ------------------------------------------------------------------------------------------------

def _small(K=5, seed=7500, C=40):
    p = _with_empty_cells(synth.make_pileup(C, 500, K, seed=seed, mean_entries=100, min_entries=10, reads_lambda=0.6,
                                            with_gp=False), [3])
    return p, spread_init(p.C, K, empty_cluster=False)


@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_hardy_weinberg_prior_is_the_null_call_bit_for_bit(devs):
    p, init = _small()
    with prepared(p, devs) as e:
        e.fmx_set_clusters(5, init)
        e.fmx_iterate(0.5, 0.1)
        a = e.fmx_unknown()
        b = e.fmx_unknown(gp0=fur.hardy_weinberg(p.af))
    for name in FIELDS:
        assert a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize("geno_error", [0.1, 0.0])
def test_one_hot_prior_against_the_restatement(geno_error):
    """a specific donor's genotypes.  At geno_error = 0 posterior entries may be exactly 0: -inf equals -inf, never NaN"""
    K = 5
    p, init = _small(K)
    e0 = ob.fmx_entry_pileup(p)
    q = cluster_posteriors(p.af, ob.fmx_build_cluster_pileup(p, e0, K, init), geno_error)
    u = np.ascontiguousarray(np.eye(3)[(np.arange(p.S) * 5 + 1) % 3])
    want = fur.unknown_tables(p, e0["gls"], q, u)
    with prepared(p) as e:
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, geno_error)
        got = e.fmx_unknown(gp0=u)
    for name in FIELDS:
        assert not np.isnan(got[name]).any(), name
    assert_tables(got, want, f"one-hot prior ge={geno_error}")


@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_bad_prior_rows_are_refused_by_marker(devs):
    p, init = _small()
    hw = fur.hardy_weinberg(p.af)
    with prepared(p, devs) as e:
        e.fmx_set_clusters(5, init)
        e.fmx_iterate(0.5, 0.1)
        first = e.fmx_unknown()
        for s, row in ((17, [0.5, 0.6, -0.1]), (0, [0.3, 0.3, 0.3]), (p.S - 1, [np.nan, 0.5, 0.5]), (5, [1.0, 1e-5, 0.0])):
            bad = hw.copy()
            bad[s] = row
            bad[min(s + 3, p.S - 1)] = row   # (the first offending marker is named)
            with pytest.raises(muxgl.MuxglError, match=rf"muxgl_fmx_unknown: gp0 row of marker {s} "):
                e.fmx_unknown(gp0=bad)
        ok = hw.copy()
        ok[5] = [1.0 - 5e-7, 2e-7, 0.0]      # within 1e-6 of 1
        e.fmx_unknown(gp0=ok)
        again = e.fmx_unknown()              # the handle is still usable
    for name in FIELDS:
        assert again[name].tobytes() == first[name].tobytes()


# ---- 3. bit-identical ---------------------------------------------------------------------------------------------------

def _long_cells_pileup(seed, C=30):
    p = synth.make_pileup(C, 9000, 8, seed=seed, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000, with_gp=False)
    assert np.diff(p.cell_ptr).max() > 2048
    return p


def _tables(p, K, init, devs=0, flags=0, iters=2):
    with prepared(p, devs, flags) as e:
        e.fmx_set_clusters(K, init)
        for _ in range(iters):
            cells, st = e.fmx_iterate(0.5, 0.1)
        return e.fmx_unknown(), cells, st


def _same(a, b, what=""):
    for name in FIELDS:
        assert a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), (name, what)


def test_two_calls_and_every_subset_of_outputs():
    p = _long_cells_pileup(7600)
    K = 48
    with prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K))
        e.fmx_iterate(0.5, 0.1)
        t0, (sum0, calls0) = e.timing(), e.timing_sum()
        a = e.fmx_unknown()
        assert a["kernel_ms"] > 0.0
        sum1, calls1 = e.timing_sum()
        assert np.array_equal(e.timing(), t0) and np.array_equal(sum1, sum0) and calls1 == calls0   # no slot, not collecting
        _same(a, e.fmx_unknown(), "second call")
        for mask in range(1, 7):
            want = tuple(n for i, n in enumerate(FIELDS) if mask >> i & 1)
            got = e.fmx_unknown(want=want)
            assert set(got) == set(want) | {"kernel_ms"}
            for n in want:
                assert got[n].tobytes() == a[n].tobytes(), (want, n)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from popscle_amd import muxgl, synth
K = 70
p = synth.make_pileup(400, 6000, 12, seed=7611, mean_entries=150, sigma=1.2, min_entries=1, max_entries=5000,
                      reads_lambda=0.5, with_gp=False)
lens = np.diff(p.cell_ptr)
assert lens.max() > 2048 and 40 * int(lens.sum()) > 3 * (1 << 20)   # several batches at 1 MB, cells in parts among them
with muxgl.Engine(0) as e:
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.fmx_prepare(p.af)
    e.fmx_set_clusters(K, ((np.arange(p.C) * 7) % K).astype(np.int32))
    e.fmx_iterate(0.5, 0.1)
    t = e.fmx_unknown()
    np.savez(sys.argv[2], **{n: t[n] for n in muxgl.FMX_UNKNOWN_FIELDS})
"""


def test_budget_does_not_matter(tmp_path):
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
    assert outs[0]["ll_ju"].shape == (400, 70)
    _same(outs[0], outs[1], "1 MB")


def test_a_droplet_over_the_budget_is_refused_and_the_handle_stays_usable(monkeypatch):
    """one droplet with an entry at each of 27 000 markers beside two short ones: at K = 2 its weights alone
    (40 bytes an entry) exceed a budget of 1 MB, whatever the batches"""
    n = 27000
    rng = np.random.default_rng(7650)
    lens = np.array([5, n, 300])
    snp = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens]).astype(np.int32)
    reads = ((rng.integers(0, 2, snp.size) << 7) | rng.integers(13, 21, snp.size)).astype(np.uint8)   # one read an entry
    cell_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    p = synth.Pileup(3, n, cell_ptr, snp, np.arange(snp.size + 1, dtype=np.int64), reads, rng.uniform(0.05, 0.95, n))
    assert 40 * n > (1 << 20)
    monkeypatch.delenv("MUXGL_FMX_SLAB_MB", raising=False)
    with prepared(p) as e:
        e.fmx_set_clusters(2, np.array([0, 1, 0], dtype=np.int32))
        e.fmx_iterate(0.5, 0.1)
        monkeypatch.setenv("MUXGL_FMX_SLAB_MB", "1")
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_unknown: droplet .* exceeds the budget .*MUXGL_FMX_SLAB_MB"):
            e.fmx_unknown()
        monkeypatch.delenv("MUXGL_FMX_SLAB_MB")
        t = e.fmx_unknown()   # the same handle, at the default budget
        assert all(t[name].shape[0] == 3 and np.isfinite(t[name]).all() for name in FIELDS)


@pytest.mark.parametrize("K", [20, 300])
def test_device_groups(K):
    p = _long_cells_pileup(7701 + K)
    init = spread_init(p.C, K)
    want, cells, st = _tables(p, K, init)
    for devs, flags in (([0, 0], 0), ([0, 0, 0], 0), ([0, 0], muxgl.FLAG_ASYNC_PHASES), ([0, 0, 0], muxgl.FLAG_ASYNC_PHASES)):
        got, gcells, gst = _tables(p, K, init, devs, flags)
        assert tuple(gst) == tuple(st)
        parity.same_records(gcells, cells)
        _same(got, want, (devs, flags))


@pytest.mark.parametrize("K,world,flags", [(20, 2, 0), (300, 3, 0), (40, 2, muxgl.FLAG_ASYNC_PHASES)])
def test_slabbed_ranks_and_the_sharded_driver(K, world, flags):
    """every rank holds its two slabs (freemuxlet.load_rank) and sweeps its own cells; the exchanges of the driver are
    device copies between the handles here (as in test_fmx_singlets_gpu.py).  The ranks' tables, concatenated, are the
    one-handle tables bit for bit; and run_em(want_unknown=True) returns them."""
    p = _long_cells_pileup(7800 + K, C=36)
    init = spread_init(p.C, K)
    want, cells, st = _tables(p, K, init, iters=2)
    (c_ranges, per_c), (s_ranges, per_s) = freemuxlet.plan_ranges(p.C, p.S, world)
    import torch

    def drain():
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
    parts = [e.fmx_unknown() for e in engs]
    for e in engs:
        e.close()
    _same({n: np.concatenate([t[n] for t in parts]) for n in FIELDS}, want, "ranks")
    with prepared(p) as e:
        out, hist, unk = freemuxlet.run_em(e, K, init, max_iter=2, early_stop=False, want_unknown=True)
    assert out.tobytes() == cells.tobytes() and set(unk) == set(FIELDS)
    _same(unk, want, "run_em")


# ---- 4. the call changes nothing ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,flags", [(6, 0), (24, 0), (40, 0), (40, XE), (300, 0)])
def test_the_call_leaves_the_em_alone(K, flags):
    # few reads per droplet and fewer used clusters than K: near-tie cells, so the exact path's bookkeeping is in play
    p = synth.make_pileup(300, 500, 4, seed=7900 + K, mean_entries=10, min_entries=2, reads_lambda=0.3, with_gp=False)
    init = (np.arange(p.C) % 3).astype(np.int32)

    def run(with_call):
        out = []
        with prepared(p, 0, flags) as e:
            e.fmx_set_clusters(K, init)
            for _ in range(4):
                cells, st = e.fmx_iterate(0.5, 0.1)
                sng = None
                if with_call:
                    sng = e.fmx_singlets()
                    e.fmx_unknown()
                    e.fmx_unknown(gp0=fur.hardy_weinberg(p.af), want=("ll_u",))
                    assert e.fmx_singlets().tobytes() == sng.tobytes()   # the other table call, before and after
                    e.fmx_inclusion(0.5)                                  # ... and it may still run
                out.append((cells.tobytes(), tuple(st), _clust_buffer(e).tobytes(),
                            tuple(x.tobytes() for x in e.fmx_cluster_pileup()), e.fmx_exact_stats()))
        return out

    a, b = run(False), run(True)
    assert a == b
    print(f"K={K} flags={flags}: near-tie cells settled = {a[-1][4][0]}")


# ---- 5. refusals --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals_leave_the_handle_usable(devs):
    K = 5
    p = synth.make_pileup(24, 300, K, seed=1, mean_entries=40, min_entries=5, with_gp=False)
    init = spread_init(p.C, K, empty_cluster=False)
    with muxgl.Engine(devs) as e:
        e.C, e.K, e.S = p.C, K, p.S   # (the binding sizes its outputs from these)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_unknown: no pileup"):
            e.fmx_unknown()
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.K = K
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_unknown: call muxgl_fmx_prepare"):
            e.fmx_unknown()
        e.fmx_prepare(p.af)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_unknown: .*E-step"):
            e.fmx_unknown()
        e.fmx_set_clusters(K, init)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_unknown: no E-step since muxgl_fmx_set_clusters"):
            e.fmx_unknown()
        e.fmx_iterate(0.5, 0.1)
        first = e.fmx_unknown()
        assert e.lib.muxgl_fmx_unknown(e.h, None, None, None, None, None) != 0
        assert b"muxgl_fmx_unknown: all three outputs are NULL" in e.lib.muxgl_last_error(e.h)
        _same(e.fmx_unknown(), first, "after all-NULL")
        e.fmx_set_clusters(K, init)   # fresh clusters: the tables of the old ones are gone
        with pytest.raises(muxgl.MuxglError, match="no E-step since muxgl_fmx_set_clusters"):
            e.fmx_unknown()
        e.fmx_iterate(0.5, 0.1)
        _same(e.fmx_unknown(), first, "the same start again")
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)   # a new pileup: nothing is prepared
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_unknown: "):
            e.fmx_unknown()
        e.fmx_prepare(p.af)
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1)
        again = e.fmx_unknown()
        _same(again, first, "after the refusals")
        assert_tables(again, oracle_run(p, K, init, max_iter=1)["tables"][0], "after the refusals")


def test_posterior_phase_without_its_estep_is_refused():
    K = 4
    p = synth.make_pileup(24, 300, K, seed=2, mean_entries=40, min_entries=5, with_gp=False)
    with prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K, False))
        e.fmx_iter_gp(0.5, 0.1)
        e.fmx_iter_estep(0.5, 0.1)
        a = e.fmx_unknown()          # after the E-step, before the M-step
        e.fmx_iter_mstep()
        _same(e.fmx_unknown(), a, "behind the M-step")
        e.fmx_iter_gp(0.5, 0.1)      # the posteriors of the NEXT iteration
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_unknown: the cluster posteriors were rewritten"):
            e.fmx_unknown()
        e.fmx_iter_estep(0.5, 0.1)
        b = e.fmx_unknown()
        assert not np.array_equal(a["ll_ju"], b["ll_ju"])
        assert a["ll_u"].tobytes() == b["ll_u"].tobytes() and a["ll_uu"].tobytes() == b["ll_uu"].tobytes()   # (no q in them)


# ---- 6. end to end: a donor no cluster was given to ---------------------------------------------------------------------

def test_third_donor_without_a_cluster():
    """three donors pooled, clusters handed in for two of them, the third donor's cells left at -1"""
    V, K = 3, 2
    p = synth.make_pileup(90, 1500, V, seed=8100, mean_entries=250, min_entries=60, reads_lambda=0.6, doublet_frac=0.0)
    donor = ob.demux(p, alphas=(0.0,), nthreads=4)["sBest"]       # who each droplet is, from the donors' genotypes
    assert np.bincount(donor, minlength=V).min() >= 10
    init = np.where(donor < K, donor, -1).astype(np.int32)
    ref = oracle_run(p, K, init, 0.1)
    n = ref["n_iter"]
    want = freemuxlet.unknown_summary(dict(zip(FIELDS, ref["tables"][n - 1])), ref["cells"][n - 1]["bestLLK"])
    with prepared(p) as e:
        out, hist, unk = freemuxlet.run_em(e, K, init, max_iter=n, want_unknown=True)
    assert len(hist) == n
    got = freemuxlet.unknown_summary(unk, out["bestLLK"])
    sure = np.abs(want["diff"]) > 1e-6
    assert np.array_equal(np.sign(got["diff"][sure]), np.sign(want["diff"][sure]))
    assert np.abs(got["diff"] - want["diff"]).max() <= 2 * parity.LL_TOL
    away = np.abs(want["diff"] + 2.0) > 1e-4                       # (no droplet sits on the margin)
    assert away.all() and got["n_better"] == want["n_better"]
    third = donor == 2
    print(f"third donor: {int((got['diff'][third] < -2).sum())} of {int(third.sum())} droplets better explained by an "
          f"unknown donor; {int((got['diff'][~third] < -2).sum())} of the others; oracle count {want['n_better']}")
    assert (want["diff"][third] < -2).sum() > third.sum() // 2      # the premise of the case, on the oracle's numbers
