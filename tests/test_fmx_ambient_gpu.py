"""GPU tests of muxgl_fmx_ambient (fmx_ambient.hip): every droplet as one cell of cluster j plus a share rho of ambient
RNA -- ll_amb [C][K][n_rho] from the posteriors the last E-step read.

The yardstick is the numpy restatement of tests/fmx_ambient_ref.py with q from the oracle's run (cluster_posteriors of its
cluster pileups of that iteration); tests/test_fmx_ambient.py shows on the CPU that its nine likelihoods are the oracle's
bit for bit and that it holds the three identities of include/muxgl.h, identity 1 against the oracle's own E-step.  Bar:
parity.LL_TOL (1e-5 absolute) on every element; every test prints the worst deviation it saw.  Beside
that: the three identities on the device, bit-identity across calls, budgets, splits of the rhos, device groups, slabbed
ranks and the sharded driver, that the call changes nothing, its refusals, and pileups with a known soup share."""
import ctypes

import numpy as np
import pytest

import ambient_ref as ar
import fmx_ambient_ref as fr
import oracle_binding as ob
import parity
from popscle_amd import freemuxlet, muxgl, synth
from test_demux_gpu import _truncate_cells, _with_empty_cells
from test_fmx_singlets import cluster_posteriors
from test_fmx_singlets_gpu import _clust_buffer, _local_allgather, prepared, spread_init

pytestmark = pytest.mark.gpu

XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
DEFAULT_RHOS = fr.DEFAULT_RHOS
G16 = tuple(float(x) for x in np.round(np.linspace(0.0, 1.0, 16) ** 1.5, 6))   # 16 rhos, 0 and 1 among them
PART = 2048


def oracle_run(p, K, init, geno_error=0.1, max_iter=10, nthreads=16):
    """the oracle's EM from `init`: per iteration its records and counters, and for the iterations 1, 2 and the last the
    cluster pileups and records the iteration started from (what its posteriors are made of)"""
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
    return dict(n_iter=n, cells=recs, counters=cnt, eplp=e, before={it: before[it] for it in sorted({0, min(1, n - 1), n - 1})})


def assert_table(got, want, what="", tol=parity.LL_TOL):
    worst = parity.compare_singlet_table(got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1), tol)
    print(f"fmx ambient {what}: {got.shape}, max |dLL| = {worst:.3e}")
    return worst


def check_vs_restatement(p, K, init, f, rhos, geno_error=0.1, what="", flags=0, max_iter=10):
    """same init on both sides; after iterations 1, 2 and the last the assignments are equal (no cell is masked) and the
    table equals the restatement with the posteriors of the oracle's run"""
    ref = oracle_run(p, K, init, geno_error, max_iter)
    w, nine = fr.all_weights(p, f, rhos)
    assert nine.tobytes() == np.ascontiguousarray(ref["eplp"]["gls"]).tobytes()
    lens = np.diff(p.cell_ptr)
    worst = 0.0
    with prepared(p, 0, flags) as e:
        e.fmx_set_clusters(K, init)
        for it in range(ref["n_iter"]):
            cells, st = e.fmx_iterate(0.5, geno_error)
            if it not in ref["before"]:
                continue
            assert tuple(st) == tuple(ref["counters"][it]), (it, st, ref["counters"][it])
            assert np.array_equal(cells["clust"], ref["cells"][it]["clust"])   # zero cells left out
            got = e.fmx_ambient(f, rhos)
            want = fr.table_of_weights(p, cluster_posteriors(p.af, ref["before"][it][0], geno_error), w)
            assert got["ll"].shape == (p.C, K, len(rhos)) and not np.isnan(got["ll"]).any()
            worst = max(worst, assert_table(got["ll"], want, f"{what} K={K} NR={len(rhos)} ge={geno_error} flags={flags} iter {it + 1}"))
            assert np.all(got["ll"][lens == 0] == 0.0)
    return worst


def general_profile(S, seed, n_rho):
    """general f with exact 0 and 1 on a tenth of the markers each, and off-grid rhos"""
    f = ar.draw_af(S, seed)
    assert (f == 0.0).any() and (f == 1.0).any()
    return f, tuple(fr.draw_rhos(n_rho, seed + 1).tolist())


# ---- 1. against the restatement: every lane width, one, two and three cluster blocks, every chunking of the rhos -------------

NR_OF = {1: 16, 3: 8, 16: 3, 17: 1, 33: 16, 64: 8, 65: 3, 130: 16}


@pytest.mark.parametrize("geno_error", [0.1, 0.0])
@pytest.mark.parametrize("K", [1, 3, 16, 17, 33, 64, 65, 130])
def test_shapes_vs_restatement(K, geno_error):
    base = synth.make_pileup(40, 400, min(K, 12), seed=9000 + K, mean_entries=60, min_entries=10, reads_lambda=0.6,
                             doublet_frac=0.2, with_gp=False)
    p = _with_empty_cells(base, [1, 39])   # two empty droplets
    f, rhos = general_profile(p.S, K, NR_OF[K])
    check_vs_restatement(p, K, spread_init(p.C, K), f, rhos, geno_error, "shapes")   # one cluster without cells (K > 2)


@pytest.mark.parametrize("n_rho", [1, 2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("K", [5, 70])
def test_every_number_of_rhos(K, n_rho):
    p = synth.make_pileup(30, 400, 6, seed=9100 + K, mean_entries=60, min_entries=5, reads_lambda=1.5, with_gp=False)
    f, rhos = general_profile(p.S, 10 * K + n_rho, n_rho)
    check_vs_restatement(p, K, spread_init(p.C, K), f, rhos, 0.1, "rhos", max_iter=2)


@pytest.mark.parametrize("K,n_rho", [(6, 16), (6, 3), (70, 8), (70, 1)])
def test_ragged_cells_of_one_to_three_parts(K, n_rho):
    base = synth.make_pileup(12, 9000, 4, seed=9200, mean_entries=6000, sigma=0.1, min_entries=5500, max_entries=7000,
                             with_gp=False)
    keep = {c: 40 + 13 * c for c in range(12)}
    keep.update({0: 2100, 1: 4200, 2: 2048, 3: 2049, 4: 1, 5: 2, 6: 7})
    p = _with_empty_cells(_truncate_cells(base, keep), [7])
    lens = np.diff(p.cell_ptr)
    assert lens[0] == 2100 and lens[1] == 4200 and lens[7] == 0 and sorted(lens[4:7].tolist()) == [1, 2, 7]
    f, rhos = general_profile(p.S, K + n_rho, n_rho)
    check_vs_restatement(p, K, spread_init(p.C, K), f, rhos, 0.1, "ragged", max_iter=3)


@pytest.mark.parametrize("K", [256, 300])
def test_many_clusters_on_the_streamed_estep(K):
    p = synth.make_pileup(K + 20, 600, 24, seed=9300 + K, mean_entries=15, min_entries=5, max_entries=60,
                          reads_lambda=0.8, doublet_frac=0.25, with_gp=False)   # (the oracle's time goes with entries x K^2)
    init = ((K - 1 - np.arange(p.C) * 7) % K).astype(np.int32)
    f, rhos = general_profile(p.S, K, 8 if K == 256 else 3)
    check_vs_restatement(p, K, init, f, rhos, 0.1, "many clusters", max_iter=2)


def test_deep_entries_and_every_base_quality():
    """entries of up to ~60 reads, base qualities 0 .. 93, reads of neither allele: the per-read division by t"""
    p = synth.make_pileup(24, 300, 4, seed=9400, mean_entries=25, min_entries=4, reads_lambda=25.0, min_bq=0, max_bq=93,
                          cap_bq=127, other=0.03, with_gp=False)
    assert np.diff(p.entry_rptr).max() > 40 and (p.reads == synth.READ_OTHER).any()
    f, rhos = general_profile(p.S, 77, 8)
    check_vs_restatement(p, 4, spread_init(p.C, 4, False), f, rhos, 0.1, "deep", max_iter=2)


# ---- 2. the three identities on the device --------------------------------------------------------------------------------

def _small(K=5, seed=9500, C=40):
    p = _with_empty_cells(synth.make_pileup(C, 400, K, seed=seed, mean_entries=60, min_entries=10, reads_lambda=0.6,
                                            with_gp=False), [3])
    return p, spread_init(p.C, K, empty_cluster=False)


@pytest.mark.parametrize("K", [3, 20, 70])
def test_identity_1_against_the_oracles_extended_estep(K):
    p, init = _small(K, seed=9500 + K)
    assert p.af.min() > 0.0 and p.af.max() < 1.0
    f = fr.draw_onehot_af(p.S, seed=K)
    ref = oracle_run(p, K, init, 0.0, max_iter=3)
    with prepared(p) as e:
        e.fmx_set_clusters(K, init)
        for it in range(ref["n_iter"]):
            cells, _st = e.fmx_iterate(0.5, 0.0)
            if it not in ref["before"]:
                continue
            assert np.array_equal(cells["clust"], ref["cells"][it]["clust"])
            got = e.fmx_ambient(f, (0.2, 0.5))["ll"]
            want = fr.oracle_slots(p, ref["eplp"], K, *ref["before"][it], f, nthreads=16)
            assert_table(np.ascontiguousarray(got[:, :, 1]), want, f"identity 1 K={K} iter {it + 1}")


@pytest.mark.parametrize("K,devs", [(5, 0), (70, 0), (20, [0, 0])])
def test_identity_2_rho_zero_is_the_singlet_table_of_the_handle(K, devs):
    p, init = _small(K, seed=9600 + K)
    f, _ = general_profile(p.S, K, 1)
    with prepared(p, devs) as e:
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1)
        sng = e.fmx_singlets()
        got = e.fmx_ambient(f, (0.3, 0.0, 0.7, 0.0, 0.1))["ll"]
    for r in (1, 3):
        assert_table(np.ascontiguousarray(got[:, :, r]), sng, f"identity 2 K={K} devs={devs}")
    print(f"identity 2: bit-identical to muxgl_fmx_singlets: {got[:, :, 1].tobytes() == sng.tobytes()}")
    assert np.abs(got[:, :, 0] - sng).max() > 1e-3


def test_identity_3_rho_one_is_the_same_for_every_cluster():
    K = 70
    p, init = _small(K, seed=9700)
    f, _ = general_profile(p.S, 3, 1)
    with prepared(p) as e:
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1)
        got = e.fmx_ambient(f, (1.0, 0.4))["ll"]
    spread = float(np.abs(got[:, :, 0] - got[:, :1, 0]).max())
    print(f"identity 3: spread across {K} clusters at rho = 1: {spread:.3e}")
    # w_e[l] is one number w for every l at rho = 1, so a factor is w (q0 + q1 + q2): the row sums of q are 1 within a few
    # ulp, a log moves by a few 1e-16, and a droplet adds at most some thousand of them
    assert spread <= 1e-9
    assert np.abs(got[:, :, 1] - got[:, :1, 1]).max() > 1.0


# ---- 3. bit-identical -----------------------------------------------------------------------------------------------------

def _long_cells_pileup(seed, C=30):
    p = synth.make_pileup(C, 9000, 8, seed=seed, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000, with_gp=False)
    assert np.diff(p.cell_ptr).max() > PART
    return p


def _table(p, K, init, f, rhos, devs=0, flags=0, iters=2):
    with prepared(p, devs, flags) as e:
        e.fmx_set_clusters(K, init)
        for _ in range(iters):
            cells, st = e.fmx_iterate(0.5, 0.1)
        return e.fmx_ambient(f, rhos), cells, st


@pytest.mark.parametrize("K", [6, 48, 130])
def test_two_calls_and_every_split_of_the_rhos(K):
    p = _long_cells_pileup(9800 + K)
    f, _ = general_profile(p.S, K, 1)
    with prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K))
        e.fmx_iterate(0.5, 0.1)
        t0, (sum0, calls0) = e.timing().copy(), e.timing_sum()
        a = e.fmx_ambient(f, G16)
        assert a["kernel_ms"] > 0.0
        sum1, calls1 = e.timing_sum()
        assert np.array_equal(e.timing(), t0) and np.array_equal(sum1, sum0) and calls1 == calls0   # no slot, not collecting
        assert e.fmx_ambient(f, G16)["ll"].tobytes() == a["ll"].tobytes()
        halves = np.concatenate([e.fmx_ambient(f, G16[:8])["ll"], e.fmx_ambient(f, G16[8:])["ll"]], axis=2)
        assert halves.tobytes() == a["ll"].tobytes()
        ones = np.concatenate([e.fmx_ambient(f, G16[r:r + 1])["ll"] for r in range(16)], axis=2)
        assert ones.tobytes() == a["ll"].tobytes()
        odd = np.concatenate([e.fmx_ambient(f, G16[:3])["ll"], e.fmx_ambient(f, G16[3:10])["ll"],
                              e.fmx_ambient(f, G16[10:])["ll"]], axis=2)          # chunks of 3, of 4 + 3, of 3 + 3
        assert odd.tobytes() == a["ll"].tobytes()


def cell_bytes(p, n_rho, K):
    lens = np.diff(p.cell_ptr)
    parts = np.maximum(1, -(-lens // PART))
    row = 8 * n_rho * K
    return lens * n_rho * 24 + parts * (row + 24) + row + 16


def test_budget_does_not_matter(monkeypatch):
    K, rhos = 40, (0.0, 0.1, 0.2, 0.4)
    p = synth.make_pileup(200, 6000, 8, seed=9911, mean_entries=700, sigma=1.0, min_entries=1, max_entries=5000, with_gp=False)
    f, _ = general_profile(p.S, 2, 1)
    lens, need = np.diff(p.cell_ptr), cell_bytes(p, len(rhos), K)
    # several batches at 1 MB, cells in parts among them, and no cell that exceeds the budget on its own
    assert lens.max() > PART and need.max() <= (1 << 20) and need.sum() > 8 * (1 << 20)
    monkeypatch.delenv("MUXGL_FMX_SLAB_MB", raising=False)
    with prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K))
        e.fmx_iterate(0.5, 0.1)
        one = e.fmx_ambient(f, rhos)["ll"]
        monkeypatch.setenv("MUXGL_FMX_SLAB_MB", "1")
        many = e.fmx_ambient(f, rhos)["ll"]
        monkeypatch.delenv("MUXGL_FMX_SLAB_MB")
    assert one.tobytes() == many.tobytes()


@pytest.mark.parametrize("K", [20, 300])
def test_device_groups(K):
    p = _long_cells_pileup(10000 + K)
    init = spread_init(p.C, K)
    f, _ = general_profile(p.S, K, 1)
    want, cells, st = _table(p, K, init, f, DEFAULT_RHOS)
    for devs, flags in (([0, 0], 0), ([0, 0, 0], 0), ([0, 0], muxgl.FLAG_ASYNC_PHASES)):
        got, gcells, gst = _table(p, K, init, f, DEFAULT_RHOS, devs, flags)
        assert tuple(gst) == tuple(st) and got["kernel_ms"] > 0.0
        parity.same_records(gcells, cells)
        assert got["ll"].tobytes() == want["ll"].tobytes(), (devs, flags)


@pytest.mark.parametrize("K,world,flags", [(20, 2, 0), (300, 3, 0), (40, 2, muxgl.FLAG_ASYNC_PHASES)])
def test_slabbed_ranks_and_the_sharded_driver(K, world, flags):
    """every rank holds its two slabs (freemuxlet.load_rank) and sweeps its own cells; the exchanges of the driver are
    device copies between the handles here (as in test_fmx_unknown_gpu.py).  The ranks' tables, concatenated, are the
    one-handle table bit for bit; and run_em(want_ambient=...) returns it."""
    p = _long_cells_pileup(10100 + K, C=36)
    init = spread_init(p.C, K)
    f, _ = general_profile(p.S, K, 1)
    rhos = DEFAULT_RHOS[:5]
    want, cells, st = _table(p, K, init, f, rhos, iters=2)
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
    parts = [e.fmx_ambient(f, rhos)["ll"] for e in engs]
    for e in engs:
        e.close()
    assert np.concatenate(parts).tobytes() == want["ll"].tobytes()
    with prepared(p) as e:
        out, hist, amb = freemuxlet.run_em(e, K, init, max_iter=2, early_stop=False, want_ambient=(f, rhos))
    assert out.tobytes() == cells.tobytes() and amb.tobytes() == want["ll"].tobytes()
    with prepared(p) as e:
        out, hist, sng, amb = freemuxlet.run_em(e, K, init, max_iter=2, early_stop=False, want_singlets=True,
                                                want_ambient=(f, rhos))
    assert amb.tobytes() == want["ll"].tobytes() and sng.shape == (p.C, K)


# ---- 4. the call changes nothing ------------------------------------------------------------------------------------------

def test_records_tables_pileups_and_timing_slots_stay():
    K = 6
    p, init = _small(K, seed=10200, C=60)
    f, _ = general_profile(p.S, 5, 1)
    with prepared(p) as e:
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1)
        e.fmx_iter_gp(0.5, 0.1)
        e.fmx_iter_estep(0.5, 0.1)

        def state():
            cells, st, full = e.fmx_iter_fetch(want_full_ll=True)
            unk = e.fmx_unknown()
            return (cells.tobytes(), tuple(st), full.tobytes(), e.fmx_singlets().tobytes(),
                    tuple(unk[n].tobytes() for n in muxgl.FMX_UNKNOWN_FIELDS), tuple(x.tobytes() for x in e.fmx_cluster_pileup()),
                    _clust_buffer(e).tobytes())

        s0 = state()
        t0, (sum0, calls0) = e.timing().copy(), e.timing_sum()
        a = e.fmx_ambient(f, G16)["ll"]
        b = e.fmx_ambient(f, DEFAULT_RHOS)["ll"]
        sum1, calls1 = e.timing_sum()
        assert np.array_equal(e.timing(), t0) and np.array_equal(sum1, sum0) and calls1 == calls0   # every timing slot
        assert state() == s0
        e.fmx_iter_mstep()
        assert e.fmx_ambient(f, G16)["ll"].tobytes() == a.tobytes()              # behind the M-step: the same posteriors
        assert a.shape == (p.C, K, 16) and b.shape == (p.C, K, 8)


@pytest.mark.parametrize("K,devs,flags", [(6, 0, 0), (40, 0, 0), (40, 0, XE), (300, 0, 0), (24, [0, 0], 0), (40, [0, 0], XE)])
def test_the_call_leaves_the_em_alone(K, devs, flags):
    # few reads per droplet and fewer used clusters than K: near-tie cells, so the exact path's bookkeeping is in play
    p = synth.make_pileup(300, 500, 4, seed=10300 + K, mean_entries=10, min_entries=2, reads_lambda=0.3, with_gp=False)
    init = (np.arange(p.C) % 3).astype(np.int32)
    f, _ = general_profile(p.S, K, 1)

    def run(with_call):
        out = []
        with prepared(p, devs, flags) as e:
            e.fmx_set_clusters(K, init)
            for _ in range(4):
                cells, st = e.fmx_iterate(0.5, 0.1)   # the twin handle never makes the call
                if with_call:
                    sng, t0 = e.fmx_singlets(), e.timing().copy()
                    e.fmx_ambient(f, DEFAULT_RHOS)
                    e.fmx_ambient(f, (0.5,))
                    assert np.array_equal(e.timing(), t0)
                    assert e.fmx_singlets().tobytes() == sng.tobytes()   # the other table call, before and after
                    e.fmx_unknown()                                      # ... and the others may still run
                    e.fmx_inclusion(0.5)
                out.append((cells.tobytes(), tuple(st), tuple(x.tobytes() for x in e.fmx_cluster_pileup()), e.fmx_exact_stats()))
        return out

    a, b = run(False), run(True)
    assert a == b
    print(f"K={K} devs={devs} flags={flags}: near-tie cells settled = {a[-1][3][0]}")


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_refusals_leave_the_handle_usable(devs, monkeypatch):
    monkeypatch.delenv("MUXGL_FMX_SLAB_MB", raising=False)
    K = 5
    p = synth.make_pileup(6, 9000, K, seed=10400, mean_entries=5000, sigma=0.1, min_entries=4000, max_entries=8000, with_gp=False)
    assert cell_bytes(p, 16, K).max() > (1 << 20)
    init = spread_init(p.C, K, empty_cluster=False)
    f, _ = general_profile(p.S, 6, 1)
    VP = ctypes.c_void_p

    def fresh_table():
        with prepared(p, devs) as e:
            e.fmx_set_clusters(K, init)
            e.fmx_iterate(0.5, 0.1)
            return e.fmx_ambient(f, G16)["ll"]

    fresh = fresh_table()

    def raw(e, af, n_rho, rhos, out):
        rh = None if rhos is None else np.ascontiguousarray(rhos, dtype=np.float64)
        return e.lib.muxgl_fmx_ambient(e.h, None if af is None else af.ctypes.data_as(VP), n_rho,
                                       None if rh is None else rh.ctypes.data_as(VP),
                                       None if out is None else out.ctypes.data_as(VP), None)

    def bad_f(s, v):
        g = f.copy()
        g[s] = v
        g[min(s + 3, p.S - 1)] = v   # (the first offending marker is named)
        return g

    with muxgl.Engine(devs) as e:
        def refused(why):
            assert why in e.lib.muxgl_last_error(e.h), e.lib.muxgl_last_error(e.h)

        def still_good():
            assert e.fmx_ambient(f, G16)["ll"].tobytes() == fresh.tobytes()

        e.C, e.K, e.S = p.C, K, p.S   # (the binding sizes its outputs from these)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_ambient: no pileup"):
            e.fmx_ambient(f, G16)
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.K = K
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_ambient: call muxgl_fmx_prepare"):
            e.fmx_ambient(f, G16)
        e.fmx_prepare(p.af)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_ambient: .*E-step"):
            e.fmx_ambient(f, G16)
        e.fmx_set_clusters(K, init)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_ambient: no E-step since muxgl_fmx_set_clusters"):
            e.fmx_ambient(f, G16)
        e.fmx_iterate(0.5, 0.1)
        still_good()
        out = np.zeros((p.C, K, 17))
        assert raw(e, f, 16, G16, None) != 0
        refused(b"muxgl_fmx_ambient: NULL output")
        still_good()
        assert raw(e, None, 16, G16, out) != 0
        refused(b"muxgl_fmx_ambient: amb_af is NULL")
        still_good()
        assert raw(e, f, 16, None, out) != 0
        refused(b"muxgl_fmx_ambient: rho is NULL")
        still_good()
        for n_rho in (0, 17, -1):
            assert raw(e, f, n_rho, G16 + (0.5,), out) != 0
            refused(b"muxgl_fmx_ambient: n_rho=")
            still_good()
        for bad in (-0.01, 1.5, float("nan"), float("inf")):
            with pytest.raises(muxgl.MuxglError, match=r"muxgl_fmx_ambient: rho\[2\]"):
                e.fmx_ambient(f, (0.0, 0.1, bad, bad))
            still_good()
            for s in (0, 17, p.S - 1):
                with pytest.raises(muxgl.MuxglError, match=f"muxgl_fmx_ambient: amb_af of marker {s} "):
                    e.fmx_ambient(bad_f(s, bad), G16)
            still_good()
        monkeypatch.setenv("MUXGL_FMX_SLAB_MB", "1")
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_ambient: droplet .* exceeds the budget .*MUXGL_FMX_SLAB_MB"):
            e.fmx_ambient(f, G16)
        monkeypatch.delenv("MUXGL_FMX_SLAB_MB")
        still_good()
        with pytest.raises(ValueError):
            e.fmx_ambient(f[:-1], G16)
        if devs == 0:                    # (the phases run on a one-device handle)
            e.fmx_iter_gp(0.5, 0.1)      # the posteriors of the NEXT iteration
            with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_ambient: the cluster posteriors were rewritten"):
                e.fmx_ambient(f, G16)
        e.fmx_set_clusters(K, init)   # fresh clusters: the table of the old ones is gone
        with pytest.raises(muxgl.MuxglError, match="no E-step since muxgl_fmx_set_clusters"):
            e.fmx_ambient(f, G16)
        e.fmx_iterate(0.5, 0.1)
        still_good()


# ---- 6. the feature does what it is for -------------------------------------------------------------------------------------

@pytest.mark.parametrize("soup", [0.2, 0.0])
def test_the_device_finds_the_cluster_and_the_soup_share(soup):
    """tests/test_fmx_ambient.py holds the model itself (the restatement) to the same checks on the same pileups"""
    p, who, _pool = ar.soup_pileup(soup=soup, **fr.SOUP)
    K = fr.SOUP["V"]
    with prepared(p) as e:
        n_ref, n_alt = e.pileup_allele_counts()
        f = muxgl.ambient_profile(n_ref, n_alt, p.af)
        e.fmx_set_clusters(K, who.astype(np.int32))   # the clusters handed in from the truth, one iteration
        e.fmx_iterate(0.5, 0.1)
        got = e.fmx_ambient(f, DEFAULT_RHOS)["ll"]
    assert np.array_equal(n_ref, ar.allele_counts(p)[0]) and np.array_equal(n_alt, ar.allele_counts(p)[1])
    eplp = ob.fmx_entry_pileup(p)
    q = cluster_posteriors(p.af, ob.fmx_build_cluster_pileup(p, eplp, K, who.astype(np.int32)), 0.1)
    want = fr.table(p, q, f, DEFAULT_RHOS)
    assert_table(got, want, f"soup {soup}")
    sm, sw = fr.check_soup_calls(got, who, DEFAULT_RHOS, soup), freemuxlet.ambient_summary(want, DEFAULT_RHOS)
    for k in ("amb_clust", "amb_rho_idx", "base_clust", "amb_sample", "base_sample"):   # every integer field
        assert np.array_equal(sm[k], sw[k]), k
