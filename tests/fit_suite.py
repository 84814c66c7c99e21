"""The test bodies that tests/test_demux_ambient_fit_gpu.py, test_demux_alpha_fit_gpu.py, test_fmx_ambient_fit_gpu.py and
test_fmx_alpha_fit_gpu.py share, as plain functions of the call's description (fit_check.Call) and an input case.  Each
test keeps its name, its parameters and its inputs in its own module; what is asserted of all four calls alike stands here.

pre: what the Engine method takes before the slots -- (alphas, f), (alphas,), (f,) or (), by Call.grid and Call.amb_af.
make(devs=0, flags=0): the module's way to a handle that is ready for the call (demuxlet: pileup and GP tensor loaded;
freemuxlet: prepared, clusters set, the E-steps of the case run), a context manager."""
import ctypes

import numpy as np

import parity
from fit_check import check_fit
from popscle_amd import freemuxlet, muxgl
from test_fmx_singlets_gpu import _clust_buffer, _local_allgather, prepared


def run(call, e, pre, slots, *x_max, **kw):
    return getattr(e, call.method)(*pre, slots, *x_max, **kw)


def same(call, a, b, fields=None):
    return all(a[k].tobytes() == b[k].tobytes() for k in (call.fields if fields is None else fields))


def demux_load(e, p):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)


def demux_open(p, devs=0, flags=0):
    e = muxgl.Engine(devs, flags)
    demux_load(e, p)
    return e


def demux_fit(call, p, pre, slots, x_max, flags=0, devs=0, want=None):
    with demux_open(p, devs, flags) as e:
        return run(call, e, pre, slots, x_max, want=call.fields if want is None else want)


def fmx_iterated(p, K, init, devs=0, flags=0, cells=None):
    """a prepared handle after two iterations from the clusters `init`; cells: the records they must have given"""
    e = prepared(p, devs, flags)
    e.fmx_set_clusters(K, init)
    for _ in range(2):
        got, _st = e.fmx_iterate(0.5, 0.1)
    if cells is not None:
        parity.same_records(got, cells)
    return e


def empty_pileup(e, p):
    e.set_pileup(p.S, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8))


# ---- sixteen slots, zero cells ---------------------------------------------------------------------------------------------

def sixteen_slots(call, case, slots, x_max, got, what):
    """every bar on all sixteen slots; slot 3 repeats slot 0 and slot 7 is skipped"""
    check_fit(call, case, slots, x_max, got, what, ll_tol=parity.LL_TOL)
    assert all(got[k][:, 3].tobytes() == got[k][:, 0].tobytes() for k in call.fields)
    assert (got["status"][:, 7] == 4).all()


def zero_cells(call, e, pre):
    """C == 0 on a handle that is otherwise ready: the call succeeds and writes nothing (host_run returns before it
    allocates, copies or launches where C * n_cand == 0), through Python and with a canary behind the C function"""
    got = run(call, e, pre, np.zeros((0, 2, 2)[:call.width + 1], np.int32))
    assert got[call.hat].shape == (0, 2) and got["kernel_ms"] == 0.0
    canary = np.full(4, 7.0)
    rc, why = raw(call, e, None, np.zeros(2 * call.width, np.int32), 0.5, af=pre[-1] if call.amb_af else None,
                  bufs=[canary] + [None] * (len(call.fields) - 1))
    assert rc == 0 and (canary == 7.0).all(), why


def fmx_zero_cells(call, p, K, pre):
    with muxgl.Engine(0) as e:
        empty_pileup(e, p)
        e.fmx_prepare(p.af)
        e.fmx_set_clusters(K, np.zeros(0, np.int32))
        e.fmx_iterate(0.5, 0.1)
        zero_cells(call, e, pre)


# ---- bit identity ----------------------------------------------------------------------------------------------------------

def identity(call, e, pre, slots, want):
    """on one handle: call to call, a column permutation, split 8 + 8, every slot twice, subsets of outputs"""
    x, F = call.x_identity, call.fields
    go = lambda s, **kw: run(call, e, pre, np.ascontiguousarray(s), x, **kw)
    assert (want["status"] == 0).any() and (want["status"] == 4).any() and slots.shape[1] == 16
    assert same(call, go(slots), want) and same(call, go(slots), want)
    perm = np.random.default_rng(1).permutation(16)
    assert same(call, go(slots[:, perm]), {k: np.ascontiguousarray(want[k][:, perm]) for k in F})
    lo, hi = go(slots[:, :8]), go(slots[:, 8:])
    assert same(call, {k: np.concatenate([lo[k], hi[k]], axis=1) for k in F}, want)
    twice = go(np.repeat(slots[:, :8], 2, axis=1))
    assert same(call, {k: np.ascontiguousarray(twice[k][:, ::2]) for k in F}, lo)
    assert same(call, {k: np.ascontiguousarray(twice[k][:, 1::2]) for k in F}, lo)
    for sub in call.subsets:
        got = go(slots, want=sub)
        assert set(got) == set(sub) | {"kernel_ms"} | set(call.extra) and same(call, got, want, sub)


def device_groups(call, make, pre, slots, want, flags=0):
    for devs in ([0, 0], [0, 0, 0]):
        with make(devs, flags) as e:
            got = run(call, e, pre, slots, call.x_identity)
        assert same(call, got, want) and got["kernel_ms"] > 0.0, devs


def fmx_slabbed_ranks(call, p, K, world, flags, init, pre, slots, want):
    """every rank holds its two slabs (freemuxlet.load_rank) and fits its own cells after two iterations; the exchanges of
    the driver are device copies between the handles here (as in test_fmx_ambient_gpu.py).  The ranks' outputs,
    concatenated, are the one-handle outputs bit for bit"""
    import torch

    (c_ranges, per_c), (s_ranges, per_s) = freemuxlet.plan_ranges(p.C, p.S, world)
    engs = [muxgl.Engine(0, flags) for _ in range(world)]
    for r, e in enumerate(engs):
        freemuxlet.load_rank(e, p, c_ranges[r], s_ranges[r])
        e.fmx_set_clusters(K, init)
    for it in range(2):
        for e in engs:
            e.fmx_iter_gp(0.5, 0.1)
        torch.cuda.synchronize()
        _local_allgather(engs, muxgl.BUF_CGP, per_s, p.S, K * 3 * 8)
        torch.cuda.synchronize()
        for e in engs:
            e.fmx_iter_estep(0.5, 0.1)
        for e in engs:
            e.fmx_iter_fetch()
        if sum(e.fmx_exact_pending() for e in engs) > 0:
            freemuxlet.settle_near_ties(engs, lambda obj: [obj], 0.5, 0.1)
        torch.cuda.synchronize()
        _local_allgather(engs, muxgl.BUF_CLUST, per_c, p.C, 4)
        torch.cuda.synchronize()
        for e in engs:
            e.fmx_iter_mstep()
    parts = [run(call, e, pre, np.ascontiguousarray(slots[c_ranges[r][0]:c_ranges[r][1]]), call.x_identity) for r, e in enumerate(engs)]
    for e in engs:
        e.close()
    assert same(call, {k: np.concatenate([x[k] for x in parts]) for k in call.fields}, want)


# ---- state -----------------------------------------------------------------------------------------------------------------

def demux_state_alone(call, p, flags, slots, pre_run, pre_other, x_max, G6):
    """the call between two demuxlet runs: records, full LL, timing slots and the cached grid stay the run's"""
    with demux_open(p, 0, flags) as e:
        full = flags == 0                                    # (the streamed call keeps no LL tensor)
        go = lambda: e.demux_run(G6, 0.5, want_full_ll=True) if full else (e.demux_run(G6, 0.5), np.zeros(0))
        r0, full0 = go()
        view, t0, pg0 = e.demux_results_view().tobytes(), e.timing().copy(), e.demux_entry_pg().tobytes()
        a0 = run(call, e, pre_run, slots, x_max)
        assert e.demux_results_view().tobytes() == view and np.array_equal(e.timing(), t0)
        run(call, e, pre_other, slots, 0.25)                 # another grid between two runs
        assert e.demux_results_view().tobytes() == view and np.array_equal(e.timing(), t0)
        assert e.demux_entry_pg().tobytes() == pg0           # the cached grid is still the run's
        r1, full1 = go()
        a1 = run(call, e, pre_run, slots, x_max)
    assert r0.tobytes() == r1.tobytes() == view and full0.tobytes() == full1.tobytes() and same(call, a0, a1)


def fmx_state_stays(call, p, K, who, anchored, pre, slots, x_max, tables):
    """between the E-step and the M-step of an iteration: records, the full LL, the table calls (tables(e): the module's
    own beside the singlet and unknown-donor tables), pileups, posteriors, assignments and every timing slot stay"""
    with prepared(p) as e:
        if anchored:
            e.demux_set_gp(p.gp, p.has_gp)
        e.fmx_set_clusters(K, who)
        if anchored:
            e.fmx_set_anchors([0, 1, 2], None if anchored == "held" else [muxgl.ANCHOR_PRIOR, muxgl.ANCHOR_HELD, muxgl.ANCHOR_PRIOR])
        e.fmx_iterate(0.5, 0.1)
        e.fmx_iter_gp(0.5, 0.1)
        e.fmx_iter_estep(0.5, 0.1)

        def state():
            cells, st, full = e.fmx_iter_fetch(want_full_ll=True)
            unk = e.fmx_unknown()
            return (cells.tobytes(), tuple(st), full.tobytes(), e.fmx_singlets().tobytes(), tables(e),
                    tuple(unk[n].tobytes() for n in muxgl.FMX_UNKNOWN_FIELDS), tuple(x.tobytes() for x in e.fmx_cluster_pileup()),
                    e.fmx_cluster_gp().tobytes(), _clust_buffer(e).tobytes())

        s0 = state()
        t0, (sum0, calls0) = e.timing().copy(), e.timing_sum()
        a = run(call, e, pre, slots, x_max)
        run(call, e, pre, slots[:, :1], 0.25)
        sum1, calls1 = e.timing_sum()
        assert np.array_equal(e.timing(), t0) and np.array_equal(sum1, sum0) and calls1 == calls0   # every timing slot
        assert state() == s0
        e.fmx_iter_mstep()
        assert same(call, run(call, e, pre, slots, x_max), a)             # behind the M-step: the same posteriors
        assert (a["status"] == 0).any()


def fmx_em_alone(call, p, K, devs, flags, init, pre, slots, x_max):
    """four iterations with the call after each, and on a twin handle that never makes it: the same EM"""
    def go(with_call):
        out = []
        with prepared(p, devs, flags) as e:
            e.fmx_set_clusters(K, init)
            for _ in range(4):
                cells, st = e.fmx_iterate(0.5, 0.1)
                if with_call:
                    sng, t0 = e.fmx_singlets(), e.timing().copy()
                    run(call, e, pre, slots, x_max)
                    assert np.array_equal(e.timing(), t0)
                    assert e.fmx_singlets().tobytes() == sng.tobytes()   # the other table calls, before and after
                    e.fmx_unknown()
                    e.fmx_inclusion(0.5)
                out.append((cells.tobytes(), tuple(st), tuple(x.tobytes() for x in e.fmx_cluster_pileup()), e.fmx_exact_stats()))
        return out

    assert go(False) == go(True)


# ---- refusals --------------------------------------------------------------------------------------------------------------

def raw(call, e, shape, slots, x_max, af=None, n_alpha=2, n_cand=2, outs=True, bufs=None):
    """the C function behind the call: handle, the grid (demuxlet), amb_af (the ambient fits), n_cand, the slots, x_max, the
    four or five double rows, status, n_steps, kernel_ms.  Returns (rc, the handle's last error)"""
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    first = []
    if call.grid:
        dp = muxgl._DemuxParams()
        dp.n_alpha = n_alpha
        dp.alpha[1] = 0.5
        dp.doublet_prior = 0.5
        first.append(ctypes.byref(dp))
    if call.amb_af:
        first.append(ptr(af))
    if bufs is None:
        bufs = [np.zeros(shape) for _ in call.fields[:-2]] + [np.zeros(shape, np.int32) for _ in range(2)]
    rc = getattr(e.lib, "muxgl_" + call.method)(e.h, *first, n_cand, ptr(slots), ctypes.c_double(x_max),
                                                 *[ptr(b) if outs else None for b in bufs], None)
    return rc, e.lib.muxgl_last_error(e.h)


def refusal_frame(call, e, pre, slots, x_max, fresh, named):
    """(refused, still_good) for a handle e: refused(word, **kw) makes the raw call with the good arguments but kw and
    expects a failure whose message holds word (named: and starts with the function's name); still_good() expects the good
    call through Python to return `fresh` bit for bit"""
    good = dict(slots=slots, x_max=x_max, af=pre[-1] if call.amb_af else None)

    def refused(word, **kw):
        rc, why = raw(call, e, slots.shape[:2], **{**good, **kw})
        assert rc != 0 and word in why and (not named or why.startswith(b"muxgl_%s: " % call.method.encode())), (kw, why)

    def still_good():
        assert same(call, run(call, e, pre, slots, x_max), fresh)

    return refused, still_good


def common_refusals(call, refused, still_good, slots, n_index):
    """what every fit call refuses alike: no output, no slots, no profile, a bad n_cand, a bad x_max, an index out of
    [-1, n_index) -- the handle stays usable after each"""
    refused(b"every output is NULL", outs=False)
    still_good()
    refused(b"%s is NULL" % call.slot_name.encode(), slots=None)
    if call.amb_af:
        refused(b"amb_af is NULL", af=None)
    still_good()
    for n_cand in (0, 17, -1):
        refused(b"n_cand", n_cand=n_cand)
    still_good()
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        refused(call.x_name.encode(), x_max=bad)
    still_good()
    for bad in (-2, n_index, 1 << 20):
        for t in range(call.width):
            s2 = slots.copy()
            s2.reshape(slots.shape[0], slots.shape[1], -1)[2, 1, t] = bad
            refused(f"{call.slot_name}[2][1]{f'[{t}]' if call.width == 2 else ''}".encode(), slots=s2)
        still_good()
