"""Host-side driver of the freemuxlet EM loop -- the sequential control flow of cmdCramFreemux2
(cmd_cram_freemux2.cpp:373-605) around the libmuxgl phases, for one GPU or for one process per GPU.

Multi-GPU scheme (exact).  Rank r holds two slabs of the packed pileup, 2/N of it in all:
its ROW slab (cells c_ranges[r], every SNP: E-step, scans, re-assignment) and its COLUMN slab (every cell, SNPs
s_ranges[r]: cluster pileups, cluster-GP rows, ordered M-step).  Per iteration:

    iter_gp     -> all-gather of the cluster-GP rows   f64[S][K][3]   (38 MB at config 3, 768 MB at config 4)
    iter_estep  -> all-gather of the assignments       i32[C]         + all-reduce of (nsingle, namb, nchanged)
    iter_mstep

Each exchange is ONE collective (all_gather_into_tensor, in place on the library's own device buffer: the ranges are
equal slices and the buffers carry a little slack).  Over RCCL (backend "nccl") nothing on the host waits between the
phases: the library enqueues on its own stream (MUXGL_FLAG_ASYNC_PHASES), that stream is torch's current stream while
the collectives are issued, and ProcessGroupNCCL orders its communication stream against it with events; the host
blocks once per iteration, on the three reduced counters the reference's early stop reads (:601-604), while the M-step
is already running.  An all-reduce of sufficient statistics would NOT reproduce the reference: merge() clamps after
every cell (sc_drop_seq.h:92-100), so the chain per (cluster, SNP) is evaluated by exactly one rank, in ascending cell id.
"""
from __future__ import annotations

import contextlib
import time

import numpy as np

from . import shard
from .muxgl import alpha_fit_summary as muxgl_alpha_fit_summary
from .muxgl import ambient_fit_summary as muxgl_ambient_fit_summary
from .muxgl import ambient_summary as muxgl_ambient_summary

UNIT_CGP, UNIT_CLUST, UNIT_STAT = 0, 1, 2


class TorchExchange:
    """Collectives over torch.distributed on tensors that alias the engine's exchange buffers.

    device_ordered=True (RCCL): the collectives are enqueued behind the engine's stream and nothing waits on the host.
    device_ordered=False (gloo staging, tests on a 1-GPU box or on CPU): every exchange returns when the data has landed."""

    def __init__(self, dist_module, rank: int, world: int, device_ordered: bool = False, always: bool = False):
        self.dist = dist_module
        self.rank = rank
        self.world = world
        self.device_ordered = device_ordered
        self.always = always  # take the exchange path even with one rank

    def allgather_equal(self, tensor, per: int):
        """tensor: [>= world*per, row]; rank r owns rows [r*per, (r+1)*per).  One collective, in place."""
        if per <= 0:
            return
        if self.world * per > tensor.shape[0]:  # slices of ceil(n / world) units overrun the buffer's XCHG_PAD slack
            raise ValueError(f"in-place all-gather of {self.world} x {per} rows needs {self.world * per} rows, the exchange "
                             f"buffer has {tensor.shape[0]} (slack of muxgl.XCHG_PAD = 64 units: at most 65 ranks)")
        out = tensor[: self.world * per]
        inp = tensor[self.rank * per:(self.rank + 1) * per]
        self.dist.all_gather_into_tensor(out, inp)
        self._landed(tensor)

    def allreduce_sum(self, tensor):
        self.dist.all_reduce(tensor, op=self.dist.ReduceOp.SUM)
        self._landed(tensor)

    def _landed(self, tensor):
        if not self.device_ordered and getattr(tensor, "is_cuda", False):
            import torch

            torch.cuda.current_stream(tensor.device).synchronize()

    def gather_objects(self, obj):
        out = [None] * self.world
        self.dist.all_gather_object(out, obj)
        return out


class NoExchange:
    rank, world, device_ordered = 0, 1, False

    def allgather_equal(self, tensor, per):
        pass

    def allreduce_sum(self, tensor):
        pass

    def gather_objects(self, obj):
        return [obj]


def engine_exchange_tensor(eng, which, device_index=0):
    """torch tensor aliasing a libmuxgl device buffer (zero-copy, __cuda_array_interface__), slack included:
    CGP -> f64[S + pad, K*3], CLUST -> i32[C_total + pad, 1], STAT -> i32[4]"""
    import torch

    from . import muxgl

    buf = {UNIT_CGP: muxgl.BUF_CGP, UNIT_CLUST: muxgl.BUF_CLUST, UNIT_STAT: muxgl.BUF_STAT}[which]
    ptr, n = eng.fmx_buffer(buf)
    row = {UNIT_CGP: eng.K * 3, UNIT_CLUST: 1, UNIT_STAT: 1}[which]
    n_all = n + (muxgl.XCHG_PAD * row if which != UNIT_STAT else 0)
    typestr, dtype = ("<f8", torch.float64) if which == UNIT_CGP else ("<i4", torch.int32)

    class _Wrap:
        __cuda_array_interface__ = {"shape": (int(n_all),), "typestr": typestr, "data": (int(ptr), False), "version": 2}

    t = torch.as_tensor(_Wrap(), device=torch.device("cuda", device_index))
    assert t.dtype == dtype and t.data_ptr() == ptr
    return t if which == UNIT_STAT else t.view(-1, row)


def plan_ranges(C: int, S: int, world: int):
    """((cell ranges, cells per rank), (SNP ranges, SNPs per rank)): equal slices, see shard.equal_ranges"""
    return shard.equal_ranges(C, world), shard.equal_ranges(S, world)


def load_rank(eng, p, c_range, s_range):
    """Hand-over of one rank's share of the pileup p: row slab, column slab, entry likelihoods.  Returns the singlet
    scores (llk0, llk2, nsnps, nreads) of the rank's own cells.  (A loader that never materialises the whole pileup on a
    rank would cut the same two slabs at file level: .plp.gz rows are sorted by SNP, then droplet.)"""
    c0, c1 = c_range
    s0, s1 = s_range
    sub = shard.take_cells(p, c0, c1)
    eng.set_pileup(p.S, sub.cell_ptr, sub.entry_snp, sub.entry_rptr, sub.reads)
    eng.fmx_set_column_slab(p.C, c0, s0, s1, *shard.take_snps(p, s0, s1))
    return eng.fmx_prepare(p.af)


def load_rank_from_files(eng, exe, plp_prefix, rank, world, scratch, extra=()):
    """load_rank() from a dsc-pileup data set on disk: the C++ loader (`popscle-amd dump-plp --rank r --world N`) keeps
    only this rank's two slabs while it parses the .plp.gz -- the whole pileup is never held by a rank, on the host or
    on the device.  Returns (scores of the own cells, the slab dictionary)."""
    import subprocess

    from . import plpio

    r = subprocess.run([exe, "dump-plp", "--plp", plp_prefix, "--out", scratch, "--rank", str(rank), "--world", str(world),
                        *extra], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    d = plpio.read_slab_dump(scratch)
    eng.set_pileup(d["S"], *d["rows"])
    eng.fmx_set_column_slab(d["C"], d["c0"], d["s0"], d["s1"], *d["cols"])
    return eng.fmx_prepare(d["af"]), d


def settle_near_ties(engs, gather, doublet_prior, geno_error):
    """The exact path for the calls rounding noise could decide (include/muxgl.h, csrc/fmx_exact.hip), across ranks:
    the SNP lists of the ranks' listed cells are united, every cluster-posterior row is recomputed exactly by the rank
    whose M-step range holds the SNP, all ranks get all rows, and every rank settles its own cells.

    engs: the engines this process drives (one per rank in a real run; several virtual ranks in tests).
    gather(obj) -> list of obj over ALL ranks of the job (identity-like for a process that drives every rank).
    Returns True when an assignment changed anywhere (assignments must be exchanged again, the M-step repeated)."""
    lists = [e.fmx_exact_snps() for e in engs]
    every = [x for part in gather(lists) for x in part]
    uni = np.unique(np.concatenate(every)).astype(np.int32) if every else np.zeros(0, dtype=np.int32)
    K = engs[0].K
    mine = []
    for e in engs:
        rows, owned = e.fmx_exact_rows(uni, doublet_prior, geno_error)
        mine.append((np.flatnonzero(owned), rows[owned]))
    full = np.zeros((uni.size, K, 3))
    seen = np.zeros(uni.size, dtype=bool)
    for part in gather(mine):
        for idx, r in part:
            full[idx] = r
            seen[idx] = True
    if not seen.all():
        raise RuntimeError("near-tie calls: no rank's M-step range holds SNP(s) " + str(uni[~seen][:5].tolist()))
    re = [e.fmx_exact_finish(uni, full, doublet_prior, geno_error)[1] for e in engs]
    return any(x for part in gather(re) for x in part)


def run_em(eng, K, clust0, doublet_prior=0.5, geno_error=0.1, max_iter=10, early_stop=True, exchange=None,
           exchange_tensor=engine_exchange_tensor, log=None, per=None, timings=None, sync=None, stream_ctx=None,
           want_singlets=False, want_inclusion=False, *, want_unknown=False, anchors=None, anchor_modes=None,
           want_ambient=None, want_ambient_fit=None, want_alpha_fit=None):
    """EM loop of cmd_cram_freemux2.cpp:373-605 on a prepared engine.  One rank: a plain engine holding the whole
    pileup.  Several ranks: an engine holding the rank's slabs (load_rank), `exchange` a TorchExchange and
    per = (cells per rank, SNPs per rank) of the equal-slice plan the slabs were cut by.  clust0 spans the whole job.
    Returns (records of ALL cells, complete on every rank; per-iteration stats).  stream_ctx: context manager that
    makes the engine's stream torch's current one (device-ordered exchanges).  want_singlets: also the job-wide [C][K]
    table of singlet log-likelihoods of the last iteration (Engine.fmx_singlets of every rank's own cells, gathered
    like the records, in the original cell order): (records, stats, sng) -- the counterpart of
    demuxlet.run_sharded(want_singlets=True).  want_inclusion: also the dict of job-wide per-droplet, per-cluster inclusion
    tables of the last iteration (Engine.fmx_inclusion, gathered the same way) as the last element:
    (records, stats, [sng,] inclusion).  want_unknown (keyword only): also the dict of the three job-wide tables of
    Engine.fmx_unknown (Hardy-Weinberg prior) of the last iteration, gathered the same way, as the last element;
    unknown_summary() turns them into per-droplet calls.  want_ambient = (amb_af, rhos) (keyword only): also the job-wide
    [C][K][n_rho] table of Engine.fmx_ambient of the last iteration, gathered the same way, as the last element;
    ambient_summary() turns it into per-droplet calls.  want_ambient_fit = (amb_af, rho_max, n_top) (keyword only): also
    the job-wide dict of Engine.fmx_ambient_fit of the last iteration for the n_top best clusters of every droplet's row of
    the singlet table (ties to the lower index), with those candidates under "cand" ([C][n_top]), gathered the same way,
    as the last element; ambient_fit_summary() gives the standard errors.  want_alpha_fit = (alpha_max,) (keyword only):
    also the job-wide dict of Engine.fmx_alpha_fit of the last iteration for the two pairs of call_pairs() of every droplet,
    with those pairs under "pair" ([C][2][2]) and alpha_max, gathered the same way, as the last element;
    alpha_fit_summary() gives the standard errors.  anchors (keyword only): a list of columns of the panel the
    engine holds (demux_set_gp); clusters 0 .. len(anchors)-1 are held to those donors' genotypes and the others are
    learned (Engine.fmx_set_anchors, after fmx_set_clusters; anchor_start() makes a clust0 for it).  One engine with the
    whole pileup or a device group only: refused with more than one rank or always=True.  anchor_modes (keyword only,
    with anchors): one of muxgl.ANCHOR_HELD / ANCHOR_PRIOR per anchor; a PRIOR donor's genotypes are the prior of the
    posterior the droplets form (Engine.fmx_cluster_gp has the refined rows afterwards, refine_summary() sums them up)."""
    ex = exchange or NoExchange()
    multi = ex.world > 1 or getattr(ex, "always", False)  # (always: the exchange path with a single rank, for tests)
    if anchors is not None and multi:
        raise ValueError("run_em: anchors need one engine with the whole job (or a device group), not ranks with slabs")
    if anchor_modes is not None and (anchors is None or len(anchor_modes) != len(anchors)):
        raise ValueError("run_em: anchor_modes needs anchors, one mode each")
    t_start = time.perf_counter()
    eng.fmx_set_clusters(K, np.ascontiguousarray(clust0, dtype=np.int32))  # :277-288, own SNP range
    if anchors is not None:
        eng.fmx_set_anchors(anchors, anchor_modes)
    if multi:
        per_c, per_s = per
        t_cgp, t_clust = exchange_tensor(eng, UNIT_CGP), exchange_tensor(eng, UNIT_CLUST)
        t_stat = exchange_tensor(eng, UNIT_STAT)
    ordered = multi and ex.device_ordered
    if ordered:
        import torch

        stat_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        stat_ready = torch.cuda.Event()
    history = []
    # device-ordered exchanges are timed with events on the engine's stream (the collective's own stream is ordered
    # against it on both sides): what the scaling model of DESIGN.md 4.3 is compared with
    marks = [] if (ordered and timings is not None) else None

    def mark():
        if marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)

    if sync:
        sync()
    t_loop = time.perf_counter()
    with (stream_ctx() if stream_ctx else contextlib.nullcontext()):
        for it in range(max_iter):
            if not multi:  # one handle, whole pileup: the three phases as ONE call (no host round trip between them)
                _, stats = eng.fmx_iterate(doublet_prior, geno_error, want_cells=False)
                history.append(stats)
                if log:
                    log(f"iter {it + 1}: {stats[0]} singlets, {eng.C_total - stats[0] - stats[1]} doublets, "
                        f"{stats[1]} ambiguous, {stats[2]} changed")
                if stats[2] == 0 and early_stop:  # :601-604
                    break
                continue
            eng.fmx_iter_gp(doublet_prior, geno_error)
            if multi:
                mark()
                ex.allgather_equal(t_cgp, per_s)
                mark()
            eng.fmx_iter_estep(doublet_prior, geno_error)
            if multi:
                mark()
                ex.allgather_equal(t_clust, per_c)
                ex.allreduce_sum(t_stat)
                mark()
            if ordered:  # counters on their way to the host; the M-step is enqueued before anybody waits for them
                stat_host.copy_(t_stat, non_blocking=True)
                stat_ready.record()
                eng.fmx_iter_mstep()
                stat_ready.synchronize()
                stats4 = tuple(int(x) for x in stat_host[:4].tolist())
            else:
                stats4 = tuple(int(x) for x in t_stat[:4].tolist())
            if stats4[3] > 0:
                # cells whose call is within rounding reach of the kernels' numbers, somewhere in the job: settled in the
                # reference's arithmetic (two small exchanges, this iteration only), then the assignments and the counters
                # once more, and the ordered merge from the corrected assignments
                reassigned = settle_near_ties([eng], ex.gather_objects, doublet_prior, geno_error)
                ex.allgather_equal(t_clust, per_c)
                ex.allreduce_sum(t_stat)
                stats4 = tuple(int(x) for x in t_stat[:4].tolist())
                if reassigned or not ordered:
                    eng.fmx_iter_mstep()
            elif not ordered:
                eng.fmx_iter_mstep()  # :516-517 + :590-596 for the own SNP range
            stats = stats4[:3]
            if hasattr(eng, "fmx_exact_hint"):
                eng.fmx_exact_hint(stats[2])  # nothing moved: the cells settled so far need not be listed again
            history.append(stats)
            if log:
                log(f"iter {it + 1}: {stats[0]} singlets, {eng.C_total - stats[0] - stats[1]} doublets, "
                    f"{stats[1]} ambiguous, {stats[2]} changed")
            if stats[2] == 0 and early_stop:  # :601-604
                break
    if sync:
        sync()
    t_end = time.perf_counter()
    if timings is not None:  # `sync` (a barrier) makes these comparable across ranks
        timings.update(setup_s=t_loop - t_start, loop_s=t_end - t_loop, iterations=len(history))
        if marks:
            torch.cuda.synchronize()
            gp = [marks[i].elapsed_time(marks[i + 1]) for i in range(0, len(marks), 4)]
            cl = [marks[i + 2].elapsed_time(marks[i + 3]) for i in range(0, len(marks), 4)]
            timings.update(exchange_ms={"cluster_gp_allgather": sum(gp) / len(gp),
                                        "assignments_allgather_and_counters": sum(cl) / len(cl)})
    cells, _ = eng.fmx_iter_fetch()  # the rank's own cells
    c0 = eng.cell_base
    parts = ex.gather_objects((c0, c0 + len(cells), cells.tobytes()))
    out = np.zeros(eng.C_total, dtype=cells.dtype)
    for b, e, raw in parts:
        out[b:e] = np.frombuffer(raw, dtype=cells.dtype)
    if not want_singlets and not want_inclusion and not want_unknown and want_ambient is None and want_ambient_fit is None \
            and want_alpha_fit is None:
        return out, history
    res = [out, history]
    if want_singlets:
        sng = np.zeros((eng.C_total, K), dtype=np.float64)  # the last E-step's posteriors are still in place: muxgl.h
        for b, e, raw in ex.gather_objects((c0, c0 + len(cells), eng.fmx_singlets().tobytes())):
            sng[b:e] = np.frombuffer(raw, dtype=np.float64).reshape(e - b, K)
        res.append(sng)
    if want_inclusion:
        mine = eng.fmx_inclusion(doublet_prior)
        incl = {n: np.zeros((eng.C_total,) + a.shape[1:], dtype=a.dtype) for n, a in mine.items()}
        for b, e, raws in ex.gather_objects((c0, c0 + len(cells), {n: a.tobytes() for n, a in mine.items()})):
            for n, raw in raws.items():
                incl[n][b:e] = np.frombuffer(raw, dtype=incl[n].dtype).reshape((e - b,) + incl[n].shape[1:])
        res.append(incl)
    if want_unknown:
        mine = {n: a for n, a in eng.fmx_unknown().items() if n != "kernel_ms"}
        unk = {n: np.zeros((eng.C_total,) + a.shape[1:], dtype=a.dtype) for n, a in mine.items()}
        for b, e, raws in ex.gather_objects((c0, c0 + len(cells), {n: a.tobytes() for n, a in mine.items()})):
            for n, raw in raws.items():
                unk[n][b:e] = np.frombuffer(raw, dtype=np.float64).reshape((e - b,) + unk[n].shape[1:])
        res.append(unk)
    if want_ambient is not None:
        amb_af, rhos = want_ambient
        amb = np.zeros((eng.C_total, K, len(rhos)), dtype=np.float64)
        for b, e, raw in ex.gather_objects((c0, c0 + len(cells), eng.fmx_ambient(amb_af, rhos)["ll"].tobytes())):
            amb[b:e] = np.frombuffer(raw, dtype=np.float64).reshape(e - b, K, len(rhos))
        res.append(amb)
    if want_ambient_fit is not None:
        amb_af, rho_max, n_top = want_ambient_fit
        n_top = min(int(n_top), K)
        cand = top_clusters(eng.fmx_singlets(), n_top)
        mine = {k: v for k, v in eng.fmx_ambient_fit(amb_af, cand, rho_max).items() if k != "kernel_ms"}
        mine["cand"] = cand
        fit = {k: np.zeros((eng.C_total, n_top), dtype=v.dtype) for k, v in mine.items()}
        for b, e, raw in ex.gather_objects((c0, c0 + len(cells), {k: v.tobytes() for k, v in mine.items()})):
            for k, v in fit.items():
                v[b:e] = np.frombuffer(raw[k], dtype=v.dtype).reshape(e - b, n_top)
        res.append(fit)
    if want_alpha_fit is not None:
        (alpha_max,) = want_alpha_fit
        got = eng.fmx_alpha_fit(call_pairs(cells), alpha_max)
        mine = {k: got[k] for k in eng.ALPHA_FIT_FIELDS + ("pair",)}
        fit = {k: np.zeros((eng.C_total,) + v.shape[1:], dtype=v.dtype) for k, v in mine.items()}
        for b, e, raw in ex.gather_objects((c0, c0 + len(cells), {k: v.tobytes() for k, v in mine.items()})):
            for k, v in fit.items():
                v[b:e] = np.frombuffer(raw[k], dtype=v.dtype).reshape((e - b,) + v.shape[1:])
        fit["alpha_max"] = float(alpha_max)
        res.append(fit)
    return tuple(res)


def anchor_start(llr, nsnps, ncells, donor, K):
    """Where an anchored run starts: the relabelling of K greedy clusters (csrc/anchor_plan.hpp is the same function in
    C++; pure numpy).  llr [K][V] = ll - ll0 of Engine.fmx_match_donors on the greedy clusters, nsnps [K] its markers,
    ncells [K] the cells of every greedy cluster, donor [n] the anchored donors (cluster i of the run is donor[i]).
    Candidates (greedy cluster k, anchor i) in order of llr[k][donor[i]] descending, then k, then i ascending, are accepted
    one to one while llr > 0 (a NaN counts as -inf; a cluster with nsnps == 0 never matches): cluster k becomes cluster i.
    An anchor without a match starts empty.  The unmatched clusters fill the free ids n .. K-1 in order of cell count
    descending, then id ascending; those that do not fit leave their cells unassigned.  Returns a dict: new_id int32 [K]
    (the run's cluster of every greedy cluster, or -1), match int32 [n] (the greedy cluster an anchor starts from, or -1)
    and match_llr float64 [n] (its llr, or NaN).  clust0 of the run is np.where(c >= 0, new_id[c], -1) of the greedy c."""
    llr = np.asarray(llr, dtype=np.float64)
    nsnps = np.asarray(nsnps)
    ncells = np.asarray(ncells, dtype=np.int64)
    donor = np.asarray(donor, dtype=np.int64).reshape(-1)
    K = int(K)
    n = donor.size
    if llr.ndim != 2 or llr.shape[0] != K or nsnps.shape != (K,) or ncells.shape != (K,) or n > K:
        raise ValueError("llr must be [K][V], nsnps and ncells [K], and at most K donors")
    if n and (donor.min() < 0 or donor.max() >= llr.shape[1]):
        raise ValueError("donor outside [0, V)")
    new_id = np.full(K, -1, dtype=np.int32)
    match = np.full(n, -1, dtype=np.int32)
    match_llr = np.full(n, np.nan)
    if n:
        v = llr[:, donor]  # [K][n]
        v = np.where(np.isnan(v) | (nsnps == 0)[:, None], -np.inf, v)
        kk, ii = np.meshgrid(np.arange(K), np.arange(n), indexing="ij")
        order = np.lexsort((ii.ravel(), kk.ravel(), -v.ravel()))  # (last key first: value descending, then k, then i)
        for c in order:
            k, i = int(kk.ravel()[c]), int(ii.ravel()[c])
            if not v[k, i] > 0.0:
                break
            if new_id[k] >= 0 or match[i] >= 0:
                continue
            new_id[k], match[i], match_llr[i] = i, k, v[k, i]
    left = [k for k in range(K) if new_id[k] < 0]
    left.sort(key=lambda k: (-int(ncells[k]), k))
    for j, k in enumerate(left[:K - n]):
        new_id[k] = n + j
    return dict(new_id=new_id, match=match, match_llr=match_llr)


def refine_modes(sample_ids, listed):
    """The modes of `freemuxlet --anchor-refine-list FILE` (csrc/anchor_plan.hpp refine_modes is the same function in C++):
    sample_ids the anchored donors in cluster order, listed the text of FILE -- one sample ID per line, the first
    white-space separated word; empty lines and lines starting with '#' do not count.  A listed donor is ANCHOR_PRIOR, the
    others ANCHOR_HELD; naming one twice is allowed, an ID that is no anchored donor is a ValueError."""
    ids = list(sample_ids)
    modes = [0] * len(ids)
    for line in listed.splitlines():
        words = line.split()
        if not words or words[0].startswith("#"):
            continue
        if words[0] not in ids:
            raise ValueError(f"--anchor-refine-list: '{words[0]}' is not a sample of the anchor VCF")
        for i, s in enumerate(ids):
            if s == words[0]:
                modes[i] = 1
    return modes


def refine_summary(panel, has_gp, rows):
    """What the droplets made of the PRIOR donors' genotypes.  panel [S][n][3]: the donors' panel rows as demux_set_gp took
    them; has_gp [S]; rows [S][n][3]: the posterior rows of their clusters (Engine.fmx_cluster_gp).  Pure numpy.  Returns a
    dict of arrays [n], over the markers with genotypes: n_geno int64 their number, n_changed int64 the markers whose
    arg-max genotype moved (first maximum on both sides), mean_max_prior and mean_max_post float64 the means of the
    largest panel and of the largest posterior probability (NaN without a marker)."""
    panel = np.asarray(panel, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    has = np.asarray(has_gp).astype(bool).reshape(-1)
    if panel.ndim != 3 or panel.shape[2] != 3 or rows.shape != panel.shape or has.shape != (panel.shape[0],):
        raise ValueError("panel and rows must be [S][n][3] and has_gp [S]")
    n = panel.shape[1]
    pw, pr = panel[has], rows[has]
    n_geno = np.full(n, pw.shape[0], dtype=np.int64)
    if pw.shape[0] == 0:
        nan = np.full(n, np.nan)
        return dict(n_geno=n_geno, n_changed=np.zeros(n, dtype=np.int64), mean_max_prior=nan, mean_max_post=nan.copy())
    return dict(n_geno=n_geno, n_changed=(pw.argmax(axis=2) != pr.argmax(axis=2)).sum(axis=0).astype(np.int64),
                mean_max_prior=pw.max(axis=2).mean(axis=0), mean_max_post=pr.max(axis=2).mean(axis=0))


def ambient_summary(ll_amb, rhos):
    """Per droplet, the best "one cell of cluster j plus a share rho of ambient RNA" reading of the table of
    Engine.fmx_ambient (ll_amb float64 [C][K][n_rho]): muxgl.ambient_summary as it is, its tie rule included (value first,
    then (cluster, rho index) ascending), with the cluster fields also under freemuxlet's names: amb_clust = amb_sample,
    base_clust = base_sample."""
    out = muxgl_ambient_summary(ll_amb, rhos)
    out["amb_clust"] = out["amb_sample"]
    out["base_clust"] = out["base_sample"]
    return out


def top_clusters(sng, n_top):
    """int32 [C][n_top]: the n_top best clusters of every row of a singlet table [C][K], best first, ties to the lower
    index"""
    sng = np.asarray(sng, dtype=np.float64)
    order = np.argsort(-np.where(np.isnan(sng), -np.inf, sng), axis=1, kind="stable")
    return np.ascontiguousarray(order[:, :n_top], dtype=np.int32)


def ambient_fit_summary(fit):
    """What a caller reads off the dict of Engine.fmx_ambient_fit: muxgl.ambient_fit_summary as it is, with clusters for
    samples -- se, the standard error of rho_hat where status is 0 and info > 0 and NaN elsewhere (an estimate on a bound
    has none), and lrt, the likelihood ratio 2 * (ll_hat - ll_zero) against rho = 0 (NaN at status 6, where both are
    -inf)."""
    with np.errstate(invalid="ignore"):
        return muxgl_ambient_fit_summary(fit)


def call_pairs(records):
    """int32 [C][2][2]: per record of the EM loop (FMX_CELL) the pairs (dBest1, dBest2) and (sBest, sNext), each (-1, -1)
    where either index is missing (negative; K == 1 has no second cluster): the slots Engine.fmx_alpha_fit takes"""
    rec = np.asarray(records)
    out = np.full((rec.shape[0], 2, 2), -1, dtype=np.int32)
    for slot, (a, b) in enumerate((("dBest1", "dBest2"), ("sBest", "sNext"))):
        ok = (rec[a] >= 0) & (rec[b] >= 0)
        out[ok, slot, 0] = rec[a][ok]
        out[ok, slot, 1] = rec[b][ok]
    return out


def alpha_fit_summary(fit):
    """What a caller reads off the dict of Engine.fmx_alpha_fit (with its "pair" and "alpha_max"): muxgl.alpha_fit_summary as
    it is, with clusters for samples -- se, the standard error of alpha_hat where status is 0 and info > 0 and NaN
    elsewhere; lrt, the likelihood ratio against the better of the two clusters alone where alpha_max is 1 and against the
    first alone where it is smaller (NaN at status 6, where all are -inf); major, the cluster of the pair that holds the
    larger share, also under major_clust."""
    with np.errstate(invalid="ignore"):
        out = muxgl_alpha_fit_summary(fit)
    out["major_clust"] = out["major"]
    return out


def unknown_summary(tables, best_llk):
    """Per droplet, how well a donor that no cluster holds explains it, from the tables of Engine.fmx_unknown (dict with
    ll_ju [C][K], ll_u [C], ll_uu [C]) and the records' bestLLK [C].  Pure numpy.  Returns a dict: half_clust int32 and
    half_llk float64 [C], the largest ll_ju of the droplet and its cluster (ties to the lowest cluster; a NaN counts as
    -inf); unk_llk [C], the largest of ll_u, ll_uu and half_llk; diff [C] = best_llk - unk_llk (-inf - -inf counts as 0:
    neither explains the droplet); n_better int, the droplets with diff < -2, the margin the reference's own calls use
    (cmd_cram_freemux2.cpp:521-584)."""
    ju = np.asarray(tables["ll_ju"], dtype=np.float64)
    lu = np.asarray(tables["ll_u"], dtype=np.float64)
    uu = np.asarray(tables["ll_uu"], dtype=np.float64)
    best = np.asarray(best_llk, dtype=np.float64)
    if ju.ndim != 2 or ju.shape[1] < 1 or lu.shape != ju.shape[:1] or uu.shape != lu.shape or best.shape != lu.shape:
        raise ValueError("tables must be ll_ju [C][K], ll_u [C], ll_uu [C] and best_llk [C]")
    Cn = ju.shape[0]
    cand = np.where(np.isnan(ju), -np.inf, ju)
    half_clust = np.argmax(cand, axis=1).astype(np.int32)  # (argmax: the first, i.e. the lowest cluster, on ties)
    half_llk = cand[np.arange(Cn), half_clust]
    unk_llk = np.maximum(np.maximum(np.where(np.isnan(lu), -np.inf, lu), np.where(np.isnan(uu), -np.inf, uu)), half_llk)
    with np.errstate(invalid="ignore"):
        diff = best - unk_llk
    diff = np.where(np.isnan(diff), 0.0, diff)
    return dict(half_clust=half_clust, half_llk=half_llk, unk_llk=unk_llk, diff=diff, n_better=int((diff < -2.0).sum()))


def match_table(ll, ll0, nsnps=None):
    """Best donors of the clusters from Engine.fmx_match_donors' tables (pure numpy).  ll [K][V], ll0 [K]; llr = ll -
    ll0[:, None] is the log Bayes factor "cluster k is donor v" against "somebody from the population".  Returns a dict,
    per cluster: best, next int32 (the donors with the largest and second largest llr; ties go to the lower donor index;
    next = -1 with a single donor), best_llr, next_llr float64 (NaN where there is none), post float64 [K][V] (softmax of
    ll over the donors with equal priors, the row maximum subtracted) and reciprocal bool (cluster k is also the best
    cluster, lowest index on ties, of its best donor).  A cluster with nsnps == 0 (given nsnps; else: a row of ll and ll0
    that is all zero) has no evidence: best = next = -1, not reciprocal, and is nobody's best cluster."""
    ll = np.asarray(ll, dtype=np.float64)
    ll0 = np.asarray(ll0, dtype=np.float64)
    if ll.ndim != 2 or ll0.shape != ll.shape[:1]:
        raise ValueError("ll must be [K][V] and ll0 [K]")
    K, V = ll.shape
    empty = (np.asarray(nsnps) == 0) if nsnps is not None else (np.all(ll == 0.0, axis=1) & (ll0 == 0.0))
    with np.errstate(invalid="ignore"):
        llr = ll - ll0[:, None]
    llr = np.where(np.isnan(llr), -np.inf, llr)  # (-inf - -inf: no evidence for that donor either)
    best = np.full(K, -1, dtype=np.int32)
    nxt = np.full(K, -1, dtype=np.int32)
    best_llr = np.full(K, np.nan)
    next_llr = np.full(K, np.nan)
    for k in range(K):
        if empty[k] or V == 0:
            continue
        order = np.argsort(-llr[k], kind="stable")  # descending, ties by ascending donor index
        best[k], best_llr[k] = order[0], llr[k, order[0]]
        if V > 1:
            nxt[k], next_llr[k] = order[1], llr[k, order[1]]
    with np.errstate(invalid="ignore", over="ignore"):
        mx = ll.max(axis=1, keepdims=True) if V else np.zeros((K, 1))
        ex = np.exp(np.where(np.isneginf(mx), 0.0, ll - mx))
        post = ex / ex.sum(axis=1, keepdims=True) if V else ex
    best_clust = np.full(V, -1, dtype=np.int64)  # per donor: the cluster with the largest llr among those with evidence
    live = np.flatnonzero(~empty)
    if live.size and V:
        best_clust = live[np.argmax(llr[live], axis=0)]  # (argmax: first = lowest cluster index on ties)
    reciprocal = np.array([best[k] >= 0 and best_clust[best[k]] == k for k in range(K)], dtype=bool)
    return dict(best=best, next=nxt, best_llr=best_llr, next_llr=next_llr, post=post, reciprocal=reciprocal)


def cluster_pair_table(llk2, llk0, nsnps=None, thres=5.41):
    """Which clusters are one donor, from Engine.fmx_cluster_pairs' tables (pure numpy).  llk2, llk0 [K (K - 1) / 2] with the
    pair a > b at a (a - 1) / 2 + b; thres is the reference's --bf-thres default.  Returns a dict: diff float64 [K][K], the
    symmetric matrix of llk2 - llk0 (the log Bayes factor "one donor" against "two unrelated donors") with a NaN diagonal;
    partner int32 [K] and partner_diff float64 [K], per cluster the other cluster with the largest diff and that diff;
    group int32 [K] and groups (a list of lists of cluster indices), the connected components of the pairs with diff >
    thres.  Tie rules: equal diffs go to the lower partner index; a diff equal to thres does not link; a pair without a
    shared marker (nsnps == 0 where nsnps is given, else llk2 == llk0 == 0) carries no evidence, never links and is nobody's
    partner, so a cluster whose pairs are all of that kind (one without cells) has partner -1, partner_diff NaN and a
    group of its own; -inf - -inf counts as -inf.  Groups are numbered in the order of their smallest member and list
    their members in ascending order."""
    llk2 = np.asarray(llk2, dtype=np.float64).ravel()
    llk0 = np.asarray(llk0, dtype=np.float64).ravel()
    n = llk2.size
    K = int(round((1.0 + np.sqrt(1.0 + 8.0 * n)) / 2.0))
    if llk0.size != n or K * (K - 1) // 2 != n:
        raise ValueError("llk2 and llk0 must both be [K (K - 1) / 2]")
    if nsnps is not None and np.asarray(nsnps).size != n:
        raise ValueError("nsnps must be [K (K - 1) / 2]")
    none = (np.asarray(nsnps).ravel() == 0) if nsnps is not None else ((llk2 == 0.0) & (llk0 == 0.0))
    with np.errstate(invalid="ignore"):
        d = llk2 - llk0
    d = np.where(np.isnan(d), -np.inf, d)
    a, b = np.tril_indices(K, -1)  # row-major over the lower triangle: exactly the order a (a - 1) / 2 + b
    diff = np.full((K, K), np.nan)
    diff[a, b] = diff[b, a] = d
    seen = np.zeros((K, K), dtype=bool)
    seen[a, b] = seen[b, a] = ~none
    partner = np.full(K, -1, dtype=np.int32)
    partner_diff = np.full(K, np.nan)
    for k in range(K):
        cand = np.flatnonzero(seen[k])
        if cand.size:
            partner[k] = cand[np.argmax(diff[k, cand])]  # (argmax: the first, i.e. the lowest index, on ties)
            partner_diff[k] = diff[k, partner[k]]
    root = list(range(K))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    for i in np.flatnonzero(~none & (d > thres)):
        ra, rb = find(int(a[i])), find(int(b[i]))
        if ra != rb:
            root[max(ra, rb)] = min(ra, rb)  # (the root of a group is its smallest member)
    roots = [find(k) for k in range(K)]
    order = sorted(set(roots))
    group = np.array([order.index(r) for r in roots], dtype=np.int32)
    groups = [[k for k in range(K) if roots[k] == r] for r in order]
    return dict(diff=diff, partner=partner, partner_diff=partner_diff, group=group, groups=groups)
