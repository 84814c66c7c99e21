"""Random and constructed call sequences for ONE long-lived muxgl handle, and a model of the handle's lifecycle.

No GPU and no library here: numpy only.  tests/test_handle_sequences.py holds the generator to its coverage on the CPU
(with the routing table of popscle_amd/csrc/path_choice.hpp through tests/csrc/path_choice_probe.cpp), and
tests/test_handle_sequences_gpu.py runs every sequence on a device, comparing each step of the long-lived handle with a
fresh handle that is given only what the step needs (DESIGN.md 2b says which state each call builds and drops).

A sequence is a list of steps, dicts with "op", the op's arguments and "expect": None when the model says the call
runs, else the text the library refuses it with on the host, before anything is launched.  Vocabulary:

    load(i)                       one of the four pileups of the seed (pileups(seed))
    panel(V, mode)                the GP tensor for the pileup in force (panel(seed, i, V, mode))
    demux_run(grid, full_ll)      grid: a name of GRIDS
    demux_singlets(grid), demux_inclusion(grid), demux_unknown(grid), demux_entry_pg
    fmx_prepare, set_clusters(K), iterate(full_ll), iter_gp
    fmx_singlets, fmx_inclusion, fmx_cluster_pileup, fmx_match_donors, fmx_cluster_pairs
    budget(name, value)           the slab budget variable `name` set to "1" (MB) or unset (None)

iter_gp (muxgl_fmx_iter_gp, the posterior phase alone) is there because it is the only way to the state "posteriors
rewritten since the last E-step", which two of the calls refuse.

Every step that meets stale state goes from the larger problem to the smaller one: a `load` that is followed by a
demuxlet call without a `panel` in between always loads a pileup with FEWER SNPs than the one before, so that even a
library without the guard of muxgl_set_pileup (which drops the panel) would read nothing past an allocation.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from popscle_amd import synth  # noqa: E402  (numpy only)

GRIDS = {"default": (0.0, 0.5), "six": (0.0, 0.1, 0.2, 0.3, 0.4, 0.5), "sng": (0.0,), "two": (0.2, 0.5)}
PANEL_V = (1, 8, 16, 17, 32, 33, 64, 65, 130, 300)
PANEL_MODES = ("hard", "float_rows", "scaled", "has_gp")
CLUSTER_K = (3, 16, 17, 33, 70, 300)
BUDGETS = ("MUXGL_DEMUX_SLAB_MB", "MUXGL_FMX_SLAB_MB")
FLAG_R, FLAG_W = 2, 4   # MUXGL_FLAG_FORCE_ROW_KERNEL, _WAVE_KERNEL: the handles on which the E-step takes the pair kernel
MAX_STEPS = 16
DEMUX_PATHS = ("oct8", "oct16", "row", "row2", "wave", "tile", "stream")
ESTEP_PATHS = ("oct", "row2", "wave", "pair", "stream")
DEMUX_TABLES = ("demux_singlets", "demux_inclusion", "demux_unknown")
FMX_TABLES = ("fmx_singlets", "fmx_inclusion", "fmx_match_donors", "fmx_cluster_pairs")
PANEL_READERS = ("demux_run",) + DEMUX_TABLES + ("demux_entry_pg", "fmx_match_donors")
TABLE_BUDGET = {**{t: BUDGETS[0] for t in DEMUX_TABLES}, **{t: BUDGETS[1] for t in FMX_TABLES}}

# ---- the refusals: key -> text the library's message contains -------------------------------------------------------
REFUSALS = {
    "demux_no_pileup": "no pileup set (muxgl_set_pileup)",
    "demux_no_panel": "no GP tensor set (muxgl_demux_set_gp)",
    "entry_pg_no_run": "muxgl_demux_get_entry_pg: no previous muxgl_demux_run",
    "demux_full_ll_streamed": "full_ll is not available on the streamed path",
    "prepare_no_pileup": "muxgl_fmx_prepare: no pileup set (muxgl_set_pileup)",
    "clusters_not_prepared": "muxgl_fmx_set_clusters: call muxgl_fmx_prepare first",
    "iterate_no_clusters": "muxgl_fmx_iterate: call muxgl_fmx_prepare and muxgl_fmx_set_clusters first",
    "iterate_full_ll_streamed": "full_ll is not available on the streamed E-step",
    "iter_gp_no_clusters": "muxgl_fmx_iter_gp: call muxgl_fmx_prepare and muxgl_fmx_set_clusters first",
    "fmx_singlets_no_pileup": "muxgl_fmx_singlets: no pileup set (muxgl_set_pileup)",
    "fmx_singlets_not_prepared": "muxgl_fmx_singlets: call muxgl_fmx_prepare first",
    "fmx_singlets_no_clusters": "muxgl_fmx_singlets: no clusters set and no E-step run",
    "fmx_singlets_no_estep": "muxgl_fmx_singlets: no E-step since muxgl_fmx_set_clusters",
    "fmx_singlets_rewritten": "muxgl_fmx_singlets: the cluster posteriors were rewritten",
    "fmx_inclusion_no_pileup": "muxgl_fmx_inclusion: no pileup set (muxgl_set_pileup)",
    "fmx_inclusion_not_prepared": "muxgl_fmx_inclusion: call muxgl_fmx_prepare first",
    "fmx_inclusion_no_clusters": "muxgl_fmx_inclusion: no clusters set and no E-step run",
    "fmx_inclusion_no_estep": "muxgl_fmx_inclusion: no E-step since muxgl_fmx_set_clusters",
    "fmx_inclusion_rewritten": "muxgl_fmx_inclusion: the cluster posteriors were rewritten",
    "cluster_pileup_no_clusters": "muxgl_fmx_get_cluster_pileup: no clusters set",
    "match_no_pileup": "muxgl_fmx_match_donors: no pileup set (muxgl_set_pileup)",
    "match_not_prepared": "muxgl_fmx_match_donors: call muxgl_fmx_prepare first",
    "match_no_clusters": "muxgl_fmx_match_donors: no clusters set (muxgl_fmx_set_clusters)",
    "match_no_panel": "muxgl_fmx_match_donors: no GP tensor set (muxgl_demux_set_gp)",
    "pairs_no_pileup": "muxgl_fmx_cluster_pairs: no pileup set (muxgl_set_pileup)",
    "pairs_not_prepared": "muxgl_fmx_cluster_pairs: call muxgl_fmx_prepare first",
    "pairs_no_clusters": "muxgl_fmx_cluster_pairs: no clusters set (muxgl_fmx_set_clusters)",
    # what a device group refuses by name, and its own wording where it checks before its members do
    "group_run_no_pileup_or_panel": "muxgl_demux_run: no pileup / GP tensor set",
    "group_match": "muxgl_fmx_match_donors: not available on a device group",
    "group_pairs": "muxgl_fmx_cluster_pairs: not available on a device group",
    "group_iter_gp": "muxgl_fmx_iter_gp: not available on a device group",
}

def is_group(seed):
    """every fourth seed runs on a device group of two members on one GPU, Engine([0, 0])"""
    return seed % 4 == 0


# ---- inputs: deterministic in (seed, ...) -----------------------------------------------------------------------------
def _pileup(rng, C, S, lens, donors=4):
    """a packed pileup with the given entries per cell (numpy only; reads as popscle_amd.synth draws them)"""
    af = rng.uniform(0.05, 0.95, size=S)
    G = rng.binomial(2, af[:, None], size=(S, donors))
    lens = np.minimum(np.asarray(lens, dtype=np.int64), S)
    cell_ptr = np.zeros(C + 1, dtype=np.int64)
    np.cumsum(lens, out=cell_ptr[1:])
    snps = [np.sort(rng.choice(S, size=int(n), replace=False)) for n in lens]
    entry_snp = (np.concatenate(snps) if snps else np.zeros(0)).astype(np.int32)
    nnz = entry_snp.size
    nreads = 1 + rng.poisson(0.3, size=nnz).astype(np.int64)
    entry_rptr = np.zeros(nnz + 1, dtype=np.int64)
    np.cumsum(nreads, out=entry_rptr[1:])
    R = int(entry_rptr[-1])
    read_entry = np.repeat(np.arange(nnz, dtype=np.int64), nreads)
    cell_of = np.repeat(np.arange(C, dtype=np.int64), lens)[read_entry]
    src = (cell_of + (rng.random(R) < 0.15)) % donors   # a few reads of a second donor: doublets and noise
    g = G[entry_snp[read_entry], src] if R else np.zeros(0)
    allele = ((rng.random(R) < g / 2.0) ^ (rng.random(R) < 0.01)).astype(np.uint8)
    bq = np.minimum(rng.integers(13, 41, size=R), 20).astype(np.uint8)
    reads = ((allele << 7) | bq).astype(np.uint8)
    reads[rng.random(R) < 0.005] = synth.READ_OTHER
    return synth.Pileup(int(C), int(S), cell_ptr, entry_snp, entry_rptr, reads, af)


def pileup_shapes(seed):
    """[(C, S, entries per cell)] of the four pileups of a seed.  0: the large one, S = 3000, with a cell beyond 2048
    entries (cut into parts by the wave plan and the table plan) and empty cells; 1: no cells at all; 2 and 3: the same
    number of SNPs, fewer than 0, different cells.  About 40 entries per cell."""
    rng = np.random.default_rng([seed, 4101])
    C0 = int(rng.integers(40, 65))
    lens0 = rng.poisson(40, size=C0)
    lens0[rng.choice(C0, size=3, replace=False)] = 0
    lens0[int(rng.integers(C0))] = int(rng.integers(2100, 2600))
    S1 = int(rng.integers(300, 900))
    S2 = int(rng.integers(900, 2000))
    C2 = int(rng.integers(24, 40))
    lens2 = np.maximum(rng.poisson(40, size=C2), 1)
    C3 = int(rng.integers(5, 23))
    lens3 = np.maximum(rng.poisson(40, size=C3), 1)
    return [(C0, 3000, lens0), (0, S1, np.zeros(0, dtype=np.int64)), (C2, S2, lens2), (C3, S2, lens3)]


def pileups(seed):
    """the four pileups of a seed (popscle_amd.synth.Pileup, without a GP tensor)"""
    return [_pileup(np.random.default_rng([seed, 4106, i]), C, S, lens) for i, (C, S, lens) in enumerate(pileup_shapes(seed))]


def pl_facts(seed):
    """(C, S, nnz, longest cell) of the four pileups: all the lifecycle model and the routing read of them"""
    return [(C, S, int(lens.sum()), int(lens.max()) if C else 0) for C, S, lens in pileup_shapes(seed)]


def panel(seed, i, S, V, mode):
    """(gp [S][V][3], has_gp [S]) of panel(V, mode) for pileup i of the seed.  hard: hard calls through the reference's
    error mixing, every triple sums to 1; float_rows: posteriors normalised in float, sums off 1 (the oct kernels' other
    row format); scaled: the hard rows times 0.2 (sums far below 0.35: the split sweep beyond 32 samples); has_gp: the
    hard rows, a tenth of the markers without genotypes."""
    assert mode in PANEL_MODES
    rng = np.random.default_rng([seed, 4102, i, V])
    af = rng.uniform(0.05, 0.95, size=S)
    G = rng.binomial(2, af[:, None], size=(S, V)).astype(np.int64)
    gp = synth.gt_to_gp(G, 0.1)
    has_gp = np.ones(S, dtype=np.uint8)
    if mode == "float_rows":
        g = rng.dirichlet([0.3, 0.3, 0.3], size=(S, V)).astype(np.float32) + np.float32(1e-4)
        g = g / g.sum(axis=2, keepdims=True, dtype=np.float32)
        gp = 0.9 * g.astype(np.float64) + 0.1 * g.astype(np.float64).mean(axis=1, keepdims=True)
    elif mode == "scaled":
        gp = gp * 0.2
    elif mode == "has_gp":
        has_gp[np.random.default_rng([seed, 4103, i, V]).random(S) < 0.1] = 0
    return np.ascontiguousarray(gp), has_gp


def panel_facts(gp, has_gp):
    """(unit sums, smallest sum) as muxgl_demux_set_gp judges them: every triple of a marker with genotypes within 2^-50
    of 1, summed as (g0 + g1) + g2"""
    rows = gp[has_gp != 0]
    if rows.size == 0:
        return True, 1.0
    sm = (rows[:, :, 0] + rows[:, :, 1]) + rows[:, :, 2]
    return bool(np.all(np.abs(sm - 1.0) <= 2.0 ** -50)), float(min(1.0, sm.min()))


def init_clusters(seed, i, C, K):
    """the recorded start of set_clusters(K) on pileup i: a cluster per cell, some cells without one (-1)"""
    rng = np.random.default_rng([seed, 4104, i, K])
    c = rng.integers(0, K, size=C).astype(np.int32)
    c[rng.random(C) < 0.1] = -1
    return c


# ---- the routing as the generator expects it (a hint: the CPU test holds every step to path_choice.hpp itself) -------
def hint_demux_path(V, grid, flags=0):
    A = len(grid)
    T, R, W = flags & 1, flags & FLAG_R, flags & FLAG_W
    if V > 255:
        return "stream"
    if V <= 32 and not (T or R or W) and tuple(grid) == GRIDS["default"]:
        return "oct8" if V <= 16 else "oct16"
    nsy = sum(1 for a in grid[1:] if a == 0.5)
    if V <= 16 and not T and not W and nsy <= 1 and A - 1 - nsy <= 5:
        return "row"
    if 16 < V <= 32 and not T and not W and A == 2 and grid[1] == 0.5 and grid[0] != 0.5:
        return "row2"
    thin = V > 64 and V % 64 != 0 and V % 64 <= 8 and V < 128
    if not T and A >= 2 and not thin and (V > 16 or W):
        return "wave"
    return "tile"


def hint_estep_path(K, flags=0):
    T, R, W = flags & 1, flags & FLAG_R, flags & FLAG_W
    if K > 255:
        return "stream"
    if K <= 16 and not T and not R:
        return "oct"
    if 16 < K <= 32 and not T and not W:
        return "row2"
    if K > 32 and not T:
        return "wave"
    return "pair"


# ---- the lifecycle model -----------------------------------------------------------------------------------------------
class Lifecycle:
    """What a handle holds after each step -- a pileup; a panel FOR THE PILEUP IN FORCE; the grid of the last run;
    prepared; clusters; an E-step since the clusters; posteriors rewritten since that E-step -- and, for each call, None
    ("runs") or the key of REFUSALS the library answers with.  pl: the four pileups' (C, S, nnz, longest cell)."""

    def __init__(self, pl, flags=0, group=False):
        self.pl, self.flags, self.group = pl, flags, group
        self.i = None          # pileup in force
        self.panel = None      # (V, mode) for that pileup
        self.grid = None       # grid of the last demux_run that ran (muxgl_demux_get_entry_pg reports with it)
        self.prepared = False
        self.K = 0
        self.iters = 0         # E-steps since set_clusters
        self.rewritten = False # iter_gp since the last E-step
        self.budget = {b: None for b in BUDGETS}

    def C(self):
        return self.pl[self.i][0] if self.i is not None else 0

    def S(self):
        return self.pl[self.i][1] if self.i is not None else 0

    def refusal(self, st):
        """key of REFUSALS, or None: the call runs"""
        op, g = st["op"], self.group
        if op in ("load", "panel", "budget"):
            return None
        if op in ("demux_run",) + DEMUX_TABLES:
            if g and op == "demux_run" and (self.i is None or self.panel is None):
                return "group_run_no_pileup_or_panel"
            if self.i is None:
                return "demux_no_pileup"
            if self.panel is None:
                return "demux_no_panel"
            if op == "demux_run" and st["full_ll"] and self.C() > 0 and self.panel[0] > 255:
                return "demux_full_ll_streamed"
            return None
        if op == "demux_entry_pg":
            return None if self.grid is not None else "entry_pg_no_run"
        if op == "fmx_prepare":
            return None if self.i is not None else "prepare_no_pileup"
        if op == "set_clusters":
            return None if self.prepared else "clusters_not_prepared"
        if op == "iterate":
            if not self.prepared or self.K < 1:
                return "iterate_no_clusters"
            return "iterate_full_ll_streamed" if st["full_ll"] and self.K > 255 else None
        if op == "iter_gp":
            if g:
                return "group_iter_gp"
            return None if self.prepared and self.K >= 1 else "iter_gp_no_clusters"
        if op in ("fmx_singlets", "fmx_inclusion"):
            if self.i is None:
                return op + "_no_pileup"
            if not self.prepared:
                return op + "_not_prepared"
            if self.K < 1:
                return op + "_no_clusters"
            if self.iters == 0:
                return op + "_no_estep"
            return op + "_rewritten" if self.rewritten else None
        if op == "fmx_cluster_pileup":
            return None if self.K >= 1 else "cluster_pileup_no_clusters"
        if op in ("fmx_match_donors", "fmx_cluster_pairs"):
            w = "match" if op == "fmx_match_donors" else "pairs"
            if g:
                return "group_" + w
            if self.i is None:
                return w + "_no_pileup"
            if not self.prepared:
                return w + "_not_prepared"
            if self.K < 1:
                return w + "_no_clusters"
            return "match_no_panel" if w == "match" and self.panel is None else None
        raise ValueError(op)

    def apply(self, st):
        """the step's refusal key (None: it runs), and the state after it; a refused call changes nothing"""
        why = self.refusal(st)
        if why is not None:
            return why
        op = st["op"]
        if op == "load":   # a new pileup drops the panel, the last grid and the freemuxlet job
            self.i, self.panel, self.grid, self.prepared, self.K, self.iters, self.rewritten = st["i"], None, None, False, 0, 0, False
        elif op == "panel":
            self.panel, self.grid = (st["V"], st["mode"]), None
        elif op == "demux_run":
            if self.C() > 0 or self.group:   # (no cells: nothing is launched and no grid remembered; a group remembers it itself)
                self.grid = st["grid"]
        elif op == "fmx_prepare":
            self.prepared, self.K, self.iters, self.rewritten = True, 0, 0, False
        elif op == "set_clusters":
            self.K, self.iters, self.rewritten = st["K"], 0, False
        elif op == "iterate":
            self.iters, self.rewritten = self.iters + 1, False
        elif op == "iter_gp":
            self.rewritten = self.iters > 0
        elif op == "budget":
            self.budget[st["name"]] = st["value"]
        return None

    def key(self):
        """everything a call's outputs depend on (two running calls of one table under the same key give the same bits)"""
        return (self.i, self.panel, self.prepared, self.K, self.iters, self.rewritten)


def replay(seq, pl, flags, group):
    """[(step, refusal key or None, a copy of the model AFTER the step)] of a sequence, for the tests"""
    import copy

    m, out = Lifecycle(pl, flags, group), []
    for st in seq:
        why = m.apply(st)
        snap = copy.copy(m)
        snap.budget = dict(m.budget)
        out.append((st, why, snap))
    return out


# ---- the generator -----------------------------------------------------------------------------------------------------
class _Full(Exception):
    pass


class _Builder:
    def __init__(self, seed, flags, group, rng):
        self.seed, self.flags, self.group, self.rng = seed, flags, group, rng
        self.pl = pl_facts(seed)
        self.m = Lifecycle(self.pl, flags, group)
        self.steps = []
        self.iter_job = 0   # iterate steps of the running freemuxlet job (at most three)
        self.panel_S = None  # SNPs of the pileup the last panel was made for
        self.limit = MAX_STEPS

    def emit(self, op, **kw):
        if len(self.steps) >= self.limit:
            raise _Full
        st = dict(op=op, **kw)
        if op == "set_clusters":
            self.iter_job = 0
        why = self.m.apply(st)
        if op == "panel":
            self.panel_S = self.m.S()
        st["expect"] = None if why is None else REFUSALS[why]
        st["why"] = why
        self.steps.append(st)
        return why

    # -- goals: each emits the steps that are missing for it
    def load(self, i):
        self.emit("load", i=int(i))

    def need_pileup(self, cells=True):
        if self.m.i is None or (cells and self.m.C() == 0):
            self.load(self.rng.choice([0, 2, 3]))

    def need_panel(self, V=None, mode=None):
        self.need_pileup(cells=False)
        if self.m.panel is None or (V is not None and self.m.panel[0] != V) or (mode is not None and self.m.panel[1] != mode):
            V = int(V if V is not None else self.rng.choice(PANEL_V))
            if mode is None:
                mode = str(self.rng.choice(["hard", "hard", "float_rows", "has_gp"] + (["scaled"] if V > 32 else [])))
            self.emit("panel", V=V, mode=mode)

    def full_ll_ok(self, V, grid):
        return V <= 255 and self.m.C() * V * V * len(GRIDS[grid]) * 8 < 3e7

    def demux(self, path, full_ll=None, mode=None):
        """a demux_run on `path` (a hint; the CPU test checks it): the panel in force if some grid gets there with it"""
        self.need_pileup()
        cands = [(V, g) for V in PANEL_V for g in GRIDS if hint_demux_path(V, GRIDS[g], self.flags) == path]
        if not cands:
            return False
        here = [c for c in cands if self.m.panel is not None and c[0] == self.m.panel[0]]
        V, g = (here or cands)[int(self.rng.integers(len(here or cands)))]
        self.need_panel(V, mode)
        if full_ll is None:
            full_ll = bool(self.rng.random() < 0.3) and self.full_ll_ok(V, g)
        self.emit("demux_run", grid=g, full_ll=bool(full_ll))
        return True

    def need_clusters(self, K=None):
        self.need_pileup()
        if not self.m.prepared:
            self.emit("fmx_prepare")
        if self.m.K < 1 or (K is not None and self.m.K != K):
            self.emit("set_clusters", K=int(K if K is not None else self.rng.choice(CLUSTER_K)))

    def estep(self, path=None, K=None, full_ll=None):
        if K is None:
            ks = [k for k in CLUSTER_K if path is None or hint_estep_path(k, self.flags) == path]
            if not ks:
                return False
            K = self.m.K if self.m.K in ks and self.iter_job < 3 else int(ks[int(self.rng.integers(len(ks)))])
        if self.iter_job >= 3 and self.m.K == K:
            self.emit("set_clusters", K=int(K))
        self.need_clusters(K)
        if full_ll is None:
            full_ll = bool(self.rng.random() < 0.3) and K <= 70
        self.emit("iterate", full_ll=bool(full_ll))
        self.iter_job += 1
        return True

    def table(self, t, flip=False):
        """a call of table t; flip: the call, the other value of its budget, the call again"""
        if t in DEMUX_TABLES:
            self.need_panel()
            kw = dict(grid=str(self.rng.choice(list(GRIDS))))
        else:
            if t == "fmx_match_donors":
                self.need_panel()
            if self.m.K < 1 or self.m.iters == 0 or self.m.rewritten:
                self.estep(K=self.m.K if self.m.K >= 1 else None)
            kw = {}
        self.emit(t, **kw)
        if flip:
            name = TABLE_BUDGET[t]
            self.emit("budget", name=name, value=None if self.m.budget[name] else "1")
            self.emit(t, **kw)

    def refused(self):
        """One call the model refuses.  Mostly in the state as it is; sometimes the state is made first: a smaller pileup
        loaded over a panel (the stale panel must be gone, not read), a job prepared but without clusters, clusters
        without an E-step."""
        m, r = self.m, self.rng
        only = None
        u = r.random()
        if u < 0.3 and m.i is not None and m.panel is not None:
            smaller = [j for j in range(4) if self.pl[j][1] < m.S()]
            if smaller:
                self.load(smaller[int(r.integers(len(smaller)))])
                only = ("demux_run",) + DEMUX_TABLES + ("demux_entry_pg",)
        elif u < 0.5 and m.i is not None:
            self.emit("fmx_prepare")
            only = ("iterate", "fmx_singlets", "fmx_inclusion", "fmx_cluster_pileup", "fmx_match_donors", "fmx_cluster_pairs")
        elif u < 0.65 and m.prepared:
            self.emit("set_clusters", K=int(r.choice(CLUSTER_K)))
            only = ("fmx_singlets", "fmx_inclusion")
        # a call that would read the panel is only made without one where the last panel was for MORE SNPs than the
        # pileup in force has (a library that kept it would stay inside it)
        unsafe = m.panel is None and self.panel_S is not None and m.S() >= self.panel_S
        cands = []
        for op in ("demux_run", "demux_singlets", "demux_inclusion", "demux_unknown", "demux_entry_pg", "fmx_prepare",
                   "set_clusters", "iterate", "iter_gp", "fmx_singlets", "fmx_inclusion", "fmx_cluster_pileup",
                   "fmx_match_donors", "fmx_cluster_pairs"):
            if unsafe and op in PANEL_READERS:
                continue
            for st in self._forms(op):
                if m.refusal(st) is not None and (only is None or op in only):
                    cands.append(st)
        if not cands:
            return False
        st = dict(cands[int(r.integers(len(cands)))])
        self.emit(st.pop("op"), **st)
        return True

    def _forms(self, op):
        if op == "demux_run":
            return [dict(op=op, grid="default", full_ll=False), dict(op=op, grid="two", full_ll=True)]
        if op in DEMUX_TABLES:
            return [dict(op=op, grid="default")]
        if op == "set_clusters":
            return [dict(op=op, K=3)]
        if op == "iterate":
            return [dict(op=op, full_ll=False), dict(op=op, full_ll=True)]
        return [dict(op=op)]


def _finish(b):
    for st in b.steps:
        st.pop("why", None)
    return b.steps


def held_to_oracle(seed, flags, seq):
    """(a demux_run at V <= 16 ran on some cells, an iterate at K <= 16 ran on some cells)"""
    d = f = False
    for st, why, m in replay(seq, pl_facts(seed), flags, is_group(seed)):
        d = d or (why is None and st["op"] == "demux_run" and m.panel[0] <= 16 and m.C() > 0)
        f = f or (why is None and st["op"] == "iterate" and m.K <= 16 and m.C() > 0)
    return d, f


def _random(seed):
    """_plan(seed); where its walks left no room for one of the two calls every sequence holds to the oracle, the plan is
    made again five steps shorter and the missing call is put behind it"""
    flags, seq = _plan(seed, MAX_STEPS)
    d, f = held_to_oracle(seed, flags, seq)
    if d and f:
        return flags, seq
    return _plan(seed, MAX_STEPS - 5, finish=True)


def _plan(seed, limit, finish=False):
    """A random plan over the goals of _Builder, dense in transitions: after a load, a walk over demuxlet paths (it
    begins at V <= 16: the run every sequence holds to the oracle), a walk over E-step paths (it begins at K <= 16: the
    iteration held to the oracle) and a block of tables under both budgets, in a random order and with random lengths
    (some of them zero); about one step in eight is a call the model refuses, some after a load of a smaller pileup."""
    rng = np.random.default_rng([seed, 4100])
    flags = int(rng.choice([0, 0, 0, FLAG_R, FLAG_W]))
    b = _Builder(seed, flags, is_group(seed), rng)
    b.limit = limit
    p_ref = float(rng.choice([0.0, 0.1, 0.125, 0.3, 0.6]))
    cut = sorted(rng.integers(0, 13, size=2))
    n_d, n_e = int(cut[0]), int(cut[1] - cut[0])   # steps of the two walks beyond their first calls; the rest: tables
    dgroup = float(rng.choice([0.3, 0.6, 0.9]))    # how often the demuxlet walk changes the panel

    def maybe_refused():
        if rng.random() < p_ref:
            b.refused()

    def demux_walk():
        first = [q for q in ("oct8", "row", "wave", "tile") if any(hint_demux_path(V, g, flags) == q for V in (1, 8, 16) for g in GRIDS.values())]
        b.need_pileup()
        cands = [(V, g) for V in (1, 8, 16) for g in GRIDS if hint_demux_path(V, GRIDS[g], flags) in first]
        V, g = cands[int(rng.integers(len(cands)))]
        b.need_panel(V, str(rng.choice(["hard", "float_rows", "has_gp"])))
        b.emit("demux_run", grid=g, full_ll=bool(rng.random() < 0.3))
        start = len(b.steps)
        while len(b.steps) - start < n_d:
            maybe_refused()
            b.need_pileup()
            Vc = b.m.panel[0] if b.m.panel else None
            here = sorted({hint_demux_path(Vc, g, flags) for g in GRIDS.values()}) if Vc else []
            if b.m.panel and rng.random() < 0.2 and b.m.grid is not None:   # the same samples, another mode, the same grid
                Vc, g0 = b.m.panel[0], b.m.grid
                modes = [q for q in ("hard", "has_gp", "float_rows") if q != b.m.panel[1]]
                b.need_panel(Vc, str(rng.choice(modes)))
                b.emit("demux_run", grid=g0, full_ll=False)
            elif here and rng.random() > dgroup:
                b.demux(here[int(rng.integers(len(here)))])
            else:
                b.demux(str(rng.choice(DEMUX_PATHS)))
            if b.m.panel and b.m.panel[0] > 255 and b.steps[-1]["op"] == "demux_run" and rng.random() < 0.3:
                b.emit("demux_run", grid=b.steps[-1]["grid"], full_ll=True)   # the streamed call keeps no tensor

    def estep_walk():
        b.estep(K=int(rng.choice([3, 16])), full_ll=bool(rng.random() < 0.3))
        start = len(b.steps)
        while len(b.steps) - start < n_e:
            maybe_refused()
            u = rng.random()
            if u < 0.08 and b.m.K >= 1:
                b.emit("fmx_cluster_pileup")
            elif u < 0.14 and b.m.K >= 1 and b.m.iters > 0 and not b.group:
                b.emit("iter_gp")   # the posteriors rewritten: the two tables of the last E-step are refused until the next
                b.emit("fmx_singlets")
                b.emit("fmx_inclusion")
            else:
                b.estep(K=int(rng.choice(CLUSTER_K)), full_ll=False)
                if b.m.K > 255 and rng.random() < 0.3:
                    b.emit("iterate", full_ll=True)   # the streamed E-step keeps no table to hand out

    def tables():
        if rng.random() < 0.5:
            b.need_panel()
            ts = [t for t in DEMUX_TABLES if rng.random() < 0.8]
            g = str(rng.choice(list(GRIDS)))
            for t in ts:
                b.emit(t, grid=g)
            if ts:
                b.emit("budget", name=BUDGETS[0], value=None if b.m.budget[BUDGETS[0]] else "1")
            for t in ts:
                b.emit(t, grid=g)
        else:
            ts = [t for t in FMX_TABLES if rng.random() < 0.8 and not (b.group and t in ("fmx_match_donors", "fmx_cluster_pairs"))]
            if "fmx_match_donors" in ts:
                b.need_panel()
            if b.m.K < 1 or b.m.iters == 0 or b.m.rewritten:
                b.estep(K=b.m.K if b.m.K >= 1 else None, full_ll=False)
            for t in ts:
                b.emit(t)
            if ts:
                b.emit("budget", name=BUDGETS[1], value=None if b.m.budget[BUDGETS[1]] else "1")
            for t in ts:
                b.emit(t)

    try:
        if rng.random() < 0.4:
            b.refused()   # before any pileup
        b.load(int(rng.choice([0, 2, 3])))
        parts = [demux_walk, estep_walk]
        if rng.random() < 0.5:
            parts.reverse()
        for part in parts:
            part()
            if rng.random() < 0.3:
                maybe_refused()
                b.load(int(rng.integers(4)))
        while True:
            u = rng.random()
            if u < 0.5:
                tables()
            elif u < 0.65:
                b.refused()
            elif u < 0.8:
                b.load(int(rng.integers(4)))
            elif u < 0.9:
                if b.m.grid is not None:
                    b.emit("demux_entry_pg")
                else:
                    b.demux(str(rng.choice(DEMUX_PATHS)))
            else:
                b.estep(K=int(rng.choice(CLUSTER_K)), full_ll=None)
    except _Full:
        pass
    if finish:
        b.limit = MAX_STEPS
        d, f = held_to_oracle(seed, flags, b.steps)
        if b.m.C() == 0:
            b.load(2)
        if not d:
            b.need_panel(8, "hard")
            b.emit("demux_run", grid="default", full_ll=False)
        if not f:
            b.estep(K=3, full_ll=False)
        try:   # what is left of the sixteen steps: more runs and iterations
            while True:
                if rng.random() < 0.6:
                    b.demux(str(rng.choice(DEMUX_PATHS)))
                else:
                    b.estep(K=int(rng.choice(CLUSTER_K)), full_ll=False)
        except _Full:
            pass
    return flags, _finish(b)


# ---- the eight constructed sequences: tours of the transitions the random ones reach too rarely -----------------------
def _tour(seed, flags, plan):
    b = _Builder(seed, flags, is_group(seed), np.random.default_rng([seed, 4105]))
    try:
        plan(b)
    except _Full:
        raise AssertionError(f"constructed sequence {seed} does not fit {MAX_STEPS} steps")
    return flags, _finish(b)


def _run(b, V, grid, mode="hard", full_ll=False):
    b.need_panel(V, mode)
    b.emit("demux_run", grid=grid, full_ll=full_ll)


# The sixteen ordered pairs of the four paths of 17..32 samples (oct16: default, row2: two, wave: six, tile: sng) are two
# walks of eight grid changes each, _c0 and _c1.
def _c0(b):
    b.load(2)
    for g in ("two", "default", "six", "default", "sng", "default", "default", "two", "two"):
        _run(b, 17, g)
    _run(b, 8, "default")
    b.estep(K=3)


def _c1(b):
    b.load(3)
    for g in ("two", "sng", "sng", "six", "six", "two", "six", "sng", "two"):
        _run(b, 32, g)
    _run(b, 16, "six")
    b.estep(K=16)


def _c2(b):   # the streamed call against the paths of few samples, V across 16, 32, 64 and 255 at once; stream -> oct E-step
    b.load(3)
    for V, g in ((300, "default"), (17, "default"), (300, "six"), (17, "sng"), (8, "default")):
        _run(b, V, g)
    b.estep(K=300, full_ll=False)
    b.estep(K=3)


def _esteps(b, Ks):
    for K in Ks:
        b.estep(K=K, full_ll=False)


def _c3(b):   # E-step paths on a plain handle: oct, row2 and the streamed one, each once more on itself
    b.load(2)
    _run(b, 1, "default")
    _esteps(b, (3, 3, 17, 17, 300))
    b.emit("iterate", full_ll=True)   # the streamed E-step has no table to hand out
    _esteps(b, (17,))


def _c4(b):   # MUXGL_FLAG_FORCE_ROW_KERNEL: K <= 16 takes the pair kernel; against itself, row2 and wave
    b.emit("fmx_match_donors")   # no pileup
    b.load(3)
    _run(b, 8, "default")
    _esteps(b, (3, 3, 17, 16, 33, 3))


def _c5(b):   # MUXGL_FLAG_FORCE_WAVE_KERNEL: 17 clusters take the pair kernel; against oct and the streamed E-step
    b.load(2)
    _run(b, 8, "default")
    _esteps(b, (3, 17, 16, 17, 300, 17))


def _c6(b):   # wave against oct, and what is left with the streamed one
    b.load(0)
    _run(b, 17, "six")
    _run(b, 16, "default", mode="has_gp")
    _esteps(b, (3, 33, 33, 16, 300, 300))


def _c7(b):   # what the donor match and the pair table refuse on a handle that is not ready; runs alternating between panels
    b.emit("fmx_cluster_pairs")   # no pileup
    b.load(2)
    b.emit("fmx_match_donors")    # not prepared
    b.emit("fmx_cluster_pairs")
    b.estep(K=16)
    b.emit("fmx_match_donors")    # this handle never had a panel
    for V, g in ((17, "default"), (8, "six"), (17, "six"), (8, "six")):
        _run(b, V, g)


CONSTRUCTED = ((0, _c0), (0, _c1), (0, _c2), (0, _c3), (FLAG_R, _c4), (FLAG_W, _c5), (0, _c6), (0, _c7))
# their seeds (which pileups, panels and starts they get): none a multiple of four, so all run on one device
CONSTRUCTED_SEEDS = (1000001, 1000002, 1000003, 1000005, 1000006, 1000007, 1000009, 1000010)


def constructed_seed(n):
    return CONSTRUCTED_SEEDS[n]


def sequence(seed):
    """the steps of a seed"""
    return sequence_and_flags(seed)[1]


def sequence_and_flags(seed):
    """(flags of the engine, steps)"""
    for n, (flags, plan) in enumerate(CONSTRUCTED):
        if seed == constructed_seed(n):
            return _tour(seed, flags, plan)
    return _random(seed)


# ---- what a set of sequences reaches ------------------------------------------------------------------------------------
V_MARKS, K_MARKS = (16, 32, 64, 255), (16, 32, 255)
TABLES = DEMUX_TABLES + FMX_TABLES


def required_coverage():
    """every item the seed list of tests/test_handle_sequences.py must reach (the list of the issue, as tuples)"""
    req = {("demux", a, b) for a in DEMUX_PATHS for b in DEMUX_PATHS}
    req |= {("estep", a, b) for a in ESTEP_PATHS for b in ESTEP_PATHS}
    req |= {("S", w) for w in ("grow", "shrink", "equal")} | {("C", w) for w in ("grow", "shrink", "zero")}
    req |= {("V", w, m) for w in ("up", "down") for m in V_MARKS} | {("K", w, m) for w in ("up", "down") for m in K_MARKS}
    req |= {("sums", "unit_to_other"), ("sums", "other_to_unit"), ("has_gp_only",), ("A", "up"), ("A", "down"),
            ("grid", "default_other_default"), ("job", "demux_after_fmx"), ("job", "fmx_after_demux"),
            ("stale", "load_without_panel_then_demux")}
    req |= {("budget", t) for t in TABLES}
    req |= {("refusal", k) for k in REFUSALS}
    return req


def coverage(seed, demux_path=None, estep_path=None):
    """The items of required_coverage() the sequence of `seed` reaches.  demux_path(V, grid, flags, pileup facts, full_ll)
    and estep_path(K, flags, pileup facts) name the kernel path of a step that runs with cells (default: the hints).
    Transitions are counted between steps that RAN, on the one handle of the sequence: consecutive demux_run steps,
    consecutive iterate steps, consecutive loads, consecutive panels that a demuxlet call used, consecutive
    set_clusters that an iterate used."""
    flags, seq = sequence_and_flags(seed)
    pl = pl_facts(seed)
    group = is_group(seed)
    if demux_path is None:
        demux_path = lambda V, grid, fl, facts, full: hint_demux_path(V, grid, fl)   # noqa: E731
    if estep_path is None:
        estep_path = lambda K, fl, facts: hint_estep_path(K, fl)   # noqa: E731
    got = set()
    last_run = None      # (path, A, grid name, panel, unit sums) of the last demux_run with cells
    runs_on_panel = []   # grid names of the runs since the last panel / load
    last_iter = None     # path of the last iterate with cells
    last_load = None
    used_panels, used_K = [], []   # (i, V, mode) / K, each once it served a call that ran
    last_job = None
    table_seen = {}      # table -> (model key, arguments, budget value) of its last running call
    stale = False        # a load came after a panel and no panel since
    unit = {}
    for st, why, m in replay(seq, pl, flags, group):
        op = st["op"]
        if why is not None:
            got.add(("refusal", why))
            if stale and op in ("demux_run",) + DEMUX_TABLES + ("demux_entry_pg", "fmx_match_donors"):
                got.add(("stale", "load_without_panel_then_demux"))
            continue
        if op == "load":
            if last_load is not None:
                (c0, s0), (c1, s1) = pl[last_load][:2], pl[st["i"]][:2]
                got.add(("S", "grow" if s1 > s0 else "shrink" if s1 < s0 else "equal"))
                if c1 == 0 and c0 > 0:
                    got.add(("C", "zero"))
                elif c1 != c0:
                    got.add(("C", "grow" if c1 > c0 else "shrink"))
            stale = False
            if last_load is not None and used_panels and used_panels[-1][0] == last_load and pl[st["i"]][1] < pl[last_load][1]:
                stale = True   # a panel was in force for the pileup that just went, and the new one is smaller
            last_load = st["i"]
            runs_on_panel = []
        elif op == "panel":
            stale = False
            runs_on_panel = []
        elif op in ("demux_run",) + DEMUX_TABLES + ("fmx_match_donors",):
            V, mode = m.panel
            p = (m.i, V, mode)
            if not used_panels or used_panels[-1] != p:
                if used_panels:
                    v0 = used_panels[-1][1]
                    for mark in V_MARKS:
                        if v0 <= mark < V:
                            got.add(("V", "up", mark))
                        if V <= mark < v0:
                            got.add(("V", "down", mark))
                    q = used_panels[-1]
                    if q[0] == p[0] and q[1] == p[1] and {q[2], p[2]} == {"hard", "has_gp"}:
                        got.add(("has_gp_only",))
                used_panels.append(p)
        if op == "demux_run" and m.C() > 0:
            V, mode = m.panel
            grid = GRIDS[st["grid"]]
            path = demux_path(V, grid, flags, pl[m.i], st["full_ll"])
            if p not in unit:   # (read between two runs of the oct kernels only: the others have one row format)
                unit[p] = panel_facts(*panel(seed, m.i, pl[m.i][1], V, mode))[0] if V <= 32 else None
            if last_run is not None:
                got.add(("demux", last_run[0], path))
                if len(grid) != last_run[1]:
                    got.add(("A", "up" if len(grid) > last_run[1] else "down"))
                if path in ("oct8", "oct16") and last_run[0] in ("oct8", "oct16") and unit[p] != last_run[4]:
                    got.add(("sums", "other_to_unit" if unit[p] else "unit_to_other"))
            runs_on_panel.append(st["grid"])
            if len(runs_on_panel) >= 3 and runs_on_panel[-3] == runs_on_panel[-1] == "default" != runs_on_panel[-2]:
                got.add(("grid", "default_other_default"))
            last_run = (path, len(grid), st["grid"], p, unit[p])
            if last_job == "fmx":
                got.add(("job", "demux_after_fmx"))
            last_job = "demux"
        if op == "iterate":
            if m.iters == 1:   # the first iteration of a set_clusters
                if used_K:
                    k0 = used_K[-1]
                    for mark in K_MARKS:
                        if k0 <= mark < m.K:
                            got.add(("K", "up", mark))
                        if m.K <= mark < k0:
                            got.add(("K", "down", mark))
                used_K.append(m.K)
            if m.C() > 0:
                path = estep_path(m.K, flags, pl[m.i])
                if last_iter is not None:
                    got.add(("estep", last_iter, path))
                last_iter = path
                if last_job == "demux":
                    got.add(("job", "fmx_after_demux"))
                last_job = "fmx"
        if op in TABLES:
            args = tuple(sorted((k, v) for k, v in st.items() if k not in ("op", "expect")))
            b = m.budget[TABLE_BUDGET[op]]
            seen = table_seen.get(op)
            if seen is not None and seen[0] == m.key() and seen[1] == args and seen[2] != b:
                got.add(("budget", op))
            table_seen[op] = (m.key(), args, b)
    return got
