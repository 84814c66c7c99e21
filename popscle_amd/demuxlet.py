"""Host-side driver of a sharded demuxlet run: one process per GPU, contiguous cell ranges balanced by entries, GP tensor
replicated, no data-path collective (cmd_cram_demuxlet.cpp:636-1013 has no cross-cell state); the per-cell records are
gathered once at the end.  The reference's own way to parallelise is the same cut at file level (`--group-list`,
README.md:168)."""
from __future__ import annotations

import numpy as np

from . import shard
from .freemuxlet import NoExchange


def top_samples(sng, n_top):
    """int32 [C][n_top]: the n_top best samples of every row of a singlet table [C][V], best first, ties to the lower
    index"""
    sng = np.asarray(sng, dtype=np.float64)
    order = np.argsort(-np.where(np.isnan(sng), -np.inf, sng), axis=1, kind="stable")
    return np.ascontiguousarray(order[:, :n_top], dtype=np.int32)


def call_pairs(records):
    """int32 [C][2][2]: per record of Engine.demux_run the pairs (dBest1, dBest2) and (sBest, sNext), each (-1, -1) where the
    record is not valid or either index is missing (negative): the slots Engine.demux_alpha_fit takes"""
    rec = np.asarray(records)
    out = np.full((rec.shape[0], 2, 2), -1, dtype=np.int32)
    for slot, (a, b) in enumerate((("dBest1", "dBest2"), ("sBest", "sNext"))):
        ok = (rec["valid"] != 0) & (rec[a] >= 0) & (rec[b] >= 0)
        out[ok, slot, 0] = rec[a][ok]
        out[ok, slot, 1] = rec[b][ok]
    return out


def merge_hists(parts):
    """(keys, counts) int64 of the read histograms `parts` (pairs of raw int64 bytes or arrays, as Engine.pileup_read_hist
    returns them) merged: keys ascending and unique, the counts of equal keys added (integers: exact in any order)"""
    ks = [np.frombuffer(k, dtype=np.int64) if isinstance(k, (bytes, bytearray)) else np.asarray(k, dtype=np.int64) for k, _ in parts]
    cs = [np.frombuffer(c, dtype=np.int64) if isinstance(c, (bytes, bytearray)) else np.asarray(c, dtype=np.int64) for _, c in parts]
    k = np.concatenate(ks) if ks else np.zeros(0, dtype=np.int64)
    c = np.concatenate(cs) if cs else np.zeros(0, dtype=np.int64)
    keys, inv = np.unique(k, return_inverse=True)
    counts = np.zeros(keys.size, dtype=np.int64)
    np.add.at(counts, inv, c)
    return keys, counts


def run_sharded(engine_factory, p, alphas=(0.0, 0.5), doublet_prior=0.5, exchange=None, want_singlets=False,
                want_inclusion=False, *, want_unknown=False, want_ambient=None, want_ambient_fit=None,
                want_alpha_fit=None, want_soup_mix=None):
    """engine_factory() -> object with set_pileup / demux_set_gp / demux_run (muxgl.Engine).  Returns the [C] records of
    the whole pileup on every rank, in the original cell order; with want_singlets also the [C][V] table of singlet
    log-likelihoods (Engine.demux_singlets), gathered the same way: (records, sng); with want_inclusion also the dict of
    per-droplet, per-sample inclusion tables (Engine.demux_inclusion): (records, [sng,] inclusion); with want_unknown
    (keyword only) also the dict of the three tables of Engine.demux_unknown (panel mean); with want_ambient = (amb_af,
    rhos) (keyword only) also the [C][V][n_rho] table of Engine.demux_ambient; with want_ambient_fit = (amb_af, rho_max,
    n_top) (keyword only) also the dict of Engine.demux_ambient_fit for the n_top best samples of every droplet's row of the
    singlet table (ties to the lower index) with those candidates under "cand" ([C][n_top]); with want_alpha_fit =
    (alpha_max,) (keyword only) also the dict of Engine.demux_alpha_fit for the two pairs of call_pairs() of every droplet
    with those pairs under "pair" ([C][2][2]); with want_soup_mix = (mask or None, with_unknown, n_iter_max, tol) (keyword
    only) also the dict of Engine.demux_soup_mix with the merged histogram under "hist", as the last element: every rank
    counts the reads of its own droplets, the histograms are gathered and merged (np.unique and an integer add), and every
    rank fits the same input, so all ranks hold the same bits.
    Cells are independent, so every rank fills the rows of its own cells."""
    ex = exchange or NoExchange()
    ranges = shard.cell_shards(p.cell_ptr, ex.world)
    c0, c1 = ranges[ex.rank]
    sub = shard.take_cells(p, c0, c1)
    eng = engine_factory()
    eng.set_pileup(sub.S, sub.cell_ptr, sub.entry_snp, sub.entry_rptr, sub.reads)
    eng.demux_set_gp(p.gp, p.has_gp)
    cells = eng.demux_run(alphas, doublet_prior)
    parts = ex.gather_objects((c0, c1, cells.tobytes()))
    out = np.zeros(p.C, dtype=cells.dtype)
    for b, e, raw in parts:
        out[b:e] = np.frombuffer(raw, dtype=cells.dtype)
    if not want_singlets and not want_inclusion and not want_unknown and want_ambient is None and want_ambient_fit is None \
            and want_alpha_fit is None and want_soup_mix is None:
        return out
    ret = [out]
    V = p.gp.shape[1]
    if want_singlets:
        sng = np.zeros((p.C, V), dtype=np.float64)
        for b, e, raw in ex.gather_objects((c0, c1, eng.demux_singlets(alphas).tobytes())):
            sng[b:e] = np.frombuffer(raw, dtype=np.float64).reshape(e - b, V)
        ret.append(sng)
    if want_inclusion:
        mine = eng.demux_inclusion(alphas, doublet_prior)
        inc = {k: np.zeros((p.C,) + v.shape[1:], dtype=v.dtype) for k, v in mine.items()}
        for b, e, raw in ex.gather_objects((c0, c1, {k: v.tobytes() for k, v in mine.items()})):
            for k, v in inc.items():
                v[b:e] = np.frombuffer(raw[k], dtype=v.dtype).reshape((e - b,) + v.shape[1:])
        ret.append(inc)
    if want_unknown:
        mine = {k: v for k, v in eng.demux_unknown(alphas).items() if k != "kernel_ms"}
        unk = {k: np.zeros((p.C,) + v.shape[1:], dtype=v.dtype) for k, v in mine.items()}
        for b, e, raw in ex.gather_objects((c0, c1, {k: v.tobytes() for k, v in mine.items()})):
            for k, v in unk.items():
                v[b:e] = np.frombuffer(raw[k], dtype=v.dtype).reshape((e - b,) + v.shape[1:])
        ret.append(unk)
    if want_ambient is not None:
        amb_af, rhos = want_ambient
        amb = np.zeros((p.C, V, len(rhos)), dtype=np.float64)
        for b, e, raw in ex.gather_objects((c0, c1, eng.demux_ambient(alphas, amb_af, rhos)["ll"].tobytes())):
            amb[b:e] = np.frombuffer(raw, dtype=np.float64).reshape(e - b, V, len(rhos))
        ret.append(amb)
    if want_ambient_fit is not None:
        amb_af, rho_max, n_top = want_ambient_fit
        n_top = min(int(n_top), V)
        cand = top_samples(eng.demux_singlets(alphas), n_top)
        mine = {k: v for k, v in eng.demux_ambient_fit(alphas, amb_af, cand, rho_max).items() if k != "kernel_ms"}
        mine["cand"] = cand
        fit = {k: np.zeros((p.C, n_top), dtype=v.dtype) for k, v in mine.items()}
        for b, e, raw in ex.gather_objects((c0, c1, {k: v.tobytes() for k, v in mine.items()})):
            for k, v in fit.items():
                v[b:e] = np.frombuffer(raw[k], dtype=v.dtype).reshape(e - b, n_top)
        ret.append(fit)
    if want_alpha_fit is not None:
        (alpha_max,) = want_alpha_fit
        got = eng.demux_alpha_fit(alphas, call_pairs(cells), alpha_max)
        mine = {k: got[k] for k in eng.ALPHA_FIT_FIELDS + ("pair",)}
        fit = {k: np.zeros((p.C,) + v.shape[1:], dtype=v.dtype) for k, v in mine.items()}
        for b, e, raw in ex.gather_objects((c0, c1, {k: v.tobytes() for k, v in mine.items()})):
            for k, v in fit.items():
                v[b:e] = np.frombuffer(raw[k], dtype=v.dtype).reshape((e - b,) + v.shape[1:])
        fit["alpha_max"] = float(alpha_max)
        ret.append(fit)
    if want_soup_mix is not None:
        mask, with_unknown, n_iter_max, tol = want_soup_mix
        if mask is not None:
            mask = np.asarray(mask)[c0:c1]
        keys, counts = merge_hists(ex.gather_objects(tuple(a.tobytes() for a in eng.pileup_read_hist(mask))))
        mix = eng.demux_soup_mix(hist=(keys, counts), with_unknown=with_unknown, n_iter_max=n_iter_max, tol=tol)
        mix["hist"] = (keys, counts)
        ret.append(mix)
    return tuple(ret)
