"""ctypes binding of libmuxgl.so (include/muxgl.h).

This is plumbing: it loads the in-tree shared library, mirrors the C structs as numpy dtypes and checks return
codes.  There is no Python or CPU implementation of the hot path behind it -- if the library is missing, or no HIP
device is usable, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MUXGL_LIB") or os.path.join(HERE, "lib", "libmuxgl.so")  # (MUXGL_LIB: kernel experiments)

MAX_ALPHA = 16
READ_OTHER = 0xFF
SNG, DBL, AMB = 0, 1, 2
TYPE_NAMES = {SNG: "SNG", DBL: "DBL", AMB: "AMB"}

# timing slots of muxgl_get_timing
T_DEMUX_REDUCE, T_DEMUX_SWEEP, T_DEMUX_CALL, T_DEMUX_D2H = 0, 1, 2, 3
FLAG_FORCE_TILE_SWEEP = 1
FLAG_FORCE_ROW_KERNEL = 2
FLAG_FORCE_WAVE_KERNEL = 4
FLAG_FORCE_BATCHED_GREEDY = 8
FLAG_DEMUX_ONLY = 16
FLAG_ASYNC_PHASES = 32
FLAG_NO_LINEAR_ENTRIES = 64
FLAG_NO_PIVOT_SUMS = 256
FLAG_SPLIT_GENERAL_SWEEP = 512
FLAG_GROUP_PROBE_SELF = 1024
FLAG_FORCE_STREAMED_CALL = 2048
FLAG_FORCE_STREAMED_ESTEP = 4096
ANCHOR_HELD, ANCHOR_PRIOR = 0, 1  # modes of an anchored cluster (MUXGL_ANCHOR_*)
MAX_CLUSTERS = 1024  # freemuxlet: largest K (MUXGL_MAX_CLUSTERS)
MAX_DEVICES = 16
XCHG_PAD = 64
T_FMX_ENTRY, T_FMX_GP, T_FMX_ESTEP, T_FMX_CALL, T_FMX_MSTEP = 4, 5, 6, 7, 8
T_FMXOLD_PAIR, T_FMXOLD_VOTE = 9, 10
T_FMX_ESTEP_SWEEP = 11
T_DEMUX_SINGLETS = 12
T_DEMUX_INCLUSION = 14
T_FMX_SINGLETS = 13
T_FMX_INCLUSION = 15
T_COUNT = 16
BUF_CGP, BUF_CLUST, BUF_CELLS, BUF_STAT = 0, 1, 2, 3

DEMUX_CELL = np.dtype(
    [(n, np.int32) for n in ("valid", "nsnps", "type", "next_type", "sBest", "sNext", "dBest1", "dBest2", "dBestA",
                             "dNext1", "dNext2", "dNextA", "jBest", "kBest", "aBest", "jNext", "kNext", "aNext")]
    + [(n, np.float64) for n in ("sngBestLLK", "sngNextLLK", "dblBestLLK", "dblNextLLK", "sumLLK", "sngLLK",
                                 "bestLLK", "nextLLK", "bestPP", "sngPP", "sngOnlyPP")],
    align=True,
)
CELL_DEEP_SNG, CELL_DEEP_DBL = 2, 4   # bits of DEMUX_CELL["valid"] next to bit 0 (include/muxgl.h)
FMX_CELL = np.dtype(
    [(n, np.int32) for n in ("type", "clust", "jBest", "kBest", "jNext", "kNext", "sBest", "sNext", "dBest1",
                             "dBest2", "dNext1", "dNext2")]
    + [(n, np.float64) for n in ("bestLLK", "nextLLK", "sngBestLLK", "sngNextLLK", "dblBestLLK", "dblNextLLK",
                                 "bestPP", "sngPP", "sngOnlyPP", "sumLLK", "sngThirdLLK", "dblThirdLLK")],
    align=True,
)
DROPD = np.dtype([("nsnps", np.int32), ("nread1", np.int32), ("nread2", np.int32), ("_pad", np.int32),
                  ("llk0", np.float64), ("llk2", np.float64)], align=True)
assert DROPD.itemsize == 32
assert DEMUX_CELL.itemsize == 18 * 4 + 11 * 8
assert FMX_CELL.itemsize == 12 * 4 + 12 * 8


class _Config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device_id", C.c_int32), ("flags", C.c_int32), ("n_devices", C.c_int32),
                ("device_ids", C.c_int32 * MAX_DEVICES)]


class _DemuxParams(C.Structure):
    _fields_ = [("n_alpha", C.c_int32), ("_pad", C.c_int32), ("alpha", C.c_double * MAX_ALPHA),
                ("doublet_prior", C.c_double)]


def _demux_params(alphas, doublet_prior=0.5):
    """the muxgl_demux_params of an alpha sequence (doublet_prior: 0.5 where the call does not read it)"""
    if len(alphas) > MAX_ALPHA:
        raise ValueError("too many alphas")
    p = _DemuxParams()
    p.n_alpha = len(alphas)
    for i, a in enumerate(alphas):
        p.alpha[i] = float(a)
    p.doublet_prior = float(doublet_prior)
    return p


class _FmxParams(C.Structure):
    _fields_ = [("doublet_prior", C.c_double), ("geno_error", C.c_double)]


# every symbol include/muxgl.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
SYMBOLS = {
    "muxgl_version": (C.c_int, []),
    "muxgl_group_peer_stats": (C.c_int, [_VP, _VP]),
    "muxgl_create": (C.c_int, [C.POINTER(_Config), C.POINTER(_VP)]),
    "muxgl_destroy": (None, [_VP]),
    "muxgl_last_error": (C.c_char_p, [_VP]),
    "muxgl_set_pileup": (C.c_int, [_VP, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _VP, _VP, _VP, _VP]),
    "muxgl_demux_set_gp": (C.c_int, [_VP, C.c_int32, _VP, _VP]),
    "muxgl_demux_run": (C.c_int, [_VP, C.POINTER(_DemuxParams), _VP, _VP]),
    "muxgl_demux_singlets": (C.c_int, [_VP, C.POINTER(_DemuxParams), _VP]),
    "muxgl_demux_inclusion": (C.c_int, [_VP, C.POINTER(_DemuxParams), _VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_demux_unknown": (C.c_int, [_VP, C.POINTER(_DemuxParams), _VP, _VP, _VP, _VP, _VP]),
    "muxgl_demux_ambient": (C.c_int, [_VP, C.POINTER(_DemuxParams), _VP, C.c_int32, _VP, _VP, _VP]),
    "muxgl_pileup_allele_counts": (C.c_int, [_VP, _VP, _VP, _VP]),
    "muxgl_pileup_read_hist": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _VP]),
    "muxgl_demux_soup_mix": (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP, C.c_int32, _VP, _VP, C.c_int32, C.c_double,
                                       _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_demux_ambient_fit": (C.c_int, [_VP, C.POINTER(_DemuxParams), _VP, C.c_int32, _VP, C.c_double,
                                          _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_demux_alpha_fit": (C.c_int, [_VP, C.POINTER(_DemuxParams), C.c_int32, _VP, C.c_double,
                                        _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_demux_results": (_VP, [_VP]),
    "muxgl_demux_oct_split": (C.c_int, [_VP, _VP]),
    "muxgl_demux_exact_calls": (C.c_int, [C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                          C.POINTER(_DemuxParams), _VP, C.c_int32, _VP]),
    "muxgl_demux_get_entry_pg": (C.c_int, [_VP, _VP]),
    "muxgl_fmx_prepare": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_get_entry_gls": (C.c_int, [_VP, _VP, _VP]),
    "muxgl_fmx_greedy_init": (C.c_int, [_VP, C.c_int32, _VP, C.c_double, C.c_double, _VP]),
    "muxgl_fmx_greedy_stats": (C.c_int, [_VP, _VP, _VP]),
    "muxgl_fmx_score_stats": (C.c_int, [_VP, _VP]),
    "muxgl_fmx_set_clusters": (C.c_int, [_VP, C.c_int32, _VP]),
    "muxgl_fmx_set_anchors": (C.c_int, [_VP, C.c_int32, _VP]),
    "muxgl_fmx_set_anchors_mode": (C.c_int, [_VP, C.c_int32, _VP, _VP]),
    "muxgl_fmx_get_cluster_gp": (C.c_int, [_VP, C.c_int32, C.c_int32, _VP]),
    "muxgl_fmx_iterate": (C.c_int, [_VP, C.POINTER(_FmxParams), _VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_singlets": (C.c_int, [_VP, _VP]),
    "muxgl_fmx_inclusion": (C.c_int, [_VP, C.POINTER(_FmxParams), _VP, _VP, _VP, _VP]),
    "muxgl_fmx_unknown": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_ambient": (C.c_int, [_VP, _VP, C.c_int32, _VP, _VP, _VP]),
    "muxgl_fmx_ambient_fit": (C.c_int, [_VP, _VP, C.c_int32, _VP, C.c_double, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_alpha_fit": (C.c_int, [_VP, C.c_int32, _VP, C.c_double, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_get_cluster_pileup": (C.c_int, [_VP, _VP, _VP]),
    "muxgl_fmx_match_donors": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_cluster_pairs": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_exact_stats": (C.c_int, [_VP, _VP, _VP, _VP]),
    "muxgl_fmx_exact_pending": (C.c_int, [_VP, _VP]),
    "muxgl_fmx_exact_hint": (C.c_int, [_VP, C.c_int32]),
    "muxgl_fmx_exact_snps": (C.c_int, [_VP, _VP, C.c_int64, _VP]),
    "muxgl_fmx_exact_rows": (C.c_int, [_VP, C.POINTER(_FmxParams), _VP, C.c_int64, _VP, _VP]),
    "muxgl_fmx_exact_finish": (C.c_int, [_VP, C.POINTER(_FmxParams), _VP, C.c_int64, _VP, _VP, _VP]),
    "muxgl_fmxold_pair_dist": (C.c_int, [_VP, C.c_double, _VP]),
    "muxgl_fmxold_get_signs": (C.c_int, [_VP, _VP]),
    "muxgl_fmxold_vote_init": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_double, _VP, _VP]),
    "muxgl_fmxold_vote_refine": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int32, _VP, _VP, _VP]),
    "muxgl_fmx_set_column_slab": (C.c_int, [_VP, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _VP, _VP,
                                            _VP, _VP]),
    "muxgl_fmx_set_shard": (C.c_int, [_VP, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "muxgl_fmx_iter_gp": (C.c_int, [_VP, C.POINTER(_FmxParams)]),
    "muxgl_fmx_iter_estep": (C.c_int, [_VP, C.POINTER(_FmxParams)]),
    "muxgl_fmx_iter_mstep": (C.c_int, [_VP]),
    "muxgl_fmx_iter_fetch": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "muxgl_fmx_buffer": (C.c_int, [_VP, C.c_int32, C.POINTER(_VP), C.POINTER(C.c_int64)]),
    "muxgl_memcpy_dev": (C.c_int, [_VP, _VP, _VP, C.c_int64]),
    "muxgl_stream": (_VP, [_VP]),
    "muxgl_get_timing": (C.c_int, [_VP, _VP]),
    "muxgl_get_timing_sum": (C.c_int, [_VP, _VP, _VP, C.c_int32]),
}

_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen libmuxgl.so and attach prototypes.  Raises if the in-tree build is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build it with `python -m popscle_amd.build` (hipcc, gfx950); "
                           "there is no fallback implementation")
    lib = C.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


class MuxglError(RuntimeError):
    pass


FMX_UNKNOWN_FIELDS = ("ll_ju", "ll_u", "ll_uu")  # the outputs of muxgl_fmx_unknown, in the order of its arguments
EXACT_STATS = ("cells", "mirror_turned", "mirror_exact_ties", "near_ties", "deep", "changed")


def demux_exact_calls(p, alphas, cells, doublet_prior=0.5, nthreads=0):
    """muxgl_demux_exact_calls: the host pass (no device) that settles, in the reference's own arithmetic, every call of
    `cells` (records of demux_run over pileup p, modified in place) that rounding noise could decide: the order of a
    mirrored alpha = 0.5 pair (cmd_cram_demuxlet.cpp:738-746,883-906) and the near ties of the scans and thresholds
    (:827-837,925-988).  Returns a dict of the six counters (EXACT_STATS)."""
    lib = load_library()
    dp = _DemuxParams()
    dp.n_alpha = len(alphas)
    for i, a in enumerate(alphas):
        dp.alpha[i] = float(a)
    dp.doublet_prior = float(doublet_prior)
    cell_ptr = _arr(p.cell_ptr, np.int64, "cell_ptr")
    entry_snp = _arr(p.entry_snp, np.int32, "entry_snp")
    entry_rptr = _arr(p.entry_rptr, np.int64, "entry_rptr")
    reads = _arr(p.reads, np.uint8, "reads")
    gp = _arr(p.gp, np.float64, "gp")
    has_gp = _arr(p.has_gp, np.uint8, "has_gp")
    if cells.dtype != DEMUX_CELL or not cells.flags.c_contiguous or cells.shape != (cell_ptr.size - 1,):
        raise ValueError("cells must be the contiguous [C] record array demux_run returned")
    stats = np.zeros(len(EXACT_STATS), dtype=np.int64)
    rc = lib.muxgl_demux_exact_calls(cell_ptr.size - 1, gp.shape[1], _ptr(cell_ptr), _ptr(entry_snp), _ptr(entry_rptr),
                                     _ptr(reads), _ptr(gp), _ptr(has_gp), C.byref(dp), _ptr(cells),
                                     int(nthreads) if nthreads else (os.cpu_count() or 1), _ptr(stats))
    if rc != 0:
        raise MuxglError(f"muxgl_demux_exact_calls failed ({rc})")
    return dict(zip(EXACT_STATS, (int(x) for x in stats)))


def singlet_posteriors(sng):
    """Per-sample posteriors of a [C][V] table of singlet log-likelihoods (Engine.demux_singlets; per-cluster ones of
    Engine.fmx_singlets' [C][K] table the same way) as the reference's
    disabled .sing2 writer forms them (cmd_cram_demuxlet.cpp:848): equal priors over the samples, i.e. a softmax over
    each row, computed with the row maximum subtracted.  A row of zeros (droplet without entries) gives 1 / V."""
    sng = np.asarray(sng, dtype=np.float64)
    if sng.ndim != 2:
        raise ValueError("sng must be [C][V]")
    if sng.shape[1] == 0:
        return np.zeros_like(sng)
    ex = np.exp(sng - sng.max(axis=1, keepdims=True))
    return ex / ex.sum(axis=1, keepdims=True)


def unknown_summary(tables, alphas):
    """Per droplet, the best hypotheses with a donor that is not in the panel, from the tables of Engine.demux_unknown
    (dict with ju, uj [C][V][A] and uu [C][A]).  Pure numpy.  Returns a dict of [C] arrays:
    uu_sng = uu[:, 0]; uu_dbl, uu_alpha_idx: the maximum of uu[:, n >= 1] and its n, first n on ties (-1e300 and -1 when
    the grid has one alpha); half_llk, half_sample, half_alpha_idx, half_known_major: the best hypothesis with one panel
    sample -- the candidates are (j, n >= 1, ju), sample j with share 1 - alpha[n] (half_known_major = 1), and
    (k, n >= 1, uj) only where alpha[n] != 0.5 (half_known_major = 0; at 0.5 it is the same hypothesis as ju, the
    reference's k < j rule for mirrored pairs, cmd_cram_demuxlet.cpp:812-815).  Ties: value descending, then (sample, n,
    ju before uj) ascending.  -1e300 and -1 where there is no candidate."""
    ju = np.asarray(tables["ju"], dtype=np.float64)
    uj = np.asarray(tables["uj"], dtype=np.float64)
    uu = np.asarray(tables["uu"], dtype=np.float64)
    al = np.asarray(alphas, dtype=np.float64)
    A = al.size
    if ju.ndim != 3 or ju.shape != uj.shape or uu.shape != (ju.shape[0], A) or ju.shape[2] != A or A < 1:
        raise ValueError("tables must be ju, uj [C][V][A] and uu [C][A] with A = len(alphas)")
    Cn, V = ju.shape[:2]
    out = {"uu_sng": uu[:, 0].copy(), "uu_dbl": np.full(Cn, -1e300), "uu_alpha_idx": np.full(Cn, -1, dtype=np.int32),
           "half_llk": np.full(Cn, -1e300), "half_sample": np.full(Cn, -1, dtype=np.int32),
           "half_alpha_idx": np.full(Cn, -1, dtype=np.int32), "half_known_major": np.full(Cn, -1, dtype=np.int32)}
    if A < 2 or Cn == 0:
        return out
    k = np.argmax(uu[:, 1:], axis=1)  # (first maximum)
    out["uu_alpha_idx"][:] = k + 1
    out["uu_dbl"][:] = uu[np.arange(Cn), k + 1]
    # candidates in tie order: sample, then n, then ju before uj
    cand = np.stack([ju[:, :, 1:], np.where(al[1:] != 0.5, uj[:, :, 1:], -np.inf)], axis=3).reshape(Cn, -1)
    cand = np.where(np.isnan(cand), -np.inf, cand)
    if cand.shape[1]:
        b = np.argmax(cand, axis=1)
        v = cand[np.arange(Cn), b]
        some = v > -np.inf
        out["half_llk"][some] = v[some]
        out["half_sample"][some] = (b // (2 * (A - 1)))[some]
        out["half_alpha_idx"][some] = ((b // 2) % (A - 1) + 1)[some]
        out["half_known_major"][some] = (1 - b % 2)[some]
    return out


def ambient_profile(n_ref, n_alt, af):
    """The ALT fraction of the pool's free-floating RNA per marker, from the read counts of Engine.pileup_allele_counts and
    the population ALT frequency af: (n_alt + af) / (n_ref + n_alt + 1), i.e. one pseudo-read at the population
    frequency, so a marker nobody covered falls back to af.  float64 [S], in [0, 1] wherever af is."""
    n_ref = np.asarray(n_ref, dtype=np.float64)
    n_alt = np.asarray(n_alt, dtype=np.float64)
    af = np.asarray(af, dtype=np.float64)
    if n_ref.shape != n_alt.shape or af.shape != n_ref.shape or n_ref.ndim != 1:
        raise ValueError("n_ref, n_alt and af must be [S]")
    return (n_alt + af) / (n_ref + n_alt + 1.0)


def soup_mix_summary(fit, names=None):
    """What a caller reads off the dict of Engine.demux_soup_mix.  Pure numpy.  Returns a dict: order, the components by
    share descending (ties to the lower index); shares, pi in that order; names, the components' names in that order where
    `names` is given (the panel's sample ids; component V is "UNKNOWN"); ll_gain, the last evaluated LL minus the LL at
    the start (>= 0 for an EM run, 0 with n_iter_max == 0); max_grad_dev, the largest |grad - 1| over the components with
    pi > 0 (0 at a maximum of the likelihood; NaN where no record took part)."""
    pi = np.asarray(fit["pi"], dtype=np.float64)
    grad = np.asarray(fit["grad"], dtype=np.float64)
    ll = np.asarray(fit["ll"], dtype=np.float64)
    order = np.argsort(-pi, kind="stable")
    seen = ll[~np.isnan(ll)]
    on = pi > 0.0
    out = {"order": order.astype(np.int32), "shares": pi[order],
           "ll_gain": float(seen[-1] - seen[0]) if seen.size else 0.0,
           "max_grad_dev": float(np.abs(grad[on] - 1.0).max()) if on.any() and fit.get("status", 0) != 2 else float("nan")}
    if names is not None:
        names = list(names)
        if len(names) == pi.size - 1:
            names.append("UNKNOWN")
        if len(names) != pi.size:
            raise ValueError("names must name every component")
        out["names"] = [names[i] for i in order]
    return out


def ambient_summary(ll, rhos):
    """Per droplet, the best "one cell of sample j plus a share rho of ambient RNA" hypothesis of the table of
    Engine.demux_ambient (ll float64 [C][V][n_rho]).  Pure numpy.  Returns a dict of [C] arrays: amb_llk, amb_sample,
    amb_rho_idx, amb_rho: the maximum over (sample, rho index), ties decided by value descending, then (sample, rho index)
    ascending; base_llk, base_sample: the maximum at the smallest rho (the first of them on ties) alone, for comparison --
    the singlet call where that rho is 0.  The rho of a droplet is the best point of the grid `rhos`;
    Engine.demux_ambient_fit estimates it."""
    ll = np.asarray(ll, dtype=np.float64)
    rh = np.asarray(rhos, dtype=np.float64)
    if ll.ndim != 3 or rh.ndim != 1 or ll.shape[2] != rh.size or rh.size < 1 or ll.shape[1] < 1:
        raise ValueError("ll must be [C][V][n_rho] with V >= 1 and n_rho = len(rhos) >= 1")
    Cn, V, NR = ll.shape
    flat = ll.reshape(Cn, V * NR)
    flat = np.where(np.isnan(flat), -np.inf, flat)
    b = np.argmax(flat, axis=1)  # (first maximum in (sample, rho index) order)
    ar = np.arange(Cn)
    r0 = int(np.argmin(rh))  # (first smallest)
    base = flat.reshape(Cn, V, NR)[:, :, r0]
    bs = np.argmax(base, axis=1)
    return {"amb_llk": flat[ar, b], "amb_sample": (b // NR).astype(np.int32), "amb_rho_idx": (b % NR).astype(np.int32),
            "amb_rho": rh[b % NR] if Cn else np.zeros(0), "base_llk": base[ar, bs], "base_sample": bs.astype(np.int32)}


def ambient_fit_summary(fit):
    """What a caller reads off the dict of Engine.demux_ambient_fit.  Pure numpy.  Returns a dict of arrays of the shape of
    fit["rho_hat"]: se, the standard error info ** -0.5 of rho_hat where status is 0 and info > 0 and NaN elsewhere (an
    estimate on a bound, status 1 or 2, has no standard error), and lrt, the likelihood ratio 2 * (ll_hat - ll_zero)
    against rho = 0 (0 where the slot was skipped or the droplet has no scored entry)."""
    info = np.asarray(fit["info"], dtype=np.float64)
    status = np.asarray(fit["status"])
    ok = (status == 0) & (info > 0.0)
    se = np.full(info.shape, np.nan)
    se[ok] = 1.0 / np.sqrt(info[ok])
    lrt = 2.0 * (np.asarray(fit["ll_hat"], dtype=np.float64) - np.asarray(fit["ll_zero"], dtype=np.float64))
    return {"se": se, "lrt": lrt}


def alpha_fit_summary(fit):
    """What a caller reads off the dict of Engine.demux_alpha_fit (with its "pair" and "alpha_max").  Pure numpy.  Returns a
    dict of arrays of the shape of fit["alpha_hat"]: se, the standard error info ** -0.5 of alpha_hat where status is 0 and
    info > 0 and NaN elsewhere (an estimate on a bound has no standard error); lrt, the likelihood ratio
    2 * (ll_hat - max(ll_zero, ll_top)) against the better of the two samples alone where alpha_max is 1 (ll_top is then
    the second sample alone) and 2 * (ll_hat - ll_zero) against the first alone where it is smaller; major, int32, the
    sample of the pair that holds the larger share: the second where alpha_hat > 0.5, else the first (-1 where the slot
    was skipped)."""
    info = np.asarray(fit["info"], dtype=np.float64)
    status = np.asarray(fit["status"])
    ok = (status == 0) & (info > 0.0)
    se = np.full(info.shape, np.nan)
    se[ok] = 1.0 / np.sqrt(info[ok])
    one = np.asarray(fit["ll_zero"], dtype=np.float64)
    if float(fit.get("alpha_max", 1.0)) == 1.0:
        one = np.maximum(one, np.asarray(fit["ll_top"], dtype=np.float64))
    lrt = 2.0 * (np.asarray(fit["ll_hat"], dtype=np.float64) - one)
    pair = np.asarray(fit["pair"]).reshape(info.shape + (2,))
    major = np.where(np.asarray(fit["alpha_hat"]) > 0.5, pair[..., 1], pair[..., 0]).astype(np.int32)
    return {"se": se, "lrt": lrt, "major": major}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_VP)


def _arr(a, dtype, name):
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.dtype != np.dtype(dtype):
        raise TypeError(name)
    return a


_NO_AF = object()  # _fit: the call takes no amb_af


def _fit(eng, fn, fields, want, params, amb_af, slots, pair, x_max):
    """What the three fit methods of Engine share: the library's fn(handle, [params,] [amb_af,] n_cand, slots, x_max, one
    pointer per field (NULL where not wanted), &kernel_ms).  slots: int32 [C][n_cand] (or [C]) candidates, or with `pair`
    [C][n_cand][2] (or [C][2]) pairs, which the dict then holds under "pair".  params None: the call takes none; amb_af
    _NO_AF likewise."""
    unknown = set(want) - set(fields)
    if unknown:
        raise ValueError(f"unknown fields {sorted(unknown)}")
    head = [] if params is None else [C.byref(params)]
    if amb_af is not _NO_AF:
        amb_af = _arr(amb_af, np.float64, "amb_af")
        if amb_af.shape != (eng.S,):
            raise ValueError("amb_af must be [S]")
        head.append(_ptr(amb_af))
    name, last = ("pairs", (2,)) if pair else ("cand", ())
    slots = _arr(slots, np.int32, name)
    if slots.ndim == 1 + len(last):
        slots = slots.reshape((-1, 1) + last)
    if slots.ndim != 2 + len(last) or slots.shape[0] != eng.C or slots.shape[2:] != last:
        raise ValueError(f"{name} must be [C][n_cand]" + "[2]" * len(last))
    out = {n: np.zeros(slots.shape[:2], dtype=np.int32 if n in ("status", "n_steps") else np.float64)
           for n in fields if n in want}
    ms = C.c_float(0.0)
    eng._check(getattr(eng.lib, fn)(eng.h, *head, slots.shape[1], _ptr(slots), float(x_max), *[_ptr(out.get(n)) for n in fields],
                                    C.byref(ms)))
    if pair:
        out["pair"] = slots
    out["kernel_ms"] = float(ms.value)
    return out


class Engine:
    """One muxgl handle: one GPU (device_id an int) or a device group (a list of device ordinals; the same ordinal may
    appear more than once = virtual ranks on one GPU).  Methods mirror the C-ABI one to one."""

    def __init__(self, device_id=0, flags: int = 0):
        self.lib = load_library()
        self.h = _VP()
        cfg = _Config()
        cfg.struct_size = C.sizeof(_Config)
        cfg.flags = flags
        if isinstance(device_id, (list, tuple)):
            if not 1 <= len(device_id) <= MAX_DEVICES:
                raise ValueError("1..MAX_DEVICES device ordinals")
            cfg.n_devices = len(device_id)
            for i, d in enumerate(device_id):
                cfg.device_ids[i] = int(d)
            cfg.device_id = int(device_id[0])
        else:
            cfg.device_id = int(device_id)
        if self.lib.muxgl_create(C.byref(cfg), C.byref(self.h)) != 0:
            raise MuxglError(self.lib.muxgl_last_error(None).decode())
        self.C = self.S = self.nnz = self.R = 0
        self.C_total = 0   # slabbed handle: cells of the whole job
        self.cell_base = 0
        self.V = 0
        self.K = 0
        self.n_anchor = 0  # clusters 0 .. n_anchor-1 are held to donors of the panel (fmx_set_anchors)
        self._anchor_modes = ()  # their modes (anchor_modes)
        self.n_alpha = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.muxgl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MuxglError(self.lib.muxgl_last_error(self.h).decode())

    # ---- pileup
    def set_pileup(self, S, cell_ptr, entry_snp, entry_rptr, reads):
        cell_ptr = _arr(cell_ptr, np.int64, "cell_ptr")
        entry_snp = _arr(entry_snp, np.int32, "entry_snp")
        entry_rptr = _arr(entry_rptr, np.int64, "entry_rptr")
        reads = _arr(reads, np.uint8, "reads")
        C_ = cell_ptr.size - 1
        nnz = entry_snp.size
        R = reads.size
        if entry_rptr.size != nnz + 1:
            raise ValueError("entry_rptr must have nnz+1 elements")
        self._check(self.lib.muxgl_set_pileup(self.h, C_, int(S), nnz, R, _ptr(cell_ptr), _ptr(entry_snp),
                                               _ptr(entry_rptr), _ptr(reads)))
        self.C, self.S, self.nnz, self.R = C_, int(S), nnz, R
        self.C_total, self.cell_base = C_, 0
        self.V = self.K = self.n_alpha = 0   # the library drops the panel, the last grid and the clusters with the pileup
        self.n_anchor = 0

    def fmx_set_column_slab(self, C_total, c0, s0, s1, cell_ptr, entry_snp, entry_rptr, reads):
        """attach the column slab (all C_total cells, entries with s0 <= SNP < s1) to a handle holding a row slab"""
        cell_ptr = _arr(cell_ptr, np.int64, "cell_ptr")
        entry_snp = _arr(entry_snp, np.int32, "entry_snp")
        entry_rptr = _arr(entry_rptr, np.int64, "entry_rptr")
        reads = _arr(reads, np.uint8, "reads")
        if cell_ptr.size != int(C_total) + 1 or entry_rptr.size != entry_snp.size + 1:
            raise ValueError("column slab: cell_ptr must have C_total+1 and entry_rptr nnz+1 elements")
        self._check(self.lib.muxgl_fmx_set_column_slab(self.h, int(C_total), int(c0), int(s0), int(s1), entry_snp.size,
                                                        reads.size, _ptr(cell_ptr), _ptr(entry_snp), _ptr(entry_rptr),
                                                        _ptr(reads)))
        self.C_total, self.cell_base = int(C_total), int(c0)
        self.n_anchor = 0

    def stream(self):
        """the hipStream_t (as an integer) the handle's kernels are enqueued on"""
        return self.lib.muxgl_stream(self.h)

    # ---- demuxlet
    def demux_set_gp(self, gp, has_gp):
        gp = _arr(gp, np.float64, "gp")
        has_gp = _arr(has_gp, np.uint8, "has_gp")
        if gp.ndim != 3 or gp.shape[0] != self.S or gp.shape[2] != 3 or has_gp.shape != (self.S,):
            raise ValueError("gp must be [S][V][3] and has_gp [S]")
        self._check(self.lib.muxgl_demux_set_gp(self.h, gp.shape[1], _ptr(gp), _ptr(has_gp)))
        self.V = gp.shape[1]
        self.n_alpha = 0   # (demux_entry_pg wants a run on this panel)
        self.n_anchor = 0  # (the anchors indexed the panel that went)

    def demux_run(self, alphas=(0.0, 0.5), doublet_prior=0.5, want_cells=True, want_full_ll=False):
        key = (tuple(alphas), float(doublet_prior))
        if getattr(self, "_dp_key", None) != key:  # (the struct of the last call is kept: a tight loop re-uses it)
            self._dp, self._dp_key = _demux_params(alphas, doublet_prior), key
        p = self._dp
        out = np.zeros(self.C, dtype=DEMUX_CELL) if want_cells else None
        full = np.zeros((self.C, self.V, self.V, len(alphas)), dtype=np.float64) if want_full_ll else None
        self._check(self.lib.muxgl_demux_run(self.h, C.byref(p), _ptr(out), _ptr(full)))
        self.n_alpha = len(alphas)
        if want_full_ll:
            return out, full
        return out

    def demux_singlets(self, alphas=(0.0, 0.5)):
        """muxgl_demux_singlets: float64 [C][V], the singlet log-likelihood llksAB[(j, 0, 0)] of every droplet against
        every sample (full_ll[:, :, 0, 0] where that tensor exists), at any V, without a previous demux_run.  The grid
        matters: the per-entry likelihoods are normalised over all of its alphas."""
        p = _demux_params(alphas)  # (doublet_prior is not read by the call)
        out = np.zeros((self.C, self.V), dtype=np.float64)
        self._check(self.lib.muxgl_demux_singlets(self.h, C.byref(p), _ptr(out)))
        return out

    INCLUSION_FIELDS = ("incl", "tot", "dbl", "partner", "alpha_idx", "first")

    def demux_inclusion(self, alphas=(0.0, 0.5), doublet_prior=0.5, want=INCLUSION_FIELDS):
        """muxgl_demux_inclusion: dict of arrays over the hypotheses H that carry prior mass (include/muxgl.h):
        incl float64 [C][V], the log evidence that sample s is in the droplet (singlet s or either half of a doublet);
        tot float64 [C], the log evidence of everything, so exp(incl - tot[:, None]) is the posterior of inclusion;
        dbl float64 [C][V], the best doublet log-likelihood with s in it (-1e300: none); partner, alpha_idx, first
        int32 [C][V]: the other sample of that doublet, its alpha index and whether s is its first sample (-1: none).
        At any V, without a previous demux_run.  want: the subset of the six to fetch (the others are passed as NULL)."""
        p = _demux_params(alphas, doublet_prior)
        unknown = set(want) - set(self.INCLUSION_FIELDS)
        if unknown:
            raise ValueError(f"unknown inclusion fields {sorted(unknown)}")
        out = {}
        for name in self.INCLUSION_FIELDS:
            if name in want:
                shape = (self.C,) if name == "tot" else (self.C, self.V)
                out[name] = np.zeros(shape, dtype=np.float64 if name in ("incl", "tot", "dbl") else np.int32)
        self._check(self.lib.muxgl_demux_inclusion(self.h, C.byref(p), *[_ptr(out.get(n)) for n in self.INCLUSION_FIELDS]))
        return out

    UNKNOWN_FIELDS = ("ju", "uj", "uu")

    def demux_unknown(self, alphas=(0.0, 0.5), gp0=None, want=UNKNOWN_FIELDS):
        """muxgl_demux_unknown: every droplet against a donor that is not in the panel (include/muxgl.h).  dict of
        ju float64 [C][V][A], sample j (share 1 - alpha) with the unknown donor (share alpha), the reference's llksA0;
        uj float64 [C][V][A], the other orientation; uu float64 [C][A], two unknown donors, the reference's llks00; and
        kernel_ms, the event time of the call's kernels.  gp0: the unknown donor's genotype prior [S][3], or None for the
        panel mean.  want: the subset of the three to fetch (the others are passed as NULL).  At any V, without a previous
        demux_run.  unknown_summary() turns the tables into per-droplet calls."""
        p = _demux_params(alphas)  # (doublet_prior is not read by the call)
        unknown = set(want) - set(self.UNKNOWN_FIELDS)
        if unknown:
            raise ValueError(f"unknown fields {sorted(unknown)}")
        if gp0 is not None:
            gp0 = _arr(gp0, np.float64, "gp0")
            if gp0.shape != (self.S, 3):
                raise ValueError("gp0 must be [S][3]")
        A = len(alphas)
        out = {}
        for name in self.UNKNOWN_FIELDS:
            if name in want:
                out[name] = np.zeros((self.C, A) if name == "uu" else (self.C, self.V, A), dtype=np.float64)
        ms = C.c_float(0.0)
        self._check(self.lib.muxgl_demux_unknown(self.h, C.byref(p), _ptr(gp0), *[_ptr(out.get(n)) for n in self.UNKNOWN_FIELDS],
                                                  C.byref(ms)))
        out["kernel_ms"] = float(ms.value)
        return out

    def demux_ambient(self, alphas, amb_af, rhos):
        """muxgl_demux_ambient: every droplet as one cell of sample j plus a share rho of ambient RNA whose ALT fraction
        at marker s is amb_af[s] (include/muxgl.h).  dict of ll float64 [C][V][n_rho], on the scale of the records'
        log-likelihoods under the grid `alphas`, and kernel_ms, the event time of the call's kernels.  At any V, without
        a previous demux_run; ambient_profile() makes amb_af from pileup_allele_counts(), ambient_summary() turns the
        table into per-droplet calls."""
        p = _demux_params(alphas)  # (doublet_prior is not read by the call)
        amb_af = _arr(amb_af, np.float64, "amb_af")
        if amb_af.shape != (self.S,):
            raise ValueError("amb_af must be [S]")
        rhos = _arr(rhos, np.float64, "rhos").reshape(-1)
        out = np.zeros((self.C, self.V, rhos.size), dtype=np.float64)
        ms = C.c_float(0.0)
        self._check(self.lib.muxgl_demux_ambient(self.h, C.byref(p), _ptr(amb_af), rhos.size, _ptr(rhos), _ptr(out),
                                                  C.byref(ms)))
        return {"ll": out, "kernel_ms": float(ms.value)}

    AMBIENT_FIT_FIELDS = ("rho_hat", "ll_hat", "ll_zero", "info", "status", "n_steps")

    def demux_ambient_fit(self, params, amb_af, cand, rho_max=0.5, want=AMBIENT_FIT_FIELDS):
        """muxgl_demux_ambient_fit: per droplet and candidate sample, the maximum-likelihood ambient share on [0, rho_max]
        under the model of demux_ambient, with its observed information (include/muxgl.h).  params: the alpha grid (a
        sequence of alphas); cand: int32 [C][n_cand] (or [C]), a sample or -1 per slot.  dict of rho_hat, ll_hat, ll_zero,
        info float64 [C][n_cand], status, n_steps int32 [C][n_cand], and kernel_ms.  want: the subset of the six to fetch
        (the others are passed as NULL).  ambient_fit_summary() gives the standard error and the likelihood ratio."""
        return _fit(self, "muxgl_demux_ambient_fit", self.AMBIENT_FIT_FIELDS, want, _demux_params(params), amb_af, cand, False,
                    rho_max)

    ALPHA_FIT_FIELDS = ("alpha_hat", "ll_hat", "ll_zero", "ll_top", "info", "status", "n_steps")

    def demux_alpha_fit(self, params, pairs, alpha_max=1.0, want=ALPHA_FIT_FIELDS):
        """muxgl_demux_alpha_fit: per droplet and pair of samples (j, k), the maximum-likelihood share alpha of k on
        [0, alpha_max] under the reference's doublet model, with its observed information (include/muxgl.h).  params: the
        alpha grid (a sequence of alphas); pairs: int32 [C][n_cand][2] (or [C][2]), (j, k) or (-1, -1) per slot.  dict of
        alpha_hat, ll_hat, ll_zero, ll_top, info float64 [C][n_cand], status, n_steps int32 [C][n_cand], the pairs under
        "pair", alpha_max, and kernel_ms.  want: the subset of the seven to fetch (the others are passed as NULL).
        alpha_fit_summary() gives the standard error, the likelihood ratio and the major sample."""
        out = _fit(self, "muxgl_demux_alpha_fit", self.ALPHA_FIT_FIELDS, want, _demux_params(params), _NO_AF, pairs, True,
                   alpha_max)
        out["alpha_max"] = float(alpha_max)
        return out

    def pileup_allele_counts(self, mask=None):
        """muxgl_pileup_allele_counts: (n_ref, n_alt), int64 [S] each, the usable reads of the droplets whose mask entry is
        true (None: all of them) by marker and allele; exact integer counts from the device."""
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if mask.shape != (self.C,):
                raise ValueError("mask must be [C]")
        n_ref = np.zeros(self.S, dtype=np.int64)
        n_alt = np.zeros(self.S, dtype=np.int64)
        self._check(self.lib.muxgl_pileup_allele_counts(self.h, _ptr(mask), _ptr(n_ref), _ptr(n_alt)))
        return n_ref, n_alt

    def pileup_read_hist(self, mask=None):
        """muxgl_pileup_read_hist: (keys, counts), int64 [n] each: the usable reads of the droplets whose mask entry is true
        (None: all of them) as a histogram, keys = marker * 256 + read byte strictly ascending, counts > 0; exact integer
        counts from the device."""
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if mask.shape != (self.C,):
                raise ValueError("mask must be [C]")
        n = C.c_int64(0)
        self._check(self.lib.muxgl_pileup_read_hist(self.h, _ptr(mask), None, None, 0, C.byref(n)))
        keys = np.zeros(n.value, dtype=np.int64)
        counts = np.zeros(n.value, dtype=np.int64)
        self._check(self.lib.muxgl_pileup_read_hist(self.h, _ptr(mask), _ptr(keys), _ptr(counts), n.value, C.byref(n)))
        return keys, counts

    SOUP_MIX_FIELDS = ("pi", "grad", "ll", "amb_af")

    def demux_soup_mix(self, mask=None, hist=None, with_unknown=False, gp0=None, pi0=None, n_iter_max=500, tol=1e-8,
                       want=SOUP_MIX_FIELDS):
        """muxgl_demux_soup_mix: the soup's ALT profile fitted as a mixture of the panel's donors (include/muxgl.h).  The
        reads are those of the droplets of `mask` (None: all), or the histogram hist = (keys, counts) of pileup_read_hist
        (mask must then be None).  with_unknown adds component V, a donor missing from the panel, with genotype prior
        gp0 [S][3] or the panel mean (None).  pi0: the start [M], or None for uniform shares.  dict of pi, grad float64 [M],
        ll float64 [n_iter_max + 1] (NaN behind the last evaluation), amb_af float64 [S] (want: the subset of the four to
        fetch), n_iter, n_reads, status (0 converged, 1 iteration cap, 2 no record took part) and kernel_ms.
        soup_mix_summary() gives the sorted shares and the fit's diagnostics."""
        unknown = set(want) - set(self.SOUP_MIX_FIELDS)
        if unknown:
            raise ValueError(f"unknown fields {sorted(unknown)}")
        M = self.V + (1 if with_unknown else 0)
        keys = counts = None
        n_rec = 0
        if hist is not None:
            if mask is not None:
                raise ValueError("mask and hist exclude each other")
            keys = _arr(hist[0], np.int64, "keys").reshape(-1)
            counts = _arr(hist[1], np.int64, "counts").reshape(-1)
            if keys.size != counts.size:
                raise ValueError("keys and counts must have one length")
            n_rec = keys.size
            if n_rec == 0:  # (an empty histogram is still a histogram: a non-NULL pointer says so)
                keys = np.zeros(1, dtype=np.int64)
                counts = np.zeros(1, dtype=np.int64)
        elif mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if mask.shape != (self.C,):
                raise ValueError("mask must be [C]")
        if gp0 is not None:
            gp0 = _arr(gp0, np.float64, "gp0")
            if gp0.shape != (self.S, 3):
                raise ValueError("gp0 must be [S][3]")
        if pi0 is not None:
            pi0 = _arr(pi0, np.float64, "pi0")
            if pi0.shape != (M,):
                raise ValueError("pi0 must be [M]")
        n_iter_max = int(n_iter_max)
        shapes = {"pi": M, "grad": M, "ll": max(n_iter_max, 0) + 1, "amb_af": self.S}
        out = {name: np.zeros(shapes[name], dtype=np.float64) for name in self.SOUP_MIX_FIELDS if name in want}
        n_iter, status, n_reads, ms = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_float(0.0)
        self._check(self.lib.muxgl_demux_soup_mix(self.h, _ptr(mask), n_rec, _ptr(keys), _ptr(counts), 1 if with_unknown else 0,
                                                   _ptr(gp0), _ptr(pi0), n_iter_max, float(tol),
                                                   *[_ptr(out.get(n)) for n in self.SOUP_MIX_FIELDS],
                                                   C.byref(n_iter), C.byref(n_reads), C.byref(status), C.byref(ms)))
        out.update(n_iter=int(n_iter.value), n_reads=int(n_reads.value), status=int(status.value), kernel_ms=float(ms.value))
        return out

    def demux_results_view(self):
        """zero-copy view of the pinned [C] record buffer of the last run"""
        p = self.lib.muxgl_demux_results(self.h)
        buf = (C.c_char * (self.C * DEMUX_CELL.itemsize)).from_address(p)
        return np.frombuffer(buf, dtype=DEMUX_CELL, count=self.C)

    def demux_oct_split(self):
        """muxgl_demux_oct_split: dict(cut, groups, round_units, units) of the last demux_run on the default-grid path"""
        info = np.zeros(4, dtype=np.int64)
        self._check(self.lib.muxgl_demux_oct_split(self.h, _ptr(info)))
        return dict(zip(("cut", "groups", "round_units", "units"), (int(x) for x in info)))

    def demux_entry_pg(self):
        pg = np.zeros((self.nnz, self.n_alpha, 3, 3), dtype=np.float64)
        self._check(self.lib.muxgl_demux_get_entry_pg(self.h, _ptr(pg)))
        return pg

    # ---- freemuxlet
    def fmx_prepare(self, af):
        af = _arr(af, np.float64, "af")
        if af.shape != (self.S,):
            raise ValueError("af must be [S]")
        llk0 = np.zeros(self.C)
        llk2 = np.zeros(self.C)
        nsnps = np.zeros(self.C, dtype=np.int32)
        nreads = np.zeros(self.C, dtype=np.int32)
        self._check(self.lib.muxgl_fmx_prepare(self.h, _ptr(af), _ptr(llk0), _ptr(llk2), _ptr(nsnps), _ptr(nreads)))
        self.n_anchor = 0
        return llk0, llk2, nsnps, nreads

    def fmx_entry_gls(self):
        gls = np.zeros((self.nnz, 9))
        cnt = np.zeros((self.nnz, 3), dtype=np.int32)
        self._check(self.lib.muxgl_fmx_get_entry_gls(self.h, _ptr(gls), _ptr(cnt)))
        return gls, cnt

    def fmx_greedy_init(self, K, scores, frac_init_clust=1.0, singlet_score_thres=-1e300):
        scores = _arr(scores, np.float64, "scores")
        if scores.shape != (self.C,):
            raise ValueError("scores must be [C]")
        clust = np.zeros(self.C, dtype=np.int32)
        self._check(self.lib.muxgl_fmx_greedy_init(self.h, int(K), _ptr(scores), float(frac_init_clust),
                                                    float(singlet_score_thres), _ptr(clust)))
        return clust

    def fmx_score_stats(self):
        """cells whose llk0 / llk2 the last fmx_prepare recomputed in the reference's arithmetic (near-tied scores)"""
        a = C.c_int64()
        self._check(self.lib.muxgl_fmx_score_stats(self.h, C.byref(a)))
        return a.value

    def fmx_greedy_stats(self):
        """(near ties decided by the exact path, of those against the kernel's choice) of the last fmx_greedy_init"""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.muxgl_fmx_greedy_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fmx_set_clusters(self, K, clust):
        clust = _arr(clust, np.int32, "clust")
        if clust.shape != (self.C_total,):
            raise ValueError("clust must be [C] (the whole job's cells for a slabbed handle)")
        self._check(self.lib.muxgl_fmx_set_clusters(self.h, int(K), _ptr(clust)))
        self.K = int(K)
        self.n_anchor = 0

    @property
    def anchor_modes(self):
        """the modes of the anchored clusters, a tuple of ANCHOR_HELD / ANCHOR_PRIOR of length n_anchor (mirrors the
        library: whatever drops the anchors empties it)"""
        return self._anchor_modes if len(self._anchor_modes) == self.n_anchor else (ANCHOR_HELD,) * self.n_anchor

    def fmx_set_anchors(self, donors, modes=None):
        """muxgl_fmx_set_anchors[_mode]: clusters 0 .. len(donors)-1 take their genotype posteriors from the panel of
        demux_set_gp, cluster i from column donors[i], instead of from their droplets; the other clusters are learned as
        ever (include/muxgl.h).  modes: None (all ANCHOR_HELD: the panel row is the posterior) or one of ANCHOR_HELD /
        ANCHOR_PRIOR per donor (PRIOR: the panel row is the prior of the posterior the droplets form).  An empty list (or
        None) removes the anchors.  After fmx_set_clusters; dropped again by fmx_set_clusters, fmx_prepare, set_pileup and
        demux_set_gp.  n_anchor and anchor_modes mirror the library."""
        d = _arr([] if donors is None else donors, np.int32, "donors")
        if d.ndim != 1:
            raise ValueError("donors must be a list of panel columns")
        if modes is None:
            self._check(self.lib.muxgl_fmx_set_anchors(self.h, int(d.size), _ptr(d) if d.size else None))
            md = np.zeros(d.size, dtype=np.uint8)
        else:
            md = _arr(modes, np.uint8, "modes")
            if md.shape != d.shape:
                raise ValueError("modes must hold one mode per donor")
            self._check(self.lib.muxgl_fmx_set_anchors_mode(self.h, int(d.size), _ptr(d) if d.size else None,
                                                            _ptr(md) if md.size else None))
        self.n_anchor = int(d.size)
        self._anchor_modes = tuple(int(x) for x in md)

    def fmx_cluster_gp(self, k0=0, k1=None):
        """muxgl_fmx_get_cluster_gp: the posterior rows [S][k1-k0][3] of clusters k0 .. k1-1 that the last posterior phase
        wrote and its E-step read (k1 None: up to K)"""
        k1 = self.K if k1 is None else int(k1)
        out = np.zeros((self.S, max(k1 - int(k0), 0), 3), dtype=np.float64)
        self._check(self.lib.muxgl_fmx_get_cluster_gp(self.h, int(k0), k1, _ptr(out)))
        return out

    def fmx_iterate(self, doublet_prior=0.5, geno_error=0.1, want_cells=True, want_full_ll=False):
        p = _FmxParams(float(doublet_prior), float(geno_error))
        out = np.zeros(self.C, dtype=FMX_CELL) if want_cells else None
        full = np.zeros((self.C, self.K * (self.K + 1) // 2)) if want_full_ll else None
        ns, na, nc = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.muxgl_fmx_iterate(self.h, C.byref(p), _ptr(out), C.byref(ns), C.byref(na), C.byref(nc),
                                                _ptr(full)))
        stats = (ns.value, na.value, nc.value)
        if want_full_ll:
            return out, stats, full
        return out, stats

    def fmx_singlets(self):
        """muxgl_fmx_singlets: float64 [C][K], the singlet log-likelihood llks[j(j+1)/2 + j] of every droplet (of the
        handle's own cells) against every cluster as the last E-step formed it -- the diagonal of fmx_iterate's full_ll
        where that exists -- at any K, on every E-step path.  singlet_posteriors() turns it into soft assignments."""
        out = np.zeros((self.C, self.K), dtype=np.float64)
        self._check(self.lib.muxgl_fmx_singlets(self.h, _ptr(out)))
        return out

    FMX_INCLUSION_FIELDS = ("incl", "tot", "dbl", "partner")

    def fmx_inclusion(self, doublet_prior=0.5, want=FMX_INCLUSION_FIELDS):
        """muxgl_fmx_inclusion: dict of arrays over the hypotheses of the last E-step (include/muxgl.h), for the handle's
        own cells: incl float64 [C][K], the log evidence that cluster s is in the droplet (singlet s or either half of a
        doublet); tot float64 [C], the log evidence of everything, so exp(incl - tot[:, None]) is the posterior of
        inclusion; dbl float64 [C][K], the best doublet log-likelihood with s in it (-1e300: none); partner int32 [C][K],
        the other cluster of that doublet (-1: none).  At any K, on every E-step path.  want: the subset of the four to
        fetch (the others are passed as NULL)."""
        unknown = set(want) - set(self.FMX_INCLUSION_FIELDS)
        if unknown:
            raise ValueError(f"unknown inclusion fields {sorted(unknown)}")
        p = _FmxParams(float(doublet_prior), 0.0)  # (geno_error is not read by the call)
        out = {}
        for name in self.FMX_INCLUSION_FIELDS:
            if name in want:
                shape = (self.C,) if name == "tot" else (self.C, self.K)
                out[name] = np.zeros(shape, dtype=np.int32 if name == "partner" else np.float64)
        self._check(self.lib.muxgl_fmx_inclusion(self.h, C.byref(p), *[_ptr(out.get(n)) for n in self.FMX_INCLUSION_FIELDS]))
        return out

    FMX_UNKNOWN_FIELDS = FMX_UNKNOWN_FIELDS

    def fmx_unknown(self, gp0=None, want=FMX_UNKNOWN_FIELDS):
        """muxgl_fmx_unknown: every droplet (of the handle's own cells) against a donor that no cluster holds, from the
        posteriors the last E-step read (include/muxgl.h).  dict of ll_ju float64 [C][K], cluster j plus the unknown
        donor; ll_u float64 [C], the unknown donor alone; ll_uu float64 [C], two unknown donors; and kernel_ms, the event
        time of the call's kernels.  gp0: the unknown donor's genotype prior [S][3] (rows must be probability triples), or
        None for the Hardy-Weinberg triple of fmx_prepare's af.  want: the subset of the three to fetch (the others are
        passed as NULL).  At any K, on every E-step path; freemuxlet.unknown_summary() turns the tables into calls."""
        unknown = set(want) - set(FMX_UNKNOWN_FIELDS)
        if unknown:
            raise ValueError(f"unknown fields {sorted(unknown)}")
        if gp0 is not None:
            gp0 = _arr(gp0, np.float64, "gp0")
            if gp0.shape != (self.S, 3):
                raise ValueError("gp0 must be [S][3]")
        out = {}
        for name in FMX_UNKNOWN_FIELDS:
            if name in want:
                out[name] = np.zeros((self.C, self.K) if name == "ll_ju" else (self.C,), dtype=np.float64)
        ms = C.c_float(0.0)
        self._check(self.lib.muxgl_fmx_unknown(self.h, _ptr(gp0), *[_ptr(out.get(n)) for n in FMX_UNKNOWN_FIELDS],
                                                C.byref(ms)))
        out["kernel_ms"] = float(ms.value)
        return out

    def fmx_ambient(self, amb_af, rhos):
        """muxgl_fmx_ambient: every droplet (of the handle's own cells) as one cell of cluster j plus a share rho of
        ambient RNA whose ALT fraction at marker s is amb_af[s], from the posteriors the last E-step read
        (include/muxgl.h).  dict of ll float64 [C][K][n_rho], on the scale of the records' log-likelihoods, and
        kernel_ms, the event time of the call's kernels.  At any K, on every E-step path; ambient_profile() makes amb_af
        from pileup_allele_counts(), freemuxlet.ambient_summary() turns the table into per-droplet calls."""
        amb_af = _arr(amb_af, np.float64, "amb_af")
        if amb_af.shape != (self.S,):
            raise ValueError("amb_af must be [S]")
        rhos = _arr(rhos, np.float64, "rhos").reshape(-1)
        out = np.zeros((self.C, self.K, rhos.size), dtype=np.float64)
        ms = C.c_float(0.0)
        self._check(self.lib.muxgl_fmx_ambient(self.h, _ptr(amb_af), rhos.size, _ptr(rhos), _ptr(out), C.byref(ms)))
        return {"ll": out, "kernel_ms": float(ms.value)}

    def fmx_ambient_fit(self, amb_af, cand, rho_max=0.5, want=AMBIENT_FIT_FIELDS):
        """muxgl_fmx_ambient_fit: per droplet (of the handle's own cells) and candidate cluster, the maximum-likelihood
        ambient share on [0, rho_max] under the model of fmx_ambient, with its observed information, from the posteriors
        the last E-step read (include/muxgl.h).  cand: int32 [C][n_cand] (or [C]), a cluster or -1 per slot.  dict of
        rho_hat, ll_hat, ll_zero, info float64 [C][n_cand], status, n_steps int32 [C][n_cand], and kernel_ms.  want: the
        subset of the six to fetch (the others are passed as NULL).  freemuxlet.ambient_fit_summary() gives the standard
        error and the likelihood ratio."""
        return _fit(self, "muxgl_fmx_ambient_fit", self.AMBIENT_FIT_FIELDS, want, None, amb_af, cand, False, rho_max)

    def fmx_alpha_fit(self, pairs, alpha_max=1.0, want=ALPHA_FIT_FIELDS):
        """muxgl_fmx_alpha_fit: per droplet (of the handle's own cells) and pair of clusters (j, k), the maximum-likelihood
        share alpha of k on [0, alpha_max] under the reference's doublet model with the share set free, with its observed
        information, from the posteriors the last E-step read (include/muxgl.h).  pairs: int32 [C][n_cand][2] (or [C][2]),
        (j, k) or (-1, -1) per slot.  dict of alpha_hat, ll_hat, ll_zero, ll_top, info float64 [C][n_cand], status, n_steps
        int32 [C][n_cand], the pairs under "pair", alpha_max, and kernel_ms.  want: the subset of the seven to fetch (the
        others are passed as NULL).  freemuxlet.alpha_fit_summary() gives the standard error, the likelihood ratio and the
        major cluster."""
        out = _fit(self, "muxgl_fmx_alpha_fit", self.ALPHA_FIT_FIELDS, want, None, _NO_AF, pairs, True, alpha_max)
        out["alpha_max"] = float(alpha_max)
        return out

    # ---- freemuxlet-old: pairwise distance matrix and voting passes (cmd_cram_freemuxlet.cpp:176-343)
    def fmxold_pair_dist(self, bf_thres=5.41, want_full=False):
        full = np.zeros(self.C * (self.C - 1) // 2, dtype=DROPD) if want_full else None
        self._check(self.lib.muxgl_fmxold_pair_dist(self.h, float(bf_thres), _ptr(full)))
        return full

    def fmxold_signs(self):
        out = np.zeros((self.C, self.C), dtype=np.int8)
        self._check(self.lib.muxgl_fmxold_get_signs(self.h, _ptr(out)))
        return out

    def fmxold_vote_init(self, K, order, jitter, frac_init_clust=1.0):
        order = _arr(order, np.int32, "order")
        jitter = _arr(jitter, np.float64, "jitter")
        clust = np.zeros(self.C, dtype=np.int32)
        cc = np.zeros(int(K), dtype=np.int32)
        self._check(self.lib.muxgl_fmxold_vote_init(self.h, int(K), _ptr(order), _ptr(jitter), float(frac_init_clust),
                                                     _ptr(clust), _ptr(cc)))
        return clust, cc

    def fmxold_vote_refine(self, K, order, jitter, clust, keep_init_missing=False):
        order = _arr(order, np.int32, "order")
        jitter = _arr(jitter, np.float64, "jitter")
        clust = np.array(clust, dtype=np.int32)
        cc = np.zeros(int(K), dtype=np.int32)
        ch = C.c_int32()
        self._check(self.lib.muxgl_fmxold_vote_refine(self.h, int(K), _ptr(order), _ptr(jitter),
                                                       int(bool(keep_init_missing)), _ptr(clust), C.byref(ch), _ptr(cc)))
        return clust, ch.value, cc

    # ---- sharded EM phases (multi-GPU); the collectives between them belong to the caller (popscle_amd/freemuxlet.py)
    def fmx_set_shard(self, c0, c1, s0, s1):
        self._check(self.lib.muxgl_fmx_set_shard(self.h, int(c0), int(c1), int(s0), int(s1)))
        if (int(c0), int(c1), int(s0), int(s1)) != (0, self.C, 0, self.S):
            self.n_anchor = 0  # (anchors live on whole-job handles and device groups only)

    def fmx_iter_gp(self, doublet_prior=0.5, geno_error=0.1):
        p = _FmxParams(float(doublet_prior), float(geno_error))
        self._check(self.lib.muxgl_fmx_iter_gp(self.h, C.byref(p)))

    def fmx_iter_estep(self, doublet_prior=0.5, geno_error=0.1):
        p = _FmxParams(float(doublet_prior), float(geno_error))
        self._check(self.lib.muxgl_fmx_iter_estep(self.h, C.byref(p)))

    def fmx_iter_mstep(self):
        self._check(self.lib.muxgl_fmx_iter_mstep(self.h))

    def fmx_iter_fetch(self, want_full_ll=False, want_cells=True):
        out = np.empty(self.C, dtype=FMX_CELL) if want_cells else None
        full = np.zeros((self.C, self.K * (self.K + 1) // 2)) if want_full_ll else None
        ns, na, nc = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.muxgl_fmx_iter_fetch(self.h, _ptr(out), C.byref(ns), C.byref(na), C.byref(nc), _ptr(full)))
        stats = (ns.value, na.value, nc.value)
        return (out, stats, full) if want_full_ll else (out, stats)

    def fmx_buffer(self, which):
        """(device pointer, element count) of an internal exchange buffer: BUF_CGP f64, BUF_CLUST i32, BUF_CELLS
        records, BUF_STAT i32[4]"""
        ptr = _VP()
        n = C.c_int64()
        self._check(self.lib.muxgl_fmx_buffer(self.h, int(which), C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def memcpy_dev(self, dst_ptr, src_ptr, nbytes):
        self._check(self.lib.muxgl_memcpy_dev(self.h, _VP(dst_ptr), _VP(src_ptr), int(nbytes)))

    def group_peer_stats(self):
        """(member pairs walked, pairs with direct peer access, pairs left on the staged copy) of a device group"""
        out = np.zeros(3, dtype=np.int32)
        self._check(self.lib.muxgl_group_peer_stats(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def fmx_exact_stats(self):
        """(near-tie cells settled by the exact path, calls it changed, near-tie cells left unresolved) since set_clusters"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.muxgl_fmx_exact_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- the exact path for the sharded phases (include/muxgl.h; freemuxlet.settle_near_ties drives it)
    def fmx_exact_pending(self):
        n = C.c_int64()
        self._check(self.lib.muxgl_fmx_exact_pending(self.h, C.byref(n)))
        return n.value

    def fmx_exact_hint(self, nchanged_jobwide):
        self._check(self.lib.muxgl_fmx_exact_hint(self.h, int(nchanged_jobwide)))

    def fmx_exact_snps(self):
        n = C.c_int64()
        self._check(self.lib.muxgl_fmx_exact_snps(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        self._check(self.lib.muxgl_fmx_exact_snps(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def fmx_exact_rows(self, snps, doublet_prior=0.5, geno_error=0.1):
        snps = _arr(snps, np.int32, "snps")
        p = _FmxParams(float(doublet_prior), float(geno_error))
        rows = np.zeros((snps.size, self.K, 3))
        owned = np.zeros(snps.size, dtype=np.uint8)
        self._check(self.lib.muxgl_fmx_exact_rows(self.h, C.byref(p), _ptr(snps), snps.size, _ptr(rows), _ptr(owned)))
        return rows, owned.astype(bool)

    def fmx_exact_finish(self, snps, rows, doublet_prior=0.5, geno_error=0.1):
        snps = _arr(snps, np.int32, "snps")
        rows = _arr(rows, np.float64, "rows")
        p = _FmxParams(float(doublet_prior), float(geno_error))
        deltas = np.zeros(3, dtype=np.int64)
        re = C.c_int32()
        self._check(self.lib.muxgl_fmx_exact_finish(self.h, C.byref(p), _ptr(snps), snps.size, _ptr(rows), _ptr(deltas),
                                                    C.byref(re)))
        return deltas, bool(re.value)

    def fmx_cluster_pileup(self):
        gls = np.zeros((self.K, self.S, 9))
        cnt = np.zeros((self.K, self.S, 3), dtype=np.int32)
        self._check(self.lib.muxgl_fmx_get_cluster_pileup(self.h, _ptr(gls), _ptr(cnt)))
        return gls, cnt

    FMX_MATCH_FIELDS = ("ll", "ll0", "nsnps")

    def fmx_match_donors(self, want=FMX_MATCH_FIELDS):
        """muxgl_fmx_match_donors: the cluster pileups as they are now scored against the donors of demux_set_gp
        (include/muxgl.h).  dict of ll float64 [K][V], the log-likelihood of cluster k being donor v over the markers the
        cluster has reads at and the donors have genotypes at; ll0 float64 [K], the same for an unrelated individual at
        the allele frequencies (ll - ll0[:, None] is the log Bayes factor of a match); nsnps int32 [K], those markers'
        number; and kernel_ms, the event time of the call's kernels.  want: the subset of the three to fetch (the others
        are passed as NULL).  freemuxlet.match_table() turns ll and ll0 into best donors."""
        unknown = set(want) - set(self.FMX_MATCH_FIELDS)
        if unknown:
            raise ValueError(f"unknown match fields {sorted(unknown)}")
        out = {}
        if "ll" in want:
            out["ll"] = np.zeros((self.K, self.V), dtype=np.float64)
        if "ll0" in want:
            out["ll0"] = np.zeros(self.K, dtype=np.float64)
        if "nsnps" in want:
            out["nsnps"] = np.zeros(self.K, dtype=np.int32)
        ms = C.c_float(0.0)
        self._check(self.lib.muxgl_fmx_match_donors(self.h, *[_ptr(out.get(n)) for n in self.FMX_MATCH_FIELDS], C.byref(ms)))
        out["kernel_ms"] = float(ms.value)
        return out

    FMX_PAIRS_FIELDS = ("llk2", "llk0", "nsnps")

    def fmx_cluster_pairs(self, want=FMX_PAIRS_FIELDS):
        """muxgl_fmx_cluster_pairs: every pair of the cluster pileups as they are now scored as one donor against two
        unrelated donors (include/muxgl.h).  dict of llk2, llk0 float64 and nsnps int32, each [K (K - 1) / 2] with the
        pair a > b at a (a - 1) / 2 + b (llk2 - llk0 is the log Bayes factor of "one donor", over the nsnps markers both
        clusters have reads at), and kernel_ms, the event time of the call's kernels.  want: the subset of the three to
        fetch (the others are passed as NULL).  freemuxlet.cluster_pair_table() turns them into a matrix and groups."""
        unknown = set(want) - set(self.FMX_PAIRS_FIELDS)
        if unknown:
            raise ValueError(f"unknown pair fields {sorted(unknown)}")
        n = self.K * (self.K - 1) // 2
        out = {f: np.zeros(n, dtype=np.int32 if f == "nsnps" else np.float64) for f in self.FMX_PAIRS_FIELDS if f in want}
        ms = C.c_float(0.0)
        self._check(self.lib.muxgl_fmx_cluster_pairs(self.h, *[_ptr(out.get(f)) for f in self.FMX_PAIRS_FIELDS], C.byref(ms)))
        out["kernel_ms"] = float(ms.value)
        return out

    # ---- measurement
    def timing_sum(self, reset=False):
        """(kernel times summed over the run / iterate calls since the last reset, ms; number of those calls)"""
        ms = np.zeros(T_COUNT, dtype=np.float64)
        n = C.c_int64(0)
        self._check(self.lib.muxgl_get_timing_sum(self.h, _ptr(ms), C.byref(n), 1 if reset else 0))
        return ms, int(n.value)

    def timing(self, out=None):
        """kernel times of the last run / iterate call, ms (out: a float32[T_COUNT] array to fill instead of a new one)"""
        ms = np.zeros(T_COUNT, dtype=np.float32) if out is None else out
        self._check(self.lib.muxgl_get_timing(self.h, _ptr(ms)))
        return ms
