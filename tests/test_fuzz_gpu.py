"""Randomised differential test: libmuxgl (HIP, through the C-ABI) against the reference's own compiled loops
(oracle/_ref/libscdrop_ref.so) on small problems drawn to be UNFRIENDLY -- cells of one to a handful of entries (most
hypotheses tie exactly in the reference's arithmetic, so every call is a question of scan order and strict '<'),
duplicated samples, markers without genotypes, entries whose reads are all of another allele, deep entries, uncapped
qualities, genotype rows that do not sum to one, unusual alpha grids and priors, every kernel family by shape.

Bar: parity.compare_* -- every integer field equal, log-likelihoods within 1e-5 (the asserts below hold them to 1e-7).

Every case also asks the same engine for the per-droplet tables -- muxgl_demux_singlets and the six tables of
muxgl_demux_inclusion against the reference's full_ll (parity.compare_singlet_table, parity.compare_inclusion on
test_demux_inclusion.restate), muxgl_fmx_singlets after every iteration against the diagonal of the reference's full_ll
-- in a quarter of the cases under a slab budget of 1 MB (several batches and groups).  Their bars: TABLE_TOL below.
A campaign line carries sng_ll, incl_ll, tot_ll, dbl_ll, fmx_sng_ll (the worst |d| of each table) and incl_decided, the
share of (cell, sample) pairs whose reference gap exceeds 2 LL_TOL: the pairs whose integers were compared exactly.

Every freemuxlet case (fmx_case; not the streamed ones) also scores its clusters against a donor panel drawn for it
(match_case below) with muxgl_fmx_match_donors, at a tile size drawn per case and under the case's table budget, and
holds the table to tests/match_ref.py restate_match twice: fed the handle's own fmx_cluster_pileup(), after every
iteration where the case runs on one handle, and fed the reference's cluster pileups of the last iteration, which does
not pass through the library's M-step.  Device groups and sharded handles refuse the call by name; their last
assignment is scored on the module's plain engine.  A campaign line of --kind fmx carries match_ll, match_ref_ll (the
worst |d| against either), match_v, match_tile, match_mode, match_dup, match_missing and match_neginf (the -inf of
the last table).

pytest runs the seeds of FUZZ_SEEDS (a minute); a campaign is
    python tests/test_fuzz_gpu.py --seeds 1000:1400 [--kind demux|fmx] [--log gpurun_out/fuzz.jsonl]
which prints one JSON line per case and exits 1 at the first failing seed (the seed reproduces the case).

The streamed paths (demux_stream.hip, fmx_stream.hip) have cases of their own, stream_demux_case / stream_fmx_case below,
run by tests/test_fuzz_stream_gpu.py and by `--kind stream-demux|stream-fmx` (profiles/stream_fuzz_campaign.md).
"""
import contextlib
import io
import json
import os
import sys
import time
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import parity  # noqa: E402
import ref_binding as rb  # noqa: E402
from match_ref import restate_match  # noqa: E402
from popscle_amd import freemuxlet, muxgl, shard, synth  # noqa: E402
from test_demux_inclusion import restate  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rb.available(), reason="oracle/_ref/libscdrop_ref.so not built")]

GRIDS = [(0.0, 0.5)] * 5 + [(0.0, 0.1, 0.2, 0.3, 0.4, 0.5)] * 2 + [(0.0, 0.25, 0.5), (0.0, 0.1, 0.3), (0.0, 0.5, 0.2),
                                                                   (0.0,), (0.0, 0.3)]
DEMUX_V = [1, 2, 3, 4, 5, 8, 12, 15, 16, 16, 16, 17, 24, 31, 32, 33, 40, 64, 65, 70, 96, 130, 255]
FMX_K = [2, 3, 4, 8, 15, 16, 16, 17, 24, 32, 33, 64, 65, 100, 130, 255]
FUZZ_SEEDS = list(range(12))
# kernel families by flag (include/muxgl.h), drawn per case: the default dispatch most of the time
DEMUX_FLAGS = [0] * 6 + [muxgl.FLAG_FORCE_ROW_KERNEL, muxgl.FLAG_FORCE_WAVE_KERNEL, muxgl.FLAG_FORCE_TILE_SWEEP,
                         muxgl.FLAG_NO_LINEAR_ENTRIES, muxgl.FLAG_SPLIT_GENERAL_SWEEP,
                         muxgl.FLAG_FORCE_ROW_KERNEL | muxgl.FLAG_NO_LINEAR_ENTRIES]
FMX_FLAGS = [0] * 6 + [muxgl.FLAG_FORCE_ROW_KERNEL, muxgl.FLAG_FORCE_WAVE_KERNEL, muxgl.FLAG_NO_LINEAR_ENTRIES,
                       muxgl.FLAG_NO_PIVOT_SUMS, muxgl.FLAG_FORCE_WAVE_KERNEL | muxgl.FLAG_NO_PIVOT_SUMS]

# The bars of the tables (none of them has an exact pass behind it).  parity.compare_* hold them to parity.LL_TOL through
# parity._close (same-signed infinities equal); on top of that a table whose worst deviation over the campaign
# `--seeds 1000:1100 --budget-s 600` and over FUZZ_SEEDS stayed within 1e-8 is held to 1e-7 like the rest of this file,
# else to LL_TOL.  Measured: sng 4.7e-11, incl / tot / dbl 3.0e-11, fmx_sng 1.6e-10 -- all five
# at 1e-7.  sng: muxgl_demux_singlets; incl, tot, dbl: muxgl_demux_inclusion; fmx_sng: muxgl_fmx_singlets.
# match, match_ref: muxgl_fmx_match_donors against restate_match of the handle's own and of the reference's cluster
# pileups (campaign `--seeds 1000:1100 --kind fmx --budget-s 600`): 1.8e-12 and 1.8e-12 over the campaign,
# 1.5e-11 and 1.5e-11 over FUZZ_SEEDS (seed 3, 16 000 markers) -- both at 1e-7.  match_ref could have been as far off as
# |U| x 1e-11 = 1.6e-7 (the library's pileups are held to the reference's at rtol 1e-11); it is not.
TABLE_TOL = dict(sng=1e-7, incl=1e-7, tot=1e-7, dbl=1e-7, fmx_sng=1e-7, match=1e-7, match_ref=1e-7)
RESTATE_BYTES = 5e7   # of full_ll per call of restate (it makes several temporaries of that size): 16 cells at V = 255, A = 6


def table_slab_mb(seed, kind):
    """the slab budget of the table calls alone, from a stream of its own (the cases' draws stay what they were):
    "1" (MB) in a quarter of the cases, else None (the variable unset: the library's default)"""
    u = np.random.default_rng([seed, 79]).random(2)[0 if kind == "demux" else 1]
    return "1" if u < 0.25 else None


@contextlib.contextmanager
def slab_env(name, value):
    """the environment variable `name` set to `value` (None: unset) inside, what it was outside"""
    old = os.environ.get(name)
    try:
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _shape(r, width, per_hyp):
    """(C, S, mean entries, min entries, sigma): tiny cells more often than not; C bounded by the reference's run time"""
    ment = float(r.choice([1.5, 3, 8, 30, 120, 400], p=[0.2, 0.2, 0.2, 0.15, 0.15, 0.1]))
    if width > 80:   # (the widest shapes: the reference's time goes with the square of the width)
        ment = min(ment, 8.0)
    S = int(max(40, ment * float(r.choice([2, 8, 40]))))
    budget = 2.5e8
    C = int(np.clip(budget / (max(ment, 4) * per_hyp), max(8, 2 * width if width <= 80 else 60), 600))
    return C, S, ment, int(r.choice([0, 1, 2])), float(r.choice([0.3, 0.8, 1.3]))


def _pileup(r, seed, C, S, V, ment, mine, sigma, with_gp):
    cap = int(r.choice([20, 20, 40, 60, 93, 127]))
    return synth.make_pileup(C, S, V, seed=seed, mean_entries=ment, sigma=sigma, min_entries=mine,
                             reads_lambda=float(r.choice([0.0, 0.3, 0.3, 1.5, 6.0, 6.0, 60.0])),
                             other=float(r.choice([0.0, 0.02, 0.5])), doublet_frac=float(r.choice([0.0, 0.25, 0.6])),
                             flip=float(r.choice([0.0, 0.01, 0.2])), max_bq=cap, cap_bq=cap,
                             missing_gp_frac=float(r.choice([0.0, 0.0, 0.03, 0.5, 1.0])) if with_gp else 0.0, with_gp=with_gp)


def _gp_mode(r, p, V):
    """one of the genotype-tensor modes drawn and applied to p.gp; returns its name"""
    mode = str(r.choice(["gt", "gt", "dup", "all_same", "float_rows", "hard"]))
    gp = p.gp
    if mode == "dup" and V > 1:       # some samples are copies of others: exact ties between hypotheses
        for _ in range(max(1, V // 3)):
            a, b = r.integers(V, size=2)
            gp[:, a, :] = gp[:, b, :]
    elif mode == "all_same":          # every sample the same: every singlet ties, every pair ties
        gp[:, :, :] = gp[:, :1, :]
    elif mode == "hard":              # hard calls with almost no error mixed in: factors down to 1e-6 x 1e-10
        gp = synth.gt_to_gp(p.truth["G"].astype(np.int64), 1e-6)
    elif mode == "float_rows":        # rows as --field GP leaves them: normalised in float, sums off one by ~1e-8
        g = r.dirichlet([0.3, 0.3, 0.3], size=(p.S, V)).astype(np.float32) + np.float32(1e-4)
        g = g / g.sum(axis=2, keepdims=True, dtype=np.float32)
        gp = 0.9 * g.astype(np.float64) + 0.1 * g.astype(np.float64).mean(axis=1, keepdims=True)
    p.gp = np.ascontiguousarray(gp)
    return mode


def demux_case(seed):
    r = np.random.default_rng([seed, 77])
    V = int(r.choice(DEMUX_V))
    alphas = GRIDS[int(r.integers(len(GRIDS)))]
    C, S, ment, mine, sigma = _shape(r, V, V * V * len(alphas) * 9)
    p = _pileup(r, 3000 + seed, C, S, V, ment, mine, sigma, True)
    mode = _gp_mode(r, p, V)
    dp = float(r.choice([0.5, 0.5, 0.1, 0.9]))
    flags = int(DEMUX_FLAGS[int(r.integers(len(DEMUX_FLAGS)))])
    how = str(r.choice(["one", "one", "one", "group"]))   # group: a device group of two members on this GPU
    return dict(kind="demux", seed=seed, V=V, alphas=alphas, C=C, S=S, ment=ment, mode=mode, dp=dp, flags=flags,
                how=how), p


def _engine(eng, info):
    """the shared engine for the default dispatch on one device, else one made for the case (closed by the caller)"""
    if info.get("how", "one") == "group":
        return muxgl.Engine([0, 0], flags=info["flags"]), True
    if info["flags"]:
        return muxgl.Engine(0, flags=info["flags"]), True
    return eng, False


def run_demux(eng, info, p):
    eng, own = _engine(eng, info)
    try:
        return _run_demux(eng, info, p)
    finally:
        if own:
            eng.close()


def _run_demux(eng, info, p):
    alphas, dp, V = info["alphas"], info["dp"], info["V"]
    want, _, want_ll = rb.RefScl.from_packed(p).demux(alphas, doublet_prior=dp, full_ll=True)
    eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    eng.demux_set_gp(p.gp, p.has_gp)
    got = eng.demux_run(alphas, dp)                      # the product path (calls made next to the sweep)
    rep = parity.compare_demux(got, want, alphas, p, doublet_prior=dp)
    st = rep["exact_pass"]
    if info.get("how", "one") == "group":
        assert rep["max_abs_ll_diff"] < 1e-7, rep
        out = dict(ll=rep["max_abs_ll_diff"], looked_at=int(st["cells"]), near=int(st["near_ties"]),
                   deep=int(st["deep"]), changed=int(st["changed"]), raw_differing=rep["raw_records_differing"])
    else:
        got2, full = eng.demux_run(alphas, dp, want_full_ll=True)   # the tensor path
        rep2 = parity.compare_demux(got2, want, alphas, p, doublet_prior=dp)
        worst = parity.compare_full_ll(full, want_ll, V, alphas)
        assert rep["max_abs_ll_diff"] < 1e-7 and rep2["max_abs_ll_diff"] < 1e-7 and worst < 1e-7, (rep, rep2, worst)
        out = dict(ll=max(rep["max_abs_ll_diff"], worst), looked_at=int(st["cells"]), near=int(st["near_ties"]),
                   deep=int(st["deep"]), changed=int(st["changed"]), raw_differing=rep["raw_records_differing"])
    out.update(_demux_tables(eng, info, want_ll))
    return out


def _demux_tables(eng, info, want_ll):
    """the singlet table and the six inclusion tables of the same engine against the reference's full_ll"""
    alphas, dp, V = info["alphas"], info["dp"], info["V"]
    slab = table_slab_mb(info["seed"], "demux")
    with slab_env("MUXGL_DEMUX_SLAB_MB", slab):
        sng = eng.demux_singlets(alphas)
        inc = eng.demux_inclusion(alphas, dp)
    out = dict(table_slab_mb=slab, sng_ll=parity.compare_singlet_table(sng, want_ll[:, :, 0, 0], TABLE_TOL["sng"]))
    worst, pairs, decided = dict(incl=0.0, tot=0.0, dbl=0.0), 0, 0
    Cn = want_ll.shape[0]
    step = int(max(16, RESTATE_BYTES // (V * V * len(alphas) * 8)))
    for b in range(0, Cn, step):
        full = want_ll[b:b + step]
        with contextlib.redirect_stdout(io.StringIO()):   # (a campaign prints one line per case)
            rep = parity.compare_inclusion({k: v[b:b + step] for k, v in inc.items()}, full, restate(full, alphas, dp),
                                           f"seed {info['seed']} cells {b}..")
        worst = {k: max(worst[k], rep[k]) for k in worst}
        pairs, decided = pairs + rep["pairs"], decided + rep["decided"]
    for k in worst:
        assert worst[k] <= TABLE_TOL[k], (k, worst[k])
    out.update(incl_ll=worst["incl"], tot_ll=worst["tot"], dbl_ll=worst["dbl"],
               incl_decided=round(decided / pairs, 4) if pairs else None)
    return out


# ---- the donor panel a freemuxlet case's clusters are scored against (muxgl_fmx_match_donors, fmx_match.hip) ---------------
# Widths: every lane width of the sweep (1, 2, 4, 8, 16, 32, 64 lanes per SNP slot), one off a power of two on either
# side, two and three donor blocks.  Draws come from a stream of their own ([seed, 82]): fmx_case stays what it is.
MATCH_V = [1, 2, 3, 5, 8, 12, 16, 17, 24, 32, 33, 64, 65, 130]
MATCH_TILES = (1, 2, 4, 8)
# The restatement takes one log and one fsum term per (cluster, donor, marker of U), about 0.1 us each, and a case asks
# for it up to twelve times (ten iterations at most, the reference's pileups, the plain engine).  K x V x S x 12 stays
# under MATCH_WORK: the panel of the widest K x S is narrowed, no element of a table is left out.
MATCH_WORK = 2e7
MATCH_CALLS = 12


def match_case(seed, info, p):
    """the panel of a freemuxlet case: V donors whose genotypes are columns of p.truth["G"] taken with replacement
    (duplicated donors are common: their columns of ll must be the same bytes), padded with random genotypes where the
    panel is wider than the pileup's donors; rows through _gp_mode or, one time in five, the mode "zeros" (a share of
    triples with one or two hard zeros, three triples zero in all three places: -inf wherever a cluster covers them);
    markers without genotypes drawn as _pileup draws missing_gp_frac (1.0: every output zero), their rows NaN.
    V is redrawn among the widths that fit MATCH_WORK where the first draw does not (the widest K x S only)."""
    r = np.random.default_rng([seed, 82])
    K, S = info["K"], p.S
    V = int(r.choice(MATCH_V))
    cap = max(1, int(MATCH_WORK // (MATCH_CALLS * K * S)))
    narrow = int(r.choice([v for v in MATCH_V if v <= cap]))   # (drawn in every case: the stream does not depend on the cap)
    if V > cap:
        V = narrow
    tile = int(r.choice(MATCH_TILES))
    G = p.truth["G"].astype(np.int64)
    take = min(V, G.shape[1])
    Gm = np.concatenate([G[:, r.integers(G.shape[1], size=take)], r.integers(0, 3, size=(S, V - take))], axis=1)
    frac = float(r.choice([0.0, 0.0, 0.03, 0.5, 1.0]))
    has_gp = np.ones(S, dtype=np.uint8)
    has_gp[r.random(S) < frac] = 0
    q = types.SimpleNamespace(S=S, gp=synth.gt_to_gp(Gm, 0.1), truth={"G": Gm})
    if r.random() < 0.2:
        mode, gp = "zeros", q.gp
        z = r.random((S, V)) < 0.3
        first = r.integers(0, 3, size=(S, V))
        second = (first + r.integers(0, 3, size=(S, V))) % 3       # (the same place one time in three: one zero, else two)
        i, j = np.nonzero(z)
        gp[i, j, first[z]] = 0.0
        gp[i, j, second[z]] = 0.0
        gp[r.integers(S, size=3), r.integers(V, size=3), :] = 0.0
    else:
        mode = _gp_mode(r, q, V)
    gp = np.ascontiguousarray(q.gp)
    cols = np.ascontiguousarray(gp[has_gp != 0].transpose(1, 0, 2))   # [V][markers with genotypes][3]
    seen, twin = {}, np.arange(V)
    for v in range(V):
        twin[v] = seen.setdefault(cols[v].tobytes(), v)              # the first donor with the same bytes
    gp[has_gp == 0] = np.nan
    return dict(V=V, tile=tile, mode=mode, gp=gp, has_gp=has_gp, twin=twin, dup_pairs=int((twin != np.arange(V)).sum()),
                missing=frac, slab=table_slab_mb(seed, "fmx"))


def _match_call(e, m):
    """the call at the case's tile size and budget; a duplicated donor's column is its twin's, byte for byte"""
    with slab_env("MUXGL_FMX_SLAB_MB", m["slab"]), slab_env("MUXGL_FMX_MATCH_TILE", str(m["tile"])):
        got = e.fmx_match_donors()
    assert got["ll"].shape[1] == m["V"]
    assert got["ll"].tobytes() == np.ascontiguousarray(got["ll"][:, m["twin"]]).tobytes(), "columns of duplicated donors differ"
    return got


def _match_worst(got, gls, cnt, m, af, tol, what):
    """every element against restate_match: nsnps equal, -inf exactly where the restatement has it, NaN and +inf nowhere,
    every finite element within tol; the worst deviation"""
    ll, ll0, nsnps = restate_match(gls, cnt, m["gp"], m["has_gp"], af)
    assert np.array_equal(got["nsnps"], nsnps), (what, "nsnps")
    worst = 0.0
    for g, w in ((got["ll"], ll), (got["ll0"], ll0)):
        assert g.shape == w.shape and not np.isnan(g).any() and not np.isposinf(g).any(), what
        assert np.array_equal(np.isneginf(g), np.isneginf(w)), (what, "-inf")
        fin = np.isfinite(w)
        if fin.any():
            worst = max(worst, float(np.max(np.abs(g[fin] - w[fin]))))
    assert worst <= tol, (what, worst)
    return worst


def _ref_cplp(w):
    """(gls, counts) of a cluster pileup of the reference, as Engine.fmx_cluster_pileup() shapes them (_check_cplp)"""
    return w["gls"], np.stack([w["nreads"], w["nref"], w["nalt"]], axis=-1)


def _match_elsewhere(eng, m, clust, K, p, w):
    """a group or a set of ranks does not answer the call: the assignment `clust` (the last iteration's) loaded into the
    plain engine, which holds the case's pileup since the start, and scored there; (match, match_ref)"""
    eng.fmx_set_clusters(K, np.ascontiguousarray(clust, dtype=np.int32))
    eng.demux_set_gp(m["gp"], m["has_gp"])
    got = _match_call(eng, m)
    g, c = eng.fmx_cluster_pileup()
    _check_cplp(g, c, w)
    return (_match_worst(got, g, c, m, p.af, TABLE_TOL["match"], "plain engine, own pileups"),
            _match_worst(got, *_ref_cplp(w), m, p.af, TABLE_TOL["match_ref"], "plain engine, reference's pileups"),
            int(np.isneginf(got["ll"]).sum()))


def fmx_case(seed):
    r = np.random.default_rng([seed, 78])
    K = int(r.choice(FMX_K))
    C, S, ment, mine, sigma = _shape(r, 2 * K, K * K * 9 * 6)
    C = max(C, 3 * K) if K <= 70 else K + 20   # (beyond 70 clusters the reference takes seconds per hundred cells)
    p = _pileup(r, 5000 + seed, C, S, max(2, int(r.choice([K, max(2, K // 2), K + 1]))), ment, mine, sigma, False)
    dp = float(r.choice([0.5, 0.5, 0.1]))
    ge = float(r.choice([0.1, 0.1, 0.01]))
    flags = int(FMX_FLAGS[int(r.integers(len(FMX_FLAGS)))])
    # one: muxgl_fmx_iterate on one handle; group: a device group of two members on this GPU; shard: the phases of a
    # multi-rank run driven by hand, two or three handles as ranks, the exact path across them (freemuxlet.settle_near_ties)
    how = str(r.choice(["one", "one", "one", "group", "shard"]))
    # the start: the greedy pass over every cell; over a fraction of them / above a score threshold (the others start
    # without a cluster); or clusters handed in (--init-cluster), some cells without one
    start = str(r.choice(["greedy", "greedy", "greedy", "partial", "given"]))
    frac = float(r.choice([0.3, 0.8])) if start == "partial" else 1.0
    thres = float(r.choice([-1e300, -0.5, 0.0])) if start == "partial" else -1e300
    init = None
    if start == "given":
        init = r.integers(-1 if r.random() < 0.7 else 0, K, size=p.C).astype(np.int32)
    return dict(kind="fmx", seed=seed, K=K, C=C, S=S, ment=ment, dp=dp, ge=ge, flags=flags, how=how,
                world=int(r.choice([2, 3])), start=start, frac=frac, thres=thres, init=init), p


def _allgather(engs, which, ranges, row_bytes):
    for owner, (b, e) in enumerate(ranges):
        if e <= b:
            continue
        src, _ = engs[owner].fmx_buffer(which)
        for r, other in enumerate(engs):
            if r != owner:
                dst, _ = other.fmx_buffer(which)
                other.memcpy_dev(dst + b * row_bytes, src + b * row_bytes, (e - b) * row_bytes)


def _check_iteration(it, ref, cells, st, K):
    rep = parity.compare_fmx(cells, ref["cells"][it])
    assert tuple(int(x) for x in st) == tuple(ref["counters"][it]), (it, st, ref["counters"][it])
    return rep


def _check_cplp(g, c, w, s0=None, s1=None):
    sl = slice(s0, s1)
    assert np.array_equal(c[:, sl], np.stack([w["nreads"], w["nref"], w["nalt"]], axis=-1)[:, sl])
    assert np.allclose(g[:, sl], w["gls"][:, sl], rtol=1e-11, atol=1e-300)


def fmx_reference(info, p):
    return rb.RefScl.from_packed(p).freemux2(info["K"], doublet_prior=info["dp"], geno_error=info["ge"],
                                            frac_init_clust=info.get("frac", 1.0),
                                            singlet_score_thres=info.get("thres", -1e300), init_clust=info.get("init"),
                                            full_ll=True, cluster_pileups=True)


def _check_raw_tie_order(raw, assigned, K):
    """The fold's order on exact ties, seen before the exact path settles them (raw: records as a rank fetched them).
    Clusters without a cell have the same pileup, so a droplet's singlet values against them are the same bits on the
    device; under (value descending, position ascending) the scans name the lowest such cluster before any other."""
    empty = np.setdiff1d(np.arange(K), assigned[assigned >= 0])
    if empty.size < 2:
        return 0
    is_empty = np.zeros(K + 1, dtype=bool)   # (slot K: "none", -1)
    is_empty[empty] = True
    b, n = raw["sBest"], raw["sNext"]
    mb, mn = is_empty[b], is_empty[n]
    assert (b[mb] == empty[0]).all() and (n[mn & mb] == empty[1]).all() and (n[mn & ~mb] == empty[0]).all(), \
        ("tie order among clusters without a cell", empty[:2], b[mb | mn][:5], n[mb | mn][:5])
    return int((mb | mn).sum())


def run_fmx(eng, info, p, ref=None, trace=None):
    """ref: fmx_reference(info, p) where the caller has it already.  trace: a list that receives, per iteration, the
    records, the counters and the cluster pileups (of a rank's own SNPs in a sharded run) as the engine gave them.
    info["stream"]: the case is expected on the streamed E-step (fmx_stream.hip) -- full_ll is refused, which is the
    documented sign of that path, and not compared; the run is made under the slab budget info["run_slab"]."""
    if info.get("stream"):
        with slab_env("MUXGL_FMX_SLAB_MB", info.get("run_slab")):
            return _run_fmx(eng, info, p, ref, trace)
    return _run_fmx(eng, info, p, ref, trace)


def _run_fmx(eng, info, p, ref, trace):
    K, dp, ge, how = info["K"], info["dp"], info["ge"], info.get("how", "one")
    init, stream = info.get("init"), bool(info.get("stream"))
    if ref is None:
        ref = fmx_reference(info, p)
    # the start on one device with the whole pileup (the greedy pass is sequential over all cells)
    eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    llk0, llk2, ns, nr = eng.fmx_prepare(p.af)
    assert np.max(np.abs(llk0 - ref["llk0"])) < 1e-7 and np.max(np.abs(llk2 - ref["llk2"])) < 1e-7
    assert np.array_equal(ns, ref["nsnps"]) and np.array_equal(nr, ref["nreads"])
    if init is None:
        clust = eng.fmx_greedy_init(K, llk2 - llk0, info.get("frac", 1.0), info.get("thres", -1e300))
        assert np.array_equal(clust, ref["clust0"]), ("greedy start", np.flatnonzero(clust != ref["clust0"])[:5])
    else:
        clust = init
    out = dict(iters=int(ref["n_iter"]), exact_scores=int(eng.fmx_score_stats()),
               greedy_near=[int(x) for x in eng.fmx_greedy_stats()])
    worst, near, sng_worst = 0.0, 0, 0.0
    slab = table_slab_mb(info["seed"], "fmx")
    m = match_case(info["seed"], info, p) if info.get("kind") == "fmx" else None   # (the streamed cases: no panel)
    match_worst = match_ref_worst = match_neginf = None
    jd = np.arange(K)
    jd = jd * (jd + 1) // 2 + jd   # the singlets among the reference's llks[K (K + 1) / 2]
    if how == "shard":
        world = info["world"]
        engs = [muxgl.Engine(0, flags=info["flags"]) for _ in range(world)]
        try:
            c_ranges = shard.cell_shards(p.cell_ptr, world)
            s_ranges = shard.snp_shards(p.entry_snp, p.S, world)
            for r, e in enumerate(engs):
                e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
                e.fmx_prepare(p.af)
                e.fmx_set_shard(*c_ranges[r], *s_ranges[r])
                e.fmx_set_clusters(K, clust)
            if m is not None:   # refused by name on a rank whose range is not everything; the ranks run on as before
                part = next(r for r in range(world) if (*c_ranges[r], *s_ranges[r]) != (0, p.C, 0, p.S))
                engs[part].demux_set_gp(m["gp"], m["has_gp"])
                with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_match_donors: not available on a sharded handle"):
                    engs[part].fmx_match_donors()
            assigned = np.asarray(clust)
            for it in range(ref["n_iter"]):
                for e in engs:
                    e.fmx_iter_gp(dp, ge)
                _allgather(engs, muxgl.BUF_CGP, s_ranges, K * 3 * 8)
                for e in engs:
                    e.fmx_iter_estep(dp, ge)
                fetched = [e.fmx_iter_fetch() for e in engs]
                if stream:
                    out["raw_ties"] = out.get("raw_ties", 0) + sum(
                        _check_raw_tie_order(cs[c_ranges[r][0]:c_ranges[r][1]], assigned, K) for r, (cs, _) in enumerate(fetched))
                if sum(e.fmx_exact_pending() for e in engs) > 0:
                    freemuxlet.settle_near_ties(engs, lambda obj: [obj], dp, ge)
                    fetched = [e.fmx_iter_fetch() for e in engs]
                _allgather(engs, muxgl.BUF_CLUST, c_ranges, 4)
                for e in engs:
                    e.fmx_iter_mstep()
                cells = np.zeros(p.C, dtype=muxgl.FMX_CELL)
                stats = np.zeros(3, dtype=np.int64)
                for r, (cs, st) in enumerate(fetched):
                    b, en = c_ranges[r]
                    cells[b:en] = cs[b:en]
                    stats += np.array(st)
                rep = _check_iteration(it, ref, cells, stats, K)
                worst, near = max(worst, rep["max_abs_ll_diff"]), near + rep["near_tie_cells"]
                assigned = cells["clust"]
                plps = []
                for r, e in enumerate(engs):
                    g, c = e.fmx_cluster_pileup()
                    _check_cplp(g, c, ref["cplp"][it], *s_ranges[r])
                    plps += [g[:, s_ranges[r][0]:s_ranges[r][1]].copy(), c[:, s_ranges[r][0]:s_ranges[r][1]].copy()]
                if trace is not None:
                    trace.append((cells, tuple(int(x) for x in stats), plps))
                with slab_env("MUXGL_FMX_SLAB_MB", slab):   # (a rank answers for its own cells)
                    sng = np.concatenate([e.fmx_singlets()[c_ranges[r][0]:c_ranges[r][1]] for r, e in enumerate(engs)])
                sng_worst = max(sng_worst, parity.compare_singlet_table(sng, ref["full_ll"][it][:, jd], TABLE_TOL["fmx_sng"]))
            out["exact"] = [int(sum(e.fmx_exact_stats()[k] for e in engs)) for k in range(3)]
            if m is not None and ref["n_iter"] > 0:
                match_worst, match_ref_worst, match_neginf = _match_elsewhere(eng, m, cells["clust"], K, p,
                                                                              ref["cplp"][ref["n_iter"] - 1])
            if stream:   # (asked last: a refused fetch has already taken the iteration's open near ties into the count)
                for e in engs:
                    with pytest.raises(muxgl.MuxglError, match="full_ll"):
                        e.fmx_iter_fetch(want_full_ll=True)
        finally:
            for e in engs:
                e.close()
    else:
        run, own = _engine(eng, info)
        try:
            if own:
                run.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
                g0, g2, _, _ = run.fmx_prepare(p.af)
                # (a device group settles near-tied scores as one device does: the same bits)
                assert np.array_equal(g0, llk0) and np.array_equal(g2, llk2), "scores of the group / flagged engine differ"
            run.fmx_set_clusters(K, clust)
            if m is not None:
                run.demux_set_gp(m["gp"], m["has_gp"])   # once: the iterations below must still be the reference's
                if how == "group":
                    with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_match_donors: not available on a device group"):
                        run.fmx_match_donors()
            if stream:   # refused before anything runs: the same handle then makes the iterations
                with pytest.raises(muxgl.MuxglError, match="full_ll"):
                    run.fmx_iterate(dp, ge, want_full_ll=True)
            for it in range(ref["n_iter"]):
                if how == "group" or stream:
                    cells, st = run.fmx_iterate(dp, ge)
                else:
                    cells, st, full = run.fmx_iterate(dp, ge, want_full_ll=True)
                    d = np.abs(full - ref["full_ll"][it])
                    d = d[np.isfinite(d)]
                    worst = max(worst, float(d.max()) if d.size else 0.0)
                rep = _check_iteration(it, ref, cells, st, K)
                worst, near = max(worst, rep["max_abs_ll_diff"]), near + rep["near_tie_cells"]
                g, c = run.fmx_cluster_pileup()
                _check_cplp(g, c, ref["cplp"][it])
                if trace is not None:
                    trace.append((cells, tuple(int(x) for x in st), [g, c]))
                with slab_env("MUXGL_FMX_SLAB_MB", slab):
                    sng = run.fmx_singlets()
                sng_worst = max(sng_worst, parity.compare_singlet_table(sng, ref["full_ll"][it][:, jd], TABLE_TOL["fmx_sng"]))
                if m is not None and how == "one":   # the table of this iteration's pileups, on the running handle
                    got = _match_call(run, m)
                    match_worst = max(match_worst or 0.0, _match_worst(got, g, c, m, p.af, TABLE_TOL["match"],
                                                                       f"iteration {it}, own pileups"))
                    if it == ref["n_iter"] - 1:
                        match_neginf = int(np.isneginf(got["ll"]).sum())
                        match_ref_worst = _match_worst(got, *_ref_cplp(ref["cplp"][it]), m, p.af, TABLE_TOL["match_ref"],
                                                       f"iteration {it}, reference's pileups")
            out["exact"] = [int(x) for x in run.fmx_exact_stats()]
            if m is not None and how == "group" and ref["n_iter"] > 0:
                match_worst, match_ref_worst, match_neginf = _match_elsewhere(eng, m, cells["clust"], K, p,
                                                                              ref["cplp"][ref["n_iter"] - 1])
        finally:
            if own:
                run.close()
    assert worst < 1e-7, worst
    out.update(ll=worst, near=near, fmx_sng_ll=sng_worst, table_slab_mb=slab)
    if m is not None:
        out.update(match_ll=match_worst, match_ref_ll=match_ref_worst, match_v=m["V"], match_tile=m["tile"],
                   match_mode=m["mode"], match_dup=m["dup_pairs"], match_missing=m["missing"], match_neginf=match_neginf)
    return out


# ---- the streamed paths: demux_stream.hip (sweep, top2 fold, call) and fmx_stream.hip (sweep, fold, call, rows of the
# exact pass).  Widths: the smallest that reach every structural case of a walk over 64 x 64 blocks -- one block, one off
# a block boundary on either side, a multiple of 64, several blocks; forced by flag up to 255, the product's own choice
# beyond.  Draws come from streams of their own ([seed, 80], [seed, 81]): demux_case / fmx_case stay what they are.
STREAM_DEMUX_V = [33, 40, 63, 64, 65, 96, 128, 129, 130, 200, 255]
STREAM_DEMUX_V_NATURAL = [256, 257, 300, 320]
STREAM_FMX_K = [33, 40, 63, 64, 65, 100, 128, 129, 200, 255]
STREAM_FMX_K_NATURAL = [256, 257, 300, 320]
STREAM_GRIDS = GRIDS + [(0.5, 0.2)]


def stream_demux_case(seed):
    r = np.random.default_rng([seed, 80])
    natural = bool(r.random() < 0.3)
    V = int(r.choice(STREAM_DEMUX_V_NATURAL if natural else STREAM_DEMUX_V))
    alphas = STREAM_GRIDS[int(r.integers(len(STREAM_GRIDS)))]
    C, S, ment, mine, sigma = _shape(r, V, V * V * len(alphas) * 9)
    p = _pileup(r, 7000 + seed, C, S, V, ment, mine, sigma, True)
    mode = _gp_mode(r, p, V)
    dp = float(r.choice([0.5, 0.1, 0.9]))
    flags = (0 if natural else muxgl.FLAG_FORCE_STREAMED_CALL) | int(r.choice([0, muxgl.FLAG_NO_LINEAR_ENTRIES]))
    how = str(r.choice(["one", "one", "one", "group"]))
    run_slab = "1" if r.random() < 0.5 else None   # MUXGL_DEMUX_SLAB_MB of the run itself (None: the default budget)
    return dict(kind="stream-demux", seed=seed, V=V, alphas=alphas, C=C, S=S, ment=ment, mode=mode, dp=dp, flags=flags,
                how=how, run_slab=run_slab, missing_gp=round(1.0 - float(np.mean(p.has_gp)), 3),
                empty_cells=int(np.sum(np.diff(p.cell_ptr) == 0))), p


def stream_fmx_case(seed):
    r = np.random.default_rng([seed, 81])
    natural = bool(r.random() < 0.3)
    K = int(r.choice(STREAM_FMX_K_NATURAL if natural else STREAM_FMX_K))
    C, S, ment, mine, sigma = _shape(r, 2 * K, K * K * 9 * 6)
    C = max(C, 3 * K) if K <= 70 else K + 20
    p = _pileup(r, 9000 + seed, C, S, max(2, int(r.choice([K, max(2, K // 2), K + 1]))), ment, mine, sigma, False)
    dp = float(r.choice([0.5, 0.1]))
    ge = float(r.choice([0.1, 0.01]))
    flags = (0 if natural else muxgl.FLAG_FORCE_STREAMED_ESTEP) | int(r.choice(
        [0, muxgl.FLAG_NO_LINEAR_ENTRIES, muxgl.FLAG_NO_PIVOT_SUMS, muxgl.FLAG_NO_LINEAR_ENTRIES | muxgl.FLAG_NO_PIVOT_SUMS]))
    how = str(r.choice(["one", "one", "group", "shard"]))
    start = str(r.choice(["greedy", "greedy", "partial", "given"]))
    frac = float(r.choice([0.3, 0.8])) if start == "partial" else 1.0
    thres = float(r.choice([-1e300, -0.5, 0.0])) if start == "partial" else -1e300
    init = None
    if start == "given":   # some cells start without a cluster, some clusters without a cell
        init = r.integers(-1, K, size=p.C).astype(np.int32)
    run_slab = "1" if r.random() < 0.5 else None   # MUXGL_FMX_SLAB_MB of the run itself
    return dict(kind="stream-fmx", seed=seed, K=K, C=C, S=S, ment=ment, dp=dp, ge=ge, flags=flags, how=how,
                world=int(r.choice([2, 3])), start=start, frac=frac, thres=thres, init=init, run_slab=run_slab,
                stream=True, empty_cells=int(np.sum(np.diff(p.cell_ptr) == 0))), p


def _demux_handle(info, p, flags):
    e = muxgl.Engine([0, 0] if info["how"] == "group" else 0, flags=flags)
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)
    return e


def run_stream_demux(eng, info, p):
    """the streamed call against the reference; below 256 samples also against the path the job takes without the flag
    and with the reference's full_ll behind the tables; under a 1 MB slab budget also against the default budget"""
    from test_demux_many_samples_gpu import _same_after_exact

    alphas, dp, V = info["alphas"], info["dp"], info["V"]
    forced = bool(info["flags"] & muxgl.FLAG_FORCE_STREAMED_CALL)
    assert forced == (V <= 255)
    want, _, want_ll = rb.RefScl.from_packed(p).demux(alphas, doublet_prior=dp, full_ll=forced)
    with _demux_handle(info, p, info["flags"]) as e:
        with slab_env("MUXGL_DEMUX_SLAB_MB", info["run_slab"]):
            with pytest.raises(muxgl.MuxglError, match="full_ll"):   # the documented sign of the streamed path
                e.demux_run(alphas, dp, want_full_ll=True)
            got = e.demux_run(alphas, dp)
        rep = parity.compare_demux(got, want, alphas, p, doublet_prior=dp)
        assert rep["max_abs_ll_diff"] < 1e-7, rep
        st = rep["exact_pass"]
        out = dict(ll=rep["max_abs_ll_diff"], looked_at=int(st["cells"]), near=int(st["near_ties"]), deep=int(st["deep"]),
                   changed=int(st["changed"]), raw_differing=rep["raw_records_differing"])
        if info["mode"] == "all_same":
            # The fold's order on exact ties, before the exact-call pass settles them: every sample has the same rows,
            # so every singlet is the same product of the same factors, on the device as in the reference, and both
            # keep the first in scan order (value descending, then position ascending; strict '<')
            v = want["valid"] == 1
            assert np.array_equal(got["sBest"][v], want["sBest"][v]) and np.array_equal(got["sNext"][v], want["sNext"][v]), \
                "raw singlet calls among identical samples"
        if info["run_slab"] is not None:   # the budget only cuts the groups: the raw records are the same bytes
            with slab_env("MUXGL_DEMUX_SLAB_MB", None):
                assert e.demux_run(alphas, dp).tobytes() == got.tobytes(), "records differ between slab budgets"
        if forced:
            out.update(_demux_tables(e, info, want_ll))
        else:   # (no full_ll of the reference at this width: the singlet table against the records' best singlet)
            with slab_env("MUXGL_DEMUX_SLAB_MB", table_slab_mb(info["seed"], "demux")):
                sng = e.demux_singlets(alphas)
            v = want["valid"] == 1
            out["sng_ll"] = parity.compare_singlet_table(sng[v, want["sBest"][v]][:, None], want["sngBestLLK"][v][:, None],
                                                         TABLE_TOL["sng"])
    if forced:
        with _demux_handle(info, p, info["flags"] & ~muxgl.FLAG_FORCE_STREAMED_CALL) as e:
            _same_after_exact(got, e.demux_run(alphas, dp), alphas, p, dp)
    return out


def _same_traces(a, b, records):
    assert len(a) == len(b)
    for (ca, sa, pa), (cb, sb, pb) in zip(a, b):
        assert sa == sb, (sa, sb)
        records(ca, cb)
        assert len(pa) == len(pb) and all(np.array_equal(x, y) for x, y in zip(pa, pb)), "cluster pileups differ"


def _same_bytes(a, b):
    assert a.tobytes() == b.tobytes(), "records differ between slab budgets"


def run_stream_fmx(eng, info, p):
    """run_fmx's checks on the streamed E-step; below 256 clusters also against the path the job takes without the flag
    (records by parity.same_records, counters and cluster pileups bit for bit); under a 1 MB slab budget also against
    the default budget (records byte for byte)"""
    forced = bool(info["flags"] & muxgl.FLAG_FORCE_STREAMED_ESTEP)
    assert forced == (info["K"] <= 255) and info["stream"]
    ref = fmx_reference(info, p)
    trace = []
    out = run_fmx(eng, info, p, ref, trace)
    if info["run_slab"] is not None:
        again = []
        run_fmx(eng, dict(info, run_slab=None), p, ref, again)
        _same_traces(trace, again, _same_bytes)
    if forced:
        plain = []
        run_fmx(eng, dict(info, flags=info["flags"] & ~muxgl.FLAG_FORCE_STREAMED_ESTEP, stream=False), p, ref, plain)
        _same_traces(trace, plain, parity.same_records)
    return out


CASES = {"demux": (demux_case, run_demux), "fmx": (fmx_case, run_fmx),
         "stream-demux": (stream_demux_case, run_stream_demux), "stream-fmx": (stream_fmx_case, run_stream_fmx)}


def run_case(eng, kind, seed):
    case, run = CASES[kind]
    info, p = case(seed)
    info["nnz"] = int(p.nnz)
    info.update(run(eng, info, p))
    info.pop("init", None)
    return info


@pytest.fixture(scope="module")
def eng():
    e = muxgl.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_demuxlet_fuzz(eng, seed):
    run_case(eng, "demux", seed)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_freemuxlet_fuzz(eng, seed):
    run_case(eng, "fmx", seed)


def test_unfiltered_droplets_among_cells():
    """a few hundred cells among thousands of droplets of one to a handful of reads (tests/stress_droplets.py): scores of
    0 +- rounding noise, noise-level ties in the greedy pass and in every iteration -- all of it the reference's"""
    import stress_droplets

    assert stress_droplets.main(["300", "3000", "8", "30000"]) == 0


def main(argv):
    import argparse
    import traceback

    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0:50")
    ap.add_argument("--kind", default="both", choices=["both"] + list(CASES))
    ap.add_argument("--log", default=None)
    ap.add_argument("--keep-going", action="store_true")
    ap.add_argument("--budget-s", type=float, default=1e9, help="stop starting new cases after this many seconds")
    a = ap.parse_args(argv)
    lo, hi = (int(x) for x in a.seeds.split(":"))
    e = muxgl.Engine(0)
    log = open(a.log, "a") if a.log else None
    t0, fails, n = time.time(), 0, 0
    for seed in range(lo, hi):
        for kind in (("demux", "fmx") if a.kind == "both" else (a.kind,)):
            if time.time() - t0 > a.budget_s:
                break
            t = time.time()
            try:
                rec = run_case(e, kind, seed)
                rec["ok"] = True
            except Exception as ex:  # noqa: BLE001  (a campaign reports and goes on or stops, as asked)
                info, _ = CASES[kind][0](seed)
                info.pop("init", None)
                rec = dict(info, ok=False, error=f"{type(ex).__name__}: {str(ex)[:600]}",
                           where=traceback.format_exc().strip().splitlines()[-3:])
                fails += 1
            rec["s"] = round(time.time() - t, 2)
            n += 1
            line = json.dumps(rec, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
            print(line, flush=True)
            if log:
                log.write(line + "\n")
                log.flush()
            if fails and not a.keep_going:
                return 1
    print(json.dumps({"cases": n, "failed": fails, "seconds": round(time.time() - t0, 1)}), flush=True)
    if log:
        log.write(json.dumps({"cases": n, "failed": fails, "seconds": round(time.time() - t0, 1)}) + "\n")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
