"""The reference of a freemuxlet run with PRIOR anchors (muxgl_fmx_set_anchors_mode), expressed through the oracle UNCHANGED.

oracle_fmx_iterate forms a cluster's posterior row from the diagonal d of its pileup and the Hardy-Weinberg triple p only
(cmd_cram_freemux2.cpp:402-415): norm(p * d), mixed with p by geno_error.  A PRIOR cluster's row is norm(w * d), mixed with
p, with w the donor's panel row.  So before every oracle iteration the diagonal of a PRIOR cluster is replaced, at the
markers with genotypes, by d' = d * w / p -- then p * d' is w * d up to three roundings -- and the oracle's own M-step
rebuilds the true pileup from the droplets afterwards, which is what the device's pileups are compared against.  af stays
inside (0.01, 0.99), so p >= 1e-4 and d' is finite; a zero in w is a zero in d' and in the row.

The substituted rows are not the device's rows bit for bit (prior_rows is the plain form; the two are within a few ulp,
tests/test_fmx_prior.py measures it), so a decision that hangs on the last bits could differ.  seed_condition() runs the
oracle's trajectory a second time with every substituted diagonal moved by one ulp (np.nextafter) and wants every integer
field and counter equal: the cases below pass it, and tests/test_fmx_prior.py keeps it so.

HELD clusters are tests/fmx_anchor_ref.py's: their panel rows ARE the oracle's rows of drawn diagonals, bit for bit.
"""
import numpy as np

import fmx_anchor_ref as ar
import oracle_binding as ob
import parity
from popscle_amd import muxgl, synth

HELD, PRIOR = muxgl.ANCHOR_HELD, muxgl.ANCHOR_PRIOR
XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
ITERS = 2
SLOTS = (0, 4, 8)


def hwe(af):
    """the Hardy-Weinberg triples [S][3] in the reference's operations (:388-390); no contraction is possible in them"""
    a = np.asarray(af, dtype=np.float64)
    return np.stack([(1 - a) * (1 - a), 2 * a * (1 - a), a * a], axis=-1)


def prior_rows(w, d, af, has_gp, geno_error):
    """The posterior rows [S][n][3] of PRIOR clusters, plain numpy float64: w [S][n][3] their donors' panel rows, d [S][n][3]
    their own pileup diagonals.  q = w d / sum(w d) with w := p at markers without genotypes, mixed with p by geno_error."""
    p = hwe(af)[:, None, :]
    w = np.where(np.asarray(has_gp).astype(bool)[:, None, None], w, p)
    g = w * d
    q = g / (g[:, :, 0] + g[:, :, 1] + g[:, :, 2])[:, :, None]
    if geno_error > 0:
        q = (1 - geno_error) * q + geno_error * p
    return q


def substituted(w, d, af, has_gp):
    """d' [S][n][3] = d * w / p at the markers with genotypes, d elsewhere"""
    p = hwe(af)[:, None, :]
    return np.where(np.asarray(has_gp).astype(bool)[:, None, None], d * w / p, d)


def ulps(a, b):
    """distance of two arrays of non-negative doubles in units of the last place"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int64) - b.view(np.int64))


def make_case(C, S, ment, V, seed, hole_frac=0.2, n_true=None, min_entries=30):
    """tests/test_fmx_anchor_gpu.py::make_case, and the genotypes G [S][V] the panel is drawn from"""
    n_true = min(V, 8) if n_true is None else n_true
    p = synth.make_pileup(C, S, n_true, seed=seed, mean_entries=ment, min_entries=min_entries, with_gp=False)
    assert p.af.min() > 0.01 and p.af.max() < 0.99
    rng = np.random.default_rng([seed, 77])
    G = np.empty((S, V), dtype=np.int64)
    m = min(V, n_true)
    G[:, :m] = p.truth["G"][:, :m]
    G[:, m:] = rng.binomial(2, p.af[:, None], size=(S, V - m))
    has_gp = (rng.random(S) >= hole_frac).astype(np.uint8)
    return p, G, has_gp


SOFT = np.array([0.90, 0.09, 0.01])   # by the distance from the donor's genotype
ZERO = np.array([0.75, 0.25, 0.0])    # an exact zero two steps away (one step away where the genotype is the heterozygote)


def make_panel(p, G, has_gp, prior_donors, geno_error, seed):
    """(panel [S][V][3] for muxgl_demux_set_gp, d [S][V][3] the diagonals behind the HELD donors' rows).  Every column starts
    as tests/fmx_anchor_ref.py's (the oracle's rows of drawn diagonals: what a HELD cluster needs).  The columns of
    prior_donors are then mixed marker by marker: a quarter each of those rows (informative, geno_error mixed in), soft rows,
    flat rows (1/3 each) and rows with an exact zero."""
    d = ar.draw_diag(G, has_gp)
    panel = ar.panel_rows(d, p.af, geno_error)
    rng = np.random.default_rng([seed, 78])
    dist = np.abs(np.arange(3)[None, :] - G[:, :, None])   # [S][V][3]
    for v in sorted(set(prior_donors)):
        kind = rng.integers(0, 4, p.S)
        col = panel[:, v].copy()
        col[kind == 1] = SOFT[dist[kind == 1, v]]
        col[kind == 2] = 1.0 / 3.0
        z = ZERO[np.minimum(dist[kind == 3, v], 2)]
        het = G[kind == 3, v] == 1
        z[het] = (0.0, 0.75, 0.25)
        col[kind == 3] = z
        panel[:, v] = col
    return ar.device_panel(panel, has_gp), d


def random_start(C, K, seed):
    rng = np.random.default_rng([seed, 3])
    c = rng.integers(0, K, C).astype(np.int32)
    c[rng.random(C) < 0.1] = -1
    return c


def _write(cplp, d_held, panel, p, has_gp, donors, modes, bump):
    """the anchored clusters' diagonals before an oracle iteration: HELD := the drawn d, PRIOR := d' of the true diagonal"""
    for i, (v, m) in enumerate(zip(donors, modes)):
        if m == HELD:
            for slot, g in zip(SLOTS, range(3)):
                cplp["gls"][i, :, slot] = d_held[:, v, g]
        else:
            true = np.stack([cplp["gls"][i, :, slot] for slot in SLOTS], axis=-1)[:, None, :]
            sub = substituted(panel[:, v][:, None, :], true, p.af, has_gp)[:, 0]
            if bump:
                sub = np.where(np.asarray(has_gp).astype(bool)[:, None], np.nextafter(sub, np.inf), sub)
            for slot, g in zip(SLOTS, range(3)):
                cplp["gls"][i, :, slot] = sub[:, g]


def oracle_trajectory(p, K, n_iter, donors, modes, panel, d_held, has_gp, clust, doublet_prior=0.5, geno_error=0.1,
                      bump=False, want_full=False, oracle_threads=4):
    """the oracle's side alone: per iteration (records, counters, full_ll or None, the true cluster pileups after it)"""
    e = ob.fmx_entry_pileup(p)
    cplp = ob.fmx_build_cluster_pileup(p, e, K, clust)
    cells = ob.fmx_init_cells(clust)
    out = []
    for _ in range(n_iter):
        _write(cplp, d_held, panel, p, has_gp, donors, modes, bump)
        st = ob.fmx_iterate(p, e, K, cplp, cells, doublet_prior, geno_error, full_ll=want_full, nthreads=oracle_threads)
        out.append((cells.copy(), tuple(st[:3]), st[3] if want_full else None, cplp.copy()))
    return out


def seed_condition(p, K, n_iter, donors, modes, panel, d_held, has_gp, clust, geno_error=0.1):
    """No decision of the oracle's trajectory hangs on bits the substitution cannot pin: with every substituted diagonal one
    ulp up, all integer fields of all records and the counters are the same.  Returns the number of records compared."""
    a = oracle_trajectory(p, K, n_iter, donors, modes, panel, d_held, has_gp, clust, geno_error=geno_error)
    b = oracle_trajectory(p, K, n_iter, donors, modes, panel, d_held, has_gp, clust, geno_error=geno_error, bump=True)
    n = 0
    for it, ((ca, sa, _, _), (cb, sb, _, _)) in enumerate(zip(a, b)):
        assert sa == sb, f"iteration {it}: counters {sa} vs {sb}"
        for name in ca.dtype.names:
            if np.issubdtype(ca.dtype[name], np.integer):
                assert np.array_equal(ca[name], cb[name]), f"iteration {it}: {name} differs"
        n += ca.size
    return n


def run_prior_em(eng, p, K, n_iter, donors, modes, panel, d_held, has_gp, clust, doublet_prior=0.5, geno_error=0.1,
                 want_full=True, want_pileups=True, oracle_threads=4):
    """tests/test_fmx_gpu.py::run_em for a run with HELD and PRIOR anchors: the plain run's bar over the whole trajectory --
    full_ll within 1e-7 (want_full), every integer field of every record exact (parity.compare_fmx), the three counters
    equal, the cluster pileups (the true, droplet-derived ones) allclose at rtol 1e-11 (want_pileups).  Returns the worst
    log-likelihood deviation of the records, the worst full_ll deviation and the last records."""
    e = ob.fmx_entry_pileup(p)
    cplp = ob.fmx_build_cluster_pileup(p, e, K, clust)
    cells = ob.fmx_init_cells(clust)
    eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    eng.fmx_prepare(p.af)
    eng.demux_set_gp(panel, has_gp)
    eng.fmx_set_clusters(K, clust)
    eng.fmx_set_anchors(donors, modes)
    assert eng.n_anchor == len(donors) and eng.anchor_modes == tuple(modes)
    worst, worst_full, gcells = 0.0, 0.0, None
    for it in range(n_iter):
        _write(cplp, d_held, panel, p, has_gp, donors, modes, False)
        ostats = ob.fmx_iterate(p, e, K, cplp, cells, doublet_prior, geno_error, full_ll=want_full, nthreads=oracle_threads)
        if want_full:
            gcells, gstats, gfull = eng.fmx_iterate(doublet_prior, geno_error, want_full_ll=True)
            dd = np.abs(gfull - ostats[3])
            dev = float(np.max(dd[np.isfinite(dd)], initial=0.0))
            worst_full = max(worst_full, dev)
            print(f"iteration {it}: full_ll max deviation {dev:.3e}")
            assert dev < 1e-7, f"iteration {it}: E-step LL tensor off by {dev}"
        else:
            gcells, gstats = eng.fmx_iterate(doublet_prior, geno_error)
        rep = parity.compare_fmx(gcells, cells)
        worst = max(worst, rep["max_abs_ll_diff"])
        assert tuple(gstats) == tuple(ostats[:3]), f"iteration {it}: (nsingle, namb, nchanged) {gstats} vs {ostats[:3]}"
        if want_pileups:
            g, c = eng.fmx_cluster_pileup()
            assert np.array_equal(c, np.stack([cplp["nreads"], cplp["nref"], cplp["nalt"]], axis=-1))
            assert np.allclose(g, cplp["gls"], rtol=1e-11, atol=1e-300), f"iteration {it}: cluster pileup differs"
    print(f"K={K} anchors={len(donors)} prior={sum(modes)}: worst record deviation {worst:.3e}, worst full_ll deviation "
          f"{worst_full:.3e}")
    return worst, worst_full, gcells


PERM39 = [int(x) for x in np.random.default_rng(39).permutation(40)[:39]]
ALT = lambda n: [PRIOR if i % 2 == 0 else HELD for i in range(n)]   # noqa: E731  (cluster 0 PRIOR, 1 HELD, ...)

# the trajectories of tests/test_fmx_prior_gpu.py, one per E-step path and edge of the kernel's lane mapping; the seed
# condition above is checked for each of them in tests/test_fmx_prior.py
#        name            K    C    S     ment V    donors            modes                 ge   holes flags full   pileups
TRAJ = [("k4",           4,   200, 1001, 200, 2,   [0, 1],           [PRIOR, HELD],        0.1, 0.2,  0,    True,  True),
        ("k5_all_prior", 5,   150, 999,  150, 3,   [2, 0, 1],        [PRIOR] * 3,          0.1, 0.2,  0,    True,  True),
        ("k16_all",      16,  120, 1500, 250, 16,  list(range(16)),  ALT(16),              0.1, 0.2,  0,    True,  True),
        ("k20_one",      20,  100, 1203, 300, 3,   [1],              [PRIOR],              0.1, 0.2,  0,    True,  True),
        ("k27_ge0",      27,  60,  2000, 300, 26,  list(range(26)),  ALT(26),              0.0, 0.2,  0,    True,  True),
        ("k40",          40,  40,  3001, 400, 40,  PERM39,           ALT(39),              0.1, 0.2,  0,    True,  True),
        ("k40_streamed", 40,  40,  3001, 400, 40,  PERM39,           ALT(39),              0.1, 0.2,  XE,   False, True),
        ("k260",         260, 24,  800,  100, 130, list(range(130)), ALT(130),             0.1, 0.2,  0,    False, False)]


def near_tie_case():
    """the shape of tests/test_fmx_anchor_gpu.py's near-tie test: droplets of a handful of entries, one HELD and one PRIOR
    anchor, two free clusters with cells and two without (exact ties in the reference, the scan order decides)"""
    K, donors, modes = 6, [1, 0], [HELD, PRIOR]
    p, G, has_gp = make_case(300, 400, 8, 2, seed=9601, n_true=3, min_entries=1)
    panel, d = make_panel(p, G, has_gp, [0], 0.1, 9601)
    rng = np.random.default_rng(K)
    clust = rng.integers(0, 4, p.C).astype(np.int32)   # clusters 4 and 5 stay empty
    clust[rng.random(p.C) < 0.1] = -1
    return p, K, 3, donors, modes, panel, d, has_gp, clust


def traj_inputs(name, K, C, S, ment, V, donors, modes, ge, holes, flags, full, pileups):
    seed = 9100 + K + len(donors)
    p, G, has_gp = make_case(C, S, ment, V, seed=seed, hole_frac=holes)
    panel, d = make_panel(p, G, has_gp, [v for v, m in zip(donors, modes) if m == PRIOR], ge, seed)
    return p, panel, d, has_gp, random_start(p.C, K, K)
