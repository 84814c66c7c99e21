"""The reference of an anchored freemuxlet run (muxgl_fmx_set_anchors), expressed through the oracle UNCHANGED.

oracle_fmx_iterate forms a cluster's posterior row from the diagonal of its pileup and from nothing else
(cmd_cram_freemux2.cpp:402-415): norm(HWE(af) * (gls[0], gls[4], gls[8])), mixed with HWE by geno_error.  So a panel whose
rows ARE such posteriors can be fed to both sides: per (marker, donor) a positive diagonal d is drawn, the panel row is
computed from (d, af, geno_error) in numpy float64 with the reference's operations in the reference's order -- it goes to
muxgl_demux_set_gp --, and before every oracle iteration d is written into the diagonals of the anchored clusters' pileups
(the oracle's own M-step rebuilds them from the droplets each time).  A marker without genotypes gets d = (1, 1, 1), the
pileup of a cluster without cells.  The rows are then equal bit for bit (assert_rows_are_the_oracles checks it, on the CPU),
and the bar of an anchored trajectory is the one tests/test_fmx_gpu.py::run_em sets for plain runs.
"""
import math

import numpy as np

import oracle_binding as ob
import parity

DIAG = (1.0, 1e-3, 1e-6)  # d at the donor's genotype, one step and two steps away from it


def draw_diag(G, has_gp):
    """d [S][V][3]: DIAG by the distance from the true genotype G [S][V]; (1, 1, 1) where has_gp is 0"""
    G = np.asarray(G, dtype=np.int64)
    d = np.take(np.array(DIAG), np.abs(np.arange(3)[None, None, :] - G[:, :, None]))
    d[np.asarray(has_gp) == 0] = 1.0
    return np.ascontiguousarray(d, dtype=np.float64)


def panel_rows(d, af, geno_error):
    """The posterior rows [S][V][3] the oracle forms from the diagonals d: elementwise float64, the reference's operations in
    its order (products left to right, the left-to-right sum, three divisions, the mix)."""
    a = np.asarray(af, dtype=np.float64)[:, None]
    p0 = (1.0 - a) * (1.0 - a)
    p1 = 2 * a * (1.0 - a)
    p2 = a * a
    g0 = p0 * d[:, :, 0]
    g1 = p1 * d[:, :, 1]
    g2 = p2 * d[:, :, 2]
    s = g0 + g1 + g2
    g0 = g0 / s
    g1 = g1 / s
    g2 = g2 / s
    if geno_error > 0:
        g0 = (1 - geno_error) * g0 + geno_error * p0
        g1 = (1 - geno_error) * g1 + geno_error * p1
        g2 = (1 - geno_error) * g2 + geno_error * p2
    return np.ascontiguousarray(np.stack([g0, g1, g2], axis=-1))


def device_panel(rows, has_gp):
    """what muxgl_demux_set_gp gets: the rows, and at markers without genotypes values nobody may read as data"""
    gp = rows.copy()
    gp[np.asarray(has_gp) == 0] = (0.2, 0.3, 0.5)
    return gp


def write_diagonals(cplp, d, donors):
    """the anchored clusters' pileup diagonals := d of their donors (in place; before every oracle_fmx_iterate)"""
    for i, v in enumerate(donors):
        for slot, g in ((0, 0), (4, 1), (8, 2)):
            cplp["gls"][i, :, slot] = d[:, v, g]


def assert_rows_are_the_oracles(seed=5, S=64, V=3, geno_error=0.1):
    """The oracle's posterior rows equal panel_rows bit for bit.  Seen through full_ll: a droplet of ONE entry at marker s has
    the singlet log-likelihood log(((gl[0] r0) + gl[4] r1) + gl[8] r2) against a cluster whose row at s is r
    (cmd_cram_freemux2.cpp:448-455; glibc's log on both sides, math.log) -- any other row moves it."""
    from popscle_amd import synth

    rng = np.random.default_rng(seed)
    cell_ptr = np.arange(S + 1, dtype=np.int64)          # cell s holds one entry, at marker s
    entry_snp = np.arange(S, dtype=np.int32)
    entry_rptr = np.arange(S + 1, dtype=np.int64)        # one read each
    reads = ((rng.integers(0, 2, S) << 7) | rng.integers(13, 21, S)).astype(np.uint8)
    af = rng.uniform(0.05, 0.95, S)
    p = synth.Pileup(S, S, cell_ptr, entry_snp, entry_rptr, reads, af)
    G = rng.integers(0, 3, (S, V))
    has_gp = (rng.random(S) > 0.25).astype(np.uint8)
    d = draw_diag(G, has_gp)
    rows = panel_rows(d, af, geno_error)
    e = ob.fmx_entry_pileup(p)
    clust = np.full(S, -1, dtype=np.int32)
    cplp = ob.fmx_build_cluster_pileup(p, e, V, clust)
    cells = ob.fmx_init_cells(clust)
    write_diagonals(cplp, d, list(range(V)))
    full = ob.fmx_iterate(p, e, V, cplp, cells, 0.5, geno_error, full_ll=True)[3]
    for s in range(S):
        gl = e["gls"][s]
        for j in range(V):
            r = rows[s, j]
            lk = 0.0
            for g in range(3):
                lk += gl[4 * g] * r[g]
            assert full[s, j * (j + 1) // 2 + j] == 0.0 + math.log(lk), (s, j)
    return int(has_gp.sum()), S


def run_anchored_em(eng, p, K, n_iter, donors, d, has_gp, clust=None, doublet_prior=0.5, geno_error=0.1, want_full=True,
                    want_pileups=True, oracle_threads=4):
    """tests/test_fmx_gpu.py::run_em for an anchored run: the engine with clusters 0 .. len(donors)-1 held to the panel of
    (d, has_gp), the oracle with d in those clusters' diagonals.  Over the whole trajectory: full_ll within 1e-7
    (want_full), every integer field of every record exact (parity.compare_fmx), the three counters equal, the cluster
    pileups allclose at rtol 1e-11 -- the anchored clusters' droplet-derived ones included (want_pileups).  Returns the
    worst log-likelihood deviation, the last records and the oracle's last full_ll."""
    e = ob.fmx_entry_pileup(p)
    llk0, llk2, _, _ = ob.fmx_cell_scores(p, e)
    if clust is None:
        clust = ob.fmx_greedy_init(p, e, K, llk2 - llk0, ob.fmx_sort(llk2 - llk0))
    cplp = ob.fmx_build_cluster_pileup(p, e, K, clust)
    cells = ob.fmx_init_cells(clust)
    eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    eng.fmx_prepare(p.af)
    eng.demux_set_gp(device_panel(panel_rows(d, p.af, geno_error), has_gp), has_gp)
    eng.fmx_set_clusters(K, clust)
    eng.fmx_set_anchors(donors)
    assert eng.n_anchor == len(donors)
    worst, gcells, ofull = 0.0, None, None
    for it in range(n_iter):
        write_diagonals(cplp, d, donors)
        ostats = ob.fmx_iterate(p, e, K, cplp, cells, doublet_prior, geno_error, full_ll=want_full, nthreads=oracle_threads)
        if want_full:
            gcells, gstats, gfull = eng.fmx_iterate(doublet_prior, geno_error, want_full_ll=True)
            ofull = ostats[3]
            dd = np.abs(gfull - ofull)
            print(f"iteration {it}: full_ll max deviation {np.max(dd[np.isfinite(dd)], initial=0.0):.3e}")
            assert np.max(dd[np.isfinite(dd)], initial=0.0) < 1e-7, f"iteration {it}: E-step LL tensor off by {dd.max()}"
        else:
            gcells, gstats = eng.fmx_iterate(doublet_prior, geno_error)
        rep = parity.compare_fmx(gcells, cells)
        worst = max(worst, rep["max_abs_ll_diff"])
        assert tuple(gstats) == tuple(ostats[:3]), f"iteration {it}: (nsingle, namb, nchanged) {gstats} vs {ostats[:3]}"
        if want_pileups:
            g, c = eng.fmx_cluster_pileup()
            assert np.array_equal(c, np.stack([cplp["nreads"], cplp["nref"], cplp["nalt"]], axis=-1))
            assert np.allclose(g, cplp["gls"], rtol=1e-11, atol=1e-300), f"iteration {it}: cluster pileup differs"
    print(f"K={K} n_anchor={len(donors)}: worst record deviation {worst:.3e}")
    return worst, gcells, ofull
