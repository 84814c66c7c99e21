"""Reference values of muxgl_demux_ambient (include/muxgl.h) for its tests.

table(): a plain restatement.  The reference's per-read loop (cmd_cram_demuxlet.cpp:655-725) runs with 3 * n_rho ambient
elements carried along, one per (rho, l), whose p is the reference's own expression with the second donor's genotype m
replaced by twice the ambient ALT fraction f of the marker: p = 0.5 * l + (2 * f - l) * 0.5 * rho.  They are divided by the
same per-read and final maxima as the grid's NA * 9 elements and take part in none of them.  Then the l loop of :738-746
with a second donor that is no donor: sumPs = sum_l gp[j][l] * w[r][l], added from 0 in the order l = 0, 1, 2, one log
per (entry, sample, rho) added into the droplet's sum.  Elementwise numpy over the elements of one entry: every operation
is the reference's, on IEEE doubles, in its order (numpy fuses nothing).

reference_slice(): where f is 0, 0.5 or 1 at every marker and the rhos are the grid, the same numbers from the reference
itself: the panel with one donor appended whose row at marker s is one-hot at genotype 2 * f[s]; llksAB[(j, V, n)] of that
run (tests/unknown_ref.py: the reference's own loop where it was built, else the oracle).  The terms the one-hot row
zeroes are exact zeros, so table(exact_log=True) must equal the slice bit for bit (tests/test_demux_ambient.py)."""
import math

import numpy as np

import oracle_binding as ob
import unknown_ref as ur
from popscle_amd import muxgl, synth

READ_OTHER = synth.READ_OTHER
ERR, MAT = ob.phred_tables()


def grid_p(alphas):
    """p of :673 for the NA * 9 elements of the grid, in the reference's element order k * 9 + l * 3 + m"""
    return np.array([0.5 * l + (m - l) * 0.5 * float(a) for a in alphas for l in range(3) for m in range(3)])


def ambient_p(f, rhos):
    """p of the 3 * n_rho ambient elements, order r * 3 + l"""
    return np.array([0.5 * l + (2.0 * float(f) - l) * 0.5 * float(r) for r in rhos for l in range(3)])


def entry_weights(reads, pg, pa):
    """:655-725 for one entry with the ambient elements carried along: w [n_rho][3] and the grid's pGs [NA * 9]"""
    g = np.ones(pg.size)
    a = np.ones(pa.size)
    for b in reads:
        b = int(b)
        if b == READ_OTHER:                                   # :664
            continue
        al, bq = b >> 7, b & 0x7F
        pR = float(MAT[bq]) if al == 0 else float(ERR[bq]) / 3.0   # :666
        pA = float(MAT[bq]) if al == 1 else float(ERR[bq]) / 3.0   # :667
        g *= (pR * (1.0 - pg) + pA * pg)                      # :685
        a *= (pR * (1.0 - pa) + pA * pa)
        mx = g.max()                                          # :686-687: the grid's elements only
        g /= mx                                               # :696
        a /= mx
    g += 1e-10                                                # :710
    a += 1e-10
    mx = g.max()                                              # :711-712
    g /= mx                                                   # :722
    a /= mx
    return a.reshape(-1, 3), g


def table(p, alphas, amb_af, rhos, exact_log=False):
    """ll_amb [C][V][n_rho] of pileup p.  exact_log: math.log (glibc, what the reference calls) per element instead of
    np.log, for the bit-for-bit comparison with the reference's slice"""
    V, NR = p.gp.shape[1], len(rhos)
    pg = grid_p(alphas)
    out = np.zeros((p.C, V, NR))
    pa_of = {}
    for c in range(p.C):
        for e in range(int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])):
            s = int(p.entry_snp[e])
            if not p.has_gp[s]:                               # :733
                continue
            f = float(amb_af[s])
            if f not in pa_of:
                pa_of[f] = ambient_p(f, rhos)
            w, _ = entry_weights(p.reads[int(p.entry_rptr[e]):int(p.entry_rptr[e + 1])], pg, pa_of[f])
            gp = p.gp[s]                                      # [V][3]
            for r in range(NR):
                sm = np.zeros(V)                              # :737
                for l in range(3):                            # :738-742 (the terms of the other m are exact zeros)
                    sm += gp[:, l] * w[r, l]
                if exact_log:
                    out[c, :, r] += [math.log(x) for x in sm]  # :746
                else:
                    out[c, :, r] += np.log(sm)
    return out


def onehot_rows(amb_af):
    """[S][3] one-hot at genotype 2 * f; f must be 0, 0.5 or 1 everywhere"""
    m = np.asarray(amb_af, dtype=np.float64) * 2.0
    assert np.isin(m, (0.0, 1.0, 2.0)).all()
    u = np.zeros((m.size, 3))
    u[np.arange(m.size), m.astype(np.int64)] = 1.0
    return u


def reference_slice(p, alphas, amb_af):
    """ll_amb [C][V][A] for rhos == alphas and f in {0, 0.5, 1}: the reference's llksAB[(j, V, n)] with the one-hot donor
    appended as sample V"""
    V = p.gp.shape[1]
    full = ur.full_ll(ur.with_panel(p, np.concatenate([p.gp, onehot_rows(amb_af)[:, None, :]], axis=1)), alphas)
    return np.ascontiguousarray(full[:, :V, V, :])


def singlet_slice(p, alphas):
    """the reference's singlet slot llksAB[(j, 0, 0)], [C][V]"""
    return np.ascontiguousarray(ur.full_ll(p, alphas)[:, :, 0, 0])


def draw_onehot_af(S, seed):
    return np.random.default_rng(seed).choice([0.0, 0.5, 1.0], size=S)


def draw_af(S, seed, corners=0.1):
    """uniform in [0, 1], exactly 0 and exactly 1 on a share `corners` of the markers each"""
    rng = np.random.default_rng(seed)
    f = rng.random(S)
    u = rng.random(S)
    f[u < corners] = 0.0
    f[u > 1.0 - corners] = 1.0
    return f


def assert_table(got, want, tol, what=""):
    """every element within tol; prints and returns the worst deviation"""
    assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape)
    d = np.abs(got - want)
    assert np.isfinite(d).all(), what
    worst = float(d.max()) if d.size else 0.0
    print(f"ambient {what}: shape {got.shape}, max |dLL| {worst:.3e}")
    assert worst <= tol, f"{what}: {int((d > tol).sum())} elements beyond {tol}; worst {worst}"
    return worst


def soup_pileup(C, S, V, markers, soup, seed, reads_mean=2.0, bq=30, geno_err=0.01):
    """A pileup made for the ambient model: droplet c holds one cell of sample c % V; a read comes with probability `soup`
    from the pool (ALT with the pool's fraction at the marker: the mean genotype of the samples / 2) and else from the
    cell (ALT with genotype / 2), and is miscalled with the probability of its base quality.  `markers` markers per
    droplet, 1 + Poisson(reads_mean - 1) reads each.  Returns (pileup, sample of every droplet, the pool's fractions)."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.1, 0.9, size=S)
    G = (rng.random((S, V)) < af[:, None]).astype(np.int64) + (rng.random((S, V)) < af[:, None]).astype(np.int64)
    pool = G.mean(axis=1) / 2.0
    who = np.arange(C) % V
    cell_ptr = np.arange(C + 1, dtype=np.int64) * markers
    snp = np.concatenate([np.sort(rng.choice(S, size=markers, replace=False)) for _ in range(C)]).astype(np.int32)
    nreads = 1 + rng.poisson(reads_mean - 1.0, size=snp.size)
    rptr = np.concatenate([[0], np.cumsum(nreads)]).astype(np.int64)
    ent = np.repeat(np.arange(snp.size), nreads)
    cell_of = np.repeat(np.arange(C), markers)[ent]
    s_of = snp[ent]
    from_soup = rng.random(ent.size) < soup
    p_alt = np.where(from_soup, pool[s_of], G[s_of, who[cell_of]] / 2.0)
    alt = rng.random(ent.size) < p_alt
    alt ^= rng.random(ent.size) < 10.0 ** (-bq / 10.0)
    reads = (alt.astype(np.uint8) << 7) | np.uint8(bq)
    p = synth.Pileup(C, S, cell_ptr, snp, rptr, reads.astype(np.uint8), af, synth.gt_to_gp(G, geno_err),
                     np.ones(S, dtype=np.uint8))
    return p, who, pool


def allele_counts(p, mask=None):
    """(n_ref, n_alt) int64 [S]: the usable reads of the droplets of the mask by marker and allele (numpy bincount)"""
    ent = np.repeat(np.arange(p.nnz), np.diff(p.entry_rptr))
    keep = p.reads != READ_OTHER
    if mask is not None:
        cell_of = np.repeat(np.arange(p.C), np.diff(p.cell_ptr))
        keep &= np.asarray(mask, dtype=bool)[cell_of[ent]]
    s = p.entry_snp[ent][keep]
    alt = (p.reads[keep] >> 7).astype(bool)
    return (np.bincount(s[~alt], minlength=p.S).astype(np.int64), np.bincount(s[alt], minlength=p.S).astype(np.int64))


# the pileup of the sanity test (CPU: the restatement, tests/test_demux_ambient.py; GPU: the device, tests/test_demux_ambient_gpu.py);
# the seed is fixed so that the model itself meets the checks below
SOUP = dict(C=24, S=1500, V=6, markers=300, soup=0.2, seed=11)


def check_soup_calls(ll, who, rhos):
    """the checks of the issue's sanity test on a table of the soup pileup"""
    sm = muxgl.ambient_summary(ll, rhos)
    assert np.array_equal(sm["amb_sample"], who)                              # the right sample for every droplet
    near = np.isin(sm["amb_rho_idx"], [i for i, r in enumerate(rhos) if r in (0.15, 0.2, 0.3)])
    print(f"soup: best rho per droplet {np.asarray(rhos)[sm['amb_rho_idx']].tolist()}")
    assert near.mean() >= 0.9                                                 # 0.2 or a neighbour on the grid
    sng = ll[np.arange(ll.shape[0]), who, list(rhos).index(0.0)]
    assert np.all(sm["amb_llk"] > sng)                                        # beats the singlet reading of the same sample
    return sm
