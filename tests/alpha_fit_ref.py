"""Reference values of muxgl_demux_alpha_fit (include/muxgl.h) for its tests, on top of ambient_fit_ref.py.

Cell(p, alphas, c, j, k).eval(): LL, LL' and LL'' of droplet c as a mix of samples j and k at a share alpha of k.  The
per-read loop is the reference's (cmd_cram_demuxlet.cpp:655-725: multiply, then divide by the grid's maximum, after every
read; + 1e-10 and the final maximum at the end) with the nine elements of one alpha and their first two derivatives
carried beside the grid's:
    t = pR * (1 - p) + pA * p,  p = 0.5 * l + (m - l) * 0.5 * alpha (:673),  v = dt/dalpha = (pA - pR) * (m - l) * 0.5
    a'' = a'' * t + 2 * a' * v;   a' = a' * t + a * v;   a = a * t
and the derivatives divided by whatever divides a (the 1e-10 is added to a alone: its derivative is 0).  Then
D = sum_l sum_m (gp[j][l] * gp[k][m]) * w[l][m] from 0 in the order l, then m (:738-742), D', D'' with (l, m) next to
(m, l), and
LL = sum log D, LL' = sum D'/D, LL'' = sum (D''/D - (D'/D)^2) over the entries whose marker has genotypes.  It runs in
float64 and in np.longdouble.  At an alpha of the grid the nine elements are the grid's own, operation for operation, so
ll_exact() (float64, math.log, the entries added one after the other as :746 does) is the reference's llksAB[j][k][n].

bracket(), maximise() and fit() are fit_ref_core.py's (they use eval() only); the scan of maximise() has 17 points in
float64 here, cheaper on the nine elements of a pair: LL differs by whole units between them, rounding by 1e-12.

doublet_pileup() / shaped_pileup(): pileups whose droplets hold cells of two samples."""
import math

import numpy as np

import ambient_fit_ref as afr
import ambient_ref as ar
import fit_ref_core as core

READ_OTHER = ar.READ_OTHER
coarse_points, bracket = core.coarse_points, core.bracket
SCAN = (16, np.float64)


class Cell(afr.Cell):
    """the entries of droplet c whose marker has genotypes, for the pair of columns (j, k), as padded numpy rows"""

    def __init__(self, p, alphas, c, j, k):
        super().__init__(p, alphas, np.zeros(p.S), c, j)
        es = [e for e in range(int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])) if p.has_gp[int(p.entry_snp[e])]]
        snp = p.entry_snp[es].astype(np.int64) if es else np.zeros(0, dtype=np.int64)
        self.gpk = np.asarray(p.gp, dtype=np.float64)[snp, k, :] if es else np.zeros((0, 3))

    def _terms(self, xs, dtype):
        """D, D', D'' and the sums of absolute summands A', A'', each [n][len(xs)]"""
        x = np.asarray(xs, dtype=dtype).reshape(-1)
        R = x.size
        mxs, mxf = self.grid_maxima(dtype)
        lm = [(l, m) for l in range(3) for m in range(3)]
        # p of :673 in its own order of operations; dp = (m - l) * 0.5
        p = np.stack([dtype(0.5) * dtype(l) + dtype(m - l) * dtype(0.5) * x for l, m in lm], axis=1)[None, :, :]   # [1][R][9]
        dp = np.array([dtype(m - l) * dtype(0.5) for l, m in lm], dtype=dtype)
        a = np.ones((self.n, R, 9), dtype=dtype)
        a1 = np.zeros_like(a)
        a2 = np.zeros_like(a)
        for r in range(self.maxr):
            idx, pR, pA = self._read_probs(r, dtype)
            t = pR[:, None, None] * (dtype(1.0) - p) + pA[:, None, None] * p                                        # :685
            v = ((pA - pR)[:, None] * dp[None, :])[:, None, :]
            mx = mxs[idx, r][:, None, None]
            x0, x1, x2 = a[idx], a1[idx], a2[idx]
            a2[idx] = (x2 * t + dtype(2.0) * x1 * v) / mx
            a1[idx] = (x1 * t + x0 * v) / mx
            a[idx] = (x0 * t) / mx                                                                                  # :696
        a = a + dtype(1e-10)                                                                                        # :710
        mx = mxf[:, None, None]
        a, a1, a2 = a / mx, a1 / mx, a2 / mx                                                                        # :722
        gj, gk = self.gp.astype(dtype), self.gpk.astype(dtype)
        D = np.zeros((self.n, R), dtype=dtype)
        D1, D2, A1, A2 = D.copy(), D.copy(), D.copy(), D.copy()
        g = [(gj[:, l] * gk[:, m])[:, None] for l, m in lm]                                                         # :740
        for i in range(9):                                                                                          # :738-742
            D = D + g[i] * a[:, :, i]
            A1 = A1 + np.abs(g[i] * a1[:, :, i])
            A2 = A2 + np.abs(g[i] * a2[:, :, i])
        # D', D'': the diagonal's terms are exact zeros; (l, m) is added next to (m, l), so that a pair of samples with the
        # same GP rows at alpha = 0.5, where a_lm' == -a_ml' bit for bit, has D' == 0 exactly as in exact arithmetic (LL is
        # symmetric about 0.5 there) instead of a residue of rounding whose sign would decide "on the bound or inside"
        for i, k in ((1, 3), (2, 6), (5, 7)):
            D1 = D1 + (g[i] * a1[:, :, i] + g[k] * a1[:, :, k])
            D2 = D2 + (g[i] * a2[:, :, i] + g[k] * a2[:, :, k])
        return D, D1, D2, A1, A2

    def eval(self, xs, dtype=np.float64):
        """(LL, LL', LL'', sum |log D|, sum |D'/D|, sum (|D''/D| + (D'/D)^2), sum A'/D, sum (A''/D + (A'/D)^2)), each
        [len(xs)], as ambient_fit_ref.Cell.eval returns them: the fourth to sixth are the sums of absolute per-entry
        terms, the last two the same over absolute summands"""
        if self.n == 0:
            return core.eval_empty(np.asarray(xs).reshape(-1).size, dtype)
        return core.eval_tail(*self._terms(xs, dtype))

    def ll_exact(self, xs):
        """LL in float64 as the reference adds it (:746): glibc's log per entry, the entries one after the other from 0"""
        xs = np.asarray(xs, dtype=np.float64).reshape(-1)
        if self.n == 0:
            return np.zeros(xs.size)
        D = self._terms(xs, np.float64)[0]
        out = np.zeros(xs.size)
        for r in range(xs.size):
            s = 0.0
            for e in range(self.n):
                s += math.log(float(D[e, r]))
            out[r] = s
        return out


def maximise(cell, lo, hi, n_scan=SCAN[0]):
    """fit_ref_core.maximise with this module's scan"""
    return core.maximise(cell, lo, hi, n_scan, SCAN[1])


def fit(p, alphas, c, j, k, alpha_max):
    """dict of the restated outputs of one (droplet, pair): alpha_hat, ll_hat, ll_zero, ll_top, info, status (0, 1, 2 or 5)"""
    return core.fit(Cell(p, alphas, c, j, k), "alpha", alpha_max, top=True, can_fail=False, scan=SCAN)


def second_sample(C, V):
    """the sample of the second cell of droplet c: never the first's (c % V) where V > 1, all others in turn"""
    c = np.arange(C)
    return (c % V + 1 + (c // V) % max(V - 1, 1)) % V


def _draw(rng, S, V):
    af = rng.uniform(0.1, 0.9, size=S)
    G = (rng.random((S, V)) < af[:, None]).astype(np.int64) + (rng.random((S, V)) < af[:, None]).astype(np.int64)
    return af, G


def doublet_pileup(C, S, V, markers, shares, seed, reads_mean=2.0, bq=30, geno_err=0.01):
    """A pileup made for the mixing share, in the manner of ambient_ref.soup_pileup: droplet c holds cells of samples
    c % V and second_sample(C, V)[c]; a read comes from the second cell with probability shares[c] (a scalar: the same for
    all) and else from the first (ALT with genotype / 2), and is miscalled with the probability of its base quality.
    `markers` markers per droplet, 1 + Poisson(reads_mean - 1) reads each.  Returns (pileup, first [C], second [C])."""
    rng = np.random.default_rng(seed)
    af, G = _draw(rng, S, V)
    first, second = np.arange(C) % V, second_sample(C, V)
    share = np.broadcast_to(np.asarray(shares, dtype=np.float64), (C,))
    cell_ptr = np.arange(C + 1, dtype=np.int64) * markers
    snp = np.concatenate([np.sort(rng.choice(S, size=markers, replace=False)) for _ in range(C)]).astype(np.int32)
    nreads = 1 + rng.poisson(reads_mean - 1.0, size=snp.size)
    rptr = np.concatenate([[0], np.cumsum(nreads)]).astype(np.int64)
    ent = np.repeat(np.arange(snp.size), nreads)
    cell_of = np.repeat(np.arange(C), markers)[ent]
    s_of = snp[ent]
    from_second = rng.random(ent.size) < share[cell_of]
    p_alt = G[s_of, np.where(from_second, second[cell_of], first[cell_of])] / 2.0
    alt = rng.random(ent.size) < p_alt
    alt ^= rng.random(ent.size) < 10.0 ** (-bq / 10.0)
    reads = (alt.astype(np.uint8) << 7) | np.uint8(bq)
    p = ar.synth.Pileup(C, S, cell_ptr, snp, rptr, reads.astype(np.uint8), af, ar.synth.gt_to_gp(G, geno_err),
                        np.ones(S, dtype=np.uint8))
    return p, first, second


def shaped_pileup(cell_entries, S, V, seed, share=0.3, **kw):
    """ambient_fit_ref.shaped_pileup (its depths, base qualities, READ_OTHER share and missing-genotype share, and its
    keywords) with another donor rule: droplet c holds cells of samples c % V and second_sample(C, V)[c] (the same one where
    V == 1) and a read comes from the second with probability `share`.  Returns (pileup, first [C], second [C])."""
    C = len(cell_entries)
    first, second = np.arange(C) % V, second_sample(C, V)
    donor = lambda G, s_of, cell_of, from_second: G[s_of, np.where(from_second, second[cell_of], first[cell_of])] / 2.0
    return afr.shaped_pileup(cell_entries, S, V, seed, share, p_alt_of=donor, **kw)[0], first, second


# the pileups of the sanity tests (CPU: the restatement, tests/test_demux_alpha_fit.py; GPU: the device,
# tests/test_demux_alpha_fit_gpu.py); the seed is fixed so that the model itself meets the checks there
MIXED_SHARES = tuple([0.15, 0.3, 0.5] * 8)
MIXED = dict(C=24, S=1500, V=6, markers=300, shares=MIXED_SHARES, seed=11)
CLEAN = dict(C=24, S=1500, V=6, markers=300, shares=0.0, seed=11)
