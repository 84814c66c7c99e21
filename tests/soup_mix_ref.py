"""Reference values of muxgl_pileup_read_hist and muxgl_demux_soup_mix (include/muxgl.h) for their tests.

fit(): the model restated in numpy, in longdouble (the yardstick) or float64, from a read histogram.  Components: the V
samples of the panel and optionally component V, whose genotype prior is the panel mean (rows added in sample order, one
division) or a caller's [S][3].  r_v = g0 + g1 / 2, a_v = g1 / 2 + g2; D = pR * R + pA * A with R = sum pi_v r_v,
A = sum pi_v a_v; LL = sum n log D; grad_v = (1 / N) sum_s [r_v sum_b n pR / D + a_v sum_b n pA / D]; pi' = pi * grad.
The records that take part are those of markers with genotypes and R + A > 0 at the start.  The iteration rule is the
header's: LL and grad at the current pi, ll[i]; stop at i == n_iter_max (status 1); else step and stop after a step with
max |pi' - pi| <= tol (status 0), LL and grad once more at the final pi in the next slot.

planted_pool(): ambient_ref.soup_pileup with unequal shares, a share of nearly empty droplets that hold only soup reads,
several base qualities and optionally a donor outside the panel."""
import numpy as np

import ambient_ref as ar
from popscle_amd import synth

READ_OTHER = ar.READ_OTHER

# |LL - LL_longdouble| allowed for a float64 evaluation with T records: LL is a sum of T terms n log D of absolute size sum_abs
# = sum |n log D|.  Each term carries a few units of relative rounding from D (two products, one sum, the M-term dots R and A:
# (M + 4) u in the worst case, u = 2^-53) through d(n log D) = n dD / D and from the log and the product; their ordered sum
# adds at most T u sum_abs.  The tests' shapes have T <= 1e4 records, sum_abs <= 2e4 (<= 1e4 reads at |log D| <= 2) and M <=
# 301, so the worst case is 1e4 * 1.1e-16 * 2e4 + 1e4 * 305 * 1.1e-16 < 3e-8; seen: ~1e-11 (errors do not align).
LL_TOL = 3e-8


def read_hist(p, mask=None):
    """(keys, counts) int64: the usable reads of the droplets of the mask as a histogram, keys = marker * 256 + byte
    ascending (numpy unique)"""
    ent = np.repeat(np.arange(p.nnz), np.diff(p.entry_rptr))
    keep = p.reads != READ_OTHER
    if mask is not None:
        cell_of = np.repeat(np.arange(p.C), np.diff(p.cell_ptr))
        keep &= np.asarray(mask, dtype=bool)[cell_of[ent]]
    k = p.entry_snp[ent][keep].astype(np.int64) * 256 + p.reads[keep].astype(np.int64)
    keys, counts = np.unique(k, return_counts=True)
    return keys.astype(np.int64), counts.astype(np.int64)


def read_hist_definition(p, mask=None):
    """the same by its definition: a loop over droplets, entries and reads into a dict"""
    h = {}
    for c in range(p.C):
        if mask is not None and not mask[c]:
            continue
        for e in range(int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])):
            for b in p.reads[int(p.entry_rptr[e]):int(p.entry_rptr[e + 1])]:
                if int(b) != READ_OTHER:
                    k = int(p.entry_snp[e]) * 256 + int(b)
                    h[k] = h.get(k, 0) + 1
    keys = np.array(sorted(h), dtype=np.int64)
    return keys, np.array([h[int(k)] for k in keys], dtype=np.int64)


def panel_mean(gp, has_gp):
    """[S][3]: the rows of the panel added in sample order, one division (muxgl_demux_unknown's prior); (1, 0, 0) without
    genotypes"""
    u = np.zeros((gp.shape[0], 3))
    for j in range(gp.shape[1]):
        u += gp[:, j, :]
    u /= float(gp.shape[1])
    u[np.asarray(has_gp) == 0] = (1.0, 0.0, 0.0)
    return u


def hwe_prior(af):
    """[S][3]: Hardy-Weinberg genotype frequencies of the ALT frequency af"""
    af = np.asarray(af, dtype=np.float64)
    return np.stack([(1.0 - af) ** 2, 2.0 * af * (1.0 - af), af ** 2], axis=1)


def components(gp, has_gp, with_unknown=False, gp0=None, dtype=np.float64):
    """(r, a), each [S][M] in dtype"""
    g = np.asarray(gp, dtype=np.float64)
    if with_unknown:
        u = panel_mean(g, has_gp) if gp0 is None else np.asarray(gp0, dtype=np.float64)
        g = np.concatenate([g, u[:, None, :]], axis=1)
    g = g.astype(dtype)
    half = dtype(0.5)
    return g[:, :, 0] + half * g[:, :, 1], half * g[:, :, 1] + g[:, :, 2]


def read_probs(bytes_, dtype=np.float64):
    """(pR, pA) of read bytes, as demux_entry.hpp takes them from the Phred table (float64 table values, then dtype)"""
    b = np.asarray(bytes_, dtype=np.int64)
    alt, bq = b >> 7, b & 0x7F
    mat = np.asarray(ar.MAT, dtype=np.float64)[bq]
    e3 = np.asarray(ar.ERR, dtype=np.float64)[bq] / 3.0
    return np.where(alt == 0, mat, e3).astype(dtype), np.where(alt == 0, e3, mat).astype(dtype)


class Model:
    """the records that take part at the start pi, and LL / grad / profile at any pi"""

    def __init__(self, keys, counts, gp, has_gp, pi_start, with_unknown=False, gp0=None, dtype=np.longdouble):
        self.dtype = dtype
        self.has_gp = np.asarray(has_gp) != 0
        self.r, self.a = components(gp, has_gp, with_unknown, gp0, dtype)
        keys = np.asarray(keys, dtype=np.int64)
        s = keys >> 8
        pi = np.asarray(pi_start, dtype=dtype)
        ra = self.r @ pi + self.a @ pi
        on = self.has_gp[s] & (ra[s] > 0) if s.size else np.zeros(0, dtype=bool)
        self.s = s[on]
        self.n = np.asarray(counts, dtype=np.int64)[on].astype(dtype)
        self.pR, self.pA = read_probs(keys[on] & 0xFF, dtype)
        self.N = int(np.asarray(counts, dtype=np.int64)[on].sum())
        self.markers, self.idx = np.unique(self.s, return_inverse=True)

    def evaluate(self, pi):
        """(LL, grad) at pi"""
        pi = np.asarray(pi, dtype=self.dtype)
        r, a = self.r[self.markers], self.a[self.markers]
        R, A = r @ pi, a @ pi
        D = self.pR * R[self.idx] + self.pA * A[self.idx]
        ll = (self.n * np.log(D)).sum()
        wR = np.zeros(self.markers.size, dtype=self.dtype)
        wA = np.zeros(self.markers.size, dtype=self.dtype)
        np.add.at(wR, self.idx, self.n * self.pR / D)
        np.add.at(wA, self.idx, self.n * self.pA / D)
        return ll, (r.T @ wR + a.T @ wA) / self.dtype(self.N)

    def profile(self, pi):
        """amb_af [S] at pi: A / (R + A), 0.5 without genotypes or with R + A == 0"""
        pi = np.asarray(pi, dtype=self.dtype)
        R, A = self.r @ pi, self.a @ pi
        t = R + A
        ok = self.has_gp & (t > 0)
        return np.where(ok, A / np.where(ok, t, 1), self.dtype(0.5))

    def information(self, pi):
        """the observed information of LL in the M shares, -d2 LL / dpi dpi: sum n d d^T / D^2, d_v = pR r_v + pA a_v"""
        pi = np.asarray(pi, dtype=np.float64)
        r = self.r[self.markers].astype(np.float64)[self.idx]
        a = self.a[self.markers].astype(np.float64)[self.idx]
        d = self.pR.astype(np.float64)[:, None] * r + self.pA.astype(np.float64)[:, None] * a
        D = d @ pi
        w = self.n.astype(np.float64) / (D * D)
        return (d * w[:, None]).T @ d


def start_of(M, pi0, dtype):
    if pi0 is None:
        return np.full(M, 1.0 / M, dtype=np.float64).astype(dtype)
    pi0 = np.asarray(pi0, dtype=np.float64)
    s = 0.0
    for x in pi0:          # (added in component order, as the library does)
        s += float(x)
    return (pi0 / s).astype(dtype)


def fit(keys, counts, gp, has_gp, with_unknown=False, gp0=None, pi0=None, n_iter_max=500, tol=1e-8, dtype=np.longdouble):
    """dict of pi, grad [M], ll [n_iter_max + 1] (NaN tail), amb_af [S] (all in dtype), n_iter, n_reads, status, model"""
    M = gp.shape[1] + (1 if with_unknown else 0)
    pi = start_of(M, pi0, dtype)
    m = Model(keys, counts, gp, has_gp, pi, with_unknown, gp0, dtype)
    ll = np.full(n_iter_max + 1, np.nan, dtype=dtype)
    if m.N == 0:
        ll[0] = 0
        return dict(pi=pi, grad=np.zeros(M, dtype=dtype), ll=ll, amb_af=m.profile(pi), n_iter=0, n_reads=0, status=2, model=m)
    n_iter, status = 0, 1
    i = 0
    while True:
        ll[i], grad = m.evaluate(pi)
        if i == n_iter_max:
            break
        new = pi * grad
        step = np.abs(new - pi).max()
        pi = new
        n_iter = i + 1
        if step <= tol:
            ll[i + 1], grad = m.evaluate(pi)
            status = 0
            break
        i += 1
    return dict(pi=pi, grad=grad, ll=ll, amb_af=m.profile(pi), n_iter=n_iter, n_reads=m.N, status=status, model=m)


def simplex_se(info):
    """standard errors of the M shares from the observed information [M][M], on the simplex sum pi = 1: the first M - 1
    shares are free, the last is 1 minus their sum; cov = J (J^T info J)^-1 J^T"""
    M = info.shape[0]
    if M == 1:
        return np.zeros(1)
    J = np.concatenate([np.eye(M - 1), -np.ones((1, M - 1))], axis=0)
    cov = J @ np.linalg.inv(J.T @ info @ J) @ J.T
    return np.sqrt(np.diag(cov))


def planted_pool(C=400, S=3000, shares=(0.40, 0.25, 0.15, 0.10, 0.07, 0.03), seed=5, n_empty=266, empty_markers=20,
                 cell_markers=150, soup=0.1, bqs=(20, 30, 37), geno_err=0.01, outside=0.0):
    """A pileup with a planted soup.  The pool's free RNA is that of the donors with the given shares; with outside > 0 a
    further donor who is NOT in the panel holds that share (the panel's shares are scaled by 1 - outside).  The first
    n_empty droplets are nearly empty: empty_markers markers, one read each, all from the soup.  The others hold one cell
    of a panel donor (cell_markers markers, 1 + Poisson(1) reads each, a read from the soup with probability `soup`).
    Every read draws its base quality from bqs and is miscalled with that quality's probability.  Returns (pileup, mask
    of the nearly empty droplets, the true pool ALT fraction [S], the true shares [V] or [V + 1])."""
    rng = np.random.default_rng(seed)
    V = len(shares)
    w = np.asarray(shares, dtype=np.float64)
    w = w / w.sum()
    if outside > 0.0:
        w = np.concatenate([w * (1.0 - outside), [outside]])
    af = rng.uniform(0.1, 0.9, size=S)
    G = (rng.random((S, w.size)) < af[:, None]).astype(np.int64) + (rng.random((S, w.size)) < af[:, None]).astype(np.int64)
    pool = (G @ w) / 2.0
    who = rng.integers(0, V, size=C)
    per = np.where(np.arange(C) < n_empty, empty_markers, cell_markers)
    cell_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    snp = np.concatenate([np.sort(rng.choice(S, size=k, replace=False)) for k in per]).astype(np.int32)
    cell_of_e = np.repeat(np.arange(C), per)
    nreads = np.where(cell_of_e < n_empty, 1, 1 + rng.poisson(1.0, size=snp.size))
    rptr = np.concatenate([[0], np.cumsum(nreads)]).astype(np.int64)
    ent = np.repeat(np.arange(snp.size), nreads)
    cell_of = cell_of_e[ent]
    s_of = snp[ent]
    from_soup = (cell_of < n_empty) | (rng.random(ent.size) < soup)
    p_alt = np.where(from_soup, pool[s_of], G[s_of, who[cell_of]] / 2.0)
    alt = rng.random(ent.size) < p_alt
    bq = rng.choice(np.asarray(bqs), size=ent.size)
    alt ^= rng.random(ent.size) < 10.0 ** (-bq / 10.0)
    reads = ((alt.astype(np.uint8) << 7) | bq.astype(np.uint8)).astype(np.uint8)
    p = synth.Pileup(C, S, cell_ptr, snp, rptr, reads, af, synth.gt_to_gp(G[:, :V], geno_err), np.ones(S, dtype=np.uint8))
    return p, np.arange(C) < n_empty, pool, w


# the planted pools of the tests (CPU: the restatement, tests/test_soup_mix.py; GPU: the device, tests/test_soup_mix_gpu.py);
# the seeds are fixed so that the restatement itself meets the checks
POOL = dict(seed=5)
POOL_OUTSIDE = dict(seed=6, outside=0.15)


def check_planted(fit_out, model, truth, pool, count_profile, what=""):
    """the planted-pool assertions on a fit (of the restatement or of the device): every share within 4 standard errors of
    the truth, and a fitted profile closer to the true pool fraction than the count profile; prints both"""
    pi = np.asarray(fit_out["pi"], dtype=np.float64)
    se = simplex_se(model.information(pi))
    z = (pi - truth) / se
    mae_fit = float(np.abs(np.asarray(fit_out["amb_af"], dtype=np.float64) - pool).mean())
    mae_cnt = float(np.abs(count_profile - pool).mean())
    print(f"soup mix {what}: shares {np.round(pi, 4).tolist()}, se {np.round(se, 4).tolist()}, z {np.round(z, 2).tolist()}; "
          f"profile MAE fit {mae_fit:.4f} / counts {mae_cnt:.4f}; {fit_out['n_iter']} steps, status {fit_out['status']}")
    assert np.all(np.abs(z) <= 4.0), z
    assert mae_fit < mae_cnt
    return z
