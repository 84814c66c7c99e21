"""Reference values of muxgl_fmx_ambient_fit (include/muxgl.h) for its tests, on top of fmx_ambient_ref.py and in the
manner of ambient_fit_ref.py.

Cell.eval(): LL, LL' and LL'' of one (droplet, cluster) at a share rho.  The per-read loop is that of
fmx_ambient_ref.entry_weights (the nine multiplied, summed in index order to t, everything divided by t; after the reads
the 1e-6 floor and the division by T, the sum of the floored nine) with the three ambient elements of one rho and their
first two derivatives carried along:
    fac = mat * x + e4,  x = ALT read ? p : 1 - p,  p = (2 * f - l) * (0.5 * rho) + 0.5 * l
    v = dfac/drho = +-mat * (2 * f - l) * 0.5                                            (+ for an ALT read)
    a'' = a'' * fac + 2 * a' * v;   a' = a' * fac + a * v;   a = a * fac;   all three divided by t
and after the reads, where a < 1e-6: a = 1e-6, a' = a'' = 0 -- the derivative of the floored function on that piece.  Then
w = a / T, D = (q[0] * w[0] + q[1] * w[1]) + q[2] * w[2], D', D'' likewise, and LL = sum log D, LL' = sum D'/D,
LL'' = sum (D''/D - (D'/D)^2) over ALL entries of the droplet (freemuxlet has no has_gp).  It runs in float64 and in
np.longdouble; the entries of a droplet are walked side by side (numpy rows), every row in the per-read order above.

bracket(), maximise() (a 65-point scan in longdouble), fit() and sign_changes() are fit_ref_core.py's: they ask a cell for
eval() only."""
import numpy as np

import ambient_fit_ref as afr
import fit_ref_core as core
import fmx_ambient_ref as fr

READ_OTHER = fr.READ_OTHER
shaped_pileup = afr.shaped_pileup
coarse_points, bracket, maximise, sign_changes = core.coarse_points, core.bracket, core.maximise, core.sign_changes


class Cell:
    """the entries of droplet c for candidate cluster j with the posteriors q [S][K][3], as padded numpy rows"""

    def __init__(self, p, q, amb_af, c, j):
        e0, e1 = int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])
        self.n = e1 - e0
        snp = p.entry_snp[e0:e1].astype(np.int64)
        self.f = np.asarray(amb_af, dtype=np.float64)[snp]
        self.q = np.asarray(q, dtype=np.float64)[snp, j, :] if self.n else np.zeros((0, 3))
        lens = np.diff(p.entry_rptr[e0:e1 + 1]).astype(np.int64) if self.n else np.zeros(0, dtype=np.int64)
        self.maxr = int(lens.max()) if self.n else 0
        self.reads = np.full((self.n, self.maxr), READ_OTHER, dtype=np.int64)
        for i in range(self.n):
            r0 = int(p.entry_rptr[e0 + i])
            self.reads[i, :lens[i]] = p.reads[r0:r0 + int(lens[i])]
        self._nine = {}
        self._probs = {}

    def _read_probs(self, r, dtype):
        """the rows whose read r is usable (:468), whether it is an ALT read, and its mat and e4, cached"""
        key = (r, dtype)
        if key not in self._probs:
            b = self.reads[:, r]
            idx = np.flatnonzero(b != READ_OTHER)
            al, bq = (b[idx] >> 7).astype(bool), b[idx] & 0x7F
            self._probs[key] = (idx, al, fr.MAT[bq].astype(dtype), fr.ERR[bq].astype(dtype) / dtype(4.0))
        return self._probs[key]

    def nine_sums(self, dtype):
        """per entry: the sum t of the nine after every read [n][maxr] (1 where the read is skipped) and T, the sum of the
        floored nine [n] (:472-504)"""
        if dtype not in self._nine:
            g = np.ones((self.n, 9), dtype=dtype)
            ts = np.ones((self.n, self.maxr), dtype=dtype)
            fref, falt = fr.FRAC_REF.astype(dtype), fr.FRAC_ALT.astype(dtype)
            for r in range(self.maxr):
                idx, al, mat, e4 = self._read_probs(r, dtype)
                gn = g[idx] * (mat[:, None] * np.where(al[:, None], falt[None, :], fref[None, :]) + e4[:, None])
                t = np.zeros(idx.size, dtype=dtype)
                for i in range(9):                                                # :493, in index order
                    t = t + gn[:, i]
                g[idx] = gn / t[:, None]
                ts[idx, r] = t
            g[g < dtype(fr.MIN_NORM_GL)] = dtype(fr.MIN_NORM_GL)                  # :498-501
            T = np.zeros(self.n, dtype=dtype)
            for i in range(9):
                T = T + g[:, i]
            self._nine[dtype] = (ts, T)
        return self._nine[dtype]

    def eval(self, rhos, dtype=np.float64):
        """(LL, LL', LL'', sum |log D|, sum |D'/D|, sum (|D''/D| + (D'/D)^2), sum A'/D, sum (A''/D + (A'/D)^2), nearest),
        each [len(rhos)].  The fourth to sixth are the sums of absolute per-entry terms; the seventh and eighth the same
        over absolute summands, A' = sum_l |q[l] w'[l]| and A'' likewise (never smaller, and not 0 where the three l
        cancel exactly); nearest is the smallest |a_l / 1e-6 - 1| over the droplet's elements before the floor (inf for
        a droplet without entries): how close the evaluated rho is to a kink of LL'."""
        rh = np.asarray(rhos, dtype=dtype).reshape(-1)
        R = rh.size
        if self.n == 0:
            return core.eval_empty(R, dtype, nearest=True)
        ts, T = self.nine_sums(dtype)
        floor = dtype(fr.MIN_NORM_GL)
        l = np.arange(3).astype(dtype)
        tfl = dtype(2.0) * self.f.astype(dtype)[:, None] - l[None, :]              # 2 f - l, [n][3]
        p = tfl[:, None, :] * (dtype(0.5) * rh[None, :, None]) + dtype(0.5) * l[None, None, :]   # [n][R][3]
        a = np.ones((self.n, R, 3), dtype=dtype)
        a1 = np.zeros_like(a)
        a2 = np.zeros_like(a)
        for r in range(self.maxr):
            idx, al, mat, e4 = self._read_probs(r, dtype)
            pi = p[idx]
            x = np.where(al[:, None, None], pi, dtype(1.0) - pi)
            fac = mat[:, None, None] * x + e4[:, None, None]
            v = (np.where(al, mat, -mat)[:, None] * tfl[idx] * dtype(0.5))[:, None, :]
            t = ts[idx, r][:, None, None]
            x0, x1, x2 = a[idx], a1[idx], a2[idx]
            a2[idx] = (x2 * fac + dtype(2.0) * x1 * v) / t
            a1[idx] = (x1 * fac + x0 * v) / t
            a[idx] = (x0 * fac) / t
        nearest = np.abs(a / floor - dtype(1.0)).min(axis=(0, 2)).astype(np.float64)
        low = a < floor
        a = np.where(low, floor, a)
        a1 = np.where(low, dtype(0.0), a1)
        a2 = np.where(low, dtype(0.0), a2)
        m = T[:, None, None]
        a, a1, a2 = a / m, a1 / m, a2 / m
        g = self.q.astype(dtype)[:, None, :]
        D = (g[:, :, 0] * a[:, :, 0] + g[:, :, 1] * a[:, :, 1]) + g[:, :, 2] * a[:, :, 2]
        D1 = (g[:, :, 0] * a1[:, :, 0] + g[:, :, 1] * a1[:, :, 1]) + g[:, :, 2] * a1[:, :, 2]
        D2 = (g[:, :, 0] * a2[:, :, 0] + g[:, :, 1] * a2[:, :, 1]) + g[:, :, 2] * a2[:, :, 2]
        A1 = np.abs(g * a1).sum(axis=2)
        A2 = np.abs(g * a2).sum(axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):          # (a posterior row of exactly 0: log(0), 0 / 0)
            return core.eval_tail(D, D1, D2, A1, A2, nearest)


def fit(p, q, amb_af, c, j, rho_max):
    """dict of the restated outputs of one (droplet, candidate): rho_hat, ll_hat, ll_zero, info, status (0, 1, 2, 5 or 6)"""
    return core.fit(Cell(p, q, amb_af, c, j), "rho", rho_max, top=False, can_fail=True)


# the inputs of the GPU shape tests (tests/test_fmx_ambient_fit_gpu.py); the CPU test holds the kink claim on them
SHAPES = (0, 1, 2, 63, 64, 65, 2048, 2049, 5003)
SHAPE_CASES = ((6, 46), (6, 7), (17, 57), (70, 110), (300, 340))       # (V, seed)


def shaped(V, seed):
    """droplets of exactly 0, 1, 2, 63, 64, 65, 2048, 2049 and 5003 entries of 1, 2, 33 and 60 reads at base qualities 2..93,
    READ_OTHER bytes, a fifth of the reads from the pool; droplet c holds a cell of donor c % V"""
    p, who, pool = shaped_pileup(list(SHAPES), 6000, V, seed, missing_gp_frac=0.0)
    assert (p.reads == READ_OTHER).any() and set(np.diff(p.entry_rptr).tolist()) == {1, 2, 33, 60}
    return p, who, pool
