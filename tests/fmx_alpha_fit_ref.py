"""Reference values of muxgl_fmx_alpha_fit (include/muxgl.h) for its tests, on top of fmx_ambient_ref.py and
fmx_ambient_fit_ref.py and in the manner of alpha_fit_ref.py.

Cell(p, q, c, j, k).eval(): LL, LL' and LL'' of droplet c as a mix of clusters j and k at a share alpha of k.  The per-read
loop is the reference's (sc_drop_seq.cpp:452-509 at alpha = 0.5: the nine multiplied, summed in index order to t,
everything divided by t; after the reads the 1e-6 floor and the division by T, the sum of the floored nine) with the nine
elements of one alpha and their first two derivatives carried beside the reference's nine:
    fac = mat * x + e4,  x = ALT read ? p : 1 - p,  p = 0.5 * l + (m - l) * 0.5 * alpha      element l * 3 + m
    v = dfac/dalpha = +-mat * (m - l) * 0.5                                                  (+ for an ALT read)
    a'' = a'' * fac + 2 * a' * v;   a' = a' * fac + a * v;   a = a * fac;   all three divided by t
and after the reads, where a < 1e-6: a = 1e-6, a' = a'' = 0 -- the derivative of the floored function on that piece.  Then
w = a / T.  On the diagonal l == m the slope is 0 and the element is the reference's own, operation for operation; at
alpha = 0.5 every element is.  D = sum_l sum_m w[l][m] * q[j][l] * q[k][m] from 0 in the order l, then m, each summand
formed as (w * q_j) * q_k (cmd_cram_freemux2.cpp:441-445); D', D'' over the six off-diagonal elements with (l, m) next to
(m, l); LL = sum log D, LL' = sum D'/D, LL'' = sum (D''/D - (D'/D)^2) over ALL entries of the droplet.  It runs in float64
and in np.longdouble.  ll_exact() (float64, math.log, the entries one after the other from 0, as :455 adds them) at
alpha = 0.5 is the reference's llks[j (j + 1) / 2 + k] for k < j.

bracket(), maximise() (a 65-point scan in longdouble), fit() and sign_changes() are fit_ref_core.py's (they use eval()
only).  search(): the device's search rule restated on the float64 evaluation, the 65-point scan of a bracket in which an
element crosses the floor included."""
import math

import numpy as np

import alpha_fit_ref as dfr
import fmx_ambient_fit_ref as ffr
import fmx_ambient_ref as fr
import fit_ref_core as core

READ_OTHER = fr.READ_OTHER
coarse_points, bracket, maximise, sign_changes = core.coarse_points, core.bracket, core.maximise, core.sign_changes
LM = [(l, m) for l in range(3) for m in range(3)]
OFF = [i for i, (l, m) in enumerate(LM) if l != m]


class Cell(ffr.Cell):
    """the entries of droplet c for the pair of clusters (j, k) with the posteriors q [S][K][3], as padded numpy rows"""

    def __init__(self, p, q, c, j, k):
        super().__init__(p, q, np.zeros(p.S), c, j)
        e0, e1 = int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])
        snp = p.entry_snp[e0:e1].astype(np.int64)
        self.qk = np.asarray(q, dtype=np.float64)[snp, k, :] if self.n else np.zeros((0, 3))

    def elements(self, xs, dtype=np.float64):
        """(a, a', a'') before the floor, each [n][len(xs)][9], on the scale of the reference's nine (divided by every
        read's t, not yet by T)"""
        x = np.asarray(xs, dtype=dtype).reshape(-1)
        R = x.size
        ts, _T = self.nine_sums(dtype)
        p = np.stack([dtype(0.5) * dtype(l) + dtype(m - l) * dtype(0.5) * x for l, m in LM], axis=1)[None, :, :]   # [1][R][9]
        dp = np.array([dtype(m - l) * dtype(0.5) for l, m in LM], dtype=dtype)
        a = np.ones((self.n, R, 9), dtype=dtype)
        a1 = np.zeros_like(a)
        a2 = np.zeros_like(a)
        for r in range(self.maxr):
            idx, al, mat, e4 = self._read_probs(r, dtype)
            xx = np.where(al[:, None, None], p, dtype(1.0) - p)
            fac = mat[:, None, None] * xx + e4[:, None, None]
            v = (np.where(al, mat, -mat)[:, None] * dp[None, :])[:, None, :]
            t = ts[idx, r][:, None, None]
            x0, x1, x2 = a[idx], a1[idx], a2[idx]
            a2[idx] = (x2 * fac + dtype(2.0) * x1 * v) / t
            a1[idx] = (x1 * fac + x0 * v) / t
            a[idx] = (x0 * fac) / t
        return a, a1, a2

    def _terms(self, xs, dtype):
        """D, D', D'' and the sums of absolute summands A', A'', each [n][len(xs)], and nearest [len(xs)]: the smallest
        |a / 1e-6 - 1| over the droplet's six alpha-dependent elements before the floor"""
        a, a1, a2 = self.elements(xs, dtype)
        floor = dtype(fr.MIN_NORM_GL)
        nearest = np.abs(a[:, :, OFF] / floor - dtype(1.0)).min(axis=(0, 2)).astype(np.float64)
        low = a < floor
        a = np.where(low, floor, a)
        a1 = np.where(low, dtype(0.0), a1)
        a2 = np.where(low, dtype(0.0), a2)
        _ts, T = self.nine_sums(dtype)
        m = T[:, None, None]
        a, a1, a2 = a / m, a1 / m, a2 / m
        gj, gk = self.q.astype(dtype), self.qk.astype(dtype)
        D = np.zeros(a.shape[:2], dtype=dtype)
        D1, D2, A1, A2 = D.copy(), D.copy(), D.copy(), D.copy()
        for i, (l, mm) in enumerate(LM):                                           # cmd_cram_freemux2.cpp:441-445
            D = D + a[:, :, i] * gj[:, l][:, None] * gk[:, mm][:, None]
        g = [(gj[:, l] * gk[:, mm])[:, None] for l, mm in LM]
        for i in OFF:
            A1 = A1 + np.abs(g[i] * a1[:, :, i])
            A2 = A2 + np.abs(g[i] * a2[:, :, i])
        for i, k in ((1, 3), (2, 6), (5, 7)):                                      # (l, m) next to (m, l)
            D1 = D1 + (g[i] * a1[:, :, i] + g[k] * a1[:, :, k])
            D2 = D2 + (g[i] * a2[:, :, i] + g[k] * a2[:, :, k])
        return D, D1, D2, A1, A2, nearest

    def eval(self, xs, dtype=np.float64):
        """(LL, LL', LL'', sum |log D|, sum |D'/D|, sum (|D''/D| + (D'/D)^2), sum A'/D, sum (A''/D + (A'/D)^2), nearest),
        each [len(xs)], as fmx_ambient_fit_ref.Cell.eval returns them"""
        if self.n == 0:
            return core.eval_empty(np.asarray(xs).reshape(-1).size, dtype, nearest=True)
        with np.errstate(divide="ignore", invalid="ignore"):          # (a posterior row of exactly 0: log(0), 0 / 0)
            return core.eval_tail(*self._terms(xs, dtype))

    def ll_exact(self, xs):
        """LL in float64 as the reference adds it (:455): glibc's log per entry, the entries one after the other from 0"""
        xs = np.asarray(xs, dtype=np.float64).reshape(-1)
        if self.n == 0:
            return np.zeros(xs.size)
        D = self._terms(xs, np.float64)[0]
        out = np.zeros(xs.size)
        for r in range(xs.size):
            s = 0.0
            for e in range(self.n):
                s += math.log(float(D[e, r])) if D[e, r] > 0 else -math.inf
            out[r] = s
        return out

    def crosses(self, xs):
        """whether one of the six elements of an entry is below the floor at one of the points xs and not at another
        (float64, as the device's coarse pass decides)"""
        if self.n == 0:
            return False
        low = self.elements(xs, np.float64)[0][:, :, OFF] < fr.MIN_NORM_GL
        return bool((low != low[:, :1, :]).any())


def fit(p, q, c, j, k, alpha_max):
    """dict of the restated outputs of one (droplet, pair): alpha_hat, ll_hat, ll_zero, ll_top, info, status (0, 1, 2, 5 or
    6)"""
    return core.fit(Cell(p, q, c, j, k), "alpha", alpha_max, top=True, can_fail=True)


def search(cell, alpha_max):
    """The device's search (csrc/ambient_fit_search.hpp, search_piecewise) on the float64 evaluation: the nine coarse
    points, the bracket's three points and whether an element crosses the floor between them, the 65-point scan where one
    does, the bound tests and the safeguarded Newton iteration with the stops 1e-9 and 48 steps.  dict of alpha_hat, ll_hat,
    info, status, n_steps and scanned (whether the 65-point scan ran)."""
    ev = lambda x: [float(v[0]) for v in cell.eval([x], np.float64)[:3]]
    xs = coarse_points(alpha_max)
    L = cell.eval(xs, np.float64)[0]
    if not np.isfinite(L).all():
        return dict(alpha_hat=0.0, ll_hat=-np.inf, info=0.0, status=6, n_steps=0, scanned=False)
    best = int(np.argmax(L))
    lo, mid, hi = xs[max(best - 1, 0)], xs[best], xs[min(best + 1, 8)]
    scanned = cell.crosses([lo, mid, hi])
    if scanned:
        pts = np.array([hi if i >= 64 else lo + (hi - lo) * i / 64.0 for i in range(65)])
        b = int(np.argmax(cell.eval(pts, np.float64)[0]))
        a, x, bb = pts[max(b - 1, 0)], pts[b], pts[min(b + 1, 64)]
        at_lo, at_hi = b == 0 and x == 0.0, b == 64 and x == alpha_max
    else:
        a, x, bb = lo, mid, hi
        at_lo, at_hi = best == 0, best == 8
    b = bb
    status, steps, step, newton, first = 3, 0, 1.0, False, True
    xb = Lb = d2b = None
    while True:
        Lx, d1, d2 = ev(x)
        if first or Lx > Lb:
            xb, Lb, d2b = x, Lx, d2
        if first:
            if at_lo and d1 <= 0.0:
                status = 1
            elif at_hi and d1 >= 0.0:
                status = 2
            if status != 3:
                break
        else:
            steps += 1
        if d1 > 0.0:
            a = x
        elif d1 < 0.0:
            b = x
        if d1 == 0.0 or (newton and step <= 1e-9):
            status = 0
            break
        if steps == 48:
            break
        with np.errstate(divide="ignore", invalid="ignore"):
            xn = float(np.float64(x) - np.float64(d1) / np.float64(d2))
        if d2 < 0.0 and xn == x:
            status = 0
            break
        newton = d2 < 0.0 and a < xn < b
        if not newton:
            if b - a <= 1e-9 or (not first and step <= 1e-9):
                status = 0
                break
            xn = 0.5 * (a + b)
        step = abs(xn - x)
        x = xn
        first = False
    if status == 3:
        x, Lx, d2 = xb, Lb, d2b
    return dict(alpha_hat=x, ll_hat=Lx, info=-d2, status=status, n_steps=steps, scanned=scanned)


# ---- pileups ------------------------------------------------------------------------------------------------------------
second_sample = dfr.second_sample
doublet_pileup = dfr.doublet_pileup
MIXED, CLEAN = dfr.MIXED, dfr.CLEAN      # the sanity pileups of DESIGN 4.1h: 24 droplets, shares cycling 0.15 / 0.3 / 0.5; all 0

SHAPES = (0, 1, 2, 63, 64, 65, 130, 300, 2049)
SHAPE_CASES = ((1, 6, 7), (6, 6, 46), (17, 17, 57), (70, 70, 110), (300, 300, 340))       # (K, V, seed)


def shaped(V, seed, entries=SHAPES, S=2600):
    """droplets of exactly 0, 1, 2, 63, 64, 65, 130, 300 and 2049 entries of 1, 2, 33 and 60 reads at base qualities 2..93,
    READ_OTHER bytes; droplet c holds cells of donors c % V and second_sample(C, V)[c], 30 % of the reads from the second.
    Returns (pileup, first [C], second [C])"""
    p, first, second = dfr.shaped_pileup(list(entries), S, V, seed, missing_gp_frac=0.0)
    if p.nnz > 500:
        assert (p.reads == READ_OTHER).any() and set(np.diff(p.entry_rptr).tolist()) == {1, 2, 33, 60}
    return p, first.astype(np.int32), second.astype(np.int32)
