"""What the four restatements of the share fits (ambient_fit_ref.py, alpha_fit_ref.py, fmx_ambient_fit_ref.py,
fmx_alpha_fit_ref.py) share: everything that asks a cell for eval() only.  The models -- the per-read loops of the four Cell
classes, each cited to the reference's lines -- stay in their modules.

eval_tail(): the tuple a Cell.eval returns, from the per-entry D, D', D'' and the sums over absolute summands A', A''.
bracket(): the coarse rule of the header: LL at i * x_max / 8, the best (ties to the lowest index), its neighbours.
maximise(): the maximiser inside the bracket WITHOUT Newton: a scan of LL, then bisection on the sign of LL' in longdouble
between the neighbours of the best scan point to a width of 1e-12.  LL' may jump where an element of the freemuxlet model
crosses its floor, but only upward (max(a, 1e-6) is convex in a), so the bisection closes on a zero LL' crosses downward: a
maximum.  fit(): the dict of restated outputs of one slot."""
import numpy as np


def eval_empty(R, dtype, nearest=False):
    """the tuple of a droplet without entries: eight rows of zeros and, for a model with a floor, nearest = inf"""
    z = np.zeros(R, dtype=dtype)
    return tuple(z.copy() for _ in range(8)) + ((np.full(R, np.inf),) if nearest else ())


def eval_tail(D, D1, D2, A1, A2, nearest=None):
    """(LL, LL', LL'', sum |log D|, sum |D'/D|, sum (|D''/D| + (D'/D)^2), sum A'/D, sum (A''/D + (A'/D)^2)) from the
    per-entry terms [n][R], and `nearest` behind them where the model has one"""
    lg, q1, q2 = np.log(D), D1 / D, D2 / D
    out = (lg.sum(axis=0), q1.sum(axis=0), (q2 - q1 * q1).sum(axis=0), np.abs(lg).sum(axis=0), np.abs(q1).sum(axis=0),
           (np.abs(q2) + q1 * q1).sum(axis=0), (A1 / D).sum(axis=0), (A2 / D + (A1 / D) ** 2).sum(axis=0))
    return out if nearest is None else out + (nearest,)


def coarse_points(x_max):
    return [i * float(x_max) / 8 for i in range(9)]


def bracket(cell, x_max):
    """(lo, hi, best index) by the coarse rule; LL in float64"""
    xs = coarse_points(x_max)
    L = cell.eval(xs, np.float64)[0]
    i = int(np.argmax(L))                                        # (first maximum: ties to the lowest index)
    return xs[max(i - 1, 0)], xs[min(i + 1, 8)], i


def maximise(cell, lo, hi, n_scan=64, scan_dtype=np.longdouble):
    """the maximiser of LL in [lo, hi]: a scan of n_scan + 1 points in scan_dtype, then bisection on the sign of LL' in
    longdouble to 1e-12.  Returns (estimate as float, at_lo, at_hi): on the bracket's own end where the scan's best point is
    that end and LL' points out"""
    ld, T = np.longdouble, scan_dtype
    xs = np.array([T(lo) + (T(hi) - T(lo)) * T(i) / T(n_scan) for i in range(n_scan + 1)], dtype=T)
    xs[-1] = T(hi)
    i = int(np.argmax(cell.eval(xs, T)[0]))
    a, b = ld(xs[max(i - 1, 0)]), ld(xs[min(i + 1, n_scan)])
    if i == 0 and cell.eval([xs[0]], ld)[1][0] <= 0:
        return float(lo), True, False
    if i == n_scan and cell.eval([xs[-1]], ld)[1][0] >= 0:
        return float(hi), False, True
    while b - a > ld(1e-12):
        m = (a + b) / ld(2)
        if cell.eval([m], ld)[1][0] > 0:
            a = m
        else:
            b = m
    return float((a + b) / ld(2)), False, False


def fit(cell, share, x_max, top, can_fail, scan=(64, np.longdouble)):
    """dict of the restated outputs of one slot: {share}_hat, ll_hat, ll_zero, ll_top where `top`, info, status -- 0, 1, 2,
    5 (no entry) and, where can_fail (freemuxlet), 6: LL at a coarse point is not finite -- and the cell itself"""
    hat, lls = f"{share}_hat", ("ll_hat", "ll_zero", "ll_top")[:3 if top else 2]
    if cell.n == 0:
        return {hat: 0.0, **dict.fromkeys(lls, 0.0), "info": 0.0, "status": 5, "cell": cell}
    if can_fail and not np.isfinite(cell.eval(coarse_points(x_max), np.float64)[0]).all():
        return {hat: 0.0, **dict.fromkeys(lls, -np.inf), "info": 0.0, "status": 6, "cell": cell}
    lo, hi, _ = bracket(cell, x_max)
    x, at_lo, at_hi = maximise(cell, lo, hi, *scan)
    L, _, d2 = [float(v[0]) for v in cell.eval([x], np.longdouble)[:3]]
    ends = cell.eval([0.0, float(x_max)] if top else [0.0], np.longdouble)[0]      # (the ends in one evaluation where two)
    status = 1 if (at_lo and x == 0.0) else 2 if (at_hi and x == float(x_max)) else 0
    return {hat: x, "ll_hat": L, **dict(zip(lls[1:], map(float, ends))), "info": -d2, "status": status, "cell": cell}


def sign_changes(cell, lo, hi, n=129):
    """the sign changes of LL' (longdouble) along an n-point scan of [lo, hi], zeros dropped"""
    ld = np.longdouble
    xs = np.array([ld(lo) + (ld(hi) - ld(lo)) * ld(i) / ld(n - 1) for i in range(n)], dtype=ld)
    s = np.sign(cell.eval(xs, ld)[1].astype(np.float64))
    s = s[s != 0]
    return int((s[1:] != s[:-1]).sum())
