"""The four per-droplet share fits described as data (Call), and check_fit: the bars a device fit of a share x (rho of a
candidate, alpha of a pair) is held to against its restatement, written once for muxgl_demux_ambient_fit,
muxgl_demux_alpha_fit, muxgl_fmx_ambient_fit and muxgl_fmx_alpha_fit.  Each GPU module binds its own Call in a thin
check_fit of its own; tests/fit_suite.py runs the test bodies the four modules share from the same description;
tests/test_fit_check.py holds this check to perturbed outputs without a device.

Bars: ll_hat, ll_zero (and ll_top) within ll_tol; info and the implied LL' (0 at an interior estimate) within 1000 x the
float64-to-longdouble disagreement of the restatement on the case, floored at 1e-9 x the sum of absolute per-entry terms
(over absolute summands where that is exactly 0: every per-entry term of the restatement is exactly 0 in both precisions,
as where the three genotype classes of a one-read entry cancel, while the device's fused dot leaves 1e-19); the restated LL
at the device's estimate within 1e-9 of the LL at the restatement's; where the restated info is >= 1 the two estimates
within 1e-6 and the statuses equal; no status 3, 0 <= n_steps <= 48; on a bound (status 1, 2) the estimate is 0 resp. x_max
and n_steps is 0 (ambient_fit_search.hpp, newton(): the bound tests run on the first evaluation only, before any step is
counted, and at_lo / at_hi hold only where x is 0 resp. x_max -- true of all four calls, so asserted of all four and on
every slot); with ll_top, at status 1 ll_hat == ll_zero and at status 2 ll_hat == ll_top bit for bit.  A skipped slot
(status 4) and a droplet without scored entries (status 5) hold zeros; status 6 exists only where the restatement returns
it (freemuxlet: a posterior row of exactly 0), with -inf in the LLs and 0 elsewhere.

A model with a floor (freemuxlet's 1e-6; Call.nearest) has kinks in LL': a slot with an element within 1e-6 relative of the
floor at the device's estimate (kink_at_ref: or at the restatement's) sits on a kink in one precision and beside it in the
other.  It skips the two derivative bars only, and such slots may be at most kink_frac of the checked ones.  The demuxlet
models have no floor: no slot skips a bar."""
import dataclasses

import numpy as np

WORST = {}   # (name, what: key) -> worst figure seen, printed by every check


@dataclasses.dataclass(frozen=True)
class Call:
    """one fit call: what differs between the four, for check_fit (the first block) and for fit_suite.py (the second)"""
    name: str                        # in the printed lines
    share: str                       # "rho" or "alpha": the estimate is {share}_hat
    fields: tuple                    # the output arrays
    width: int                       # indices per slot: a candidate (1) or a pair (2)
    top: bool                        # has ll_top
    fit: object                      # the restatement's fit(*case, c, *indices, x_max); case: (p, alphas, f), (p, q) ...
    closing: str                     # the end of the closing line: on_kink, mean and max (of n_steps) may appear
    nearest: bool = False            # the model has a floor: Cell.eval returns a ninth value, the distance to a kink
    kink_at_ref: bool = False        # a slot is on a kink at the restatement's estimate too
    kink_frac: float = 0.0           # the share of checked slots that may be on a kink (a condition on the inputs)
    no_nan: bool = False             # no field holds a NaN anywhere
    bounds_everywhere: bool = False  # the bit equalities on a bound hold on every slot, not on the checked ones alone
    guard_info_note: bool = False    # the figure |info - ref| / tol is noted only where tol > 0 (the bar is unguarded)
    # ---- for fit_suite.py ----
    method: str = ""                 # of muxgl.Engine
    grid: bool = False               # takes the alpha grid first (demuxlet)
    amb_af: bool = False             # takes the ambient profile
    x_name: str = ""                 # rho_max or alpha_max, as the refusals name it
    slot_name: str = ""              # cand or pair, likewise
    extra: tuple = ()                # what the returned dict holds beside the wanted fields and kernel_ms
    subsets: tuple = ()              # the subsets of outputs the identity test asks for
    x_identity: float = 0.0          # the x_max of the identity tests

    @property
    def hat(self):
        return f"{self.share}_hat"

    @property
    def lls(self):
        return ("ll_hat", "ll_zero", "ll_top")[:3 if self.top else 2]


def check_fit(call, case, slots, x_max, got, what, pairs=None, ll_tol=None):
    """case: what call.fit takes before (droplet, indices, x_max), the pileup first; slots: [C][n] or [C][n][2] indices;
    pairs: the (droplet, slot) pairs to check (None: all).  Returns the number of interior fits and of those with restated
    info >= 1"""
    ld = np.longdouble
    name, hat, lls, fields, C = call.name, call.hat, call.lls, call.fields, case[0].C
    slots = np.asarray(slots).reshape(C, -1, call.width)
    if pairs is None:
        pairs = [(c, t) for c in range(C) for t in range(slots.shape[1])]

    def note(key, v):
        WORST[(name, f"{what}: {key}")] = max(WORST.get((name, f"{what}: {key}"), 0.0), float(v))

    assert all(got[k].shape == slots.shape[:2] for k in fields)
    assert (got["n_steps"] <= 48).all() and (got["n_steps"] >= 0).all() and not (got["status"] == 3).any()
    assert not call.no_nan or not any(np.isnan(got[k]).any() for k in fields)
    b1, b2 = got["status"] == 1, got["status"] == 2
    assert (got[hat][b1] == 0.0).all() and (got[hat][b2] == x_max).all() and (got["n_steps"][b1 | b2] == 0).all()
    if call.top:
        sel = np.ones(b1.shape, bool) if call.bounds_everywhere else np.zeros(b1.shape, bool)
        sel[tuple(np.array(pairs, dtype=np.int64).reshape(-1, 2).T)] = True
        assert got["ll_hat"][b1 & sel].tobytes() == got["ll_zero"][b1 & sel].tobytes()
        assert got["ll_hat"][b2 & sel].tobytes() == got["ll_top"][b2 & sel].tobytes()
    fitted = strong = checked = on_kink = 0
    seen = {}
    for c, t in pairs:
        idx = tuple(int(i) for i in slots[c, t])
        g = {n: got[n][c, t] for n in fields}
        if idx[0] < 0:
            assert all(i < 0 for i in idx) and g["status"] == 4 and all(g[n] == 0 for n in fields if n != "status"), (c, t, g)
            continue
        if (c,) + idx not in seen:
            seen[(c,) + idx] = call.fit(*case, c, *idx, x_max)
        r = seen[(c,) + idx]
        cell = r["cell"]
        if cell.n == 0:
            assert g["status"] == 5 and all(g[n] == 0 for n in fields if n != "status"), (c, t, g)
            continue
        if r["status"] == 6:
            assert g["status"] == 6 and g[hat] == 0 and all(g[n] == -np.inf for n in lls) and g["info"] == 0 \
                and g["n_steps"] == 0, (c, t, g)
            continue
        x = float(g[hat])
        assert g["status"] in (0, 1, 2) and 0.0 <= x <= x_max, (c, t, g)
        L, d1, d2, aL, a1, a2, s1, s2, *near = [float(v[0]) for v in cell.eval([x], ld)]
        L64, d164, d264 = [float(v[0]) for v in cell.eval([x], np.float64)[:3]]
        tol1 = max(1000.0 * abs(d164 - d1), 1e-9 * a1)
        tol2 = max(1000.0 * abs(d264 - d2), 1e-9 * a2)
        if tol1 == 0.0 or tol2 == 0.0:   # every term exactly 0 in both precisions: the floor over absolute summands
            tol1, tol2 = max(tol1, 1e-9 * s1), max(tol2, 1e-9 * s2)
        assert len(near) == call.nearest
        kink = call.nearest and near[0] < 1e-6   # an element on the floor's edge: the derivative bars do not apply
        if call.kink_at_ref:
            kink = kink or float(cell.eval([r[hat]], ld)[8][0]) < 1e-6
        checked += 1
        on_kink += kink
        for n in lls:
            ref = L if n == "ll_hat" else r[n]
            note(f"|{n} - ref|", abs(g[n] - ref))
            assert abs(g[n] - ref) <= ll_tol, (c, t, n, g, ref)
        if not kink:
            if tol2 > 0.0 or not call.guard_info_note:
                note("|info - ref| / tol", abs(g["info"] + d2) / tol2)
            assert abs(g["info"] + d2) <= tol2, (c, t, g, d2, tol2)
        if g["status"] == 1:
            assert x == 0.0 and (kink or d1 <= tol1), (c, t, g, d1)
        elif g["status"] == 2:
            assert x == x_max and (kink or d1 >= -tol1), (c, t, g, d1)
        else:
            if not kink:
                note(f"|LL'({hat})| / tol", abs(d1) / tol1)
                assert abs(d1) <= tol1, (c, t, g, d1, tol1)
            fitted += 1
        note(f"LL(ref {call.share}) - LL(device {call.share})", r["ll_hat"] - L)
        assert L >= r["ll_hat"] - 1e-9, (c, t, g, r[hat], r["ll_hat"], L)
        if r["info"] >= 1.0:
            strong += g["status"] == 0
            note(f"|{hat} - ref|", abs(x - r[hat]))
            assert abs(x - r[hat]) <= 1e-6, (c, t, g, r[hat], r["info"])
            assert g["status"] == r["status"], (c, t, g, r["status"])
    assert on_kink <= call.kink_frac * checked, (on_kink, checked)
    for key in sorted(k for n, k in WORST if n == name and k.startswith(what + ":")):
        print(f"{name} {key} {WORST[(name, key)]:.3e}")
    on = got["status"] == 0
    print(f"{name} {what}: {fitted} interior fits, {strong} with info >= 1, " + call.closing.format(
        on_kink=on_kink, mean=float(got["n_steps"][on].mean()) if on.any() else 0.0,
        max=int(got["n_steps"].max()) if got["n_steps"].size else 0))
    return fitted, strong
