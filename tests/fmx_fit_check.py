"""check_fit of tests/test_fmx_ambient_fit_gpu.py and tests/test_fmx_alpha_fit_gpu.py: the bars a device fit of a share x
(rho of a candidate cluster, alpha of a pair of clusters) is held to against its restatement, written once.  What differs
between the two calls is handed in: the share's name, the restatement's `fit`, whether the call has ll_top, and each
module's own rule for elements on the floor's edge.

Bars: ll_hat, ll_zero (and ll_top) within ll_tol; info and the implied LL' (0 at an interior estimate) within 1000 x the
float64-to-longdouble disagreement of the restatement on the case, floored at 1e-9 x the sum of absolute per-entry terms
(over absolute summands where that is exactly 0); the restated LL at the device's estimate within 1e-9 of the LL at the
restatement's; where the restated info is >= 1 the two estimates within 1e-6 and the statuses equal; with ll_top, at status
1 ll_hat == ll_zero and at status 2 ll_hat == ll_top bit for bit.  A slot with an element within 1e-6 relative of the 1e-6
floor at the device's estimate (kink_at_ref: or at the restatement's) sits on a kink of LL' in one precision and beside it
in the other: it skips the two derivative bars only, and such slots may be at most kink_frac of the checked ones."""
import numpy as np

WORST = {}   # (name, what) -> worst figure seen, printed by every check


def check_fit(name, share, fields, fit, top, kink_at_ref, kink_frac, C, slots, x_max, got, what, pairs, ll_tol):
    """name: the call, for the printed lines; share: "rho" or "alpha"; fit(c, *indices): the restatement's fit of a slot's
    indices on droplet c; slots: [C][n] or [C][n][2] indices; pairs: the (droplet, slot) pairs to check (None: all).
    Returns the number of interior fits and of those with restated info >= 1"""
    ld = np.longdouble
    hat = f"{share}_hat"
    slots = np.asarray(slots).reshape(C, -1, 2 if top else 1)
    lls = ("ll_hat", "ll_zero", "ll_top") if top else ("ll_hat", "ll_zero")

    def note(key, v):
        WORST[(name, f"{what}: {key}")] = max(WORST.get((name, f"{what}: {key}"), 0.0), float(v))

    assert all(got[k].shape == slots.shape[:2] for k in fields)
    assert (got["n_steps"] <= 48).all() and (got["n_steps"] >= 0).all() and not (got["status"] == 3).any()
    assert not any(np.isnan(got[k]).any() for k in fields)
    if top:
        b1, b2 = got["status"] == 1, got["status"] == 2
        assert got["ll_hat"][b1].tobytes() == got["ll_zero"][b1].tobytes() and (got[hat][b1] == 0.0).all()
        assert got["ll_hat"][b2].tobytes() == got["ll_top"][b2].tobytes() and (got[hat][b2] == x_max).all()
    fitted = strong = checked = on_kink = 0
    seen = {}
    for c, t in (pairs if pairs is not None else [(c, t) for c in range(C) for t in range(slots.shape[1])]):
        idx = tuple(int(i) for i in slots[c, t])
        g = {n: got[n][c, t] for n in fields}
        if idx[0] < 0:
            assert all(i < 0 for i in idx) and g["status"] == 4 and all(g[n] == 0 for n in fields if n != "status"), (c, t, g)
            continue
        if (c,) + idx not in seen:
            seen[(c,) + idx] = fit(c, *idx)
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
        L, d1, d2, aL, a1, a2, s1, s2, near = [float(v[0]) for v in cell.eval([x], ld)]
        L64, d164, d264 = [float(v[0]) for v in cell.eval([x], np.float64)[:3]]
        tol1 = max(1000.0 * abs(d164 - d1), 1e-9 * a1)
        tol2 = max(1000.0 * abs(d264 - d2), 1e-9 * a2)
        if tol1 == 0.0 or tol2 == 0.0:   # every term exactly 0 in both precisions: the floor over absolute summands
            tol1, tol2 = max(tol1, 1e-9 * s1), max(tol2, 1e-9 * s2)
        kink = near < 1e-6               # an element on the floor's edge: the derivative bars do not apply
        if kink_at_ref:
            kink = kink or float(cell.eval([r[hat]], ld)[8][0]) < 1e-6
        checked += 1
        on_kink += kink
        for n in lls:
            ref = L if n == "ll_hat" else r[n]
            note(f"|{n} - ref|", abs(g[n] - ref))
            assert abs(g[n] - ref) <= ll_tol, (c, t, n, g, ref)
        if not kink:
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
        note(f"LL(ref {share}) - LL(device {share})", r["ll_hat"] - L)
        assert L >= r["ll_hat"] - 1e-9, (c, t, g, r[hat], r["ll_hat"], L)
        if r["info"] >= 1.0:
            strong += g["status"] == 0
            note(f"|{hat} - ref|", abs(x - r[hat]))
            assert abs(x - r[hat]) <= 1e-6, (c, t, g, r[hat], r["info"])
            assert g["status"] == r["status"], (c, t, g, r["status"])
    assert on_kink <= kink_frac * checked, (on_kink, checked)
    for key in sorted(k for n, k in WORST if n == name and k.startswith(what + ":")):
        print(f"{name} {key} {WORST[(name, key)]:.3e}")
    print(f"{name} {what}: {fitted} interior fits, {strong} with info >= 1, {on_kink} on a kink, mean n_steps "
          f"{float(got['n_steps'][got['status'] == 0].mean()) if (got['status'] == 0).any() else 0.0:.2f}")
    return fitted, strong
