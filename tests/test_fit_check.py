"""fit_check.check_fit held to itself, without a device: for each of the four descriptions (the CALL of the four fit GPU
modules) a small case is built on the CPU and a "device output" is made from the restatement -- its estimate, its float64
evaluation there and at the ends, its status, n_steps 1 where interior and 0 elsewhere.  check_fit passes that output, and
fails with an AssertionError on each single perturbation of it: an LL moved by twice its bar, an estimate by 1e-5, an info
by 1 %, a relabelled status, a status 3, 49 steps, a non-zero field on a skipped slot and on a droplet without entries, a
last bit between ll_hat and ll_top on the upper bound, and for the freemuxlet calls a NaN, a finite ll_hat on a status-6
row and a slot on a kink where none may be.

Droplets of 0, 1, 2 and 65 entries (seven of the last, of three donors), S = 200, three donors or clusters, two slots of
which one is -1 on every other droplet, x_max below the top of the range so that the upper bound is hit.  The freemuxlet
posteriors are those of the donors' cluster pileups (test_fmx_singlets.cluster_posteriors), with one row zeroed."""
import copy
import dataclasses
import functools

import numpy as np
import pytest

import alpha_fit_ref as alr
import ambient_fit_ref as afr
import fit_check
import oracle_binding as ob
import parity
import test_demux_alpha_fit_gpu
import test_demux_ambient_fit_gpu
import test_fmx_alpha_fit_gpu
import test_fmx_ambient_fit_gpu
from test_fmx_singlets import cluster_posteriors

ENTRIES, S, V = [0, 1, 2, 65, 65, 65, 65, 65, 65, 65], 200, 3
CALLS = {m.CALL.name: m.CALL for m in (test_demux_ambient_fit_gpu, test_demux_alpha_fit_gpu, test_fmx_ambient_fit_gpu,
                                       test_fmx_alpha_fit_gpu)}
X_MAX = {"rho": 0.3, "alpha": 0.6}
TOL = parity.LL_TOL


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(call with its restated fits memoised, case, slots, x_max, the restated fit of every slot, the made-up device output)"""
    call = CALLS[name]
    x_max = X_MAX[call.share]
    fmx = call.nearest
    if call.width == 1:
        p, own, pool = afr.shaped_pileup(ENTRIES, S, V, seed=21, missing_gp_frac=0.0 if fmx else 0.03)
        slots = np.stack([own, (own + 1) % V], axis=1).astype(np.int32)
        slots[::2, 1] = -1
    else:
        p, own, second = alr.shaped_pileup(ENTRIES, S, V, seed=21, missing_gp_frac=0.0 if fmx else 0.03)
        slots = np.stack([np.stack([own, second], axis=1), np.stack([second, own], axis=1)], axis=1).astype(np.int32)
        slots[::2, 1] = -1
    case = (p, (0.0, 0.25, 0.5))
    if fmx:
        q = cluster_posteriors(p.af, np.ascontiguousarray(ob.fmx_build_cluster_pileup(p, ob.fmx_entry_pileup(p), V, own.astype(np.int32))), 0.1)
        q[int(p.entry_snp[int(p.cell_ptr[9]) + 5]), int(slots[9].ravel()[0])] = 0.0     # status 6 on droplet 9, slot 0
        case = (p, q)
    if call.amb_af:
        case += (pool,)
    memo = {}
    call = dataclasses.replace(call, fit=lambda *a: memo[a[len(case):]] if a[len(case):] in memo else
                               memo.setdefault(a[len(case):], CALLS[name].fit(*a)))
    C, n = slots.shape[:2]
    got = {k: np.zeros((C, n), np.int32 if k in ("status", "n_steps") else np.float64) for k in call.fields}
    fits = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(C):
            for t in range(n):
                idx = tuple(int(i) for i in slots[c, t].ravel())
                if idx[0] < 0:
                    got["status"][c, t] = 4
                    continue
                r = fits[(c, t)] = call.fit(*case, c, *idx, x_max)
                got["status"][c, t] = r["status"]
                if r["status"] >= 5:
                    for k in call.lls:
                        got[k][c, t] = r[k]                                              # (0, or -inf at status 6)
                    continue
                at = lambda x: [float(v[0]) for v in r["cell"].eval([x], np.float64)[:3]]
                got[call.hat][c, t] = r[call.hat]
                got["ll_hat"][c, t], _, d2 = at(r[call.hat])
                got["info"][c, t] = -d2
                got["ll_zero"][c, t] = at(0.0)[0]
                if call.top:
                    got["ll_top"][c, t] = at(x_max)[0]
                got["n_steps"][c, t] = r["status"] == 0
    return call, case, slots, x_max, fits, got


def check(name, got, **changes):
    call, case, slots, x_max, _fits, _got = case_of(name)
    with np.errstate(divide="ignore", invalid="ignore"):
        return fit_check.check_fit(dataclasses.replace(call, **changes), case, slots, x_max, got, "made up", ll_tol=TOL)


def slot_where(name, cond):
    """the first (droplet, slot) whose restated fit meets cond; the case must hold one"""
    fits = case_of(name)[4]
    found = [k for k, r in sorted(fits.items()) if cond(r)]
    assert found, name
    return found[0]


class OnKink:
    """a restated cell that reports an element on the floor's edge at every share"""

    def __init__(self, cell):
        self.cell, self.n = cell, cell.n

    def eval(self, xs, dtype=np.float64):
        out = self.cell.eval(xs, dtype)
        return out[:8] + (np.zeros_like(out[8]),)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_restatement_as_device_output_passes(name):
    call, case, slots, x_max, fits, got = case_of(name)
    statuses = set(got["status"].ravel().tolist())
    assert {0, 2, 4, 5} <= statuses and (6 in statuses) == call.nearest and any(r["status"] == 0 and r["info"] >= 1.0 for r in fits.values())
    fitted, strong = check(name, got)
    assert fitted == (got["status"] == 0).sum() and 1 <= strong <= fitted


@pytest.mark.parametrize("name", sorted(CALLS))
def test_every_single_perturbation_fails(name):
    call, case, slots, x_max, fits, base = case_of(name)
    hat = call.hat
    interior = slot_where(name, lambda r: r["status"] == 0 and r["info"] >= 1.0)
    upper = slot_where(name, lambda r: r["status"] == 2)
    skipped = tuple(np.argwhere(base["status"] == 4)[0])
    empty = tuple(np.argwhere(base["status"] == 5)[0])
    # 1 % of the interior slot's info exceeds its bar, so the scaled info cannot pass vacuously
    cell, x = fits[interior]["cell"], fits[interior][hat]
    ld, f64 = cell.eval([x], np.longdouble), cell.eval([x], np.float64)
    tol2 = max(1000.0 * abs(float(f64[2][0]) - float(ld[2][0])), 1e-9 * float(ld[5][0]))
    assert tol2 > 0.0 and 0.01 * base["info"][interior] > 2.0 * tol2 and (not call.nearest or float(ld[8][0]) >= 1e-6)

    def put(k, where, v):
        return lambda g: g[k].__setitem__(where, v)

    changes = [(f"{k} moved by twice its bar", put(k, interior, base[k][interior] + 2.0 * TOL)) for k in call.lls]
    changes += [
        ("the estimate moved by 1e-5", put(hat, interior, base[hat][interior] + 1e-5)),
        ("info scaled by 1.01", put("info", interior, base["info"][interior] * 1.01)),
        ("an interior slot relabelled status 1", put("status", interior, 1)),
        ("a status 3", put("status", interior, 3)),
        ("49 steps", put("n_steps", interior, 49)),
        ("a step on a bound", put("n_steps", upper, 1)),
        ("an estimate on a skipped slot", put(hat, skipped, 0.1)),
        ("a step on a skipped slot", put("n_steps", skipped, 1)),
        ("an LL on a droplet without entries", put("ll_zero", empty, -1.0)),
    ]
    if call.top:
        changes.append(("ll_hat a last bit from ll_top on the upper bound", put("ll_hat", upper, np.nextafter(base["ll_top"][upper], 0.0))))
    if call.nearest:
        failed = tuple(np.argwhere(base["status"] == 6)[0])
        changes += [("a NaN", put("info", skipped, np.nan)), ("a finite ll_hat at status 6", put("ll_hat", failed, -50.0))]
    for what, change in changes:
        got = copy.deepcopy(base)
        change(got)
        with pytest.raises(AssertionError):
            check(name, got)
            print(f"{name}: {what} passed")
    if call.nearest:                         # a slot on a kink: no bar of its own fails it, only the count
        on_kink = dict(fit=lambda *a: dict(call.fit(*a), cell=OnKink(call.fit(*a)["cell"])))
        check(name, base, kink_frac=1.0, **on_kink)
        with pytest.raises(AssertionError):
            check(name, base, kink_frac=0.0, **on_kink)
