"""A long-lived muxgl handle against fresh ones, over the call sequences of tests/handle_sequences.py.

One handle lives through a whole sequence: several pileups, panels, grids, demuxlet and freemuxlet jobs, slab budgets.
After every step that runs, a FRESH handle of the same flags (one device, or the same device group) is given only what
the step needs -- the pileup in force, the panel, for freemuxlet the preparation, the recorded start and the same number
of iterations -- and makes the same call.  Every output array of the long-lived handle must equal the fresh one's byte
for byte: whatever the long-lived handle kept from earlier steps (DESIGN.md 2b lists it) must not show.  For demux_run
and fmx_iterate the set of timing slots that recorded something must be the same too: the same kernels ran.  Every step
the lifecycle model refuses must raise with the model's text, and the next step must still pass.  One run at V <= 16
and one iteration at K <= 16 per sequence (all of them, in fact) are also held to the CPU oracle.

The seeds of the suite are those tests/test_handle_sequences.py proves to reach every transition.  A campaign over more:

    python tests/test_handle_sequences_gpu.py --seeds 0:200 [--log handle_sequences.jsonl] [--keep-going]

prints one JSON line per sequence (profiles/handle_sequences_campaign.md records what ran).
"""
import dataclasses
import json
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import handle_sequences as hs  # noqa: E402
import oracle_binding as ob  # noqa: E402
import parity  # noqa: E402
from popscle_amd import muxgl  # noqa: E402
from test_handle_sequences import SEEDS  # noqa: E402

pytestmark = pytest.mark.gpu

# Calls that do not promise the same bits from two handles, with the reason; they are compared with
# parity.same_records instead.  None so far: every call of the vocabulary is deterministic in its inputs.
NOT_BIT_IDENTICAL = {}


class Inputs:
    """the pileups, panels and recorded starts of a seed, each made once"""

    def __init__(self, seed):
        self.seed = seed
        self.pls = hs.pileups(seed)
        self._panels, self._eplp = {}, {}

    def panel(self, i, V, mode):
        k = (i, V, mode)
        if k not in self._panels:
            self._panels[k] = hs.panel(self.seed, i, self.pls[i].S, V, mode)
        return self._panels[k]

    def init(self, i, K):
        return hs.init_clusters(self.seed, 9 if i is None else i, self.pls[i].C if i is not None else 0, K)

    def eplp(self, i):
        if i not in self._eplp:
            self._eplp[i] = ob.fmx_entry_pileup(self.pls[i])
        return self._eplp[i]


def make_engine(seed, flags):
    return muxgl.Engine([0, 0], flags=flags) if hs.is_group(seed) else muxgl.Engine(0, flags=flags)


def slots(eng):
    return tuple(int(i) for i in np.flatnonzero(eng.timing() > 0))


def call(eng, st, inp, m):
    """the step on `eng` (m: the model after the step); returns {name: array} of everything the call gives back, and for
    demux_run and iterate "slots", the timing slots that recorded something"""
    op = st["op"]
    if op == "load":
        p = inp.pls[st["i"]]
        eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        return {}
    if op == "panel":
        eng.demux_set_gp(*inp.panel(m.i, st["V"], st["mode"]))
        return {}
    if op == "budget":
        if st["value"] is None:
            os.environ.pop(st["name"], None)
        else:
            os.environ[st["name"]] = st["value"]
        return {}
    if op == "demux_run":
        got = eng.demux_run(hs.GRIDS[st["grid"]], 0.5, want_full_ll=st["full_ll"])
        out = {"cells": got[0], "full_ll": got[1]} if st["full_ll"] else {"cells": got}
        out["slots"] = slots(eng)
        return out
    if op == "demux_singlets":
        return {"sng": eng.demux_singlets(hs.GRIDS[st["grid"]])}
    if op == "demux_inclusion":
        return eng.demux_inclusion(hs.GRIDS[st["grid"]], 0.5)
    if op == "demux_unknown":
        out = eng.demux_unknown(hs.GRIDS[st["grid"]])
        out.pop("kernel_ms")
        return out
    if op == "demux_entry_pg":
        return {"pg": eng.demux_entry_pg()}
    if op == "fmx_prepare":
        af = inp.pls[m.i].af if m.i is not None else np.zeros(0)
        return dict(zip(("llk0", "llk2", "nsnps", "nreads"), eng.fmx_prepare(af)))
    if op == "set_clusters":
        eng.fmx_set_clusters(st["K"], inp.init(m.i, st["K"]))
        return {}
    if op == "iterate":
        got = eng.fmx_iterate(0.5, 0.1, want_full_ll=st["full_ll"])
        out = {"cells": got[0], "stats": np.array(got[1], dtype=np.int64)}
        if st["full_ll"]:
            out["full_ll"] = got[2]
        out["slots"] = slots(eng)
        return out
    if op == "iter_gp":
        eng.fmx_iter_gp(0.5, 0.1)
        return {}
    if op == "fmx_singlets":
        return {"sng": eng.fmx_singlets()}
    if op == "fmx_inclusion":
        return eng.fmx_inclusion(0.5)
    if op == "fmx_cluster_pileup":
        return dict(zip(("gls", "cnt"), eng.fmx_cluster_pileup()))
    if op in ("fmx_match_donors", "fmx_cluster_pairs"):
        out = eng.fmx_match_donors() if op == "fmx_match_donors" else eng.fmx_cluster_pairs()
        out.pop("kernel_ms")
        return out
    raise ValueError(op)


def fresh_call(seed, flags, st, inp, m):
    """the same call on a fresh engine that is given only what the step needs (m: the model after the step)"""
    op = st["op"]
    with make_engine(seed, flags) as e:
        p = inp.pls[m.i]
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        if op in hs.PANEL_READERS:
            e.demux_set_gp(*inp.panel(m.i, *m.panel))
        if op == "demux_entry_pg":
            e.demux_run(hs.GRIDS[m.grid], 0.5)
        if op == "iterate" or op in hs.FMX_TABLES or op == "fmx_cluster_pileup":
            e.fmx_prepare(p.af)
            e.fmx_set_clusters(m.K, inp.init(m.i, m.K))
            for _ in range(m.iters - (1 if op == "iterate" else 0)):
                e.fmx_iterate(0.5, 0.1)
            if m.rewritten:
                e.fmx_iter_gp(0.5, 0.1)
        return call(e, st, inp, m)


def same_bytes(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in got:
        if k == "slots":
            assert got[k] == want[k], f"{what}: timing slots {got[k]} on the long-lived handle, {want[k]} on a fresh one"
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            if a.dtype.names:
                bad = {f: int((a[f] != b[f]).sum()) for f in a.dtype.names if not np.array_equal(a[f], b[f])}
            else:
                bad = int((a != b).sum())
            raise AssertionError(f"{what}: {k} differs from a fresh handle's: {bad}")


def oracle_demux(st, inp, m, got, group):
    p = inp.pls[m.i]
    gp, has_gp = inp.panel(m.i, *m.panel)
    P = dataclasses.replace(p, gp=gp, has_gp=has_gp)
    alphas = hs.GRIDS[st["grid"]]
    want = ob.demux(P, alphas=alphas, nthreads=4)
    return parity.compare_demux(got["cells"], want, alphas, P)["max_abs_ll_diff"]


def oracle_fmx(inp, m, got, group):
    p, e, K = inp.pls[m.i], inp.eplp(m.i), m.K
    init = inp.init(m.i, K)
    cplp = ob.fmx_build_cluster_pileup(p, e, K, init)
    cells = ob.fmx_init_cells(init)
    for _ in range(m.iters):
        ostats = ob.fmx_iterate(p, e, K, cplp, cells)
    rep = parity.compare_fmx(got["cells"], cells, resolved=not group)
    if not group:   # (a group counts its near-tie cells instead of settling them: its counters may differ by those)
        assert tuple(int(x) for x in got["stats"]) == tuple(int(x) for x in ostats[:3]), (got["stats"], ostats)
    return rep["max_abs_ll_diff"]


def run_sequence(seed):
    """runs the sequence of `seed`; returns a report (steps, refusals, comparisons, oracle checks, worst oracle deviation)"""
    flags, seq = hs.sequence_and_flags(seed)
    group = hs.is_group(seed)
    inp = Inputs(seed)
    rep = dict(seed=seed, flags=flags, group=group, steps=len(seq), refused=0, compared=0, oracle_demux=0, oracle_fmx=0,
               worst=0.0, ops=[])
    saved = {b: os.environ.get(b) for b in hs.BUDGETS}
    for b in hs.BUDGETS:
        os.environ.pop(b, None)
    try:
        with make_engine(seed, flags) as eng:
            for k, (st, why, m) in enumerate(hs.replay(seq, hs.pl_facts(seed), flags, group)):
                what = f"seed {seed} step {k} {({a: b for a, b in st.items() if a != 'expect'})}"
                rep["ops"].append(st["op"] + ("!" if why else ""))
                if why is not None:
                    try:
                        call(eng, st, inp, m)
                    except muxgl.MuxglError as ex:
                        assert st["expect"] in str(ex), f"{what}: refused with {str(ex)!r}, the model says {st['expect']!r}"
                    else:
                        raise AssertionError(f"{what}: ran; the model says it is refused with {st['expect']!r}")
                    rep["refused"] += 1
                    continue
                try:
                    got = call(eng, st, inp, m)
                except muxgl.MuxglError as ex:
                    raise AssertionError(f"{what}: the model says it runs; refused with {str(ex)!r}")
                if not got:
                    continue
                want = fresh_call(seed, flags, st, inp, m)
                if st["op"] in NOT_BIT_IDENTICAL:
                    parity.same_records(got["cells"], want["cells"])
                else:
                    same_bytes(got, want, what)
                rep["compared"] += 1
                if st["op"] == "demux_run" and m.panel[0] <= 16 and m.C() > 0:
                    rep["worst"] = max(rep["worst"], oracle_demux(st, inp, m, got, group))
                    rep["oracle_demux"] += 1
                if st["op"] == "iterate" and m.K <= 16 and m.C() > 0:
                    rep["worst"] = max(rep["worst"], oracle_fmx(inp, m, got, group))
                    rep["oracle_fmx"] += 1
    finally:
        for b, v in saved.items():
            if v is None:
                os.environ.pop(b, None)
            else:
                os.environ[b] = v
    return rep


@pytest.mark.parametrize("seed", SEEDS)
def test_long_lived_handle_equals_fresh_ones(seed):
    rep = run_sequence(seed)
    print(json.dumps(rep))
    assert rep["oracle_demux"] >= 1 and rep["oracle_fmx"] >= 1, rep   # every sequence is also held to the oracle
    assert rep["worst"] < parity.LL_TOL


def main(argv):
    import argparse
    import traceback

    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0:20")
    ap.add_argument("--log", default=None)
    ap.add_argument("--keep-going", action="store_true")
    ap.add_argument("--budget-s", type=float, default=1e9, help="stop starting new sequences after this many seconds")
    a = ap.parse_args(argv)
    lo, hi = (int(x) for x in a.seeds.split(":"))
    log = open(a.log, "a") if a.log else None
    t0, fails, n = time.time(), 0, 0
    for seed in range(lo, hi):
        if time.time() - t0 > a.budget_s:
            break
        t = time.time()
        try:
            rec = run_sequence(seed)
            rec["ok"] = True
        except Exception as ex:  # noqa: BLE001  (a campaign reports and goes on or stops, as asked)
            rec = dict(seed=seed, ok=False, error=f"{type(ex).__name__}: {str(ex)[:800]}",
                       where=traceback.format_exc().strip().splitlines()[-3:])
            fails += 1
        rec["s"] = round(time.time() - t, 2)
        n += 1
        line = json.dumps(rec)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
        if fails and not a.keep_going:
            break
        if not rec["ok"] and "hip" in rec["error"].lower():   # an error of the runtime, not a finding: nothing more on this device
            break
    tail = json.dumps({"sequences": n, "failed": fails, "seconds": round(time.time() - t0, 1)})
    print(tail, flush=True)
    if log:
        log.write(tail + "\n")
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
