"""One step of the default-grid demuxlet path (demux_oct.hip) as the caller sees it: each cell group's sweep and finish
on a stream of its own, joined by the host before muxgl_demux_run reads the records, and the two timing slots of the step.

Stale records: forty consecutive runs on one engine alternate the doublet prior, which enters every cell's record, so a
record read before its finish kernel ended is the other prior's and differs from the one-group engine's.  The forced
boundaries put 10 %, 55 % and 90 % of the cells into the first group: either finish may be the one that ends last.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_binding as ob
import parity
from popscle_amd import muxgl, synth

pytestmark = pytest.mark.gpu

ALPHAS = (0.0, 0.5)
PRIORS = (0.5, 0.05)
KNOB = "MUXGL_OCT_SPLIT"
C_CELLS, RUNS = 600, 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[16, 20])
def case(request):
    """the pileup, the oracle's records at the first prior, and the one-group engine's records at both"""
    V = request.param
    p = synth.make_pileup(C_CELLS, 2000, V, seed=7200 + V, mean_entries=300)
    want = ob.demux(p, alphas=ALPHAS, nthreads=4)
    old = os.environ.get(KNOB)
    os.environ[KNOB] = "0"
    try:
        with muxgl.Engine(0) as e:
            e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
            e.demux_set_gp(p.gp, p.has_gp)
            one = {pr: e.demux_run(ALPHAS, pr).copy() for pr in PRIORS}
            assert e.demux_oct_split()["groups"] == 1
    finally:
        if old is None:
            del os.environ[KNOB]
        else:
            os.environ[KNOB] = old
    return V, p, want, one


def every_record_differs(a, b):
    w = a.dtype.itemsize
    x = np.frombuffer(a.tobytes(), dtype=np.uint8).reshape(-1, w)
    y = np.frombuffer(b.tobytes(), dtype=np.uint8).reshape(-1, w)
    return (x != y).any(axis=1)


@pytest.mark.parametrize("share", [0.10, 0.55, 0.90])
@pytest.mark.parametrize("between", [False, True], ids=["runs", "runs_singlets_set_gp"])
def test_no_stale_record_in_forty_runs(case, monkeypatch, share, between):
    V, p, want, one = case
    differ = every_record_differs(one[PRIORS[0]], one[PRIORS[1]])
    assert differ.all(), f"{(~differ).sum()} cells have the same record at both priors: they could hide a stale read"
    cut = int(round(share * p.C))
    monkeypatch.setenv(KNOB, str(cut))
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        for i in range(RUNS):
            pr = PRIORS[i % 2]
            rec = e.demux_run(ALPHAS, pr)
            assert rec.tobytes() == one[pr].tobytes(), f"run {i}, prior {pr}: records differ from the one-group engine's"
            if i == 0:
                info = e.demux_oct_split()
                assert info["groups"] == 2 and info["cut"] == cut
                rep = parity.compare_demux(rec, want, ALPHAS, p)  # (raises on a call that differs)
                assert rep["max_abs_ll_diff"] < 1e-7
            if between and i % 4 == 1:
                sng = e.demux_singlets(ALPHAS)
                assert np.isfinite(sng).all()
            if between and i % 8 == 3:
                e.demux_set_gp(p.gp, p.has_gp)  # the same tensor: a new plan, the same boundary


def timed_run(e, **kw):
    t0 = time.perf_counter()
    out = e.demux_run(ALPHAS, 0.5, **kw)
    wall_ms = (time.perf_counter() - t0) * 1e3
    return out, wall_ms


@pytest.mark.parametrize("how", ["one_group", "two_groups", "no_linear_entries", "behind_the_tensor"])
def test_timing_slots(case, monkeypatch, how):
    V, p, want, one = case
    monkeypatch.setenv(KNOB, str(p.C // 2) if how in ("two_groups", "behind_the_tensor") else "0")
    flags = muxgl.FLAG_NO_LINEAR_ENTRIES if how == "no_linear_entries" else 0
    with muxgl.Engine(0, flags) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        e.demux_run(ALPHAS, 0.5)  # (the plan is built by the first run)
        e.timing_sum(reset=True)
        for i in range(3):
            _, wall = timed_run(e, want_full_ll=how == "behind_the_tensor")
            assert e.demux_oct_split()["groups"] == (2 if how == "two_groups" else 1)
            ms = e.timing().copy()
            sweep, reduce_ = float(ms[muxgl.T_DEMUX_SWEEP]), float(ms[muxgl.T_DEMUX_REDUCE])
            print(f"V={V} {how}: sweep {sweep:.4f} ms, reduce {reduce_:.4f} ms, call {wall:.4f} ms")
            assert sweep > 0 and reduce_ >= 0
            assert sweep + reduce_ <= wall
            assert e.timing_sum()[1] == i + 1
        before = e.timing().copy()  # the slots of the last run
        assert before[muxgl.T_DEMUX_SWEEP] > 0
        e.demux_singlets(ALPHAS)
        after = e.timing()
        assert after[muxgl.T_DEMUX_SWEEP] == before[muxgl.T_DEMUX_SWEEP]
        assert after[muxgl.T_DEMUX_REDUCE] == before[muxgl.T_DEMUX_REDUCE]


CHILD = r"""
import sys
import numpy as np
from popscle_amd import muxgl, synth
V, cut = int(sys.argv[1]), sys.argv[2]
p = synth.make_pileup(%d, 2000, V, seed=7200 + V, mean_entries=300)
with muxgl.Engine(0) as e:
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)
    recs = [e.demux_run((0.0, 0.5), pr).tobytes() for pr in (0.5, 0.05, 0.5)]
    ms = e.timing()
    print("GROUPS", e.demux_oct_split()["groups"], "SLOTS", float(ms[muxgl.T_DEMUX_SWEEP]), float(ms[muxgl.T_DEMUX_REDUCE]))
    sys.stdout.flush()
    sys.stdout.buffer.write(b"RECORDS\n" + b"".join(recs))
""" % C_CELLS


@pytest.mark.parametrize("groups", [1, 2])
def test_without_events_the_records_are_the_same_and_the_slots_zero(case, groups):
    """MUXGL_NO_EVENTS is read once per process: a child"""
    V, p, want, one = case
    env = dict(os.environ, MUXGL_NO_EVENTS="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env[KNOB] = str(p.C // 2) if groups == 2 else "0"
    r = subprocess.run([sys.executable, "-c", CHILD, str(V), env[KNOB]], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    head, _, body = r.stdout.partition(b"RECORDS\n")
    words = head.decode().split()
    assert int(words[words.index("GROUPS") + 1]) == groups
    i = words.index("SLOTS")
    assert float(words[i + 1]) == 0.0 and float(words[i + 2]) == 0.0
    assert body == b"".join(one[pr].tobytes() for pr in (0.5, 0.05, 0.5))  # the records of all three runs
