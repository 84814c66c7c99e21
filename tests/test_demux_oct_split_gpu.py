"""The default-grid demuxlet path (demux_oct.hip) with its cells run as two groups on two streams: the group key in the
launch order, units that hold chunks of one group only (padded to eight units per group, empty slots), the sweep's unit
base, the finish kernel's cell range, fork and join on the handle's stream.

Every case places the boundary with MUXGL_OCT_SPLIT before the plan is built and asks of the records that they
  * equal, byte for byte, those of the same engine with MUXGL_OCT_SPLIT=0 (one group: the two launches of before),
  * make the oracle's calls exactly, with log-likelihoods within 1e-7 (the bar of tests/test_demux_oct_finish_gpu.py),
  * equal those made behind the LL tensor (that run takes one group over the same plan),
  * come out the same from a second run on the same plan.
"""
import numpy as np
import pytest

import oracle_binding as ob
import parity
from popscle_amd import muxgl, synth
from test_demux_oct_finish_gpu import ALPHAS, CHUNK, FILL, SPECIAL, pileup_of

pytestmark = pytest.mark.gpu

KNOB = "MUXGL_OCT_SPLIT"


@pytest.fixture(scope="module")
def eng():
    e = muxgl.Engine(0)
    yield e
    e.close()


def plan_and_run(eng, p, monkeypatch, boundary):
    """a fresh plan for pileup p with the boundary at cell `boundary` (None: the default rule): the records of three runs
    (plain, behind the LL tensor, plain again) and what the probe says of the first"""
    if boundary is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(boundary))
    eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    eng.demux_set_gp(p.gp, p.has_gp)
    rec = eng.demux_run(ALPHAS, 0.5).copy()
    info = eng.demux_oct_split()
    behind_tensor, _ = eng.demux_run(ALPHAS, 0.5, want_full_ll=True)
    assert eng.demux_oct_split()["groups"] == 1  # the reduce kernel's path is one group
    behind_tensor = behind_tensor.copy()
    again = eng.demux_run(ALPHAS, 0.5).copy()
    return rec, behind_tensor, again, info


def check_boundaries(eng, p, monkeypatch, boundaries, linear=True):
    want = ob.demux(p, alphas=ALPHAS, nthreads=4)
    one, one_t, one_again, info = plan_and_run(eng, p, monkeypatch, 0)
    assert info["cut"] == 0 and info["groups"] == 1
    rep = parity.compare_demux(one, want, ALPHAS, p)  # (raises on a call that differs)
    assert rep["max_abs_ll_diff"] < 1e-7
    assert one.tobytes() == one_t.tobytes() == one_again.tobytes()
    for b in boundaries:
        rec, rec_t, again, info = plan_and_run(eng, p, monkeypatch, b)
        two = linear and 0 < b < p.C
        print(f"C={p.C} boundary {b}: {info}")
        assert info["groups"] == (2 if two else 1) and info["cut"] == (b if two else 0)
        assert info["units"] % 8 == 0
        assert rec.tobytes() == one.tobytes(), f"boundary {b}: records differ from the one-group run"
        assert rec_t.tobytes() == one.tobytes(), f"boundary {b}: records behind the LL tensor differ"
        assert again.tobytes() == one.tobytes(), f"boundary {b}: the second run differs"
        rep = parity.compare_demux(rec, want, ALPHAS, p)
        assert rep["max_abs_ll_diff"] < 1e-7


@pytest.mark.parametrize("V", [1, 7, 16, 17, 32])
def test_thirteen_cells_every_boundary(eng, monkeypatch, V):
    """thirteen cells of about forty entries, one chunk each; eight lanes per entry (four cells per finish workgroup) and
    sixteen (one): no boundary (0, 13: a group would be empty), boundaries that are no multiple of four, a group of fewer
    chunks than a unit (1 .. 5 in front, 1 behind at 12), and of exactly nine and eight chunks behind (4, 5)"""
    p = synth.make_pileup(13, 500, V, seed=6400 + V, mean_entries=40, min_entries=5)
    check_boundaries(eng, p, monkeypatch, (0, 1, 2, 3, 4, 5, 12, 13))


@pytest.mark.parametrize("V", [16, 20])
def test_boundary_around_the_empty_and_the_nine_chunk_cell(eng, monkeypatch, V):
    """cells of 300, 0, 1, 192, 193, 768, 769, 1537 and 40 entries: the boundary directly before the cell without a chunk
    (its group then starts with a cell that has none), directly behind it and one further, and one before, directly
    before and directly behind the cell of nine chunks"""
    lens = np.roll(np.array(SPECIAL + FILL), 1).tolist()
    assert lens[1] == 0 and lens[7] == 8 * CHUNK + 1
    p = pileup_of(lens, 2000, V, seed=6500 + V)
    check_boundaries(eng, p, monkeypatch, (1, 2, 3, 6, 7, 8))


def test_empty_cells_in_front(eng, monkeypatch):
    """the first group holds cells without entries only: no unit, no sweep launch, a finish that writes their zero records"""
    lens = [0, 0, 0] + SPECIAL[1:] + FILL
    p = pileup_of(lens, 2000, 16, seed=6600)
    check_boundaries(eng, p, monkeypatch, (1, 3, 4))


def test_without_linear_entries_is_one_group(monkeypatch):
    """MUXGL_FLAG_NO_LINEAR_ENTRIES has no launch order to carry the group key: one group whatever the knob says"""
    p = synth.make_pileup(13, 500, 16, seed=6700, mean_entries=40, min_entries=5)
    with muxgl.Engine(0, muxgl.FLAG_NO_LINEAR_ENTRIES) as e:
        check_boundaries(e, p, monkeypatch, (5,), linear=False)


def test_a_new_gp_tensor_and_a_new_pileup_get_a_new_plan(eng, monkeypatch):
    """the boundary belongs to the plan: muxgl_demux_set_gp and muxgl_set_pileup on the same engine rebuild it"""
    pa = synth.make_pileup(13, 500, 16, seed=6800, mean_entries=40, min_entries=5)
    pb = pileup_of(np.roll(np.array(SPECIAL + FILL), 4).tolist(), 2000, 16, seed=6801)
    one_a = plan_and_run(eng, pa, monkeypatch, 0)[0]
    one_b = plan_and_run(eng, pb, monkeypatch, 0)[0]
    rec, _, _, info = plan_and_run(eng, pa, monkeypatch, 3)
    assert info["cut"] == 3 and rec.tobytes() == one_a.tobytes()
    monkeypatch.setenv(KNOB, "7")
    eng.demux_set_gp(pa.gp, pa.has_gp)  # the same pileup, the tensor set again
    rec = eng.demux_run(ALPHAS, 0.5).copy()
    info = eng.demux_oct_split()
    assert info["cut"] == 7 and info["groups"] == 2 and rec.tobytes() == one_a.tobytes()
    monkeypatch.setenv(KNOB, "5")
    eng.set_pileup(pb.S, pb.cell_ptr, pb.entry_snp, pb.entry_rptr, pb.reads)  # nine cells where there were thirteen
    eng.demux_set_gp(pb.gp, pb.has_gp)
    rec = eng.demux_run(ALPHAS, 0.5).copy()
    info = eng.demux_oct_split()
    assert info["cut"] == 5 and info["groups"] == 2 and rec.tobytes() == one_b.tobytes()
    parity.compare_demux(rec, ob.demux(pb, alphas=ALPHAS, nthreads=4), ALPHAS, pb)


def test_the_default_rule(eng, monkeypatch):
    """without the knob: two groups only inside the window of sweep sizes where the split was measured to gain (1.5 to
    2.3 residency rounds of the device, chunks at least half full), the first group 0.55 of the chunks; a small pileup
    and one of many nearly empty chunks take the one-group path -- and the records are those of one group"""
    small = synth.make_pileup(13, 500, 16, seed=6900, mean_entries=40, min_entries=5)
    info = plan_and_run(eng, small, monkeypatch, None)[3]
    assert info["cut"] == 0 and info["groups"] == 1
    round_units = info["round_units"]
    assert round_units > 0 and info["units"] <= round_units
    # one chunk per cell, eight chunks per unit: 1.6 rounds
    C = round_units * 8 * 16 // 10
    sparse = pileup_of([4] * C, 400, 16, seed=6901)  # ... of chunks that hold four entries of 192: the finish dominates
    info = plan_and_run(eng, sparse, monkeypatch, None)[3]
    assert info["cut"] == 0 and info["groups"] == 1 and info["units"] > round_units
    p = pileup_of([100] * C, 2000, 16, seed=6902)
    one = plan_and_run(eng, p, monkeypatch, 0)[0]
    rec, rec_t, again, info = plan_and_run(eng, p, monkeypatch, None)
    print(f"C={C}: {info}")
    assert info["groups"] == 2 and info["cut"] == int(0.55 * C)  # every cell is one chunk
    assert rec.tobytes() == rec_t.tobytes() == again.tobytes() == one.tobytes()
