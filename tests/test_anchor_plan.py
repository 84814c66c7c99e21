"""CPU test of where an anchored freemuxlet run starts (popscle_amd/csrc/anchor_plan.hpp): the relabelling of the greedy
clusters from the donor match.  The C++ plan (what `popscle-amd freemuxlet --anchor-vcf` runs) is held equal to
freemuxlet.anchor_start (what the Python driver runs) on random tables with ties, NaNs, empty clusters, more leftovers than
free ids, no anchors and nothing but anchors; five hand-written cases pin both to the rule itself.

The header is compiled into a small shared object with hipcc (plain C++: no device code, no device is touched)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from popscle_amd import freemuxlet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAN = float("nan")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "anchor_plan_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "anchor_plan_probe.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.probe_anchor_plan.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.probe_anchor_plan.restype = None
    return lib


def plan_cpp(lib, llr, nsnps, ncells, donor):
    llr = np.ascontiguousarray(llr, dtype=np.float64)
    K, V = llr.shape
    nsnps = np.ascontiguousarray(nsnps, dtype=np.int32)
    ncells = np.ascontiguousarray(ncells, dtype=np.int64)
    donor = np.ascontiguousarray(donor, dtype=np.int32)
    n = donor.size
    new_id = np.full(K, -7, dtype=np.int32)
    match = np.full(max(n, 1), -7, dtype=np.int32)
    mllr = np.zeros(max(n, 1))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.probe_anchor_plan(K, V, ptr(llr), ptr(nsnps), ptr(ncells), n, ptr(donor), ptr(new_id), ptr(match), ptr(mllr))
    return dict(new_id=new_id, match=match[:n], match_llr=mllr[:n])


def same(a, b):
    assert np.array_equal(a["new_id"], b["new_id"]), (a, b)
    assert np.array_equal(a["match"], b["match"]), (a, b)
    assert np.array_equal(a["match_llr"], b["match_llr"], equal_nan=True), (a, b)


def check_rule(r, llr, nsnps, ncells, donor):
    """what the rule promises, on the result alone"""
    K, n = len(ncells), len(donor)
    ids = r["new_id"]
    assert ids.shape == (K,) and r["match"].shape == (n,)
    used = ids[ids >= 0]
    assert len(set(used.tolist())) == used.size and (used < K).all()          # one greedy cluster per id
    for i in range(n):
        k = r["match"][i]
        if k < 0:
            assert np.isnan(r["match_llr"][i]) and not (ids == i).any()        # an unmatched anchor starts empty
        else:
            v = llr[k][donor[i]]
            assert ids[k] == i and v > 0 and nsnps[k] != 0 and r["match_llr"][i] == v
    left = [k for k in range(K) if ids[k] < 0 or ids[k] >= n]
    placed = [k for k in left if ids[k] >= n]
    assert len(placed) == min(len(left), K - n)
    assert sorted(ids[placed].tolist()) == list(range(n, n + len(placed)))     # the free ids are filled from n upwards
    order = sorted(left, key=lambda k: (-int(ncells[k]), k))
    assert [k for k in order[:len(placed)]] == sorted(placed, key=lambda k: ids[k])


HAND = [
    # 1. two anchors, three clusters: the best pair first, then the best of what is left; the leftover takes id 2
    dict(llr=[[5.0, 1.0], [4.0, 3.0], [-1.0, -2.0]], nsnps=[9, 9, 9], ncells=[10, 20, 30], donor=[0, 1],
         new_id=[0, 1, 2], match=[0, 1], match_llr=[5.0, 3.0]),
    # 2. nothing above zero (0 itself is no match): both anchors start empty, the two largest clusters fill the one free id
    dict(llr=[[0.0, -1.0], [-3.0, 0.0], [NAN, -2.0]], nsnps=[5, 5, 5], ncells=[7, 9, 9], donor=[1, 0],
         new_id=[-1, 2, -1], match=[-1, -1], match_llr=[NAN, NAN]),
    # 3. a tie on the value: the lower cluster wins the donor, then the lower anchor (the same donor twice)
    dict(llr=[[2.0], [2.0], [2.0]], nsnps=[1, 1, 1], ncells=[1, 1, 5], donor=[0, 0],
         new_id=[0, 1, 2], match=[0, 1], match_llr=[2.0, 2.0]),
    # 4. a cluster without markers never matches however large its number; NaN counts as -inf
    dict(llr=[[100.0, NAN], [1.0, NAN], [NAN, 0.5]], nsnps=[0, 3, 3], ncells=[50, 1, 1], donor=[0, 1],
         new_id=[2, 0, 1], match=[1, 2], match_llr=[1.0, 0.5]),
    # 5. K = n: no free id; the unmatched cluster leaves its cells unassigned
    dict(llr=[[-1.0, -1.0], [3.0, 8.0]], nsnps=[4, 4], ncells=[100, 1], donor=[0, 1],
         new_id=[-1, 1], match=[-1, 1], match_llr=[NAN, 8.0]),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_written_cases(probe, case):
    h = HAND[case]
    want = dict(new_id=np.array(h["new_id"], dtype=np.int32), match=np.array(h["match"], dtype=np.int32),
                match_llr=np.array(h["match_llr"], dtype=np.float64))
    K = len(h["ncells"])
    llr = np.array(h["llr"], dtype=np.float64)
    same(freemuxlet.anchor_start(llr, h["nsnps"], h["ncells"], h["donor"], K), want)
    same(plan_cpp(probe, llr, h["nsnps"], h["ncells"], h["donor"]), want)
    check_rule(want, llr, h["nsnps"], h["ncells"], h["donor"])


def test_probe_equals_numpy_on_random_tables(probe):
    rng = np.random.default_rng(2024)
    seen = dict(ties=0, nans=0, empty=0, overflow=0, none=0, all=0)
    for trial in range(400):
        K = int(rng.integers(1, 13))
        V = int(rng.integers(1, 9))
        n = int(rng.choice([0, K, rng.integers(0, K + 1)]))
        donor = rng.integers(0, V, n)                         # duplicates allowed
        llr = np.round(rng.normal(0.5, 3.0, (K, V)))          # integers: many exact ties, many zeros
        llr[rng.random((K, V)) < 0.1] = NAN
        llr[rng.random((K, V)) < 0.03] = -np.inf
        nsnps = np.where(rng.random(K) < 0.2, 0, rng.integers(1, 50, K))
        ncells = rng.integers(0, 4, K) * 10                   # ties in the cell counts too
        a = freemuxlet.anchor_start(llr, nsnps, ncells, donor, K)
        b = plan_cpp(probe, llr, nsnps, ncells, donor)
        same(a, b)
        check_rule(a, llr, nsnps, ncells, donor)
        pos = llr[:, donor][np.isfinite(llr[:, donor])] if n else np.zeros(0)
        seen["ties"] += int(pos.size != np.unique(pos).size)
        seen["nans"] += int(np.isnan(llr).any())
        seen["empty"] += int((nsnps == 0).any())
        seen["overflow"] += int((a["new_id"] < 0).any())
        seen["none"] += int(n == 0)
        seen["all"] += int(n == K)
    assert all(v > 20 for v in seen.values()), seen


def test_anchor_start_refuses_bad_shapes():
    with pytest.raises(ValueError):
        freemuxlet.anchor_start(np.zeros((3, 2)), [1, 1], [1, 1, 1], [0], 3)
    with pytest.raises(ValueError):
        freemuxlet.anchor_start(np.zeros((3, 2)), [1, 1, 1], [1, 1, 1], [2], 3)
    with pytest.raises(ValueError):
        freemuxlet.anchor_start(np.zeros((2, 2)), [1, 1], [1, 1], [0, 1, 0], 2)
