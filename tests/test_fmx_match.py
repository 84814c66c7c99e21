"""CPU checks behind muxgl_fmx_match_donors (fmx_match.hip): the header declares the call and the library exports it, no
timing slot and no ABI version were spent on it, a NULL handle is an error; the numpy restatement the GPU tests of
tests/test_fmx_match_gpu.py are held to (tests/match_ref.py) on a case computed by hand; freemuxlet.match_table; the cut
of a call (popscle_amd/csrc/match_plan.hpp through tests/csrc/match_plan_probe.cpp) pinned at a few shapes; and a count,
made without a GPU, of the kernel variants that the grid of tests/test_fmx_match_gpu.py and the fuzz seeds reach."""
import atexit
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from match_ref import restate_match
from popscle_amd import freemuxlet, muxgl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "muxgl.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# the grid of tests/test_fmx_match_gpu.py section 1b: every donor width (both ends of each where they differ) and one,
# two, three and five donor blocks; K = 11 leaves 1, 3 and 3 clusters over at tiles of 2, 4 and 8
GRID_V = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 64, 65, 128, 129, 257]
SHORT_V = [1, 5, 17, 65]
GRID_K = 11
TILES = (1, 2, 4, 8)


def grid_s(P, UNR):
    """the marker axes of the grid: three parts with a tail of five markers (GRID_V), and for SHORT_V one marker, below
    one unrolled group at G = 1, just past one at G = 64, and two parts with a tail of one marker"""
    return 2 * P + 5, (1, UNR - 1, 64 * UNR + 1, P + 1)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(muxgl.LIB_PATH):
        from popscle_amd.build import build_lib

        build_lib()
    return muxgl.load_library()


def test_header_declares_the_exact_prototype():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+muxgl_fmx_match_donors\s*\(\s*muxgl_handle\s*\*\s*h\s*,\s*double\s*\*\s*ll\s*,\s*double\s*\*\s*ll0\s*,"
                     r"\s*int32_t\s*\*\s*nsnps\s*,\s*float\s*\*\s*kernel_ms\s*\)\s*;", text)
    full = open(HEADER).read()
    assert int(re.search(r"MUXGL_T_COUNT\s*=\s*(\d+)", full).group(1)) == 16 and muxgl.T_COUNT == 16
    assert int(re.search(r"#define MUXGL_VERSION (\d+)", full).group(1)) == 3


def test_symbol_is_bound_and_exported(lib):
    res, args = muxgl.SYMBOLS["muxgl_fmx_match_donors"]
    assert len(args) == 5
    assert hasattr(lib, "muxgl_fmx_match_donors")
    nm = subprocess.run(["nm", "-D", "--defined-only", muxgl.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT muxgl_fmx_match_donors$", nm, flags=re.M)
    assert lib.muxgl_version() == 3


def test_null_handle_is_an_error(lib):
    assert lib.muxgl_fmx_match_donors(None, None, None, None, None) != 0


def _hand_case():
    """two SNPs, two clusters, two donors; a third and a fourth SNP carry the special cases"""
    K, S, V = 2, 4, 2
    gls = np.full((K, S, 9), 0.123)          # (off-diagonal values must not matter)
    counts = np.zeros((K, S, 3), dtype=np.int32)
    # cluster 0: reads at SNPs 0, 1, 2; cluster 1: reads at SNPs 1, 2, 3 (and none at SNP 0)
    counts[0, (0, 1, 2), 0] = (3, 1, 2)
    counts[1, (1, 2, 3), 0] = (5, 1, 1)
    diag = {(0, 0): (0.5, 0.25, 0.125), (0, 1): (0.1, 0.2, 0.4), (0, 2): (0.3, 0.3, 0.3), (0, 3): (1.0, 1.0, 1.0),
            (1, 0): (1.0, 1.0, 1.0), (1, 1): (0.25, 0.5, 0.125), (1, 2): (0.2, 0.2, 0.2), (1, 3): (0.5, 0.25, 0.25)}
    for (k, s), d in diag.items():
        gls[k, s, (0, 4, 8)] = d
    gp = np.zeros((S, V, 3))
    gp[0] = [[1.0, 0.0, 0.0], [0.0, 0.5, 0.5]]
    gp[1] = [[0.0, 1.0, 0.0], [0.5, 0.5, 0.0]]
    gp[2] = np.nan                             # SNP 2: no genotypes, the row is garbage
    gp[3] = [[0.0, 0.0, 0.0], [0.25, 0.25, 0.5]]   # donor 0: a zero factor
    has_gp = np.array([1, 1, 0, 1], dtype=np.uint8)
    af = np.array([0.5, 0.25, 0.1, 0.5])
    return gls, counts, gp, has_gp, af


def test_restatement_on_a_hand_computed_case():
    gls, counts, gp, has_gp, af = _hand_case()
    ll, ll0, nsnps = restate_match(gls, counts, gp, has_gp, af)
    assert nsnps.tolist() == [2, 2]              # cluster 0: SNPs 0, 1; cluster 1: SNPs 1, 3 (2: no genotypes; 0: no reads)
    log = math.log
    want = np.array([
        # cluster 0: SNP 0 (0.5, 0.25, 0.125), SNP 1 (0.1, 0.2, 0.4)
        [log(0.5) + log(0.2), log(0.25 * 0.5 + 0.125 * 0.5) + log(0.1 * 0.5 + 0.2 * 0.5)],
        # cluster 1: SNP 1 (0.25, 0.5, 0.125), SNP 3 (0.5, 0.25, 0.25); donor 0's triple at SNP 3 is all zero
        [-math.inf, log(0.25 * 0.5 + 0.5 * 0.5) + log(0.5 * 0.25 + 0.25 * 0.25 + 0.25 * 0.5)]])
    assert np.array_equal(np.isneginf(ll), np.isneginf(want)) and not np.isnan(ll).any()
    fin = np.isfinite(want)
    assert np.max(np.abs(ll[fin] - want[fin])) < 1e-15
    want0 = [log(0.5 * 0.25 + 0.25 * 0.5 + 0.125 * 0.25) + log(0.1 * 0.5625 + 0.2 * 0.375 + 0.4 * 0.0625),
             log(0.25 * 0.5625 + 0.5 * 0.375 + 0.125 * 0.0625) + log(0.5 * 0.25 + 0.25 * 0.5 + 0.25 * 0.25)]
    assert np.max(np.abs(ll0 - want0)) < 1e-15


def test_restatement_edges():
    gls, counts, gp, has_gp, af = _hand_case()
    ll, ll0, nsnps = restate_match(gls, counts, gp, np.zeros(4, dtype=np.uint8), af)   # no marker with genotypes
    assert not ll.any() and not ll0.any() and not nsnps.any()
    counts[1] = 0                                                                        # a cluster without cells
    ll, ll0, nsnps = restate_match(gls, counts, gp, has_gp, af)
    assert nsnps.tolist() == [2, 0] and not ll[1].any() and ll0[1] == 0.0 and np.isfinite(ll[0]).all()


def test_match_table_on_a_crafted_table():
    #            donor 0  donor 1  donor 2
    llr = np.array([[5.0, 5.0, -3.0],     # cluster 0: tie of donors 0 and 1 -> best 0, next 1
                    [-9.0, 7.0, 2.0],     # cluster 1: best 1, next 2
                    [0.0, 0.0, 0.0],      # cluster 2: empty
                    [6.0, 1.0, 4.0],      # cluster 3: best 0 -- and a better cluster for donor 0 than cluster 0
                    [-2.0, -8.0, 4.0]])   # cluster 4: best 2, tie with cluster 3 on donor 2 -> donor 2's best cluster is 3
    ll0 = np.array([-100.0, -50.0, 0.0, -10.0, -20.0])
    ll = llr + ll0[:, None]
    nsnps = np.array([10, 10, 0, 10, 10])
    for t in (freemuxlet.match_table(ll, ll0, nsnps), freemuxlet.match_table(ll, ll0)):
        assert t["best"].tolist() == [0, 1, -1, 0, 2] and t["next"].tolist() == [1, 2, -1, 2, 0]
        assert t["best"].dtype == np.int32
        assert np.array_equal(t["best_llr"], [5.0, 7.0, np.nan, 6.0, 4.0], equal_nan=True)
        assert np.array_equal(t["next_llr"], [5.0, 2.0, np.nan, 4.0, -2.0], equal_nan=True)
        # donor 0's best cluster is 3, donor 1's is 1, donor 2's is 3 (tie 4.0 with cluster 4: lower index)
        assert t["reciprocal"].tolist() == [False, True, False, True, False]
        assert np.allclose(t["post"].sum(axis=1), 1.0)
        e = np.exp(llr[1] - llr[1].max())
        assert np.allclose(t["post"][1], e / e.sum(), rtol=1e-14)
        assert np.allclose(t["post"][2], 1.0 / 3.0)
    # -inf scores: never NaN, and a donor at -inf is never the best while another is finite
    ll2 = ll.copy()
    ll2[1, 1] = -np.inf
    t = freemuxlet.match_table(ll2, ll0, nsnps)
    assert t["best"][1] == 2 and t["next"][1] == 0 and t["post"][1, 1] == 0.0 and not np.isnan(t["post"]).any()
    one = freemuxlet.match_table(np.array([[-3.0], [0.0]]), np.array([-5.0, 0.0]), np.array([4, 0]))   # a single donor
    assert one["best"].tolist() == [0, -1] and one["next"].tolist() == [-1, -1] and one["reciprocal"].tolist() == [True, False]


# ---- the cut of a call ----------------------------------------------------------------------------------------------------

_PROBE = []


def load_plan_probe():
    """tests/csrc/match_plan_probe.cpp compiled on its own (plain C++, no device), once per process"""
    if not _PROBE:
        cxx = HIPCC if os.path.exists(HIPCC) else shutil.which("g++") or shutil.which("c++")
        if not cxx:
            pytest.skip("no C++ compiler found")
        td = tempfile.mkdtemp(prefix="match_plan_probe")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "match_plan_probe.so")
        r = subprocess.run([cxx, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                            os.path.join(ROOT, "tests", "csrc", "match_plan_probe.cpp"), "-o", so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lib = C.CDLL(so)
        lib.probe_match_plan.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_uint64, C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        lib.probe_match_plan.restype = None
        _PROBE.append(lib)
    return _PROBE[0]


def match_plan(lib, S, V, K, part, want_ll=True, budget=4 << 30):
    """dict of np (parts), vh (donor lanes of a SNP slot), per_k (bytes of a cluster in a batch), kb (clusters of a batch)"""
    n, vh, per, kb = C.c_int(), C.c_int(), C.c_double(), C.c_int()
    lib.probe_match_plan(S, V, K, part, 1 if want_ll else 0, budget, C.byref(n), C.byref(vh), C.byref(per), C.byref(kb))
    return dict(np=n.value, vh=vh.value, per_k=per.value, kb=kb.value)


def _part():
    src = open(os.path.join(ROOT, "popscle_amd", "csrc", "fmx_match.hip")).read()
    assert "match_plan::parts(S, FMM_PART)" in src and "match_plan::lane_width(V)" in src   # the unit calls the header
    return int(re.search(r"FMM_PART\s*=\s*(\d+)", src).group(1)), int(re.search(r"FMM_UNR\s*=\s*(\d+)", src).group(1))


def test_plan_is_pinned():
    lib, (P, UNR) = load_plan_probe(), _part()
    assert (P, UNR) == (2048, 8)
    MB = 1 << 20
    # (S, V, K, want_ll, budget) -> parts, lanes, bytes per cluster, clusters per batch
    table = [
        ((1, 1, 1, True, 4 << 30), (1, 1, 8 + 8 + 12 + 4 + 12, 1)),
        ((2 * P + 5, 9, 130, True, MB), (3, 16, 8 * 3 * 9 + 8 * 9 + 36 + 4 * 4101 + 12, 62)),     # the many-cluster GPU test
        ((2 * P + 5, 9, 300, True, MB), (3, 16, 16740, 62)),
        ((2 * P + 5, 9, 300, True, 4 << 30), (3, 16, 16740, 300)),
        ((2 * P + 5, 9, 300, False, MB), (3, 16, 36 + 16404 + 12, 63)),                          # ll0 / nsnps alone: no donor logs
        ((150000, 65, 5, True, MB), (74, 64, 8 * 74 * 65 + 8 * 65 + 12 * 74 + 600000 + 12, 1)),  # test_budget_does_not_matter
        ((150000, 65, 5, True, 2 * MB), (74, 64, 639900, 3)),
        ((P, 32, 1024, True, MB), (1, 32, 8 * 32 + 8 * 32 + 12 + 4 * P + 12, 120)),
        ((P + 1, 33, 1024, True, 4 << 30), (2, 64, 8 * 2 * 33 + 8 * 33 + 24 + 4 * (P + 1) + 12, 1024)),
        ((100000, 1024, 1024, True, MB // 2), (49, 64, 8 * 49 * 1024 + 8 * 1024 + 12 * 49 + 400000 + 12, 1)),   # not even one fits: one
    ]
    for (S, V, K, want_ll, budget), want in table:
        got = match_plan(lib, S, V, K, P, want_ll, budget)
        assert (got["np"], got["vh"], got["per_k"], got["kb"]) == want, ((S, V, K, want_ll, budget), got, want)
    for V, vh in [(1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64),
                  (65, 64), (1024, 64)]:
        assert match_plan(lib, 1, V, 1, P)["vh"] == vh
    rng = np.random.default_rng(11)
    for _ in range(2000):
        S, V, K = int(rng.integers(1, 10 ** 6)), int(rng.integers(1, 1025)), int(rng.integers(1, 1025))
        bud = int(rng.integers(1, 1 << 33))
        g = match_plan(lib, S, V, K, P, True, bud)
        assert (g["np"] - 1) * P < S <= g["np"] * P and g["vh"] in (1, 2, 4, 8, 16, 32, 64)
        assert min(V, 64) <= g["vh"] and (g["vh"] == 1 or g["vh"] // 2 < V)
        assert 1 <= g["kb"] <= K and (g["kb"] == 1 or g["kb"] * g["per_k"] <= bud) and (g["kb"] == K or (g["kb"] + 1) * g["per_k"] > bud)


def cases_plans(cases):
    return [m["plan"] for m in cases]


def test_grid_and_fuzz_seeds_reach_every_variant():
    """what section 1b of tests/test_fmx_match_gpu.py and the match of the FUZZ_SEEDS cases (tests/test_fuzz_gpu.py
    match_case) run, counted from the plan probe and the generators: a later edit of either cannot lose a kernel variant or
    a hard input without this test saying so"""
    import test_fuzz_gpu as fz

    lib, (P, UNR) = load_plan_probe(), _part()
    long_s, short_s = grid_s(P, UNR)
    grid = [match_plan(lib, long_s, V, GRID_K, P) for V in GRID_V]
    assert {g["vh"] for g in grid} == {1, 2, 4, 8, 16, 32, 64} and all(g["np"] == 3 for g in grid)
    short = [match_plan(lib, S, V, GRID_K, P) for S in short_s for V in SHORT_V]
    assert {(g["vh"], g["np"]) for g in short} == {(vh, n) for vh in (1, 8, 32, 64) for n in (1, 2)}
    assert {min(3, (V + 63) // 64) for V in GRID_V} == {1, 2, 3}                       # one, two, three or more donor blocks
    assert all(GRID_K % t for t in TILES if t > 1)                                     # a tile remainder at every tile size

    cases = []
    for seed in fz.FUZZ_SEEDS:
        info, p = fz.fmx_case(seed)
        m = fz.match_case(seed, info, p)
        m["plan"] = match_plan(lib, p.S, m["V"], info["K"], P)
        m["K"] = info["K"]
        cases.append(m)
        assert m["V"] in fz.MATCH_V and m["tile"] in TILES and m["gp"].shape == (p.S, m["V"], 3)
        assert info["K"] * m["V"] * p.S <= fz.MATCH_WORK
    vhs = {m["plan"]["vh"] for m in cases} | {g["vh"] for g in grid}
    assert vhs == {1, 2, 4, 8, 16, 32, 64}
    assert {m["tile"] for m in cases} == set(TILES)
    assert len({m["plan"]["vh"] for m in cases}) >= 4                                  # the fuzz alone: most donor widths
    parts = {min(3, g["np"]) for g in cases_plans(cases) + grid + short}
    assert parts == {1, 2, 3} and {min(3, g["np"]) for g in cases_plans(cases)} >= {1, 3}
    assert any(m["K"] % m["tile"] for m in cases)                                      # a tile remainder in the fuzz too
    assert any(m["mode"] == "zeros" for m in cases)
    assert any(m["dup_pairs"] > 0 and m["has_gp"].any() for m in cases)
    assert any(not m["has_gp"].any() for m in cases)
    assert any(m["slab"] == "1" for m in cases) and any(m["slab"] is None for m in cases)
