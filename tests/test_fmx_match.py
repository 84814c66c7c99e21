"""CPU checks behind muxgl_fmx_match_donors (fmx_match.hip): the header declares the call and the library exports it, no
timing slot and no ABI version were spent on it, a NULL handle is an error; the numpy restatement the GPU tests of
tests/test_fmx_match_gpu.py are held to (tests/match_ref.py) on a case computed by hand; and freemuxlet.match_table."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from match_ref import restate_match
from popscle_amd import freemuxlet, muxgl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "muxgl.h")


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
