"""CPU checks behind muxgl_fmx_unknown: the library exports the call and the header declares it with its signature, the
unchanged ABI version and timing-slot count, the cost function of a cell in table_plan.hpp, unknown_summary, and the
premise of the yardstick the GPU tests of tests/test_fmx_unknown_gpu.py lean on: the oracle's E-step with K + 2 clusters,
two of them empty, leaves the K-cluster triangle bit for bit as it is and holds, in its slots (K, j), (K, K) and
(K + 1, K), the three formulas of include/muxgl.h (tests/fmx_unknown_ref.py restates them in numpy).  Where oracle/_ref
is built the same is checked on the reference's own loop, restarted with K + 2 clusters from an iteration's assignments."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fmx_unknown_ref as fur
import oracle_binding as ob
import ref_binding as rb
from popscle_amd import freemuxlet, muxgl, synth
from test_demux_gpu import _with_empty_cells
from test_fmx_singlets import cluster_posteriors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "muxgl.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(muxgl.LIB_PATH):
        from popscle_amd.build import build_lib

        build_lib()
    return muxgl.load_library()


def test_library_exports_and_header_declares_the_call(lib):
    assert hasattr(lib, "muxgl_fmx_unknown")
    assert "muxgl_fmx_unknown" in muxgl.SYMBOLS
    assert muxgl.FMX_UNKNOWN_FIELDS == ("ll_ju", "ll_u", "ll_uu") == muxgl.Engine.FMX_UNKNOWN_FIELDS
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+muxgl_fmx_unknown\s*\(\s*muxgl_handle\s*\*\s*h\s*,\s*const\s+double\s*\*\s*gp0\s*,\s*"
                     r"double\s*\*\s*ll_ju\s*,\s*double\s*\*\s*ll_u\s*,\s*double\s*\*\s*ll_uu\s*,\s*float\s*\*\s*kernel_ms\s*\)\s*;",
                     text)
    assert lib.muxgl_fmx_unknown(None, None, None, None, None, None) != 0   # no handle: an error, not a crash


def test_version_and_timing_slots_are_unchanged(lib):
    text = open(HEADER).read()
    assert int(re.search(r"MUXGL_T_COUNT\s*=\s*(\d+)", text).group(1)) == 16 == muxgl.T_COUNT
    assert int(re.search(r"#define MUXGL_VERSION (\d+)", text).group(1)) == 3
    assert lib.muxgl_version() == 3


# ---- the premise of the yardstick ---------------------------------------------------------------------------------------

def _case(K):
    p = _with_empty_cells(synth.make_pileup(30, 400, max(K, 2), seed=77 + K, mean_entries=60, min_entries=5, with_gp=False),
                          [4, 29])
    init = (np.arange(p.C) % K).astype(np.int32)   # an empty droplet and an empty cluster among the inputs
    if K > 2:
        init[init == K - 1] = 0
    return p, init


def _check_triangle(ext, full, want, K, what):
    """ext: the K + 2 cluster triangle; full: the K cluster one; want: the restated tables"""
    nk = K * (K + 1) // 2
    assert ext[:, :nk].tobytes() == full.tobytes(), what              # the first K clusters: untouched
    rk, rk1 = nk, (K + 1) * (K + 2) // 2
    assert ext[:, rk1:rk1 + K].tobytes() == ext[:, rk:rk + K].tobytes(), what    # row K + 1 is row K ...
    assert ext[:, rk1 + K + 1].tobytes() == ext[:, rk + K].tobytes(), what       # ... and so is its singlet
    worst = 0.0
    for got, w in zip(fur.slots(ext, K), want):
        d = float(np.abs(got - w).max())
        worst = max(worst, d)
        assert d <= 1e-9, (what, d)
    return worst


@pytest.mark.parametrize("K,geno_error", [(1, 0.1), (3, 0.1), (6, 0.0), (9, 0.1)])
def test_two_empty_clusters_hold_the_three_tables(K, geno_error):
    p, init = _case(K)
    eplp = ob.fmx_entry_pileup(p)
    egl = eplp["gls"]
    assert np.array_equal(egl[:, [1, 2, 5]], egl[:, [3, 6, 7]])       # bitwise symmetric: one orientation is enough
    cplp = ob.fmx_build_cluster_pileup(p, eplp, K, init)
    cells = ob.fmx_init_cells(init)
    u = fur.hardy_weinberg(p.af)
    worst = 0.0
    for it in range(3):
        want = fur.unknown_tables(p, egl, cluster_posteriors(p.af, cplp, geno_error), u)
        ext = fur.extended_estep(p, eplp, K, cplp, cells, geno_error, nthreads=2)   # (on copies)
        *_, full = ob.fmx_iterate(p, eplp, K, cplp, cells, 0.5, geno_error, full_ll=True, nthreads=2)
        worst = max(worst, _check_triangle(ext, full, want, K, (K, geno_error, it)))
    lens = np.diff(p.cell_ptr)
    assert (lens == 0).sum() == 2 and all(np.all(w[lens == 0] == 0.0) for w in want)
    print(f"K={K} ge={geno_error}: max |restatement - oracle slots| = {worst:.3e}")
    if rb.available():
        scl = rb.RefScl.from_packed(p)
        ref = scl.freemux2(K, geno_error=geno_error, init_clust=init, full_ll=True, cluster_pileups=True)
        for t in range(min(2, ref["n_iter"] - 1)):
            # restarted from the assignments of iteration t: its first iteration is iteration t + 1 of the K-cluster run
            r2 = rb.RefScl.from_packed(p).freemux2(K + 2, geno_error=geno_error, init_clust=ref["cells"][t]["clust"],
                                                   full_ll=True)
            want = fur.unknown_tables(p, egl, cluster_posteriors(p.af, ref["cplp"][t], geno_error), u)
            _check_triangle(r2["full_ll"][0], ref["full_ll"][t + 1], want, K, ("reference", K, geno_error, t))


def test_restatement_against_a_one_hot_prior():
    """a specific donor's genotypes as gp0: the tables are then the singlet / doublet likelihoods with that genotype"""
    K = 3
    p, init = _case(K)
    eplp = ob.fmx_entry_pileup(p)
    egl = eplp["gls"]
    q = cluster_posteriors(p.af, ob.fmx_build_cluster_pileup(p, eplp, K, init), 0.1)
    geno = np.arange(p.S) % 3
    u = np.eye(3)[geno]
    ju, lu, uu = fur.unknown_tables(p, egl, q, u)
    ge = geno[p.entry_snp]
    e = np.arange(p.nnz)
    f = (egl[e, 3 * ge, None] * q[p.entry_snp, :, 0] + egl[e, 3 * ge + 1, None] * q[p.entry_snp, :, 1]) + \
        egl[e, 3 * ge + 2, None] * q[p.entry_snp, :, 2]
    c_of = np.repeat(np.arange(p.C), np.diff(p.cell_ptr))
    want = np.zeros((p.C, K))
    np.add.at(want, c_of, np.log(f))
    assert np.abs(ju - want).max() <= 1e-9
    d = np.zeros(p.C)
    np.add.at(d, c_of, np.log(egl[e, 4 * ge]))
    assert np.abs(lu - d).max() <= 1e-9 and np.abs(uu - d).max() <= 1e-9


# ---- unknown_summary ----------------------------------------------------------------------------------------------------

def test_unknown_summary():
    ju = np.array([[-5.0, -3.0, -3.0], [-9.0, -8.0, -7.0], [np.nan, -np.inf, -np.inf], [0.0, 0.0, 0.0]])
    t = dict(ll_ju=ju, ll_u=np.array([-4.0, -2.0, -np.inf, 0.0]), ll_uu=np.array([-6.0, -1.0, -np.inf, 0.0]))
    best = np.array([-3.5, -3.5, -np.inf, 0.0])
    s = freemuxlet.unknown_summary(t, best)
    assert s["half_clust"].tolist() == [1, 2, 0, 0] and s["half_clust"].dtype == np.int32    # ties: the lowest cluster
    assert s["half_llk"].tolist() == [-3.0, -7.0, -np.inf, 0.0]
    assert s["unk_llk"].tolist() == [-3.0, -1.0, -np.inf, 0.0]
    assert s["diff"].tolist() == [-0.5, -2.5, 0.0, 0.0] and s["n_better"] == 1
    with pytest.raises(ValueError):
        freemuxlet.unknown_summary(t, best[:3])


# ---- the cost of a cell in table_plan.hpp -------------------------------------------------------------------------------

_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "table_plan.hpp"
int main(int argc, char** argv) {
  std::printf("%zu %zu\n", sizeof(table_plan::item), sizeof(double));
  for (int i = 1; i + 1 < argc; i += 2) {
    const long long len = std::atoll(argv[i]);
    const int K = std::atoi(argv[i + 1]);
    std::printf("%zu\n", table_plan::fmx_unknown_bytes(len, table_plan::parts(len), K));
  }
  return 0;
}
"""


def test_cost_of_a_cell_is_the_literal_sum(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    open(src, "w").write(_PROBE)
    r = subprocess.run([cxx, "-x", "c++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "popscle_amd", "csrc"), src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = [(n, K) for n in (0, 1, 2047, 2048, 2049, 4096, 4097, 6145, 100000) for K in (1, 16, 64, 65, 300, 1024)]
    r = subprocess.run([exe] + [str(x) for c in cases for x in c], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "24 8"
    for (n, K), got in zip(cases, lines[1:]):
        parts = -(-n // 2048) if n > 2048 else 1
        # 40 bytes of weights an entry; per part a slab row of K + 2 doubles and its item; the rows of the three tables
        assert int(got) == 40 * n + parts * (8 * (K + 2) + 24) + 8 * K + 8 + 8, (n, K, got)
