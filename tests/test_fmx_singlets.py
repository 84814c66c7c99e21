"""CPU checks behind muxgl_fmx_singlets: the library exports the call and the header declares it, its timing slot, the
unchanged ABI version, and the definition the GPU tests of tests/test_fmx_singlets_gpu.py lean on -- a numpy restatement
of

    sng[c][j] = sum over the entries e of c of log(egl_e[0] q[s_e][j][0] + egl_e[4] q[s_e][j][1] + egl_e[8] q[s_e][j][2])

from the oracle's entry likelihoods and the cluster posteriors of cmd_cram_freemux2.cpp:402-415 equals the diagonal
llks[j(j+1)/2 + j] of the oracle's (and, where oracle/_ref is built, the reference's) full_ll of that iteration."""
import os
import re

import numpy as np
import pytest

import oracle_binding as ob
import ref_binding as rb
from popscle_amd import muxgl, synth
from test_demux_gpu import _with_empty_cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "muxgl.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(muxgl.LIB_PATH):
        from popscle_amd.build import build_lib

        build_lib()
    return muxgl.load_library()


def test_library_exports_and_header_declares_the_call(lib):
    assert hasattr(lib, "muxgl_fmx_singlets")
    assert "muxgl_fmx_singlets" in muxgl.SYMBOLS
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+muxgl_fmx_singlets\s*\(\s*muxgl_handle\s*\*\s*h\s*,\s*double\s*\*\s*sng\s*\)\s*;", text)
    assert lib.muxgl_fmx_singlets(None, None) != 0   # no handle: an error, not a crash


def test_timing_slot_and_version(lib):
    text = open(HEADER).read()
    slot = int(re.search(r"MUXGL_T_FMX_SINGLETS\s*=\s*(\d+)", text).group(1))
    count = int(re.search(r"MUXGL_T_COUNT\s*=\s*(\d+)", text).group(1))
    assert slot == 13 and slot < count
    assert muxgl.T_FMX_SINGLETS == slot and muxgl.T_COUNT == count
    assert int(re.search(r"#define MUXGL_VERSION (\d+)", text).group(1)) == 3
    assert lib.muxgl_version() == 3


def cluster_posteriors(af, cplp, geno_error):
    """q[S][K][3] of cmd_cram_freemux2.cpp:402-415 from the cluster pileups cplp[K][S] (oracle_binding.PLP)"""
    gl = cplp["gls"]                                   # [K][S][9]
    af = np.asarray(af, dtype=np.float64)[None, :]
    g0 = (1.0 - af) * (1.0 - af) * gl[:, :, 0]
    g1 = 2 * af * (1.0 - af) * gl[:, :, 4]
    g2 = af * af * gl[:, :, 8]
    s = g0 + g1 + g2
    q = np.stack([g0 / s, g1 / s, g2 / s], axis=-1)    # [K][S][3]
    if geno_error > 0:
        hw = np.stack([(1.0 - af) * (1.0 - af), 2 * af * (1.0 - af), af * af], axis=-1)
        q = (1 - geno_error) * q + geno_error * hw
    return np.ascontiguousarray(q.transpose(1, 0, 2))


def singlet_table(p, egl, q):
    """the formula of include/muxgl.h, entry by entry: [C][K]"""
    K = q.shape[1]
    f = (egl[:, None, 0] * q[p.entry_snp, :, 0] + egl[:, None, 4] * q[p.entry_snp, :, 1]) + egl[:, None, 8] * q[p.entry_snp, :, 2]
    lf = np.log(f)
    out = np.zeros((p.C, K))
    for c in range(p.C):
        for e in range(p.cell_ptr[c], p.cell_ptr[c + 1]):   # in entry order, as the reference accumulates (:454-455)
            out[c] += lf[e]
    return out


def diagonal(full, K):
    j = np.arange(K)
    return full[:, j * (j + 1) // 2 + j]


@pytest.mark.parametrize("K,geno_error", [(1, 0.1), (3, 0.1), (6, 0.0), (9, 0.1)])
def test_formula_is_the_diagonal_of_full_ll(K, geno_error):
    p = _with_empty_cells(synth.make_pileup(30, 400, max(K, 2), seed=77 + K, mean_entries=60, min_entries=5, with_gp=False),
                          [4, 29])
    # an empty droplet and an empty cluster among the inputs
    init = (np.arange(p.C) % K).astype(np.int32)
    if K > 2:
        init[init == K - 1] = 0
    eplp = ob.fmx_entry_pileup(p)
    cplp = ob.fmx_build_cluster_pileup(p, eplp, K, init)
    cells = ob.fmx_init_cells(init)
    worst = 0.0
    for it in range(3):
        q = cluster_posteriors(p.af, cplp, geno_error)   # before the iteration rewrites cplp
        want = singlet_table(p, eplp["gls"], q)
        *_, full = ob.fmx_iterate(p, eplp, K, cplp, cells, 0.5, geno_error, full_ll=True, nthreads=2)
        d = np.abs(want - diagonal(full, K))
        worst = max(worst, float(d.max()))
        assert d.max() <= 1e-9, (it, d.max())
    lens = np.diff(p.cell_ptr)
    assert (lens == 0).sum() == 2 and np.all(want[lens == 0] == 0.0)
    print(f"K={K}: max |formula - oracle diagonal| = {worst:.3e}")
    if rb.available():
        ref = rb.RefScl.from_packed(p).freemux2(K, geno_error=geno_error, init_clust=init, full_ll=True, cluster_pileups=True)
        cplp = ob.fmx_build_cluster_pileup(p, eplp, K, init)
        for it in range(min(3, ref["n_iter"])):
            want = singlet_table(p, eplp["gls"], cluster_posteriors(p.af, cplp, geno_error))
            d = np.abs(want - diagonal(ref["full_ll"][it], K))
            assert d.max() <= 1e-9, (it, d.max())
            cplp = ref["cplp"][it]   # the pileups the next iteration's posteriors are made of
