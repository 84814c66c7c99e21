"""CPU checks behind muxgl_fmx_inclusion (fmx_incl.hip): `restate_fmx`, a numpy restatement of the call's definitions
(include/muxgl.h) on a [C][K(K+1)/2] table of log-likelihoods, checked against the reference's own records; the
declarations and the exported symbol; and the bytes and the cut of the batches (popscle_amd/csrc/incl_plan.hpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import ref_binding as rb
from popscle_amd import build, muxgl, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SLAB_BLOCK = 64 * 64 * 8           # one (cell, block) of the sweep's slab
SLAB1_KS = (65, 130, 300)          # the K the GPU tests run under MUXGL_FMX_SLAB_MB=1 (tests/test_fmx_inclusion_gpu.py)


def _logsumexp(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def restate_fmx(full_ll, K, doublet_prior):
    """The definitions of muxgl_fmx_inclusion on full_ll[C][K(K+1)/2] (llks of cmd_cram_freemux2.cpp:383-456): dict of
    incl, tot, dbl, partner -- and gap[C][K], the best value over H_s minus the runner-up's (inf with fewer than two
    hypotheses), which says where `partner` is decided beyond rounding."""
    full = np.asarray(full_ll, dtype=np.float64)
    Cn = full.shape[0]
    assert full.shape == (Cn, K * (K + 1) // 2)
    dp = float(doublet_prior)
    lsp = np.log((1.0 - dp) / K)                                   # :379
    with np.errstate(divide="ignore", invalid="ignore"):
        ldp = np.log(np.float64(dp) / K / np.float64(K - 1) * 2.0)  # :380 (K = 1: no doublet reads it)
    d = np.arange(K)
    sng = full[:, d * (d + 1) // 2 + d]
    hi, lo = np.tril_indices(K, -1)
    pos = hi * (hi + 1) // 2 + lo
    L = np.full((Cn, K, K), -np.inf)                                # LL(h) seen from either member; the diagonal: none
    L[:, hi, lo] = full[:, pos]
    L[:, lo, hi] = full[:, pos]
    P = np.full((K, K), np.iinfo(np.int64).max)
    P[hi, lo] = pos
    P[lo, hi] = pos
    with np.errstate(invalid="ignore"):
        incl = np.logaddexp(sng + lsp, _logsumexp(L + ldp, axis=2)) if K > 1 else sng + lsp
        tot = _logsumexp(sng + lsp, axis=1)
        if K > 1:
            tot = np.logaddexp(tot, _logsumexp(full[:, pos] + ldp, axis=1))
    dbl = np.full((Cn, K), -1e300)
    partner = np.full((Cn, K), -1, dtype=np.int32)
    gap = np.full((Cn, K), np.inf)
    c = np.arange(Cn)
    for s in range(K if K > 1 else 0):
        order = np.argsort(P[s], kind="stable")[: K - 1]            # ties: position ascending (the diagonal sorts last)
        vals = L[:, s, order]
        i = np.argmax(vals, axis=1)                                 # (the first of equal maxima)
        best = vals[c, i]
        some = np.isfinite(best)
        dbl[some, s] = best[some]
        partner[some, s] = order[i][some]
        if K > 2:
            second = np.partition(vals, -2, axis=1)[:, -2]
            with np.errstate(invalid="ignore"):
                gap[some, s] = (best - second)[some]
    return dict(incl=incl, tot=tot, dbl=dbl, partner=partner, gap=gap)


def reference_run(p, K, init, geno_error=0.1, doublet_prior=0.5):
    """the reference's EM from `init` (its own loop where oracle/_ref is built, else the oracle): per iteration full_ll,
    the records and the counters"""
    if rb.available():
        r = rb.RefScl.from_packed(p).freemux2(K, doublet_prior, geno_error, init_clust=init, full_ll=True)
        n = r["n_iter"]
        return dict(n_iter=n, full=r["full_ll"][:n], cells=r["cells"][:n], counters=r["counters"][:n])
    e = ob.fmx_entry_pileup(p)
    cplp = ob.fmx_build_cluster_pileup(p, e, K, init)
    cells = ob.fmx_init_cells(init)
    fulls, recs, cnt = [], [], []
    for _ in range(10):
        ns, na, nch, full = ob.fmx_iterate(p, e, K, cplp, cells, doublet_prior, geno_error, full_ll=True, nthreads=8)
        fulls.append(full.copy())
        recs.append(cells.copy())
        cnt.append((ns, na, nch))
        if nch == 0:
            break
    return dict(n_iter=len(fulls), full=np.stack(fulls), cells=np.stack(recs), counters=np.array(cnt))


@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_restate_against_the_records(K):
    dp = 0.3
    p = synth.make_pileup(16, 400, max(K, 2), seed=190 + K, mean_entries=60, min_entries=10, doublet_frac=0.4, with_gp=False)
    init = (np.arange(p.C) % K).astype(np.int32)
    ref = reference_run(p, K, init, 0.1, dp)
    for it in range(ref["n_iter"]):
        full, rec = ref["full"][it], ref["cells"][it]
        r = restate_fmx(full, K, dp)
        assert not np.isnan(r["incl"]).any() and not np.isnan(r["tot"]).any()
        # the record's sumLLK is the same sum behind a seed of -1e300, which adds nothing
        assert np.all(np.abs(r["tot"] - rec["sumLLK"]) <= 1e-9), np.abs(r["tot"] - rec["sumLLK"]).max()
        # every doublet is in H_j and in H_k: sum_s exp(incl_s - tot) = P(singlet) + 2 P(doublet) = 1 + P(doublet)
        d = np.arange(K)
        sgl = _logsumexp(full[:, d * (d + 1) // 2 + d] + np.log((1.0 - dp) / K), axis=1)
        p_dbl = 1.0 - np.exp(sgl - r["tot"])
        assert np.allclose(np.exp(r["incl"] - r["tot"][:, None]).sum(axis=1), 1.0 + p_dbl, rtol=0.0, atol=1e-12)
        if K == 1:
            assert np.all(r["dbl"] == -1e300) and np.all(r["partner"] == -1)
            assert np.array_equal(r["incl"][:, 0], r["tot"])
            continue
        hi, lo = np.tril_indices(K, -1)
        best = full[:, hi * (hi + 1) // 2 + lo].max(axis=1)
        assert np.array_equal(r["dbl"].max(axis=1), best)
        assert np.all(np.abs(best - rec["dblBestLLK"]) <= 1e-9)
        s = np.argmax(r["dbl"], axis=1)
        pr = r["partner"][np.arange(p.C), s]
        decided = rec["dblBestLLK"] != rec["dblNextLLK"]
        assert decided.any()
        assert np.array_equal(np.maximum(s, pr)[decided], rec["dBest1"][decided])
        assert np.array_equal(np.minimum(s, pr)[decided], rec["dBest2"][decided])
        assert np.all(r["partner"] != np.arange(K)[None, :]) and np.all(r["partner"] >= 0)
        # the named hypothesis carries the value
        for s in range(K):
            h, l = np.maximum(s, r["partner"][:, s]), np.minimum(s, r["partner"][:, s])
            assert np.array_equal(full[np.arange(p.C), h * (h + 1) // 2 + l], r["dbl"][:, s])


def test_restate_ties_and_missing_clusters():
    # a flat table: every hypothesis ties, the earliest position wins: (1, 0) for clusters 0 and 1, (s, 0) for the others
    for K in (2, 3, 7):
        r = restate_fmx(np.zeros((2, K * (K + 1) // 2)), K, 0.5)
        assert np.all(r["partner"][:, 0] == 1) and np.all(r["partner"][:, 1:] == 0)
        assert np.all(r["dbl"] == 0.0) and np.allclose(r["tot"], 0.0, rtol=0, atol=1e-12)
        if K > 2:
            assert np.all(r["gap"] == 0.0)
    # a cluster whose every hypothesis is -inf (its posterior rows were never filled): -inf / -1e300 / -1, no NaN
    K, dead = 4, 2
    rng = np.random.default_rng(3)
    full = -rng.uniform(10, 60, size=(5, K * (K + 1) // 2))
    for j in range(K):
        for k in range(j + 1):
            if dead in (j, k):
                full[:, j * (j + 1) // 2 + k] = -np.inf
    r = restate_fmx(full, K, 0.5)
    for name in ("incl", "tot", "dbl"):
        assert not np.isnan(r[name]).any(), name
    assert np.all(r["incl"][:, dead] == -np.inf) and np.all(r["dbl"][:, dead] == -1e300) and np.all(r["partner"][:, dead] == -1)
    live = [s for s in range(K) if s != dead]
    assert np.all(np.isfinite(r["incl"][:, live])) and np.all(r["partner"][:, live] != dead) and np.all(np.isfinite(r["tot"]))
    # all of it -inf: every sum is -inf, never NaN
    r = restate_fmx(np.full((1, 6), -np.inf), 3, 0.5)
    assert np.all(r["incl"] == -np.inf) and np.all(r["tot"] == -np.inf) and np.all(r["partner"] == -1)


# ---- declarations and the symbol --------------------------------------------------------------------------------------

def test_header_declares_the_call_and_its_timing_slot():
    h = open(os.path.join(ROOT, "include", "muxgl.h")).read()
    assert re.search(r"int\s+muxgl_fmx_inclusion\(muxgl_handle\*\s*h,\s*const muxgl_fmx_params\*\s*p,\s*double\*\s*incl,"
                     r"\s*double\*\s*tot,\s*double\*\s*dbl,\s*int32_t\*\s*partner\);", h)
    assert re.search(r"MUXGL_T_FMX_INCLUSION\s*=\s*15\b", h)
    assert re.search(r"MUXGL_T_COUNT\s*=\s*16\b", h)
    assert muxgl.T_FMX_INCLUSION == 15 and muxgl.T_COUNT == 16
    assert "muxgl_fmx_inclusion" in muxgl.SYMBOLS


def test_library_exports_the_symbol_and_refuses_a_null_handle():
    if not os.path.exists(build.LIB):
        pytest.skip("libmuxgl.so is not built")
    r = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert re.search(r"\bT muxgl_fmx_inclusion$", r.stdout, re.M)
    lib = muxgl.load_library()
    assert lib.muxgl_fmx_inclusion(None, None, None, None, None, None) != 0


# ---- the bytes of a cell and the cut into batches ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "fmx_incl_plan_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "fmx_incl_plan_probe.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.probe_fmx_state_bytes.argtypes = [C.c_int]
    lib.probe_fmx_state_bytes.restype = C.c_uint64
    lib.probe_fmx_batches.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    lib.probe_fmx_batches.restype = C.c_int
    return lib


def batches(lib, cells, blocks, K, per, budget):
    b, g = C.c_int64(), C.c_int64()
    msg = C.create_string_buffer(400)
    ok = lib.probe_fmx_batches(cells, blocks, K, per, budget, C.byref(b), C.byref(g), msg, 400)
    return (b.value, g.value) if ok else msg.value.decode()


def tri_blocks(K):
    n = (K + 63) // 64
    return n * (n + 1) // 2


def test_state_bytes(plan):
    # 32 B of state and 8 + 8 + 4 B of outputs per cluster, 16 B per row block, 8 B per cell
    assert plan.probe_fmx_state_bytes(1) == 52 + 16 + 8
    assert plan.probe_fmx_state_bytes(64) == 64 * 52 + 16 + 8
    assert plan.probe_fmx_state_bytes(65) == 65 * 52 + 32 + 8
    assert plan.probe_fmx_state_bytes(1024) == 1024 * 52 + 16 * 16 + 8


def test_budget_identities(plan):
    K, cells = 300, 1000
    blocks = tri_blocks(K)
    assert blocks == 15
    spc = plan.probe_fmx_state_bytes(K)
    per = SLAB_BLOCK
    assert batches(plan, cells, blocks, K, per, 8 << 30) == (1000, 15)                          # everything at once
    assert batches(plan, cells, blocks, K, per, cells * (spc + 15 * per)) == (1000, 15)         # exactly
    assert batches(plan, cells, blocks, K, per, cells * (spc + 15 * per) - 1) == (1000, 14)
    assert batches(plan, cells, blocks, K, per, cells * (spc + per)) == (1000, 1)               # a block at a time
    assert batches(plan, cells, blocks, K, per, cells * (spc + per) - 1) == (999, 1)            # several batches
    assert batches(plan, cells, blocks, K, per, spc + per) == (1, 1)
    assert batches(plan, 1, blocks, K, per, spc + 3 * per + 5) == (1, 3)
    rng = np.random.default_rng(7)
    for _ in range(3000):
        cells = int(rng.integers(1, 10 ** 6))
        K = int(rng.integers(1, 1025))
        blocks = tri_blocks(K)
        bud = int(rng.integers(0, 1 << 34))
        spc = plan.probe_fmx_state_bytes(K)
        got = batches(plan, cells, blocks, K, per, bud)
        if bud < spc + per:
            assert isinstance(got, str)
            continue
        b, g = got
        assert 1 <= b <= cells and 1 <= g <= blocks
        assert b * spc + b * g * per <= bud                       # state and slab share the budget
        assert b == cells or (b + 1) * (spc + per) > bud          # as many cells as fit with one block each


def test_one_megabyte_holds_a_cell_and_a_block_at_every_k(plan):
    """the GPU tests run K = SLAB1_KS under MUXGL_FMX_SLAB_MB=1, in several batches; and so does every K up to the
    largest the call takes (53 512 B of state + 32 768 B of slab at K = 1024)"""
    for K in tuple(SLAB1_KS) + (1, 64, 1024):
        got = batches(plan, 64, tri_blocks(K), K, SLAB_BLOCK, 1 << 20)
        assert isinstance(got, tuple) and got[0] >= 1 and got[1] >= 1, (K, got)
    assert plan.probe_fmx_state_bytes(1024) + SLAB_BLOCK == 53512 + 32768
    assert batches(plan, 64, tri_blocks(300), 300, SLAB_BLOCK, 1 << 20) == ((1 << 20) // (300 * 52 + 80 + 8 + 32768), 1)
    assert (1 << 20) // (300 * 52 + 80 + 8 + 32768) == 21        # 64 cells: four batches, a block at a time


def test_one_cell_larger_than_the_budget_is_an_error(plan):
    K = 1024
    spc = plan.probe_fmx_state_bytes(K)
    msg = batches(plan, 10, tri_blocks(K), K, SLAB_BLOCK, 1 << 16)
    assert spc + SLAB_BLOCK > 1 << 16
    assert isinstance(msg, str) and "MUXGL_FMX_SLAB_MB" in msg and "K=1024" in msg and str(1 << 16) in msg
    assert msg.startswith("muxgl_fmx_inclusion:")
    assert isinstance(batches(plan, 10, 15, 300, SLAB_BLOCK, plan.probe_fmx_state_bytes(300) + SLAB_BLOCK - 1), str)
    assert isinstance(batches(plan, 10, 15, 300, SLAB_BLOCK, 0), str)
