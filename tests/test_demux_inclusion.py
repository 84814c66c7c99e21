"""CPU checks behind muxgl_demux_inclusion (demux_incl.hip): `restate`, a numpy restatement of the call's definitions
(include/muxgl.h) on a [C][V][V][A] tensor of log-likelihoods, checked against the reference's own records; the
declarations and the exported symbol; and the cut of the cells into batches (popscle_amd/csrc/incl_plan.hpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import ref_binding as rb
from parity import hypothesis_value  # noqa: F401  (its users import it from here)
from popscle_amd import build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
G3 = (0.0, 0.3, 0.7)
G1 = (0.0,)


def _logsumexp(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def restate(full_ll, alphas, doublet_prior):
    """The definitions of muxgl_demux_inclusion on full_ll[C][V][V][A] (llksAB of cmd_cram_demuxlet.cpp:733-747):
    dict of incl, tot, dbl, partner, alpha_idx, first -- and gap[C][V], the best value over H_s minus the runner-up's
    (inf with fewer than two hypotheses), which says where the three integers are decided beyond rounding."""
    full = np.asarray(full_ll, dtype=np.float64)
    Cn, V, _, A = full.shape
    al = np.asarray(alphas, dtype=np.float64)
    dp = float(doublet_prior)
    lsp = np.log((1.0 - dp) / V)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp1 = np.log(np.float64(dp) / V / np.float64(V - 1.0) / np.float64(A - 1.0))
        lp2 = np.log(np.float64(dp) / V / np.float64(V - 1.0) / np.float64(A - 1.0) * 2)
    jj, kk = np.indices((V, V))
    H = np.zeros((V, V, A), dtype=bool)
    prior = np.zeros(A)
    for n in range(1, A):
        sym = al[n] == 0.5
        H[:, :, n] = (jj != kk) & ((kk < jj) if sym else True)
        prior[n] = lp2 if sym else lp1
    ninf = -np.inf
    L = np.where(H[None], full, ninf)                    # LL(h), h in H
    T = np.where(H[None], full + prior, ninf)            # LL(h) + prior(h)
    sng = full[:, :, 0, 0] + lsp
    row = _logsumexp(T.reshape(Cn, V, V * A), axis=2)    # s is j
    col = _logsumexp(np.moveaxis(T, 2, 1).reshape(Cn, V, V * A), axis=2)  # s is k
    incl = np.logaddexp(sng, np.logaddexp(row, col))
    tot = np.logaddexp(_logsumexp(sng, axis=1), _logsumexp(T.reshape(Cn, -1), axis=1))
    dbl = np.full((Cn, V), -1e300)
    partner = np.full((Cn, V), -1, dtype=np.int32)
    alpha_idx = np.full((Cn, V), -1, dtype=np.int32)
    first = np.full((Cn, V), -1, dtype=np.int32)
    gap = np.full((Cn, V), np.inf)
    o, n_ = np.indices((V, A))
    for s in range(V):
        vals = np.concatenate([L[:, s, :, :].reshape(Cn, -1), L[:, :, s, :].reshape(Cn, -1)], axis=1)
        pos = np.concatenate([((s * V + o) * A + n_).ravel(), ((o * V + s) * A + n_).ravel()])
        order = np.argsort(pos, kind="stable")          # ties: scan position ascending
        vals, pos = vals[:, order], pos[order]
        i = np.argmax(vals, axis=1)                      # (the first of equal maxima)
        best = vals[np.arange(Cn), i]
        some = np.isfinite(best)
        if not some.any():
            continue
        p = pos[i]
        q = p // A
        j, k = q // V, q % V
        dbl[some, s] = best[some]
        alpha_idx[some, s] = (p % A)[some]
        first[some, s] = (j == s)[some]
        partner[some, s] = np.where(j == s, k, j)[some]
        if vals.shape[1] > 1:
            second = np.partition(vals, -2, axis=1)[:, -2]
            with np.errstate(invalid="ignore"):
                gap[some, s] = (best - second)[some]
    return dict(incl=incl, tot=tot, dbl=dbl, partner=partner, alpha_idx=alpha_idx, first=first, gap=gap)


def reference_run(p, alphas, doublet_prior=0.5):
    """(records, full_ll) of the reference's own demuxlet loop where it was built, else of the oracle"""
    if rb.available():
        rec, _, full = rb.RefScl.from_packed(p).demux(alphas, doublet_prior=doublet_prior, full_ll=True)
        return rec, full
    return ob.demux(p, alphas=alphas, doublet_prior=doublet_prior, full_ll=True, nthreads=4)


def _logadd(a, b):
    return rb.logadd(a, b) if rb.available() else ob.logadd(a, b)


@pytest.mark.parametrize("source", ["oracle", "reference"])
@pytest.mark.parametrize("alphas", [G2, G6, G3])
@pytest.mark.parametrize("V", [1, 2, 3, 5])
def test_restate_against_the_records(V, alphas, source):
    dp = 0.3
    p = synth.make_pileup(12, 400, V, seed=90 + V, mean_entries=60, min_entries=10, missing_gp_frac=0.05, doublet_frac=0.4)
    if source == "reference":
        if not rb.available():
            pytest.skip("reference library not built")
        rec, _, full = rb.RefScl.from_packed(p).demux(alphas, doublet_prior=dp, full_ll=True)
    else:
        rec, full = ob.demux(p, alphas=alphas, doublet_prior=dp, full_ll=True)
    r = restate(full, alphas, dp)
    valid = (rec["valid"] & 1) == 1
    assert valid.all()
    A = len(alphas)
    # every doublet is in H_j and in H_k: sum_s exp(incl_s - tot) = P(singlet) + 2 P(doublet) = 1 + P(doublet)
    sgl = _logsumexp(full[:, :, 0, 0] + np.log((1.0 - dp) / V), axis=1)
    p_dbl = 1.0 - np.exp(sgl - r["tot"])
    assert np.allclose(np.exp(r["incl"] - r["tot"][:, None]).sum(axis=1), 1.0 + p_dbl, rtol=0.0, atol=1e-12)
    # the record's sumLLK is the same sum behind the reference's seed of -1e-300 (sic, :791)
    chain = np.array([_logadd(t, -1e-300) for t in r["tot"]])
    assert np.all(np.abs(chain - rec["sumLLK"]) <= 1e-9), np.abs(chain - rec["sumLLK"]).max()
    # the best doublet over all of H
    if V > 1:
        jj, kk = np.indices((V, V))
        best = np.full(p.C, -np.inf)
        for n in range(1, A):
            m = (jj != kk) & ((kk < jj) if alphas[n] == 0.5 else True)
            best = np.maximum(best, full[:, :, :, n][:, m].max(axis=1))
        assert np.array_equal(r["dbl"].max(axis=1), best)
        assert np.all(np.abs(best - rec["dblBestLLK"]) <= 1e-9)
        c = np.arange(p.C)
        for s in range(V):
            v = hypothesis_value(full, s, r["partner"][:, s], r["alpha_idx"][:, s], r["first"][:, s])
            assert np.array_equal(v, r["dbl"][:, s])
            assert np.all(r["partner"][:, s] != s) and np.all(r["alpha_idx"][:, s] >= 1)
    else:
        assert np.all(r["dbl"] == -1e300) and np.all(r["partner"] == -1) and np.all(r["first"] == -1)
        assert np.allclose(r["incl"][:, 0], r["tot"], rtol=0, atol=1e-12)


def test_restate_singlets_only_grid_and_ties():
    p = synth.make_pileup(6, 300, 4, seed=3, mean_entries=40, min_entries=10)
    _, full = ob.demux(p, alphas=G1, full_ll=True)
    r = restate(full, G1, 0.5)
    assert np.all(r["dbl"] == -1e300) and np.all(r["partner"] == -1) and np.all(r["alpha_idx"] == -1)
    assert np.array_equal(r["incl"], full[:, :, 0, 0] + np.log(0.5 / 4))
    assert np.allclose(np.exp(r["incl"] - r["tot"][:, None]).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # a flat tensor: every hypothesis ties, the earliest scan position wins.  V = 3, alphas (0, 0.3, 0.5):
    flat = np.zeros((1, 3, 3, 3))
    r = restate(flat, (0.0, 0.3, 0.5), 0.5)
    # s = 0: earliest of H_0 is (0, 1, n = 1) at (0 * 3 + 1) * 3 + 1; s = 1: (0, 1, 1) again, as k; s = 2: (0, 2, 1) as k
    assert r["partner"].tolist() == [[1, 0, 0]] and r["alpha_idx"].tolist() == [[1, 1, 1]]
    assert r["first"].tolist() == [[1, 0, 0]] and np.all(r["gap"] == 0.0)


# ---- declarations and the symbol --------------------------------------------------------------------------------------

def test_header_declares_the_call_and_its_timing_slot():
    h = open(os.path.join(ROOT, "include", "muxgl.h")).read()
    assert re.search(r"int\s+muxgl_demux_inclusion\(muxgl_handle\*\s*h,\s*const muxgl_demux_params\*\s*p,\s*double\*\s*incl,"
                     r"\s*double\*\s*tot,\s*double\*\s*dbl,\s*int32_t\*\s*partner,\s*int32_t\*\s*alpha_idx,\s*int32_t\*\s*first\);", h)
    assert re.search(r"MUXGL_T_DEMUX_INCLUSION\s*=\s*14\b", h)
    assert re.search(r"MUXGL_T_COUNT\s*=\s*16\b", h)


def test_library_exports_the_symbol():
    if not os.path.exists(build.LIB):
        pytest.skip("libmuxgl.so is not built")
    r = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert re.search(r"\bT muxgl_demux_inclusion$", r.stdout, re.M)


# ---- the cut into batches ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "incl_plan_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "incl_plan_probe.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.probe_state_bytes.argtypes = [C.c_int]
    lib.probe_state_bytes.restype = C.c_uint64
    lib.probe_batches.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    lib.probe_batches.restype = C.c_int
    return lib


def batches(lib, cells, blocks, V, per, budget):
    b, g = C.c_int64(), C.c_int64()
    msg = C.create_string_buffer(400)
    ok = lib.probe_batches(cells, blocks, V, per, budget, C.byref(b), C.byref(g), msg, 400)
    return (b.value, g.value) if ok else msg.value.decode()


PER6 = 6 * 4096 * 8  # one (cell, block) of slab at six alphas


def test_state_bytes(plan):
    assert plan.probe_state_bytes(1) == 60 + 16 + 8
    assert plan.probe_state_bytes(64) == 64 * 60 + 16 + 8
    assert plan.probe_state_bytes(65) == 65 * 60 + 32 + 8
    assert plan.probe_state_bytes(1024) == 1024 * 60 + 16 * 16 + 8


def test_a_state_that_fits(plan):
    V, cells, blocks = 300, 1000, 25
    spc = plan.probe_state_bytes(V)
    assert batches(plan, cells, blocks, V, PER6, 8 << 30) == (1000, 25)                       # everything at once
    assert batches(plan, cells, blocks, V, PER6, cells * (spc + 25 * PER6)) == (1000, 25)     # exactly
    assert batches(plan, cells, blocks, V, PER6, cells * (spc + 25 * PER6) - 1) == (1000, 24)
    assert batches(plan, cells, blocks, V, PER6, cells * (spc + PER6)) == (1000, 1)           # one batch, a block at a time


def test_a_state_of_several_batches(plan):
    V, cells, blocks = 300, 1000, 25
    spc = plan.probe_state_bytes(V)
    assert batches(plan, cells, blocks, V, PER6, cells * (spc + PER6) - 1) == (999, 1)
    assert batches(plan, cells, blocks, V, PER6, 1 << 20) == ((1 << 20) // (spc + PER6), 1)   # the GPU tests' 1 MB: 4 cells
    assert (1 << 20) // (spc + PER6) == 4
    assert batches(plan, cells, blocks, V, PER6, spc + PER6) == (1, 1)
    # a batch of one cell can still take several blocks
    assert batches(plan, 1, 25, V, PER6, spc + 3 * PER6 + 5) == (1, 3)
    rng = np.random.default_rng(5)
    for _ in range(3000):
        cells = int(rng.integers(1, 10 ** 6))
        blocks = int(rng.integers(1, 300))
        V = int(rng.integers(1, 11586))
        per = int(rng.integers(1, 17)) * 4096 * 8
        bud = int(rng.integers(0, 1 << 34))
        spc = plan.probe_state_bytes(V)
        got = batches(plan, cells, blocks, V, per, bud)
        if bud < spc + per:
            assert isinstance(got, str)
            continue
        b, g = got
        assert 1 <= b <= cells and 1 <= g <= blocks
        assert b * spc + b * g * per <= bud                       # state and slab share the budget
        assert b == cells or (b + 1) * (spc + per) > bud          # as many cells as fit with one block each


def test_the_fuzz_shapes_fit_one_megabyte(plan):
    """tests/test_fuzz_gpu.py asks for the tables under MUXGL_DEMUX_SLAB_MB=1 in a quarter of its cases: one cell's state
    and one block of slab must fit that for every (V, A) it draws (the widest: 255 * 60 + 64 + 8 + 6 * 32 KB = 212 KB)"""
    import test_fuzz_gpu as fz

    for V in sorted(set(fz.DEMUX_V)):
        nblk = (V + 63) // 64
        for A in sorted({len(g) for g in fz.GRIDS}):
            got = batches(plan, 60, nblk * nblk, V, A * 4096 * 8, 1 << 20)
            assert isinstance(got, tuple) and got[0] >= 1 and got[1] >= 1, (V, A, got)
    assert plan.probe_state_bytes(255) + PER6 == 255 * 60 + 64 + 8 + 6 * 32768 <= (1 << 20) // 4
    assert batches(plan, 60, 16, 255, PER6, 1 << 20) == (4, 1)   # several batches, a block at a time


def test_one_cell_larger_than_the_budget_is_an_error(plan):
    V = 11585
    spc = plan.probe_state_bytes(V)
    per16 = 16 * 4096 * 8
    assert spc + per16 > 1 << 20
    msg = batches(plan, 10, 5, V, per16, 1 << 20)
    assert isinstance(msg, str) and "MUXGL_DEMUX_SLAB_MB" in msg and "V=11585" in msg and str(1 << 20) in msg
    assert isinstance(batches(plan, 10, 5, 300, PER6, plan.probe_state_bytes(300) + PER6 - 1), str)
    assert isinstance(batches(plan, 10, 5, 300, PER6, 0), str)
