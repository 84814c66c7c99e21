"""CPU side of freemuxlet's PRIOR anchors (muxgl_fmx_set_anchors_mode): the reference the GPU tests hold them to is sound.

tests/fmx_prior_ref.py expresses a PRIOR cluster through the unchanged oracle by substituting its pileup diagonal.  Here:
the oracle's rows of substituted diagonals equal the plain numpy rows within 4 ulp; for every trajectory of
tests/test_fmx_prior_gpu.py no decision of the oracle hangs on the bits the substitution cannot pin (the seed condition);
refine_summary and the --anchor-refine-list parsing on hand-made cases; and the new kernel's resources from the code object's
metadata."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fmx_anchor_ref as ar
import fmx_prior_ref as pr
import oracle_binding as ob
from popscle_amd import freemuxlet, synth
from test_isa import isa, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("geno_error", [0.1, 0.0])
def test_substituted_oracle_rows_equal_the_numpy_rows_to_4_ulp(geno_error, S=400, V=4, seed=11):
    """One-entry droplets at marker s see a cluster's row through full_ll (tests/fmx_anchor_ref.py): the oracle's rows of the
    substituted diagonals are ar.panel_rows(d') bit for bit -- checked here for these d' -- and those are within 4 ulp of
    prior_rows(w, d), zeros exact.  Random true diagonals between 1e-6 and 1, every kind of panel row."""
    rng = np.random.default_rng(seed)
    cell_ptr = np.arange(S + 1, dtype=np.int64)
    entry_snp = np.arange(S, dtype=np.int32)
    entry_rptr = np.arange(S + 1, dtype=np.int64)
    reads = ((rng.integers(0, 2, S) << 7) | rng.integers(13, 21, S)).astype(np.uint8)
    af = rng.uniform(0.011, 0.989, S)
    p = synth.Pileup(S, S, cell_ptr, entry_snp, entry_rptr, reads, af)
    G = rng.integers(0, 3, (S, V))
    has_gp = (rng.random(S) > 0.25).astype(np.uint8)
    panel, _ = pr.make_panel(p, G, has_gp, list(range(V)), geno_error, seed)
    true = 10.0 ** rng.uniform(-6, 0, (S, V, 3))
    sub = pr.substituted(panel, true, af, has_gp)
    assert np.isfinite(sub).all() and (sub == 0).any() and (sub[has_gp == 0] == true[has_gp == 0]).all()
    rows = ar.panel_rows(sub, af, geno_error)
    e = ob.fmx_entry_pileup(p)
    clust = np.full(S, -1, dtype=np.int32)
    cplp = ob.fmx_build_cluster_pileup(p, e, V, clust)
    cells = ob.fmx_init_cells(clust)
    for v in range(V):
        for slot, g in zip(pr.SLOTS, range(3)):
            cplp["gls"][v, :, slot] = sub[:, v, g]
    full = ob.fmx_iterate(p, e, V, cplp, cells, 0.5, geno_error, full_ll=True)[3]
    for s in range(S):
        gl = e["gls"][s]
        for j in range(V):
            lk = 0.0
            for g in range(3):
                lk += gl[4 * g] * rows[s, j, g]
            assert full[s, j * (j + 1) // 2 + j] == 0.0 + math.log(lk), (s, j)
    want = pr.prior_rows(panel, true, af, has_gp, geno_error)
    u = pr.ulps(rows, want)
    print(f"geno_error={geno_error}: oracle rows of substituted diagonals against numpy q, worst {u.max()} ulp")
    assert u.max() <= 4
    if geno_error == 0:
        assert ((rows == 0) == (want == 0)).all() and (want == 0).any()   # a zero in w is a zero in q


@pytest.mark.parametrize("case", pr.TRAJ, ids=[t[0] for t in pr.TRAJ])
def test_seed_condition(case):
    name, K, C_, S, ment, V, donors, modes, ge, holes, flags, full, pileups = case
    p, panel, d, has_gp, clust = pr.traj_inputs(*case)
    n = pr.seed_condition(p, K, pr.ITERS, donors, modes, panel, d, has_gp, clust, geno_error=ge)
    assert n == pr.ITERS * p.C


def test_seed_condition_of_the_near_tie_case():
    p, K, iters, donors, modes, panel, d, has_gp, clust = pr.near_tie_case()
    assert pr.seed_condition(p, K, iters, donors, modes, panel, d, has_gp, clust) == iters * p.C


def test_prior_rows_by_hand():
    af = np.array([0.5, 0.5])
    w = np.array([[[0.5, 0.5, 0.0]], [[9.0, 9.0, 9.0]]])
    d = np.array([[[0.2, 0.6, 1.0]], [[0.2, 0.2, 0.4]]])
    q = pr.prior_rows(w, d, af, np.array([1, 0]), 0.0)
    assert np.allclose(q[0, 0], [0.25, 0.75, 0.0], rtol=1e-15) and q[0, 0, 2] == 0.0
    assert np.allclose(q[1, 0], [0.2, 0.4, 0.4], rtol=1e-15)            # no genotypes: the free cluster's row
    q = pr.prior_rows(w, d, af, np.array([1, 0]), 0.1)
    assert np.allclose(q[0, 0], [0.9 * 0.25 + 0.025, 0.9 * 0.75 + 0.05, 0.025], rtol=1e-15)


def test_refine_summary_by_hand():
    has_gp = np.array([1, 1, 0, 1], dtype=np.uint8)
    panel = np.array([[[0.8, 0.1, 0.1], [1 / 3, 1 / 3, 1 / 3]],
                      [[0.1, 0.8, 0.1], [0.2, 0.2, 0.6]],
                      [[0.2, 0.3, 0.5], [0.2, 0.3, 0.5]],      # no genotypes: not counted
                      [[0.0, 0.5, 0.5], [0.1, 0.6, 0.3]]])
    rows = np.array([[[0.7, 0.2, 0.1], [0.1, 0.1, 0.8]],       # donor 1: flat (arg-max 0, the first) -> 2: moved
                     [[0.6, 0.3, 0.1], [0.1, 0.1, 0.8]],       # donor 0: 1 -> 0: moved
                     [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]],
                     [[0.0, 0.5, 0.5], [0.2, 0.5, 0.3]]])      # donor 0: a tie keeps the first on both sides
    r = freemuxlet.refine_summary(panel, has_gp, rows)
    assert r["n_geno"].tolist() == [3, 3] and r["n_changed"].tolist() == [1, 1]
    assert np.allclose(r["mean_max_prior"], [(0.8 + 0.8 + 0.5) / 3, (1 / 3 + 0.6 + 0.6) / 3], rtol=1e-15)
    assert np.allclose(r["mean_max_post"], [(0.7 + 0.6 + 0.5) / 3, (0.8 + 0.8 + 0.5) / 3], rtol=1e-15)
    r = freemuxlet.refine_summary(panel, np.zeros(4, dtype=np.uint8), rows)
    assert r["n_geno"].tolist() == [0, 0] and r["n_changed"].tolist() == [0, 0] and np.isnan(r["mean_max_post"]).all()
    with pytest.raises(ValueError):
        freemuxlet.refine_summary(panel, has_gp, rows[:, :1])


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"run_em touched the engine ({name}) before refusing")


def test_run_em_refuses_modes_without_anchors():
    with pytest.raises(ValueError, match="anchor_modes needs anchors"):
        freemuxlet.run_em(_NoDevice(), 4, np.zeros(8, dtype=np.int32), anchor_modes=[1])
    with pytest.raises(ValueError, match="anchor_modes needs anchors"):
        freemuxlet.run_em(_NoDevice(), 4, np.zeros(8, dtype=np.int32), anchors=[0, 1], anchor_modes=[1])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "refine_list_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "refine_list_probe.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.probe_refine_modes.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.probe_refine_modes.restype = C.c_int
    return lib


def _modes_cpp(lib, ids, listed):
    mode = np.full(max(len(ids), 1), 7, dtype=np.uint8)
    bad = C.create_string_buffer(64)
    ok = lib.probe_refine_modes(len(ids), "\n".join(ids).encode(), listed.encode(), mode.ctypes.data_as(C.c_void_p), bad, 64)
    if not ok:
        raise ValueError(bad.value.decode())
    return mode[:len(ids)].tolist()


LISTS = [(["S0", "S1", "S2"], "S2\nS0\n", [1, 0, 1]),
         (["S0", "S1", "S2"], "", [0, 0, 0]),
         (["S0", "S1", "S2"], "# donors with low-pass genotypes\n\n  S1\tlow-pass\r\nS1\n   \n", [0, 1, 0]),
         (["A", "B", "A"], "A", [1, 0, 1]),                                  # one donor in two clusters; no final newline
         ([], "\n#x\n", [])]


@pytest.mark.parametrize("ids,listed,want", LISTS)
def test_refine_list_parsing(probe, ids, listed, want):
    assert freemuxlet.refine_modes(ids, listed) == want
    assert _modes_cpp(probe, ids, listed) == want


@pytest.mark.parametrize("ids,listed,bad", [(["S0", "S1"], "S0\nS3\n", "S3"), (["S0"], "s0", "s0"), ([], "S0", "S0")])
def test_refine_list_refuses_an_unknown_id(probe, ids, listed, bad):
    with pytest.raises(ValueError, match=f"'{bad}' is not a sample"):
        freemuxlet.refine_modes(ids, listed)
    with pytest.raises(ValueError, match=f"^{bad}$"):
        _modes_cpp(probe, ids, listed)


def test_prior_kernel_uses_no_scratch_no_lds_and_no_agprs(tmp_path_factory):
    """from the code object's metadata only, in the manner of tests/test_isa_fmx_anchor.py: the third writer of the posterior
    tensor keeps its row in registers"""
    text = isa(tmp_path_factory, "fmx_anchor")
    ks = kernels(text, "fmx_prior_kernel")
    assert len(ks) == 1
    for name, (_body, meta) in ks.items():
        assert meta["private_seg_size"] == 0, f"{name}: scratch"
        assert meta.get("group_segment_fixed_size", 0) == 0, (name, meta)
        assert meta["num_agpr"] == 0 and meta["num_vgpr"] <= 64, (name, meta)
