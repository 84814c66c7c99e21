"""CPU checks behind muxgl_pileup_read_hist and muxgl_demux_soup_mix (soup_mix.hip): the header declares the two calls and
the library exports them; the restatement of the model (tests/soup_mix_ref.py) has the properties the device is held to --
a longdouble LL trajectory that never decreases, a float64 evaluation within LL_TOL of it, the planted shares recovered
within 4 standard errors, a fitted profile closer to the true pool fraction than the count profile, a donor outside the
panel taken up by the extra component --; the numpy histogram equals its definition; the plan header
(popscle_amd/csrc/soup_mix_plan.hpp) is held against a direct loop; and the writer of the two files of --ambient-mix is run
through a small probe program and compared with the rows stated here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ambient_ref as ar
import soup_mix_ref as sr
from popscle_amd import muxgl, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---- 1. the C-ABI ----------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "muxgl.h")).read()
    assert re.search(r"\bint\s+muxgl_pileup_read_hist\s*\(\s*muxgl_handle\s*\*\s*h\s*,\s*const\s+uint8_t\s*\*\s*cell_mask", hdr)
    assert re.search(r"\bint\s+muxgl_demux_soup_mix\s*\(\s*muxgl_handle\s*\*\s*h\s*,\s*const\s+uint8_t\s*\*\s*cell_mask", hdr)
    assert len(muxgl.SYMBOLS["muxgl_pileup_read_hist"][1]) == 6 and len(muxgl.SYMBOLS["muxgl_demux_soup_mix"][1]) == 18
    lib = muxgl.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
    assert re.search(r"\bT muxgl_pileup_read_hist$", nm, flags=re.M) and re.search(r"\bT muxgl_demux_soup_mix$", nm, flags=re.M)
    n = C.c_int64(0)
    assert lib.muxgl_pileup_read_hist(None, None, None, None, 0, C.byref(n)) != 0       # no handle: an error, not a crash
    assert lib.muxgl_demux_soup_mix(None, None, 0, None, None, 0, None, None, 0, 0.0, *([None] * 8)) != 0


# ---- 2. the restatement on the planted pool ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pool():
    p, mask, truth_af, w = sr.planted_pool(**sr.POOL)
    keys, counts = sr.read_hist(p, mask)
    return dict(p=p, mask=mask, pool=truth_af, w=w, keys=keys, counts=counts,
                ld=sr.fit(keys, counts, p.gp, p.has_gp, n_iter_max=500, tol=1e-8),
                f64=sr.fit(keys, counts, p.gp, p.has_gp, n_iter_max=500, tol=1e-8, dtype=np.float64))


@pytest.fixture(scope="module")
def outside():
    p, mask, truth_af, w = sr.planted_pool(**sr.POOL_OUTSIDE)
    keys, counts = sr.read_hist(p, mask)
    return dict(p=p, mask=mask, pool=truth_af, w=w, keys=keys, counts=counts, gp0=sr.hwe_prior(p.af))


def test_pool_is_the_issues_shape(pool):
    p, mask = pool["p"], pool["mask"]
    assert p.C == 400 and p.S == 3000 and p.gp.shape[1] == 6
    nreads = np.add.reduceat(np.diff(p.entry_rptr), p.cell_ptr[:-1])
    assert np.array_equal(mask, nreads <= 40) and mask.sum() == 266      # the droplets of --ambient-max-reads 40
    assert len(set((p.reads & 0x7F).tolist())) >= 3                        # several base qualities


def test_longdouble_trajectory_never_decreases(pool):
    ll = pool["ld"]["ll"]
    ll = ll[~np.isnan(ll)]
    assert ll.size >= 3 and np.all(np.diff(ll) >= 0), float(np.diff(ll).min())
    assert abs(float(pool["ld"]["pi"].sum()) - 1.0) < 1e-12              # the step keeps the simplex, no renormalisation


def test_float64_follows_longdouble(pool):
    ld, f64 = pool["ld"], pool["f64"]
    n = min(ld["n_iter"], f64["n_iter"]) + 1
    dll = float(np.max(np.abs(f64["ll"][:n] - ld["ll"][:n])))
    dpi = float(np.max(np.abs(f64["pi"] - ld["pi"])))
    print(f"float64 against longdouble: max |dLL| {dll:.3e}, max |dpi| {dpi:.3e}")
    assert dll <= sr.LL_TOL and dpi <= 1e-6


def test_planted_shares_and_profile(pool):
    p = pool["p"]
    counts_profile = muxgl.ambient_profile(*ar.allele_counts(p, pool["mask"]), p.af)
    sr.check_planted(pool["ld"], pool["ld"]["model"], pool["w"], pool["pool"], counts_profile, "restatement")
    sm = muxgl.soup_mix_summary({k: np.asarray(pool["f64"][k], dtype=np.float64) for k in ("pi", "grad", "ll")})
    assert np.all(np.diff(sm["shares"]) <= 0) and sm["ll_gain"] > 0 and sm["order"][0] == 0


def test_outside_donor_is_taken_up(outside):
    """The donor missing from the panel, with the Hardy-Weinberg prior at the population frequency.  (With the panel mean,
    the library's default, the extra column is the mean of the panel's columns: the likelihood is flat along that direction
    and the share is not identified -- checked below.)"""
    o = outside
    p = o["p"]
    f = sr.fit(o["keys"], o["counts"], p.gp, p.has_gp, with_unknown=True, gp0=o["gp0"], n_iter_max=500, tol=1e-8)
    counts_profile = muxgl.ambient_profile(*ar.allele_counts(p, o["mask"]), p.af)
    z = sr.check_planted(f, f["model"], o["w"], o["pool"], counts_profile, "outside donor")
    assert abs(z[-1]) <= 4.0
    # without the component some donor's grad stays at 1 (a maximum of the smaller model) while the LL is lower
    g = sr.fit(o["keys"], o["counts"], p.gp, p.has_gp, n_iter_max=500, tol=1e-8)
    ll_with, ll_without = float(np.nanmax(f["ll"])), float(np.nanmax(g["ll"]))
    print(f"outside donor: LL {ll_with:.3f} with the component, {ll_without:.3f} without; grad without {np.asarray(g['grad'], float)}")
    assert np.any(np.abs(np.asarray(g["grad"], dtype=np.float64)[g["pi"] > 0] - 1.0) < 1e-6) and ll_without < ll_with - 2.0
    # the panel mean: the same LL as without the component, and an information matrix without full rank
    m = sr.fit(o["keys"], o["counts"], p.gp, p.has_gp, with_unknown=True, n_iter_max=500, tol=1e-8)
    eig = np.linalg.eigvalsh(m["model"].information(np.asarray(m["pi"], dtype=np.float64)))
    assert abs(float(np.nanmax(m["ll"])) - ll_without) < 1e-3 and abs(eig[0]) < 1e-6 * eig[-1]


def test_evaluation_mode_and_status(pool):
    p = pool["p"]
    pi0 = np.asarray(pool["ld"]["pi"], dtype=np.float64)
    e = sr.fit(pool["keys"], pool["counts"], p.gp, p.has_gp, pi0=pi0, n_iter_max=0)
    assert e["status"] == 1 and e["n_iter"] == 0 and not np.isnan(e["ll"][0])
    none = sr.fit(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), p.gp, p.has_gp, n_iter_max=3)
    assert none["status"] == 2 and none["ll"][0] == 0 and np.isnan(none["ll"][1:]).all() and not none["grad"].any()
    assert np.all(none["amb_af"] >= 0) and np.all(none["amb_af"] <= 1)


# ---- 3. the histogram ---------------------------------------------------------------------------------------------------------

def test_numpy_histogram_equals_its_definition():
    p = synth.make_pileup(40, 300, 4, seed=3, mean_entries=60, min_entries=0, other=0.2)
    p.cell_ptr[5] = p.cell_ptr[6]                                          # (an empty droplet in the middle is harmless to both)
    rng = np.random.default_rng(1)
    for mask in (None, rng.random(p.C) < 0.5, np.zeros(p.C, dtype=bool)):
        k, c = sr.read_hist(p, mask)
        k2, c2 = sr.read_hist_definition(p, mask)
        assert np.array_equal(k, k2) and np.array_equal(c, c2)
        assert np.all(np.diff(k) > 0) and np.all(c > 0) and not np.any((k & 0xFF) == 0xFF)
        n_ref, n_alt = ar.allele_counts(p, mask)
        alt = (k & 0x80) != 0
        assert np.array_equal(np.bincount(k[~alt] >> 8, weights=c[~alt], minlength=p.S).astype(np.int64), n_ref)
        assert np.array_equal(np.bincount(k[alt] >> 8, weights=c[alt], minlength=p.S).astype(np.int64), n_alt)
    assert (p.reads == synth.READ_OTHER).any()


# ---- 4. the plan header -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "soup_mix_plan_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "soup_mix_plan_probe.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.probe_soup_mix_cut.argtypes = [C.c_int, C.c_int64, vp]
    lib.probe_soup_mix_cut.restype = None
    lib.probe_soup_mix_check.argtypes = [C.c_int64, vp, vp, C.c_int64, vp]
    lib.probe_soup_mix_check.restype = C.c_int
    lib.probe_soup_mix_lists.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.probe_soup_mix_lists.restype = C.c_int64
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_plan_cut(plan):
    for M in (1, 2, 3, 6, 32, 33, 63, 64, 65, 130, 300, 11586):
        for n in (0, 1, 255, 256, 257, 1000):
            out = np.zeros(5, dtype=np.int64)
            plan.probe_soup_mix_cut(M, n, _ptr(out))
            W = 64 if M > 32 else next(w for w in (1, 2, 4, 8, 16, 32) if w >= M)
            assert out.tolist() == [256, W, 64 // W, -(-n // (64 // W)), -(-n // 256)], (M, n, out)


def test_plan_lists_against_a_direct_loop(plan):
    rng = np.random.default_rng(7)
    for trial in range(20):
        S = int(rng.integers(1, 60))
        has_gp = (rng.random(S) < 0.8).astype(np.uint8)
        full = np.arange(S * 256, dtype=np.int64)
        full = full[(full & 0xFF) != 0xFF]
        keys = np.sort(rng.choice(full, size=int(rng.integers(0, 120)), replace=False))
        counts = rng.integers(1, 9, size=keys.size).astype(np.int64)
        n = keys.size
        at = C.c_int64(-1)
        assert plan.probe_soup_mix_check(n, _ptr(keys), _ptr(counts), S, C.byref(at)) == 0
        want = [(s, [i for i in range(n) if keys[i] >> 8 == s]) for s in range(S) if has_gp[s] and np.any(keys >> 8 == s)]
        for ra in (None, rng.choice([0.0, 0.5, 2.0], size=max(len(want), 1))):
            w = want if ra is None else [x for x, r in zip(want, ra) if r > 0]
            marker, rec_ptr, rec = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 2, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
            nr = C.c_int64(-1)
            m = plan.probe_soup_mix_lists(n, _ptr(keys), _ptr(counts), _ptr(has_gp), _ptr(ra), _ptr(marker), _ptr(rec_ptr), _ptr(rec),
                                          C.byref(nr))
            assert m == len(w) and marker[:m].tolist() == [s for s, _ in w]
            assert rec[:rec_ptr[m]].tolist() == [i for _, r in w for i in r]
            assert rec_ptr[:m + 1].tolist() == np.concatenate([[0], np.cumsum([len(r) for _, r in w])]).astype(int).tolist()
            assert nr.value == sum(int(counts[i]) for _, r in w for i in r)


def test_plan_refuses_bad_histograms(plan):
    def code(keys, counts, S=10):
        k, c = np.asarray(keys, dtype=np.int64), np.asarray(counts, dtype=np.int64)
        at = C.c_int64(-1)
        return plan.probe_soup_mix_check(k.size, _ptr(k), _ptr(c), S, C.byref(at)), at.value
    assert code([5, 300, 301], [1, 2, 3]) == (0, 2)
    assert code([5, 5], [1, 1]) == (1, 1) and code([300, 5], [1, 1]) == (1, 1)          # unsorted
    assert code([5, 10 * 256], [1, 1]) == (2, 1) and code([-1], [1]) == (2, 0)          # no such marker
    assert code([5, 256 + 255], [1, 1]) == (3, 1)                                       # byte 0xFF
    assert code([5, 300], [1, 0]) == (4, 1) and code([5], [-2]) == (4, 0)               # a count <= 0


# ---- 5. the writer ------------------------------------------------------------------------------------------------------------

def test_writer_rows(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "soup_mix_writer_probe")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unused-parameter",
                        os.path.join(ROOT, "tests", "csrc", "soup_mix_writer_probe.cpp"), "-o", exe, "-lz"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    ids = ["S0", "donor-B", "S2"]
    af = [0.5, 0.1, 1.0 / 3.0, 0.0, 1.0, 0.12345678901234567]
    for unknown in (False, True):
        pi = [0.6, 0.0, 0.4 - 1e-9] + ([1e-9] if unknown else [])
        grad = [1.0, 0.25, 1.0000004] + ([0.9999996] if unknown else [])
        out = tmp_path / ("out%d" % unknown)
        out.mkdir()
        (tmp_path / "in.txt").write_text("".join(n + " " + " ".join(v if isinstance(v, str) else repr(v) for v in a) + "\n"
                                                 for n, a in (("ids", ids), ("pi", pi), ("grad", grad), ("af", af))))
        r = subprocess.run([exe, str(tmp_path / "in.txt"), str(out)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        names = ids + (["UNKNOWN"] if unknown else [])
        want = "SM_ID\tSHARE\tGRAD\n" + "".join("%s\t%.6f\t%.6f\n" % (n, s, g) for n, s, g in zip(names, pi, grad))
        assert (out / "soupmix").read_text() == want
        lines = (out / "soupmix.af").read_text().split("\n")
        assert lines[-1] == "" and [float(x) for x in lines[:-1]] == af                  # the doubles come back exactly
