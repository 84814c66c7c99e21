"""muxgl_fmx_alpha_fit without a device: the restatement (tests/fmx_alpha_fit_ref.py) against the oracle's freemuxlet E-step
(the slot of (j, k) at alpha = 0.5, bit for bit; the singlet columns at alpha = 0 and 1), against finite differences of its
own LL, the floored piece, the mirror, the search rule (65-point scan included) against the dense-scan maximiser on the fuzz
generator's pileups, the model on synthetic doublets, and the boundary (header, binding, library)."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fmx_alpha_fit_ref as far
import fmx_ambient_fit_ref as ffr
import oracle_binding as ob
from popscle_amd import freemuxlet, muxgl, synth
from test_fmx_singlets import cluster_posteriors, singlet_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_call():
    raw = open(os.path.join(ROOT, "include", "muxgl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ptr = lambda t, n: rf"\s*{t}\s*\*\s*{n}\s*"
    assert re.search(r"\bint\s+muxgl_fmx_alpha_fit\s*\(" + ptr("muxgl_handle", "h") + r",\s*int32_t\s+n_cand\s*,"
                     + ptr(r"const\s+int32_t", "pair") + r",\s*double\s+alpha_max\s*," + ptr("double", "alpha_hat") + ","
                     + ptr("double", "ll_hat") + "," + ptr("double", "ll_zero") + "," + ptr("double", "ll_top") + ","
                     + ptr("double", "info") + "," + ptr("int32_t", "status") + "," + ptr("int32_t", "n_steps") + ","
                     + ptr("float", "kernel_ms") + r"\)\s*;", text)
    doc = raw[raw.index("The mixing share alpha of a freemuxlet doublet"):raw.index("int muxgl_fmx_alpha_fit")]
    for word in ("sc_drop_seq.cpp:452-509", "cmd_cram_freemux2.cpp:394-455", "no slab budget applies", "MUXGL_FMX_SLAB_MB is not read",
                 "-inf", "65 points", "bit for bit", "exactly one negative index"):
        assert word in doc, word
    if not os.path.exists(muxgl.LIB_PATH):
        from popscle_amd.build import build_lib

        build_lib()
    lib = muxgl.load_library()
    assert len(muxgl.SYMBOLS["muxgl_fmx_alpha_fit"][1]) == 12
    nm = subprocess.run(["nm", "-D", "--defined-only", muxgl.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT muxgl_fmx_alpha_fit$", nm, flags=re.M)
    assert lib.muxgl_fmx_alpha_fit(None, 1, None, 1.0, *[None] * 8) != 0               # no handle: an error, not a crash
    assert lib.muxgl_version() == 3 and muxgl.T_COUNT == 16                             # (tests/test_abi.py pins them)
    assert "fmx_alpha_fit.hip" in open(os.path.join(ROOT, "popscle_amd", "csrc", "Makefile")).read()


def test_summary_and_call_pairs_hand_made():
    fit = {"info": np.array([[4.0, 0.0], [25.0, 0.0]]), "status": np.array([[0, 0], [1, 6]]),
           "alpha_hat": np.array([[0.25, 0.75], [0.0, 0.0]]),
           "ll_hat": np.array([[-10.0, -5.0], [-3.0, -np.inf]]), "ll_zero": np.array([[-12.0, -5.0], [-3.0, -np.inf]]),
           "ll_top": np.array([[-11.0, -9.0], [-7.0, -np.inf]]), "pair": np.array([[[0, 1], [2, 3]], [[4, 5], [6, 7]]]),
           "alpha_max": 1.0}
    sm = freemuxlet.alpha_fit_summary(fit)
    assert sm["se"][0, 0] == 0.5 and np.isnan(sm["se"]).sum() == 3
    assert np.array_equal(sm["lrt"][0], [2.0, 0.0]) and sm["lrt"][1, 0] == 0.0 and np.isnan(sm["lrt"][1, 1])   # status 6: no ratio
    assert sm["major_clust"].tolist() == [[0, 3], [4, 6]] and sm["major_clust"].dtype == np.int32
    assert freemuxlet.alpha_fit_summary(dict(fit, alpha_max=0.5))["lrt"][0].tolist() == [4.0, 0.0]            # ll_top is no singlet then
    rec = np.zeros(4, dtype=muxgl.FMX_CELL)
    rec["dBest1"], rec["dBest2"] = [3, 2, -1, 0], [4, 2, 5, 0]
    rec["sBest"], rec["sNext"] = [3, 2, 5, 0], [1, -1, 0, -1]
    got = freemuxlet.call_pairs(rec)
    assert got.dtype == np.int32 and got.shape == (4, 2, 2)
    assert got.tolist() == [[[3, 4], [3, 1]], [[2, 2], [-1, -1]], [[-1, -1], [5, 0]], [[0, 0], [-1, -1]]]
    assert freemuxlet.call_pairs(rec[:0]).shape == (0, 2, 2)


# ---- the restated LL is the reference's slot at alpha = 0.5 and the singlet columns at the ends --------------------------------

def deep_pileup(V, seed):
    """cells of a dozen entries of 1, 2, 33 and 60 reads (most of them deep), base qualities 2..93, reads of neither allele"""
    p, who, pool = ffr.shaped_pileup([12, 9, 14, 1, 11, 13], 120, V, seed, depth_p=(0.15, 0.15, 0.35, 0.35), missing_gp_frac=0.0)
    assert set(np.diff(p.entry_rptr).tolist()) == {1, 2, 33, 60} and (p.reads == synth.READ_OTHER).any()
    bq = p.reads[p.reads != synth.READ_OTHER] & 0x7F
    assert bq.min() == 2 and bq.max() == 93
    return p, who, pool


@functools.lru_cache(maxsize=None)
def oracle_case(K, seed, geno_error=0.1):
    """a deep pileup, clusters c % K, the posteriors the oracle's E-step forms of their pileups and its full_ll [C][K (K + 1) / 2]"""
    p, _who, _pool = deep_pileup(K, seed)
    init = (np.arange(p.C) % K).astype(np.int32)
    eplp = ob.fmx_entry_pileup(p)
    cplp = ob.fmx_build_cluster_pileup(p, eplp, K, init)
    q = cluster_posteriors(p.af, cplp, geno_error)          # before the iteration rewrites cplp
    sng = singlet_table(p, eplp["gls"], q)
    *_, full = ob.fmx_iterate(p, eplp, K, cplp, ob.fmx_init_cells(init), 0.5, geno_error, full_ll=True, nthreads=2)
    return p, q, sng, np.ascontiguousarray(full)


@pytest.mark.parametrize("K,seed", [(3, 7), (5, 8)])
def test_the_restatement_at_one_half_is_the_reference_slot_bit_for_bit(K, seed):
    """every pair k < j: ll_exact(0.5) (the reference's per-read divide, its summand (w * q_j) * q_k, glibc log, the entries
    one after the other) has the bytes of full_ll[c][j (j + 1) / 2 + k].  The slot k == j of the reference is the singlet
    sum over the diagonal (:448-452), not a pair: it is held under the singlet bar below, at alpha = 0 of the pair (j, j)."""
    p, q, sng, full = oracle_case(K, seed)
    n = 0
    for c in range(p.C):
        for j in range(K):
            for k in range(j):
                got = far.Cell(p, q, c, j, k).ll_exact([0.5])[0]
                want = full[c, j * (j + 1) // 2 + k]
                assert np.float64(got).tobytes() == np.float64(want).tobytes(), (c, j, k, got, want)
                n += 1
            cell = far.Cell(p, q, c, j, j)
            L, _, _, aL = [v[0] for v in cell.eval([0.0])[:4]]
            assert abs(L - full[c, j * (j + 1) // 2 + j]) <= 8 * EPS * max(cell.n, 1) * max(aL, 1.0), (c, j)
    print(f"fmx alpha fit restatement == full_ll bit for bit on {n} slots (K = {K})")


@pytest.mark.parametrize("K,seed", [(3, 7), (5, 8)])
def test_the_ends_are_the_singlet_columns(K, seed):
    """LL(0) is cluster j's singlet log-likelihood and LL(1) cluster k's, whatever the other cluster: a few ulp of the sum
    (sum_m q[m] is 1 to rounding, and the logs are added by numpy's sum here and one by one there)"""
    p, q, sng, _full = oracle_case(K, seed)
    worst = 0.0
    for c in range(p.C):
        for j in range(K):
            for k in range(K):
                cell = far.Cell(p, q, c, j, k)
                L, _, _, aL = cell.eval([0.0, 1.0])[:4]
                tol = 8 * EPS * cell.n * max(float(aL.max()), 1.0)
                assert abs(L[0] - sng[c, j]) <= tol and abs(L[1] - sng[c, k]) <= tol, (c, j, k, L, sng[c, j], sng[c, k])
                worst = max(worst, abs(L[0] - sng[c, j]), abs(L[1] - sng[c, k]))
    print(f"K={K}: worst |LL(0) - sng[j]|, |LL(1) - sng[k]| {worst:.3e}")


# ---- the analytic derivatives are the derivatives of LL away from the floor -------------------------------------------------

@pytest.mark.parametrize("K,seed", [(3, 7), (5, 8)])
def test_analytic_derivatives_equal_richardson_central_differences(K, seed):
    """DESIGN 4.1g's bar: 1e-6 relative after one Richardson step (h = 1e-4 and 2 h), in longdouble, at the points where no
    element of the droplet is within 1e-3 relative of the floor at one of the five points"""
    ld = np.longdouble
    p, q, _sng, _full = oracle_case(K, seed)
    h = ld(1e-4)
    worst, used, near = 0.0, 0, 0
    rel = lambda x, y: abs(float(x - y)) / max(abs(float(x)), 1e-300)
    for c in range(p.C):
        for j in range(K):
            for k in range(K):
                if j == k:
                    continue
                cell = far.Cell(p, q, c, j, k)
                for x in (0.05, 0.4, 0.9):
                    pts = [ld(x) - 2 * h, ld(x) - h, ld(x), ld(x) + h, ld(x) + 2 * h]
                    out = cell.eval(pts, ld)
                    if out[8].min() < 1e-3:
                        near += 1
                        continue
                    Lm2, Lm, L, Lp, Lp2 = out[0]
                    d1, d2 = out[1][2], out[2][2]
                    c1, c1w = (Lp - Lm) / (2 * h), (Lp2 - Lm2) / (4 * h)
                    c2, c2w = (Lp - 2 * L + Lm) / (h * h), (Lp2 - 2 * L + Lm2) / (4 * h * h)
                    fd1, fd2 = (4 * c1 - c1w) / 3, (4 * c2 - c2w) / 3
                    e1, e2 = rel(d1, fd1), rel(d2, fd2)
                    worst, used = max(worst, e1, e2), used + 1
                    assert e1 <= 1e-6 and e2 <= 1e-6, (c, j, k, x, float(d1), float(fd1), float(d2), float(fd2))
    print(f"analytic vs Richardson central differences: worst relative {worst:.3e} over {used} points ({near} near the floor)")
    assert used >= 30 and used >= 5 * near


def test_a_floored_element_contributes_the_floor_and_no_slope():
    """one entry of 8 ALT reads at base quality 40, cluster j REF/REF and cluster k ALT/ALT: only element (0, 2) counts,
    p = alpha, so a is about alpha^8: below the floor up to alpha = 0.18; the element is 1e-6 / T there with derivative 0,
    and LL' jumps UPWARD where it leaves the floor"""
    ld = np.longdouble
    reads = np.full(8, (1 << 7) | 40, dtype=np.uint8)
    p = synth.Pileup(1, 1, np.array([0, 1], np.int64), np.zeros(1, np.int32), np.array([0, 8], np.int64), reads,
                     np.array([0.3]), None, None)
    q = np.array([[[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])
    cell = far.Cell(p, q, 0, 0, 1)
    xs = np.linspace(0.0, 1.0, 2001)
    L, d1, d2 = cell.eval(xs, ld)[:3]
    _, T = cell.nine_sums(ld)
    low = np.flatnonzero(np.isclose(L.astype(np.float64), float(np.log(ld(1e-6) / T[0])), rtol=0, atol=1e-15))
    assert low.size > 10 and low[0] == 0 and (np.diff(low) == 1).all() and low[-1] < 2000   # floored on [0, x*), not beyond
    assert (d1[low] == 0).all() and (d2[low] == 0).all()
    k = low[-1] + 1
    assert d1[k] > 0 and (np.diff(L.astype(np.float64)) >= 0).all()  # continuous and rising: the jump of LL' is upward
    assert cell.crosses([0.0, 0.5, 1.0]) and not cell.crosses([0.5, 0.5, 0.5])
    r = far.search(cell, 1.0)
    assert r["status"] == 2 and r["alpha_hat"] == 1.0 and r["n_steps"] == 0     # LL rises to the upper bound
    top = float(xs[k]) * 1.05                                                    # the crossing lies inside this bound's bracket
    r = far.search(cell, top)
    assert r["scanned"] and r["status"] == 2 and r["alpha_hat"] == top, r


def test_mirror():
    """(j, k) at alpha is (k, j) at 1 - alpha: LL, -LL' and LL'' to 1e-12 x the sum of absolute terms"""
    ld = np.longdouble
    K = 4
    p, q, _sng, _full = oracle_case(K, 5)
    worst = 0.0
    for c in range(p.C):
        for j in range(K):
            for k in range(K):
                a, b = far.Cell(p, q, c, j, k), far.Cell(p, q, c, k, j)
                for x in (0.0, 0.05, 0.4, 0.9, 1.0):
                    L, d1, d2, aL, a1, a2, s1, s2 = a.eval([ld(x)], ld)[:8]
                    M, e1, e2 = b.eval([ld(1.0) - ld(x)], ld)[:3]
                    for u, v, s in ((L, M, aL), (d1, -e1, s1), (d2, e2, s2)):
                        assert abs(float(u[0] - v[0])) <= 1e-12 * float(s[0]) + 1e-300, (c, j, k, x, u, v, s)
                        worst = max(worst, abs(float(u[0] - v[0])) / max(float(s[0]), 1e-300))
    print(f"mirror: worst |difference| / sum |terms| {worst:.3e}")


# ---- the search rule against the dense-scan maximiser on the fuzz generator's pileups ------------------------------------------

@pytest.mark.parametrize("seed", [0, 2, 5, 11])
def test_the_search_rule_finds_the_dense_scan_maximum_on_the_fuzz_pileups(seed):
    """the search as the kernel runs it (far.search, float64) ends where the Newton-free maximiser (dense scan and bisection in
    longdouble) ends: the restated LL at its estimate is not below the maximiser's by more than 1e-9.  Twelve drawn (droplet,
    pair) per seed, the pairs drawn over all clusters (j == k among them), alpha_max drawn"""
    import test_fuzz_gpu as tf

    info, p = tf.fmx_case(seed)
    K, ge = info["K"], info["ge"]
    clust0 = info["init"] if info["init"] is not None else (np.arange(p.C) % K).astype(np.int32)
    eplp = ob.fmx_entry_pileup(p)
    q = cluster_posteriors(p.af, np.ascontiguousarray(ob.fmx_build_cluster_pileup(p, eplp, K, np.ascontiguousarray(clust0, np.int32))), ge)
    r = np.random.default_rng([seed, 131])
    alpha_max = float(r.choice([1.0, 1.0, 0.8, 0.5, float(r.uniform(0.05, 1.0))]))
    scanned = multi = fitted = 0
    for _ in range(12):
        c, j, k = int(r.integers(p.C)), int(r.integers(K)), int(r.integers(K))
        cell = far.Cell(p, q, c, j, k)
        if cell.n == 0:
            continue
        s = far.search(cell, alpha_max)
        if s["status"] == 6:
            continue
        w = far.fit(p, q, c, j, k, alpha_max)
        fitted += 1
        scanned += s["scanned"]
        lo, hi, _ = far.bracket(cell, alpha_max)
        multi += far.sign_changes(cell, lo, hi) > 1
        L = float(cell.eval([s["alpha_hat"]], np.longdouble)[0][0])
        assert s["status"] in (0, 1, 2) and s["n_steps"] <= 48, (c, j, k, s)
        assert L >= w["ll_hat"] - 1e-9, (c, j, k, s, w["alpha_hat"], w["ll_hat"], L)
        if w["info"] >= 1.0:
            assert abs(s["alpha_hat"] - w["alpha_hat"]) <= 1e-6 and s["status"] == w["status"], (c, j, k, s, w)
    print(f"fuzz seed {seed}: K={K} alpha_max={alpha_max:.4f}: {fitted} pairs, the 65-point scan ran on {scanned}, "
          f"{multi} brackets with more than one sign change of LL'")
    assert fitted >= 6


# ---- the model does what it is for -------------------------------------------------------------------------------------

def check_mixed(alpha_hat, info, status, ll_hat, ll_zero, ll_top, shares):
    """the sanity check on the MIXED pileup (24 droplets, shares cycling 0.15 / 0.3 / 0.5), shared with the GPU test: every fit
    is interior with positive information, the mix beats the better singlet by more than 10 in the likelihood ratio, and at
    least nine in ten estimates lie within 4 standard errors of the truth"""
    assert (status == 0).all() and (info > 0).all(), status
    se = info ** -0.5
    lrt = 2.0 * (ll_hat - np.maximum(ll_zero, ll_top))
    inside = int((np.abs(alpha_hat - shares) <= 4.0 * se).sum())
    print(f"mixed: {int((status == 0).sum())} of {len(shares)} interior, {inside} within 4 standard errors of the truth; "
          f"(share, alpha_hat, se) {[(float(s), round(float(a), 4), round(float(e), 4)) for s, a, e in zip(shares, alpha_hat, se)]}")
    assert (lrt > 10.0).all(), lrt
    assert inside >= 0.9 * len(shares), inside
    return inside


def check_clean(status, ll_hat, ll_zero):
    """the same pileup with all shares 0: more than half of the droplets on the lower bound, and no likelihood ratio against
    the first cluster alone above 10"""
    at0 = int((status == 1).sum())
    lrt = 2.0 * (ll_hat - ll_zero)
    print(f"clean: {at0} of {len(status)} droplets on the lower bound, largest LRT against the first cluster alone {lrt.max():.2f}")
    assert at0 > len(status) / 2 and lrt.max() <= 10.0
    return at0


def test_the_fit_finds_the_mixing_share_with_an_honest_error_bar():
    p, first, second = far.doublet_pileup(**far.MIXED)
    fits = [far.fit(p, p.gp, c, int(first[c]), int(second[c]), 1.0) for c in range(p.C)]
    get = lambda n: np.array([r[n] for r in fits])
    check_mixed(get("alpha_hat"), get("info"), get("status"), get("ll_hat"), get("ll_zero"), get("ll_top"),
                np.array(far.MIXED["shares"]))


def test_clean_singlets_sit_on_the_lower_bound():
    p, first, second = far.doublet_pileup(**far.CLEAN)
    fits = [far.fit(p, p.gp, c, int(first[c]), int(second[c]), 1.0) for c in range(p.C)]
    get = lambda n: np.array([r[n] for r in fits])
    check_clean(get("status"), get("ll_hat"), get("ll_zero"))


# ---- argument checks that need no device -------------------------------------------------------------------------------------

def test_no_handle_and_the_python_argument_checks():
    lib = muxgl.load_library()
    out = np.zeros((2, 1))
    VP = ctypes.c_void_p
    assert lib.muxgl_fmx_alpha_fit(None, 1, np.zeros((2, 1, 2), np.int32).ctypes.data_as(VP), 1.0, out.ctypes.data_as(VP),
                                   *[None] * 7) != 0
    with pytest.raises(ValueError, match="unknown fields"):
        muxgl.Engine.fmx_alpha_fit(muxgl.Engine, np.zeros((2, 1, 2), np.int32), want=("alpha_hat", "se"))
