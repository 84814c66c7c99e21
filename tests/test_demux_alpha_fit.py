"""muxgl_demux_alpha_fit without a device: the boundary (header, binding, library), the restatement
(tests/alpha_fit_ref.py) against the reference's own llksAB at every alpha of a grid, its analytic derivatives against
finite differences, its mirror symmetry, the helpers, and the model on the two sanity pileups."""
import os
import re
import subprocess

import numpy as np
import pytest

import alpha_fit_ref as alr
import unknown_ref as ur
from popscle_amd import demuxlet, muxgl, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G2 = (0.0, 0.5)
G6 = (0.0, 0.13, 0.37, 0.5, 0.71, 1.0)


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_call():
    raw = open(os.path.join(ROOT, "include", "muxgl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ptr = lambda t, n: rf"\s*{t}\s*\*\s*{n}\s*"
    assert re.search(r"\bint\s+muxgl_demux_alpha_fit\s*\(" + ptr("muxgl_handle", "h") + "," + ptr(r"const\s+muxgl_demux_params", "p")
                     + r",\s*int32_t\s+n_cand\s*," + ptr(r"const\s+int32_t", "pair") + r",\s*double\s+alpha_max\s*,"
                     + ptr("double", "alpha_hat") + "," + ptr("double", "ll_hat") + "," + ptr("double", "ll_zero") + ","
                     + ptr("double", "ll_top") + "," + ptr("double", "info") + "," + ptr("int32_t", "status") + ","
                     + ptr("int32_t", "n_steps") + "," + ptr("float", "kernel_ms") + r"\)\s*;", text)
    doc = raw[raw.index("The mixing share of a doublet"):raw.index("int muxgl_demux_alpha_fit")]
    assert "NO standard error" in doc and "no slab budget applies" in doc and "cmd_cram_demuxlet.cpp:655-746" in doc
    assert "exactly one negative index" in doc and "llksAB[j][k][n]" in doc
    if not os.path.exists(muxgl.LIB_PATH):
        from popscle_amd.build import build_lib

        build_lib()
    lib = muxgl.load_library()
    # (thirteen: the signature of the header -- handle, params, n_cand, pair, alpha_max, seven outputs, kernel_ms)
    assert len(muxgl.SYMBOLS["muxgl_demux_alpha_fit"][1]) == 13
    assert muxgl.Engine.ALPHA_FIT_FIELDS == ("alpha_hat", "ll_hat", "ll_zero", "ll_top", "info", "status", "n_steps")
    nm = subprocess.run(["nm", "-D", "--defined-only", muxgl.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT muxgl_demux_alpha_fit$", nm, flags=re.M)
    assert lib.muxgl_demux_alpha_fit(None, None, 1, None, 1.0, *[None] * 8) != 0   # no handle: an error, not a crash
    assert lib.muxgl_version() == 3 and muxgl.T_COUNT == 16                          # (tests/test_abi.py pins them)


def test_alpha_fit_summary_hand_made():
    fit = {"info": np.array([[4.0, 0.0], [25.0, -1.0], [100.0, 16.0]]), "status": np.array([[0, 0], [1, 0], [2, 3]]),
           "alpha_hat": np.array([[0.25, 0.5], [0.0, 0.75], [1.0, 0.5000001]]),
           "ll_hat": np.array([[-10.0, -5.0], [-3.0, -2.0], [-1.0, 0.0]]),
           "ll_zero": np.array([[-12.0, -5.0], [-3.0, -2.5], [-4.0, 0.0]]),
           "ll_top": np.array([[-11.0, -9.0], [-7.0, -2.25], [-1.0, 0.0]]),
           "pair": np.array([[[0, 1], [2, 3]], [[4, 5], [6, 7]], [[8, 9], [-1, -1]]]), "alpha_max": 1.0}
    sm = muxgl.alpha_fit_summary(fit)
    assert sm["se"][0, 0] == 0.5 and np.isnan(sm["se"]).sum() == 5
    assert np.array_equal(sm["lrt"], [[2.0, 0.0], [0.0, 0.5], [0.0, 0.0]])        # against the BETTER singlet
    assert sm["major"].tolist() == [[0, 2], [4, 7], [9, -1]] and sm["major"].dtype == np.int32
    sm = muxgl.alpha_fit_summary(dict(fit, alpha_max=0.5))                         # ll_top is no singlet then
    assert np.array_equal(sm["lrt"], [[4.0, 0.0], [0.0, 1.0], [6.0, 0.0]])


def test_call_pairs_hand_made():
    rec = np.zeros(5, dtype=muxgl.DEMUX_CELL)
    rec["valid"] = [1, 1, 1, 0, 1]
    rec["dBest1"], rec["dBest2"] = [3, 2, -1, 1, 0], [4, 2, 5, 2, 0]
    rec["sBest"], rec["sNext"] = [3, 2, 5, 1, 0], [1, -1, 0, 2, -1]
    got = demuxlet.call_pairs(rec)
    assert got.dtype == np.int32 and got.shape == (5, 2, 2)
    assert got.tolist() == [[[3, 4], [3, 1]], [[2, 2], [-1, -1]], [[-1, -1], [5, 0]], [[-1, -1], [-1, -1]],
                            [[0, 0], [-1, -1]]]
    assert demuxlet.call_pairs(rec[:0]).shape == (0, 2, 2)


# ---- the restatement is the reference at every alpha of the grid ---------------------------------------------------------

def deep_pileup(V, seed):
    """cells of a dozen entries, most of them of 33 or 60 reads, base qualities 2..93, reads of neither allele, markers
    without genotypes"""
    p, _, _ = alr.shaped_pileup([12, 9, 14, 1, 11, 13], 120, V, seed, depth_p=(0.1, 0.1, 0.4, 0.4), missing_gp_frac=0.05)
    assert np.diff(p.entry_rptr).max() == 60 and np.diff(p.entry_rptr).min() <= 33 and (p.reads == synth.READ_OTHER).any()
    return p


@pytest.mark.parametrize("V,seed", [(3, 1), (5, 2)])
@pytest.mark.parametrize("alphas", [G2, G6])
def test_the_restatement_equals_the_reference_bit_for_bit_on_the_grid(V, seed, alphas):
    p = deep_pileup(V, seed)
    full = ur.full_ll(p, alphas)                                                   # [C][V][V][A], the reference's llksAB
    n = 0
    for c in range(p.C):
        for j in range(V):
            for k in range(V):
                got = alr.Cell(p, alphas, c, j, k).ll_exact(alphas)
                assert got.tobytes() == np.ascontiguousarray(full[c, j, k]).tobytes(), (c, j, k, got, full[c, j, k])
                n += len(alphas)
    print(f"alpha fit restatement == llksAB bit for bit on {n} slots (V = {V}, {len(alphas)} alphas)")


# ---- the analytic derivatives are the derivatives of LL -----------------------------------------------------------------

@pytest.mark.parametrize("V,alphas,seed", [(3, G2, 1), (5, G6, 2)])
def test_analytic_derivatives_equal_central_differences(V, alphas, seed):
    """The bar and the reasoning of tests/test_demux_ambient_fit.py: plain central differences at h = 1e-4 carry
    h^2 LL''' / 6, above 1e-6 relative on 60-read entries however right the analytic value is, so the h^2 term is
    removed by one Richardson step with the differences at 2 h (what is left is O(h^4)), and 1e-6 relative is held on that."""
    ld = np.longdouble
    p = deep_pileup(V, seed)
    h = ld(1e-4)
    worst = plain = 0.0
    rel = lambda x, y: abs(float(x - y)) / max(abs(float(x)), 1e-300)
    for c in range(p.C):
        for j in range(V):
            for k in range(V):
                cell = alr.Cell(p, alphas, c, j, k)
                for x in (0.05, 0.4, 0.9):
                    L, d1, d2 = [v[0] for v in cell.eval([x], ld)[:3]]
                    Lm2, Lm, Lp, Lp2 = cell.eval([ld(x) - 2 * h, ld(x) - h, ld(x) + h, ld(x) + 2 * h], ld)[0]
                    c1, c1w = (Lp - Lm) / (2 * h), (Lp2 - Lm2) / (4 * h)
                    c2, c2w = (Lp - 2 * L + Lm) / (h * h), (Lp2 - 2 * L + Lm2) / (4 * h * h)
                    fd1, fd2 = (4 * c1 - c1w) / 3, (4 * c2 - c2w) / 3
                    e1, e2 = rel(d1, fd1), rel(d2, fd2)
                    worst = max(worst, e1, e2)
                    plain = max(plain, rel(d1, c1), rel(d2, c2))
                    assert e1 <= 1e-6 and e2 <= 1e-6, (c, j, k, x, float(d1), float(fd1), float(d2), float(fd2))
    print(f"plain central differences (with their h^2 term): worst relative {plain:.3e}")
    print(f"analytic vs central differences: worst relative {worst:.3e}")


def test_mirror_and_ends():
    """(j, k) at alpha is (k, j) at 1 - alpha; alpha = 0 is j alone and alpha = 1 is k alone, whatever the other sample"""
    ld = np.longdouble
    V = 4
    p = deep_pileup(V, 5)
    worst = 0.0
    for c in range(p.C):
        for j in range(V):
            for k in range(V):
                a, b = alr.Cell(p, G6, c, j, k), alr.Cell(p, G6, c, k, j)
                for x in (0.0, 0.05, 0.4, 0.9, 1.0):
                    L, d1, d2, aL, a1, a2 = a.eval([ld(x)], ld)[:6]
                    M, e1, e2 = b.eval([ld(1.0) - ld(x)], ld)[:3]
                    for u, v, s in ((L, M, aL), (d1, -e1, a1), (d2, e2, a2)):
                        assert abs(float(u[0] - v[0])) <= 1e-12 * float(s[0]), (c, j, k, x, u, v, s)
                        worst = max(worst, abs(float(u[0] - v[0])) / max(float(s[0]), 1e-300))
                ends = a.eval([0.0, 1.0], ld)[0]
                solo = [alr.Cell(p, G6, c, j, j).eval([0.0], ld)[0][0], alr.Cell(p, G6, c, k, k).eval([1.0], ld)[0][0]]
                assert abs(float(ends[0] - solo[0])) <= 1e-12 * float(aL[0]) + 1e-15
                assert abs(float(ends[1] - solo[1])) <= 1e-12 * float(aL[0]) + 1e-15
    print(f"mirror: worst |difference| / sum |terms| {worst:.3e}")


# ---- the model does what it is for -------------------------------------------------------------------------------------

def test_the_fit_finds_the_mixing_share_with_an_honest_error_bar():
    p, first, second = alr.doublet_pileup(**alr.MIXED)
    inside, rows = 0, []
    for c in range(p.C):
        r = alr.fit(p, G2, c, int(first[c]), int(second[c]), 1.0)
        assert r["status"] == 0 and r["info"] > 0, (c, r["status"])                # interior for every droplet
        se = r["info"] ** -0.5
        lrt = 2.0 * (r["ll_hat"] - max(r["ll_zero"], r["ll_top"]))                 # against the better singlet
        rows.append((alr.MIXED_SHARES[c], round(r["alpha_hat"], 4), round(se, 4), round(lrt, 1)))
        inside += abs(r["alpha_hat"] - alr.MIXED_SHARES[c]) <= 4.0 * se
        assert lrt > 10.0, (c, lrt)
    print(f"mixed: (share, alpha_hat, se, lrt) per droplet {rows}")
    assert inside >= 0.9 * p.C, inside


def test_clean_singlets_sit_on_the_lower_bound():
    p, first, second = alr.doublet_pileup(**alr.CLEAN)
    at0, lrts = 0, []
    for c in range(p.C):
        r = alr.fit(p, G2, c, int(first[c]), int(second[c]), 1.0)
        at0 += r["status"] == 1
        lrts.append(2.0 * (r["ll_hat"] - r["ll_zero"]))                            # against j alone
    print(f"clean: {at0} of {p.C} droplets on the lower bound, largest LRT against the first sample alone {max(lrts):.2f}")
    assert at0 > p.C / 2 and max(lrts) <= 10.0
