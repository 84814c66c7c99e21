"""muxgl_demux_ambient_fit without a device: the restatement (tests/ambient_fit_ref.py) against finite differences of the
table restatement it extends, the model on the soup pileup, and the boundary (header, binding, library)."""
import os
import re
import subprocess

import numpy as np
import pytest

import ambient_fit_ref as afr
import ambient_ref as ar
from popscle_amd import muxgl, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_call():
    raw = open(os.path.join(ROOT, "include", "muxgl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ptr = lambda t, n: rf"\s*{t}\s*\*\s*{n}\s*"
    assert re.search(r"\bint\s+muxgl_demux_ambient_fit\s*\(" + ptr("muxgl_handle", "h") + "," + ptr(r"const\s+muxgl_demux_params", "p")
                     + "," + ptr(r"const\s+double", "amb_af") + r",\s*int32_t\s+n_cand\s*," + ptr(r"const\s+int32_t", "cand")
                     + r",\s*double\s+rho_max\s*," + ptr("double", "rho_hat") + "," + ptr("double", "ll_hat") + ","
                     + ptr("double", "ll_zero") + "," + ptr("double", "info") + "," + ptr("int32_t", "status") + ","
                     + ptr("int32_t", "n_steps") + "," + ptr("float", "kernel_ms") + r"\)\s*;", text)
    doc = raw[raw.index("The ambient share of muxgl_demux_ambient"):raw.index("int muxgl_demux_ambient_fit")]
    assert "NO standard error" in doc and "no slab budget applies" in doc and "cmd_cram_demuxlet.cpp:655-725" in doc
    table_doc = raw[raw.index("Every droplet as ONE cell of sample j"):raw.index("int muxgl_demux_ambient(")]
    assert "not an estimate with an error bar" not in table_doc and "muxgl_demux_ambient_fit" in table_doc
    assert re.search(r"#define\s+MUXGL_MAX_FIT_CAND\s+16\b", raw)
    if not os.path.exists(muxgl.LIB_PATH):
        from popscle_amd.build import build_lib

        build_lib()
    lib = muxgl.load_library()
    assert len(muxgl.SYMBOLS["muxgl_demux_ambient_fit"][1]) == 13
    nm = subprocess.run(["nm", "-D", "--defined-only", muxgl.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT muxgl_demux_ambient_fit$", nm, flags=re.M)
    assert lib.muxgl_demux_ambient_fit(None, None, None, 1, None, 0.5, *[None] * 7) != 0   # no handle: an error, not a crash
    assert lib.muxgl_version() == 3 and muxgl.T_COUNT == 16                                 # (tests/test_abi.py pins them)


def test_ambient_fit_summary_hand_made():
    fit = {"info": np.array([[4.0, 0.0], [25.0, -1.0], [100.0, 16.0]]), "status": np.array([[0, 0], [1, 0], [2, 3]]),
           "ll_hat": np.array([[-10.0, -5.0], [-3.0, -2.0], [-1.0, 0.0]]), "ll_zero": np.array([[-12.0, -5.0], [-3.0, -2.5], [-4.0, 0.0]])}
    sm = muxgl.ambient_fit_summary(fit)
    assert sm["se"][0, 0] == 0.5 and np.isnan(sm["se"]).sum() == 5
    assert np.array_equal(sm["lrt"], [[4.0, 0.0], [0.0, 1.0], [6.0, 0.0]])


def test_top_samples_ties_go_to_the_lower_index():
    from popscle_amd import demuxlet

    sng = np.array([[-3.0, -1.0, -1.0, -2.0], [-5.0, -5.0, -5.0, -5.0], [-1.0, np.nan, -0.5, -0.5]])
    assert demuxlet.top_samples(sng, 2).tolist() == [[1, 2], [0, 1], [2, 3]]
    assert demuxlet.top_samples(sng, 1).dtype == np.int32


# ---- the analytic derivatives are the derivatives of the table ----------------------------------------------------------

def deep_pileup(V, seed):
    """cells of a dozen entries, most of them of 33 or 60 reads, base qualities 2..93, reads of neither allele, markers
    without genotypes"""
    p, _, _ = afr.shaped_pileup([12, 9, 14, 1, 11, 13], 120, V, seed, depth_p=(0.1, 0.1, 0.4, 0.4), missing_gp_frac=0.05)
    assert np.diff(p.entry_rptr).max() == 60 and (p.reads == synth.READ_OTHER).any()
    return p


@pytest.mark.parametrize("V,alphas,seed", [(3, (0.0, 0.5), 1), (5, (0.1, 0.3, 0.7), 2), (2, (0.0, 0.13, 0.37, 0.5, 0.71, 1.0), 3)])
def test_analytic_derivatives_equal_central_differences_of_the_table(V, alphas, seed):
    ld = np.longdouble
    p = deep_pileup(V, seed)
    f = ar.draw_af(p.S, seed=seed, corners=0.25)                    # f exactly 0 and exactly 1 on half of the markers
    assert (f == 0.0).any() and (f == 1.0).any()
    # Central differences at h = 1e-4 carry their own truncation, h^2 / 6 times the third derivative (h^2 / 12 times the
    # fourth): with 60-read entries at base quality 93 the third derivative is ~1e5 where the first is ~1e2, i.e. 2e-6
    # relative, above the bar although the analytic value is right.  The h^2 term is therefore removed by one Richardson
    # step with the differences at 2 h (both are central differences of the same LL; what is left is O(h^4)), and the
    # bar of 1e-6 relative is held on that.
    h = ld(1e-4)
    worst = plain = 0.0
    rel = lambda x, y: abs(float(x - y)) / max(abs(float(x)), 1e-300)
    for c in range(p.C):
        for j in range(V):
            cell = afr.Cell(p, alphas, f, c, j)
            for rho in (0.05, 0.2, 0.45):
                L, d1, d2 = [v[0] for v in cell.eval([rho], ld)[:3]]
                Lm2, Lm, Lp, Lp2 = cell.eval([ld(rho) - 2 * h, ld(rho) - h, ld(rho) + h, ld(rho) + 2 * h], ld)[0]
                c1, c1w = (Lp - Lm) / (2 * h), (Lp2 - Lm2) / (4 * h)
                c2, c2w = (Lp - 2 * L + Lm) / (h * h), (Lp2 - 2 * L + Lm2) / (4 * h * h)
                fd1, fd2 = (4 * c1 - c1w) / 3, (4 * c2 - c2w) / 3
                e1, e2 = rel(d1, fd1), rel(d2, fd2)
                worst = max(worst, e1, e2)
                plain = max(plain, rel(d1, c1), rel(d2, c2))
                assert e1 <= 1e-6 and e2 <= 1e-6, (c, j, rho, float(d1), float(fd1), float(d2), float(fd2))
    print(f"plain central differences (with their h^2 term): worst relative {plain:.3e}")
    print(f"analytic vs central differences: worst relative {worst:.3e}")


def test_analytic_derivatives_equal_central_differences_of_ambient_ref_table_itself():
    """The same comparison with ambient_ref.table as it stands supplying LL.  It is float64 only, so besides the 1e-6
    relative the bar carries the rounding of its own differences: an LL summed over n entries is good to about
    n eps sum|terms|, which the Richardson weights (4/3 + 1/3) and the division by 2 h resp. h^2 turn into the two
    allowances below (4 values resp. 4 values and 2 L enter)."""
    V, alphas = 3, (0.0, 0.5)
    p = deep_pileup(V, 1)
    f = ar.draw_af(p.S, seed=1, corners=0.25)
    h, eps = 1e-4, np.finfo(np.float64).eps
    worst = 0.0
    for rho in (0.05, 0.2, 0.45):
        T = ar.table(p, alphas, f, (rho - 2 * h, rho - h, rho, rho + h, rho + 2 * h))      # [C][V][5]
        for c in range(p.C):
            for j in range(V):
                cell = afr.Cell(p, alphas, f, c, j)
                _, d1, d2, absL = [float(v[0]) for v in cell.eval([rho], np.longdouble)[:4]]
                Lm2, Lm, L, Lp, Lp2 = T[c, j]
                fd1 = (4 * (Lp - Lm) / (2 * h) - (Lp2 - Lm2) / (4 * h)) / 3
                fd2 = (4 * (Lp - 2 * L + Lm) / (h * h) - (Lp2 - 2 * L + Lm2) / (4 * h * h)) / 3
                noise = max(cell.n, 1) * eps * absL
                assert abs(d1 - fd1) <= 1e-6 * abs(d1) + 2 * noise / h, (c, j, rho, d1, fd1)
                assert abs(d2 - fd2) <= 1e-6 * abs(d2) + 8 * noise / (h * h), (c, j, rho, d2, fd2)
                worst = max(worst, abs(d1 - fd1) / max(abs(d1), 1e-300), abs(d2 - fd2) / max(abs(d2), 1e-300))
    print(f"analytic vs central differences of ambient_ref.table (float64): worst relative {worst:.3e}")


def test_the_restated_ll_is_the_table_restatement():
    """LL of the fit restatement in float64 equals ambient_ref.table, the restatement the device's table is held to"""
    p = deep_pileup(3, 7)
    f = ar.draw_af(p.S, seed=5)
    rhos = (0.0, 0.125, 0.3)
    want = ar.table(p, (0.0, 0.5), f, rhos)
    for c in range(p.C):
        for j in range(3):
            got = afr.Cell(p, (0.0, 0.5), f, c, j).eval(rhos)[0]
            assert np.abs(got - want[c, j]).max() <= 1e-10 * max(1.0, np.abs(want[c, j]).max())
    L, d1, d2 = afr.ll_d1_d2(p, (0.0, 0.5), f, 2, 1, 0.3)
    assert L == afr.Cell(p, (0.0, 0.5), f, 2, 1).eval([0.3])[0][0] and np.isfinite([d1, d2]).all()


# ---- the model does what it is for -------------------------------------------------------------------------------------

def test_the_fit_finds_the_soup_share_with_an_honest_error_bar():
    p, who, pool = ar.soup_pileup(**ar.SOUP)
    inside, rows = 0, []
    for c in range(p.C):
        r = afr.fit(p, (0.0, 0.5), pool, c, int(who[c]), 0.5)          # the true profile, not the pileup's own counts
        assert r["status"] == 0 and r["info"] > 0
        se = r["info"] ** -0.5
        lrt = 2.0 * (r["ll_hat"] - r["ll_zero"])
        rows.append((round(r["rho_hat"], 4), round(se, 4), round(lrt, 1)))
        inside += abs(r["rho_hat"] - 0.2) <= 4.0 * se
        assert lrt > 10.0, (c, lrt)
    print(f"soup: (rho_hat, se, lrt) per droplet {rows}")
    assert inside >= 0.9 * p.C, inside
