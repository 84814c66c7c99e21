"""CPU checks behind muxgl_demux_unknown (demux_unknown.hip): the header declares the call and the library exports it; the
premise of its GPU tests -- the reference's dead llksA0 / llks00 accumulation (cmd_cram_demuxlet.cpp:428-440, 598-616,
749-773), restated literally, equals bit for bit the slices of full_ll of the panel with the mean row appended as sample
V, and those slices read only column j and the appended row --; and muxgl.unknown_summary against a brute-force loop."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import unknown_ref as ur
from popscle_amd import muxgl, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the boundary ------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_call():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "muxgl.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+muxgl_demux_unknown\s*\(\s*muxgl_handle\s*\*\s*h\s*,\s*const\s+muxgl_demux_params\s*\*\s*p\s*,"
                     r"\s*const\s+double\s*\*\s*gp0\s*,\s*double\s*\*\s*ll_ju\s*,\s*double\s*\*\s*ll_uj\s*,"
                     r"\s*double\s*\*\s*ll_uu\s*,\s*float\s*\*\s*kernel_ms\s*\)\s*;", text)
    if not os.path.exists(muxgl.LIB_PATH):
        from popscle_amd.build import build_lib

        build_lib()
    lib = muxgl.load_library()
    res, args = muxgl.SYMBOLS["muxgl_demux_unknown"]
    assert res is not None and len(args) == 7
    assert hasattr(lib, "muxgl_demux_unknown")
    nm = subprocess.run(["nm", "-D", "--defined-only", muxgl.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT muxgl_demux_unknown$", nm, flags=re.M)
    assert lib.muxgl_demux_unknown(None, None, None, None, None, None, None) != 0   # no handle: an error, not a crash
    assert lib.muxgl_version() == 3 and muxgl.T_COUNT == 16                          # (tests/test_abi.py pins them)


# ---- (a) the premise -----------------------------------------------------------------------------------------------------

def literal_restatement(p, alphas):
    """:428-440, :598-616 and :749-773 line by line over the oracle's per-entry likelihoods (ob.demux_entry_pg = :655-725);
    returns (llksA0 [C][V][A], llks00 [C][A])"""
    S, V, A = p.S, p.gp.shape[1], len(alphas)
    gp0s = [0.0] * (S * 3)                                     # :428
    for i in range(S):
        if p.has_gp[i]:
            for j in range(V):
                for g in range(3):
                    gp0s[i * 3 + g] += float(p.gp[i, j, g])    # :432-434
            for g in range(3):
                gp0s[i * 3 + g] /= V                           # :436-438
    gpA0, gp00 = [None] * S, [None] * S                        # :590-591
    for i in range(S):
        if p.has_gp[i]:
            gpA0[i], gp00[i] = [0.0] * (V * 9), [0.0] * 9
            for j in range(V):
                for l in range(3):
                    for m in range(3):
                        gpA0[i][j * 9 + l * 3 + m] = float(p.gp[i, j, l]) * gp0s[i * 3 + m]   # :610
                        gp00[i][l * 3 + m] = gp0s[i * 3 + l] * gp0s[i * 3 + m]                # :611
    A0, L00 = np.zeros((p.C, V, A)), np.zeros((p.C, A))
    for c in range(p.C):
        for e in range(int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])):
            isnp = int(p.entry_snp[e])
            if not p.has_gp[isnp]:                             # :733
                continue
            pGs = ob.demux_entry_pg(p.reads[int(p.entry_rptr[e]):int(p.entry_rptr[e + 1])], alphas).reshape(-1)
            for j in range(V):
                sumPs = [0.0] * A                              # :750
                for l in range(3):
                    for m in range(3):
                        pp = gpA0[isnp][j * 9 + l * 3 + m]     # :754
                        for n in range(A):
                            sumPs[n] += pp * float(pGs[n * 9 + l * 3 + m])   # :756
                for n in range(A):
                    A0[c, j, n] += math.log(sumPs[n])          # :760
            sumPs = [0.0] * A                                  # :763
            for l in range(3):
                for m in range(3):
                    pp = gp00[isnp][l * 3 + m]                 # :767
                    for n in range(A):
                        sumPs[n] += pp * float(pGs[n * 9 + l * 3 + m])       # :769
            for n in range(A):
                L00[c, n] += math.log(sumPs[n])                # :773
    return A0, L00


def tiny():
    p = synth.make_pileup(8, 200, 3, seed=77, mean_entries=40, min_entries=5, missing_gp_frac=0.1)
    assert (p.has_gp == 0).any() and (p.has_gp != 0).any()
    return p


@pytest.mark.parametrize("alphas", [(0.0, 0.5), (0.0, 0.2, 0.5)])
def test_dead_accumulation_equals_the_augmented_panel_slices(alphas):
    p = tiny()
    A0, L00 = literal_restatement(p, alphas)
    t = ur.tables(p, alphas, ur.panel_mean(p.gp, p.has_gp))
    assert np.array_equal(t["ju"], A0)
    assert np.array_equal(t["uu"], L00)
    assert t["uj"].shape == A0.shape and np.isfinite(t["uj"]).all()
    # the two orientations are the same hypothesis at alpha = 0.5 only (up to the order of the nine terms)
    n = alphas.index(0.5)
    assert np.allclose(t["uj"][:, :, n], t["ju"][:, :, n], rtol=0, atol=1e-9)
    assert not np.allclose(t["uj"][:, :, 1], t["ju"][:, :, 1], rtol=0, atol=1e-9) or alphas[1] == 0.5


@pytest.mark.parametrize("alphas", [(0.0, 0.5), (0.2, 0.5, 0.3)])
def test_half_known_values_read_only_their_column_and_the_appended_row(alphas):
    """what the V > 255 comparison of tests/test_demux_unknown_gpu.py rests on: the reference on `chunk + [u]`, u from the
    whole panel, reproduces the slices of the run on the whole augmented panel bit for bit"""
    V = 20
    p = synth.make_pileup(10, 600, V, seed=41, mean_entries=50, min_entries=5, missing_gp_frac=0.03)
    u = ur.panel_mean(p.gp, p.has_gp)
    whole = ur.tables(p, alphas, u)
    for cols in ([0, 1, 2], list(range(3, 20)), [19, 4, 11]):
        t = ur.tables(p, alphas, u, cols)
        assert np.array_equal(t["ju"], whole["ju"][:, cols]) and np.array_equal(t["uj"], whole["uj"][:, cols])
        assert np.array_equal(t["uu"], whole["uu"])
    by = ur.tables_by_columns(p, alphas, u, chunk=7)
    assert all(np.array_equal(by[k], whole[k]) for k in ur.FIELDS)


# ---- (b) unknown_summary -------------------------------------------------------------------------------------------------

def brute_summary(t, alphas):
    ju, uj, uu = t["ju"], t["uj"], t["uu"]
    Cn, V, A = ju.shape
    out = {k: [] for k in ("uu_sng", "uu_dbl", "uu_alpha_idx", "half_llk", "half_sample", "half_alpha_idx", "half_known_major")}
    for c in range(Cn):
        out["uu_sng"].append(uu[c, 0])
        best, at = -1e300, -1
        for n in range(1, A):
            if uu[c, n] > best:
                best, at = uu[c, n], n
        out["uu_dbl"].append(best)
        out["uu_alpha_idx"].append(at)
        best, who = -1e300, (-1, -1, -1)
        for j in range(V):
            for n in range(1, A):
                if ju[c, j, n] > best:
                    best, who = ju[c, j, n], (j, n, 1)
                if alphas[n] != 0.5 and uj[c, j, n] > best:
                    best, who = uj[c, j, n], (j, n, 0)
        out["half_llk"].append(best)
        out["half_sample"].append(who[0])
        out["half_alpha_idx"].append(who[1])
        out["half_known_major"].append(who[2])
    return {k: np.array(v, dtype=np.float64 if k in ("uu_sng", "uu_dbl", "half_llk") else np.int32) for k, v in out.items()}


def assert_summary(t, alphas):
    got, want = muxgl.unknown_summary(t, alphas), brute_summary(t, alphas)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, got[k], want[k])
    return got


def random_tables(rng, Cn, V, A, ties):
    ju, uj, uu = (-rng.gamma(2.0, 30.0, size=s) for s in ((Cn, V, A), (Cn, V, A), (Cn, A)))
    if ties:   # values drawn from a handful: exact ties between samples, alphas and orientations
        pool = -np.array([3.0, 3.0, 7.5, 11.25, 40.0])
        ju, uj, uu = (pool[rng.integers(pool.size, size=x.shape)] for x in (ju, uj, uu))
    return dict(ju=ju, uj=uj, uu=uu)


@pytest.mark.parametrize("V,alphas", [(5, (0.0, 0.5)), (7, (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)), (4, (0.0, 0.3)), (3, (0.2, 0.5)),
                                      (1, (0.0, 0.25, 0.5)), (1, (0.0, 0.5)), (6, (0.0,)), (9, (0.0, 0.5, 0.2))])
@pytest.mark.parametrize("ties", [False, True])
def test_unknown_summary_against_brute_force(V, alphas, ties):
    rng = np.random.default_rng(V * 100 + len(alphas) + ties)
    got = assert_summary(random_tables(rng, 40, V, len(alphas), ties), alphas)
    if len(alphas) == 1:
        assert np.all(got["uu_dbl"] == -1e300) and np.all(got["uu_alpha_idx"] == -1)
        assert np.all(got["half_llk"] == -1e300) and np.all(got["half_sample"] == -1)
        assert np.all(got["half_alpha_idx"] == -1) and np.all(got["half_known_major"] == -1)
    else:
        assert np.all(got["half_sample"] >= 0) and np.all(got["half_alpha_idx"] >= 1)


def test_unknown_summary_hand_made_ties():
    alphas = (0.0, 0.5, 0.2)
    ju = np.full((4, 3, 3), -50.0)
    uj = np.full((4, 3, 3), -50.0)
    uu = np.array([[-1.0, -9.0, -9.0], [-1.0, -9.0, -8.0], [-1.0, -7.0, -8.0], [-1.0, -2.0, -2.0]])
    uj[0, 0, 1] = -1.0                      # cell 0: the best value sits in uj at alpha 0.5 -- no candidate; all else ties
    ju[1, 2, 2] = uj[1, 1, 2] = -3.0        # cell 1: tie between (2, n=2, ju) and (1, n=2, uj): the smaller sample wins
    ju[2, 1, 2] = uj[2, 1, 2] = -3.0        # cell 2: same sample and alpha: ju before uj
    ju[3, 2, 1] = ju[3, 2, 2] = -3.0        # cell 3: same sample: the smaller n
    ju[3, 0, 0] = uj[3, 0, 0] = 0.0         # (slot n = 0 is no doublet candidate)
    got = assert_summary(dict(ju=ju, uj=uj, uu=uu), alphas)
    assert got["uu_alpha_idx"].tolist() == [1, 2, 1, 1] and got["uu_dbl"].tolist() == [-9.0, -8.0, -7.0, -2.0]
    assert got["half_sample"].tolist() == [0, 1, 1, 2]
    assert got["half_alpha_idx"].tolist() == [1, 2, 2, 1]
    assert got["half_known_major"].tolist() == [1, 0, 1, 1]
    assert got["half_llk"].tolist() == [-50.0, -3.0, -3.0, -3.0]
    assert got["uu_sng"].tolist() == [-1.0] * 4
    empty = muxgl.unknown_summary(dict(ju=np.zeros((0, 3, 2)), uj=np.zeros((0, 3, 2)), uu=np.zeros((0, 2))), (0.0, 0.5))
    assert all(v.shape == (0,) for v in empty.values())
    with pytest.raises(ValueError):
        muxgl.unknown_summary(dict(ju=ju, uj=uj, uu=uu), (0.0, 0.5))
