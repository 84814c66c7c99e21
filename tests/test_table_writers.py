"""CPU test of the front end's text writers (popscle_amd/host/table_writers.hpp): every writer is run by a stand-alone
program, tests/csrc/table_writers_probe.cpp, over the arrays below -- no library, no device -- and each file it leaves is
compared, whole, with the text stated here from the same numbers.

The expectations restate the column rules of the comment at the top of popscle_amd/host/main.cpp (and table_rows.py, which
the *_cli_gpu.py tests share); nothing is read from the C++.  Four droplets, three columns (samples S0 S1 S2 for demuxlet's
tables, clusters 0 1 2 for freemuxlet's), three alphas, two rhos.  What the numbers are chosen to reach:
  * the demuxlet row list: barcode order differs from index order; droplet 3 is dropped by valid = 0, droplet 2 by
    NUM.SNPS < --min-snp; INT_ID-style positions count the dropped ones;
  * .incl: a partner of -1 (NA columns), DBL.ALPHA = alpha or 1 - alpha by `first`;
  * the fits: status 0 / 1 / 2 / 3, info <= 0 at status 0 (SE NA), ll_hat = -inf (LRT NA), a candidate and a pair of -1
    (no row), an interval below 1 (SNG2.LLK NA, MIX.LRT against SNG1.LLK alone, and a different count for the notice);
  * a NaN in freemuxlet's ju and amb rows at index 0, ranked as -inf and never printed (only freemuxlet prints droplet 3);
  * exact ties in every argmax: the lowest index wins; in demuxlet's .unk the known-donor-first orientation wins, and an
    alpha of 0.5 has one orientation only;
  * a barcode of 1100 characters, past every fixed buffer."""
import math
import os
import shutil
import subprocess

import pytest

import table_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")

C, N = 4, 3
BCS = ["TTTT-1", "AAAA-1", "GGGG-1", "C" * 1100 + "-1"]
IDS = ["S0", "S1", "S2"]
ALPHA = [0.0, 0.25, 0.5]
RHOS = [0.0, 0.125]
LIMITS = [10, 10, 10]                      # --min-total --min-umi --min-snp
REC = {
    "valid": [1, 1, 1, 0], "nsnps": [40, 30, 5, 20], "type": [0, 1, 2, 0], "clust": [0, -1, -1, 2],
    "jBest": [0, 1, 0, 2], "kBest": [0, 2, 2, 2], "jNext": [1, 1, 2, 1], "kNext": [1, 1, 2, 2],
    "sBest": [0, 1, 2, 2], "sNext": [1, 2, 0, -1], "dBest1": [0, 1, 0, -1], "dBest2": [1, 2, 2, -1],
    "bestLLK": [-100.5, -90.25, -80.125, -70.0625], "nextLLK": [-103.0, -90.75, -80.126, -79.5],
    "sngBestLLK": [-100.5, -94.0, -84.0, -70.0625], "sngNextLLK": [-106.0, -96.0, -86.5, -1e300],
    "dblBestLLK": [-110.0, -90.25, -85.5, -75.0], "bestPP": [0.999, 0.5, 1e-05, 0.25], "sngPP": [0.99, 0.004, 0.5, 1.0],
    "sngOnlyPP": [0.99999, 0.12345, 0.5, 1.0],
}
TOTL, UNIQ = [60, 55, 40, 35], [50, 45, 30, 25]
F_NSNPS, F_NREADS = [41, 31, 6, 21], [51, 46, 31, 26]
SNG = [[-10.5, -20.25, -30.0], [-5.0, -5.0, -7.5], [-1.0, -2.0, -3.0], [-300.0, -2.5, -2.5]]
INCL = [[-10.0, -12.5, -30.0], [-4.5, -4.75, -7.0], [-1.0, -2.0, -3.0], [-3.0, -2.5, -2.25]]
TOT = [-9.5, -4.0, -0.5, -2.0]
DBL = [[-11.0, -13.5, -31.0], [-6.0, -6.5, 0.0], [-2.0, -3.0, -4.0], [0.0, -3.5, -3.25]]
PARTNER = [[1, 0, 0], [2, 2, -1], [1, 0, 0], [-1, 2, 1]]
AIDX = [[1, 1, 2], [2, 1, 0], [1, 1, 1], [0, 1, 1]]
FIRST = [[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0]]
AMB = [[[-101.0, -100.75], [-120.0, -121.0], [-130.0, -131.0]],
       [[-95.0, -88.0], [-91.0, -88.0], [-99.0, -98.0]],        # a tie of (S0, 0.125) and (S1, 0.125)
       [[-81.0, -82.0], [-83.0, -80.0], [-85.0, -86.0]],
       [[NAN, -75.0], [-74.0, -76.0], [-77.0, -78.0]]]
FIT = {
    "status": [[0, 1], [2, 0], [0, 3], [0, 0]],
    "info": [[4.0, 9.0], [1.0, 0.0], [-1.0, 2.0], [16.0, 1.0]],
    "est": [[0.125, 0.0], [0.5, 0.25], [0.0625, 0.3], [0.2, 0.1]],
    "ll_hat": [[-99.5, -101.5], [-89.0, -INF], [-79.0, -78.0], [-69.0, -68.0]],
    "ll_zero": [[-100.5, -106.0], [-95.0, -96.0], [-80.125, -84.0], [-70.0625, -71.0]],
    "ll_top": [[-101.0, -102.0], [-94.0, -97.0], [-79.5, -83.0], [-72.0, -73.0]],
}
LOW = -500.0
D_JU = [[[0.0, -99.0, -120.0], [0.0, LOW, LOW], [0.0, LOW, LOW]],          # droplet 0: ju and uj tie at (S0, 0.25)
        [[0.0, -93.0, -94.0], [0.0, LOW, LOW], [0.0, LOW, LOW]],
        [[0.0, LOW, LOW]] * 3, [[0.0, LOW, LOW]] * 3]
D_UJ = [[[0.0, -99.0, -50.0], [0.0, LOW, LOW], [0.0, LOW, LOW]],           # (the -50 stands at alpha = 0.5: one orientation only)
        [[0.0, LOW, LOW], [0.0, LOW, LOW], [0.0, -89.5, LOW]],
        [[0.0, LOW, LOW]] * 3, [[0.0, LOW, LOW]] * 3]
D_UU = [[-102.0, -103.0, -101.5], [-91.0, -95.0, -96.0], [-1.0, -2.0, -3.0], [-1.0, -2.0, -3.0]]
F_JU = [[-99.0, -98.0, -98.0], [-95.0, -96.0, -97.0], [-90.0, -85.0, -81.0], [NAN, -75.0, -72.0]]
F_LU, F_UU = [-103.0, -89.0, -82.0, -73.0], [-104.0, -92.0, -83.0, -71.0]
LLK0, LLK2 = [-200.5, -150.25, -120.0, -90.75], [-190.0, -155.5, -119.0, -95.0]
NVIS, SRTED = 3, [2, 0, 3, 1]
DD = {"dd_nsnps": [3, 4, 5, 6, 7, 8], "dd_nread1": [10, 12, 9, 4, 5, 6], "dd_nread2": [11, 8, 9, 7, 3, 2],
      "dd_llk0": [-1.5, -2.5, -3.5, -4.5, -5.5, -6.5], "dd_llk2": [-1.0, -3.0, -3.5, -4.0, -6.0, -6.25]}
ANCHOR_START, ANCHOR_LLR, ANCHOR_MODE = [1, -1], [12.5, NAN], [1, 0]        # S0 PRIOR, S1 HELD; cluster 2 is free
HAS_GP = [1, 0, 1]
GP = [[[0.7, 0.2, 0.1], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [[0.3, 0.3, 0.4]] * 3, [[0.1, 0.1, 0.8], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]]
POST = [[[0.2, 0.7, 0.1], [1.0, 0.0, 0.0]], [[0.5, 0.25, 0.25]] * 2, [[0.05, 0.05, 0.9], [0.0, 0.0, 1.0]]]
MATCH_LL = [[-50.0, -60.0, -70.0], [-40.0, -40.0, -45.0], [-INF, -INF, -INF]]
MATCH_LL0, MATCH_NSNPS = [-65.0, -50.0, -30.0], [100, 80, 0]
PAIRS_L2, PAIRS_L0, PAIRS_NS = [-10.5, -20.25, -30.0], [-12.0, -19.0, -33.5], [10, 0, 7]


def flat(x):
    return [v for y in x for v in flat(y)] if isinstance(x, (list, tuple)) else [x]


def input_text():
    arrays = dict(REC)
    arrays.update(FIT)
    arrays.update(DD)
    arrays.update({
        "bcs": BCS, "ids": IDS, "alpha": ALPHA, "rhos": RHOS, "min_read_umi_snp": LIMITS, "totl_reads": TOTL, "uniq_reads": UNIQ,
        "f_nsnps": F_NSNPS, "f_nreads": F_NREADS, "sng": SNG, "incl": INCL, "tot": TOT, "dbl": DBL, "partner": PARTNER, "aidx": AIDX,
        "first": FIRST, "amb": AMB, "d_ju": D_JU, "d_uj": D_UJ, "d_uu": D_UU, "f_ju": F_JU, "f_lu": F_LU, "f_uu": F_UU, "llk0": LLK0,
        "llk2": LLK2, "nvis": [NVIS], "drops_srted": SRTED, "anchor_start": ANCHOR_START, "anchor_start_llr": ANCHOR_LLR,
        "anchor_mode": ANCHOR_MODE, "has_gp": HAS_GP, "gp": GP, "post": POST, "match_ll": MATCH_LL, "match_ll0": MATCH_LL0,
        "match_nsnps": MATCH_NSNPS, "pairs_l2": PAIRS_L2, "pairs_l0": PAIRS_L0, "pairs_nsnps": PAIRS_NS})
    return "".join(name + " " + " ".join(v if isinstance(v, str) else repr(v) for v in flat(a)) + "\n" for name, a in arrays.items())


def build(exe, sanitize):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Wno-unused-parameter"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    return subprocess.run(cmd + [os.path.join(ROOT, "tests", "csrc", "table_writers_probe.cpp"), "-o", exe, "-lz"],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> text of every file the probe left"""
    d = tmp_path_factory.mktemp("writers")
    exe, out = str(d / "table_writers_probe"), d / "out"
    r = build(exe, True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr):
        r = build(exe, False)               # a host compiler without the sanitizers' runtimes: the plain program
    assert r.returncode == 0, r.stderr[-3000:]
    out.mkdir()
    (d / "input.txt").write_text(input_text())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", POPSCLE_AMD_THREADS="3")
    r = subprocess.run([exe, str(d / "input.txt"), str(out)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return {n: (out / n).read_text() for n in os.listdir(out)}


# ---- the rules, restated ----
def val(v):
    return -INF if math.isnan(v) else v


def first_max(values):
    """index of the largest value, the lowest index on ties"""
    return max(range(len(values)), key=lambda i: (values[i], -i))


def type_name(t):
    return {0: "SNG", 1: "DBL", 2: "AMB"}[t]


def printed_demux():
    """(droplet, NUM.SNPS, NUM.READS, position in barcode order) of the droplets .best prints"""
    rows = []
    for pos, i in enumerate(sorted(range(C), key=lambda i: BCS[i])):
        if TOTL[i] >= LIMITS[0] and UNIQ[i] >= LIMITS[1] and REC["nsnps"][i] >= LIMITS[2] and REC["valid"][i]:
            rows.append((i, REC["nsnps"][i], UNIQ[i], pos))
    return rows


def printed_fmx():
    return [(i, F_NSNPS[i], F_NREADS[i], i) for i in range(C)]


TABLES = {"d": (printed_demux, lambda j: IDS[j] if 0 <= j < len(IDS) else "NA", "SM_ID", "SM1_ID\tSM2_ID"),
          "f": (printed_fmx, str, "CLUST", "CLUST1\tCLUST2")}


def head(row):
    return [BCS[row[0]], "%d" % row[1], "%d" % row[2]]


def text(header, rows):
    return "".join(ln + "\n" for ln in [header] + rows)


def slots(which):
    """per droplet the candidates [2] and the pairs [2][2] a fit is asked for: -1 where the record has no such column; a
    demuxlet record without entries has none"""
    cand, pair = [], []
    for i in range(C):
        ok = lambda s: 0 <= s < N and (which == "f" or REC["valid"][i] != 0)
        cand.append([REC[k][i] if ok(REC[k][i]) else -1 for k in ("sBest", "sNext")])
        pair.append([[REC[a][i], REC[b][i]] if ok(REC[a][i]) and ok(REC[b][i]) else [-1, -1]
                     for a, b in (("dBest1", "dBest2"), ("sBest", "sNext"))])
    return cand, pair


def summary(alone):
    se = [[1.0 / math.sqrt(FIT["info"][i][k]) if FIT["status"][i][k] == 0 and FIT["info"][i][k] > 0 else NAN for k in range(2)]
          for i in range(C)]
    lrt = [[2.0 * (FIT["ll_hat"][i][k] - alone[i][k]) for k in range(2)] for i in range(C)]
    return {"se": se, "lrt": lrt}


# ---- the tests ----
def test_the_probe_left_every_file_and_no_other(files):
    per_table = ["sing2", "incl", "unk", "amb", "ambfit", "alphafit", "alphafit_capped"]
    assert set(files) == ({w + "." + t for w in "df" for t in per_table} |
                          {"rows.txt", "slots.txt", "counts.txt", "f.lmix", "f.lmix_old", "f.clust0", "f.clust1", "old.ldist",
                           "old.ldist_header", "anchors", "anchors_mode", "refined", "match", "match.best", "clust.ldist"})


def test_row_lists(files):
    assert [r[0] for r in printed_demux()] == [1, 0] and [r[3] for r in printed_demux()] == [0, 3]
    want = ["d\t%d\t%d\t%d\t%d" % r for r in printed_demux()] + ["f\t%d\t%d\t%d\t%d" % r for r in printed_fmx()]
    assert files["rows.txt"] == text(want[0], want[1:])


def test_fit_slots(files):
    (dc, dp), (fc, fp) = slots("d"), slots("f")
    assert dc[3] == [-1, -1] and fc[3] == [2, -1] and fp[3] == [[-1, -1], [-1, -1]]
    want = ["%d %d\t%d %d %d %d\t%d %d\t%d %d %d %d" % tuple(flat([dc[i], dp[i], fc[i], fp[i]])) for i in range(C)]
    assert files["slots.txt"] == text(want[0], want[1:])


@pytest.mark.parametrize("which", ["d", "f"])
def test_singlets(files, which):
    printed, label, word, _ = TABLES[which]
    rows = []
    for r in printed():
        mx = max(SNG[r[0]])
        total = sum(math.exp(v - mx) for v in SNG[r[0]])
        rows += ["\t".join([BCS[r[0]], label(j), "%d" % r[1], "%d" % r[2], "%.4f" % v, "%.3g" % (math.exp(v - mx) / total)])
                 for j, v in enumerate(SNG[r[0]])]
    assert files[which + ".sing2"] == text("BARCODE\t%s\tNUM.SNPS\tNUM.READS\tLLK1\tPOSTPRB" % word, rows)


@pytest.mark.parametrize("which", ["d", "f"])
def test_inclusion(files, which):
    printed, label, word, _ = TABLES[which]
    rows = []
    for r in printed():
        i = r[0]
        for j in range(N):
            f = [BCS[i], label(j), "%d" % r[1], "%d" % r[2], "%.4f" % INCL[i][j], "%.3g" % math.exp(INCL[i][j] - TOT[i])]
            if PARTNER[i][j] < 0:
                f += ["NA"] * (3 if which == "d" else 2)
            else:
                a = ALPHA[AIDX[i][j]]
                f += [label(PARTNER[i][j])] + (["%.3f" % (1.0 - a if FIRST[i][j] else a)] if which == "d" else []) + ["%.4f" % DBL[i][j]]
            rows.append("\t".join(f))
    assert any(ln.endswith("NA") for ln in rows)
    assert files[which + ".incl"] == text("BARCODE\t%s\tNUM.SNPS\tNUM.READS\tLLK.INCL\tPOSTPRB.INCL\tDBL.PARTNER\t%sDBL.LLK"
                                         % (word, "DBL.ALPHA\t" if which == "d" else ""), rows)


def test_unknown_demux(files):
    rows = []
    for r in printed_demux():
        i = r[0]
        dn = first_max(D_UU[i][1:]) + 1
        # the hypotheses with one panel sample in (sample, alpha index, known donor first) order; the first largest wins
        half = [(D_JU[i][j][n] if major else D_UJ[i][j][n], j, n, major)
                for j in range(N) for n in range(1, len(ALPHA)) for major in (1, 0) if major or ALPHA[n] != 0.5]
        v, j, n, major = half[first_max([h[0] for h in half])]
        guess = "%s,%s,%.2f" % ((IDS[j], "*", ALPHA[n]) if major else ("*", IDS[j], ALPHA[n]))
        top = max(D_UU[i][0], D_UU[i][dn], v)
        rows.append("\t".join(head(r) + ["%.4f" % REC["bestLLK"][i], "%.4f" % D_UU[i][0], "%.2f" % ALPHA[dn], "%.4f" % D_UU[i][dn],
                                         guess, "%.4f" % v, "%.4f" % (REC["bestLLK"][i] - top)]))
    assert [ln.split("\t")[7] for ln in rows] == ["*,S2,0.25", "S0,*,0.25"]
    assert files["d.unk"] == text("BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.ALPHA\tUNK.DBL.LLK\tHALF.GUESS\t"
                                  "HALF.LLK\tDIFF.LLK.PANEL.UNK", rows)


def test_unknown_fmx(files):
    rows, better = [], 0
    for r in printed_fmx():
        i = r[0]
        ranked = [val(v) for v in F_JU[i]]
        b = first_max(ranked)
        diff = REC["bestLLK"][i] - max(val(F_LU[i]), val(F_UU[i]), ranked[b])
        better += diff < -2.0
        rows.append("\t".join(head(r) + ["%.4f" % REC["bestLLK"][i], "%.4f" % F_LU[i], "%.4f" % F_UU[i], "%d" % b, "%.4f" % ranked[b],
                                         "%.4f" % diff]))
    assert [ln.split("\t")[6] for ln in rows] == ["1", "0", "2", "2"] and better == 1
    assert files["f.unk"] == text("BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.LLK\tHALF.CLUST\tHALF.LLK\t"
                                  "DIFF.LLK.CLUST.UNK", rows)
    assert "f.unk\t%d\n" % better in files["counts.txt"]


@pytest.mark.parametrize("which", ["d", "f"])
def test_ambient(files, which):
    printed, label, _, _ = TABLES[which]
    rows, rescued = [], 0
    for r in printed():
        i = r[0]
        row = flat(AMB[i])
        at = first_max([val(v) for v in row] if which == "f" else row)      # (demuxlet prints no droplet with a NaN)
        assert not math.isnan(row[at])
        rescued += REC["type"][i] == 1 and row[at] > REC["dblBestLLK"][i] + 2.0
        rows.append("\t".join(head(r) + [type_name(REC["type"][i]), "%.4f" % REC["bestLLK"][i], label(REC["sBest"][i]),
                                         "%.4f" % REC["sngBestLLK"][i], label(at // len(RHOS)), "%.2f" % RHOS[at % len(RHOS)],
                                         "%.4f" % row[at], "%.4f" % (row[at] - REC["bestLLK"][i])]))
    assert rescued == 1 and rows[0 if which == "d" else 1].split("\t")[7:9] == [label(0), "0.12"]     # the tie: the lower column
    assert files[which + ".amb"] == text("BARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.LLK\tSNG.BEST.GUESS\tSNG.BEST.LLK\t"
                                         "AMB.GUESS\tAMB.RHO\tAMB.LLK\tDIFF.LLK.AMB.BEST", rows)
    assert "%s.amb\t%d\n" % (which, rescued) in files["counts.txt"]


@pytest.mark.parametrize("which", ["d", "f"])
def test_ambient_fit(files, which):
    printed, label, word, _ = TABLES[which]
    cand, _ = slots(which)
    fit = {"ll_zero": FIT["ll_zero"], "rho_hat": FIT["est"], "ll_hat": FIT["ll_hat"], "status": FIT["status"]}
    rows = table_rows.ambient_fit_rows([(r[0], head(r)) for r in printed()], label, cand, fit, summary(FIT["ll_zero"]))
    assert len(rows) == (4 if which == "d" else 7)
    assert {ln.split("\t")[6] for ln in rows} >= {"NA", "0.5000"} and "NA" in {ln.split("\t")[8] for ln in rows}
    assert files[which + ".ambfit"] == text("BARCODE\tNUM.SNPS\tNUM.READS\t%s\tSNG.LLK\tAMB.RHO.MLE\tAMB.RHO.SE\tAMB.LLK.MLE\tAMB.LRT\t"
                                           "STATUS" % word, rows)


@pytest.mark.parametrize("whole", [True, False])
@pytest.mark.parametrize("which", ["d", "f"])
def test_alpha_fit(files, which, whole):
    printed, label, _, words = TABLES[which]
    _, pair = slots(which)
    alone = [[max(FIT["ll_zero"][i][k], FIT["ll_top"][i][k]) if whole else FIT["ll_zero"][i][k] for k in range(2)] for i in range(C)]
    fit = {"pair": pair, "alpha_max": 1.0 if whole else 0.5, "ll_zero": FIT["ll_zero"], "ll_top": FIT["ll_top"], "alpha_hat": FIT["est"],
           "ll_hat": FIT["ll_hat"], "status": FIT["status"]}
    rows = table_rows.alpha_fit_rows([(r[0], head(r)) for r in printed()], label, fit, summary(alone))
    assert len(rows) == (4 if which == "d" else 6) and {ln.split("\t")[7] == "NA" for ln in rows} == {not whole}
    # the notice's count: droplets called SNG whose SNG row beats what it is held against by more than 2
    mixed = sum(1 for r in printed() if REC["type"][r[0]] == 0 and pair[r[0]][1][0] >= 0 and FIT["ll_hat"][r[0]][1] > alone[r[0]][1] + 2.0)
    assert mixed == (0 if whole else 1)
    name = which + (".alphafit" if whole else ".alphafit_capped")
    assert files[name] == text("BARCODE\tNUM.SNPS\tNUM.READS\tPAIR\t%s\tSNG1.LLK\tSNG2.LLK\tALPHA.MLE\tALPHA.SE\tMIX.LLK.MLE\tMIX.LRT\t"
                               "STATUS" % words, rows)
    assert "%s\t%d\n" % (name, mixed) in files["counts.txt"]


def test_lmix_and_cluster_assignments(files):
    for name, words, sign in (("f.lmix", "BF.SINGLET\tBF.SINGLET.PER.SNP", 1.0), ("f.lmix_old", "LOG.BF\tBFpSNP", -1.0)):
        rows = ["\t".join(["%d" % i, BCS[i], "%d" % F_NSNPS[i], "%d" % F_NREADS[i], "%.2f" % LLK0[i], "%.2f" % LLK2[i],
                           "%.2f" % (sign * (LLK2[i] - LLK0[i])), "%.4f" % (sign * (LLK2[i] - LLK0[i]) / F_NSNPS[i])]) for i in range(C)]
        assert files[name] == text("INT_ID\tBARCODE\tNSNPs\tNREADs\tDBL.LLK\tSNG.LLK\t" + words, rows)
    assert files["f.clust0"] == text("INT_ID\tBARCODE\tCLUST0", ["%d\t%s\t%d" % (i, BCS[i], REC["clust"][i]) for i in range(C)])


def test_clust1_samples(files):
    c = REC
    rows = ["\t".join(["%d" % i, BCS[i], "%d" % F_NSNPS[i], "%d" % F_NREADS[i], type_name(c["type"][i]),
                       "%d,%d" % (c["jBest"][i], c["kBest"][i]), "%.2f" % c["bestLLK"][i], "%d,%d" % (c["jNext"][i], c["kNext"][i]),
                       "%.2f" % c["nextLLK"][i], "%.2f" % (c["bestLLK"][i] - c["nextLLK"][i]), "%.5f" % c["bestPP"][i],
                       "%.2g" % c["sngPP"][i], "%d" % c["sBest"][i], "%.2f" % c["sngBestLLK"][i], "%d" % c["sNext"][i],
                       "%.2f" % c["sngNextLLK"][i], "%.5f" % c["sngOnlyPP"][i], "%d,%d" % (c["dBest1"][i], c["dBest2"][i]),
                       "%.2f" % c["dblBestLLK"][i], "%.2f" % (c["sngBestLLK"][i] - c["dblBestLLK"][i])]) for i in range(C)]
    assert len(rows[3]) > 1100 + 300                       # the long barcode and a 300-digit number: past every fixed buffer
    assert files["f.clust1"] == text(
        "INT_ID\tBARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.GUESS\tBEST.LLK\tNEXT.GUESS\tNEXT.LLK\tDIFF.LLK.BEST.NEXT\t"
        "BEST.POSTERIOR\tSNG.POSTERIOR\tSNG.BEST.GUESS\tSNG.BEST.LLK\tSNG.NEXT.GUESS\tSNG.NEXT.LLK\tSNG.ONLY.POSTERIOR\tDBL.BEST.GUESS\t"
        "DBL.BEST.LLK\tDIFF.LLK.SNG.DBL", rows)


def test_droplet_ldist(files):
    header = "ID1\tID2\tNSNP\tREAD1\tREAD2\tREADMIN\tLLK0\tLLK2\tLDIFF\tDIFF.SNP"
    rows = []
    for a in range(NVIS):                                  # the pairs of the first NVIS droplets of the sorted order
        for b in range(a):
            si, sj = SRTED[a], SRTED[b]
            hi, lo = max(si, sj), min(si, sj)
            n, r1, r2, l0, l2 = (DD[k][hi * (hi - 1) // 2 + lo] for k in ("dd_nsnps", "dd_nread1", "dd_nread2", "dd_llk0", "dd_llk2"))
            rows.append("%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%.2f\t%.2f\t%.4f" % (si, sj, n, r1, r2, min(r1, r2), l0, l2, l2 - l0,
                                                                            (l2 - l0) / (n + 1e-6)))
    assert len(rows) == 3
    assert files["old.ldist"] == text(header, rows) and files["old.ldist_header"] == text(header, [])


def test_anchor_tables(files):
    K, nA = N, len(ANCHOR_MODE)
    nsng = [sum(1 for c in REC["clust"] if c == k) for k in range(K)]
    for name, with_mode in (("anchors", False), ("anchors_mode", True)):
        rows = []
        for k in range(K):
            f = ["%d" % k, IDS[k] if k < nA else "NA"]
            f += ["%d" % ANCHOR_START[k], "%.4f" % ANCHOR_LLR[k]] if k < nA and ANCHOR_START[k] >= 0 else ["NA", "NA"]
            f += ["%d" % nsng[k]] + ([("NA" if k >= nA else "PRIOR" if ANCHOR_MODE[k] == 1 else "HELD")] if with_mode else [])
            rows.append("\t".join(f))
        assert files[name] == text("CLUST\tSM_ID\tSTART.CLUST\tSTART.LLR\tN.SNG" + ("\tMODE" if with_mode else ""), rows)
    rows = []
    for k in range(nA):                                    # .clust1.refined.gz: the PRIOR donors over the markers with genotypes
        if ANCHOR_MODE[k] != 1:
            continue
        s_with = [s for s in range(len(HAS_GP)) if HAS_GP[s]]
        changed = sum(first_max(GP[s][k]) != first_max(POST[s][k]) for s in s_with)
        rows.append("%d\t%s\t%d\t%d\t%.4f\t%.4f" % (k, IDS[k], len(s_with), changed, sum(max(GP[s][k]) for s in s_with) / len(s_with),
                                                    sum(max(POST[s][k]) for s in s_with) / len(s_with)))
    assert rows == ["0\tS0\t2\t1\t0.7500\t0.8000"]
    assert files["refined"] == text("CLUST\tSM_ID\tN.GENO\tN.CHANGED\tMEAN.MAXGP.PRIOR\tMEAN.MAXGP.POST", rows)


def test_match_tables(files):
    K, V = len(MATCH_NSNPS), len(IDS)
    llr = [[val(MATCH_LL[k][v] - MATCH_LL0[k]) for v in range(V)] for k in range(K)]
    rows = []
    for k in range(K):
        mx = max(MATCH_LL[k])
        mx = 0.0 if math.isinf(mx) else mx
        total = sum(math.exp(v - mx) for v in MATCH_LL[k])
        rows += ["%d\t%s\t%d\t%.4f\t%.4f\t%.4f\t%.3g" % (k, IDS[v], MATCH_NSNPS[k], MATCH_LL[k][v], MATCH_LL0[k], llr[k][v],
                                                         math.exp(MATCH_LL[k][v] - mx) / total if total > 0 else 1.0 / V) for v in range(V)]
    assert files["match"] == text("CLUST\tSM_ID\tNUM.SNPS\tLLK\tLLK0\tLLR\tPOSTPRB", rows)
    scored = [k for k in range(K) if MATCH_NSNPS[k] > 0]
    best_clust = [scored[first_max([llr[k][v] for k in scored])] for v in range(V)]
    rows = []
    for k in range(K):
        if k not in scored:
            rows.append("%d\t%d\tNA\tNA\tNA\tNA\tNA\tNA" % (k, MATCH_NSNPS[k]))
            continue
        b = first_max(llr[k])
        rest = [v for v in range(V) if v != b]
        nx = rest[first_max([llr[k][v] for v in rest])]
        rows.append("%d\t%d\t%s\t%.4f\t%s\t%.4f\t%.4f\t%d" % (k, MATCH_NSNPS[k], IDS[b], llr[k][b], IDS[nx], llr[k][nx],
                                                              llr[k][b] - llr[k][nx], best_clust[b] == k))
    assert [ln.split("\t")[2] for ln in rows] == ["S0", "S0", "NA"] and [ln.split("\t")[-1] for ln in rows] == ["1", "0", "NA"]
    assert files["match.best"] == text("CLUST\tNUM.SNPS\tBEST.SM_ID\tBEST.LLR\tNEXT.SM_ID\tNEXT.LLR\tDIFF.LLR\tRECIPROCAL", rows)


def test_cluster_ldist(files):
    pairs = [(a, b) for a in range(1, N) for b in range(a)]
    rows = ["%d\t%d\t%d\t%.2f\t%.2f\t%.2f\t%.4f" % (a, b, PAIRS_NS[i], PAIRS_L0[i], PAIRS_L2[i], PAIRS_L2[i] - PAIRS_L0[i],
                                                     (PAIRS_L2[i] - PAIRS_L0[i]) / (PAIRS_NS[i] + 1e-6)) for i, (a, b) in enumerate(pairs)]
    assert files["clust.ldist"] == text("ID1\tID2\tNSNP\tLLK0\tLLK2\tLDIFF\tDIFF.SNP", rows)
