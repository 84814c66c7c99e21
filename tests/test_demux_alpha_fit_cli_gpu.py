"""`popscle-amd demuxlet --fit-alpha` on a small synthetic pileup: <out>.alphafit.gz has, per row of .best and in its order,
one row DBL for the two samples of DBL.BEST.GUESS and one row SNG for (SNG.BEST.GUESS, SNG.NEXT.GUESS); the rows are
Engine.demux_alpha_fit on the same pairs through the format strings; --alpha-fit-max sets the upper bound, and SNG2.LLK is
NA and MIX.LRT against SNG1.LLK alone below 1; and the flag changes nothing else: .best is the same bytes with and without
it, and there is no .alphafit.gz without it."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import table_rows
from popscle_amd import muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup

pytestmark = pytest.mark.gpu

HEADER = ("BARCODE\tNUM.SNPS\tNUM.READS\tPAIR\tSM1_ID\tSM2_ID\tSNG1.LLK\tSNG2.LLK\tALPHA.MLE\tALPHA.SE\tMIX.LLK.MLE\tMIX.LRT\t"
          "STATUS")


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stderr


def best_pairs(best_rows, index, ids, C):
    """[C][2][2] from the rows of .best themselves: the samples of DBL.BEST.GUESS, and (SNG.BEST.GUESS, SNG.NEXT.GUESS)"""
    num = {s: v for v, s in enumerate(ids)}
    pairs = np.full((C, 2, 2), -1, dtype=np.int32)
    for brow in best_rows:
        i = index[brow[1]]
        for slot, names in enumerate((brow[17].split(",")[:2], [brow[12], brow[14]])):
            if all(n in num for n in names):
                pairs[i, slot] = [num[n] for n in names]
    return pairs


def expected_rows(best_rows, index, ids, fit):
    return table_rows.alpha_fit_rows([(index[brow[1]], brow[1:4]) for brow in best_rows], lambda j: ids[j], fit,
                                     muxgl.alpha_fit_summary(fit))


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_demuxlet_cli_fit_alpha(tmp_path, devices):
    import pyplp

    V, S = 8, 1200
    p = synth.make_pileup(60, S, V, seed=5, mean_entries=150, min_entries=20, doublet_frac=0.3, reads_lambda=1.0)
    prefix = str(tmp_path / "plp")
    plpio.write_plp(prefix, p, seed=5, extra_cells=1)
    vcf = str(tmp_path / "g.vcf.gz")
    plpio.write_vcf(vcf, p, p.truth["G"].astype(np.int64), field="GT", missing_frac=0.02, drop_snps=range(0, S, 37))
    alphas = (0.0, 0.25, 0.5)
    base = ([BIN, "demuxlet", "--plp", prefix, "--vcf", vcf, "--field", "GT"] + [x for a in alphas for x in ("--alpha", str(a))]
            + (["--devices", devices] if devices else []))
    plain, out, capped = (str(tmp_path / n) for n in ("plain", "out", "capped"))
    run(base + ["--out", plain])
    log = run(base + ["--out", out, "--fit-alpha"])
    run(base + ["--out", capped, "--fit-alpha", "--alpha-fit-max", "0.0625"])
    best = open(plain + ".best", "rb").read()
    assert not os.path.exists(plain + ".alphafit.gz")
    assert best == open(out + ".best", "rb").read() == open(capped + ".best", "rb").read()
    # every other output file of the run is the plain run's, byte for byte
    made ={n for n in os.listdir(tmp_path) if n.startswith("out.")} - {"out.alphafit.gz"}
    assert made == {n.replace("plain.", "out.") for n in os.listdir(tmp_path) if n.startswith("plain.")}
    for n in made:
        assert open(str(tmp_path / n), "rb").read() == open(str(tmp_path / n.replace("out.", "plain.")), "rb").read(), n
    got = gzip.open(out + ".alphafit.gz", "rt").read().splitlines()

    d = pyplp.load(prefix, vcf=vcf, field="GT")
    q = as_pileup(d)
    ids = [f"S{v}" for v in range(V)]
    best_rows = [ln.split("\t") for ln in best.decode().splitlines()[1:]]
    index = {bc: i for i, bc in enumerate(d["bcs"])}
    pairs = best_pairs(best_rows, index, ids, q.C)
    with muxgl.Engine(0) as e:
        e.set_pileup(q.S, q.cell_ptr, q.entry_snp, q.entry_rptr, q.reads)
        e.demux_set_gp(q.gp, q.has_gp)
        fit = e.demux_alpha_fit(alphas, pairs, 1.0)
        fit_capped = e.demux_alpha_fit(alphas, pairs, 0.0625)
    assert got[0] == HEADER and len(best_rows) > 0
    want = expected_rows(best_rows, index, ids, fit)
    assert len(want) == 2 * len(best_rows) and got[1:] == want
    assert {r.split("\t")[3] for r in got[1:]} == {"DBL", "SNG"} and "NA" not in {r.split("\t")[7] for r in got[1:]}
    capped_rows = gzip.open(capped + ".alphafit.gz", "rt").read().splitlines()
    assert capped_rows[1:] == expected_rows(best_rows, index, ids, fit_capped)
    assert {r.split("\t")[7] for r in capped_rows[1:]} == {"NA"}                  # SNG2.LLK: ll_top is no singlet below 1
    assert (fit_capped["alpha_hat"] <= 0.0625).all() and (fit_capped["status"] == 2).any()
    assert "NA" in {r.split("\t")[9] for r in capped_rows[1:]}                    # ALPHA.SE on a bound
    # the notice counts the droplets called SNG whose SNG row beats the better singlet by more than 2
    sm_rows = [r.split("\t") for r in got[1:]]
    types = {brow[1]: brow[4] for brow in best_rows}
    n = sum(1 for r in sm_rows if r[3] == "SNG" and types[r[0]] == "SNG"
            and fit["ll_hat"][index[r[0]], 1] > max(fit["ll_zero"][index[r[0]], 1], fit["ll_top"][index[r[0]], 1]) + 2.0)
    assert f"Mixing share: {n} droplets called SNG" in log, log
