"""`popscle-amd freemuxlet --fit-alpha` on a small file set: <out>.clust1.alphafit.gz has, per droplet of .clust1.samples.gz and
in its order, one row DBL for the two clusters of DBL.BEST.GUESS and one row SNG for (SNG.BEST.GUESS, SNG.NEXT.GUESS) with the
columns of demuxlet's .alphafit.gz and CLUST1 CLUST2 in place of SM1_ID SM2_ID; the rows are Engine.fmx_alpha_fit of the last
iteration on freemuxlet.call_pairs() through the format strings; the standard error is NA on a bound and SNG2.LLK where
--alpha-fit-max is below 1; and the flag changes nothing else: every other output is byte-equal with and without it, and
there is no .clust1.alphafit.gz without it."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import table_rows
from popscle_amd import freemuxlet, plpio, synth
from test_cli_gpu import BIN, as_pileup
from test_fmx_singlets_gpu import _read, prepared, spread_init

pytestmark = pytest.mark.gpu

HEADER = "BARCODE\tNUM.SNPS\tNUM.READS\tPAIR\tCLUST1\tCLUST2\tSNG1.LLK\tSNG2.LLK\tALPHA.MLE\tALPHA.SE\tMIX.LLK.MLE\tMIX.LRT\tSTATUS"


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stderr


def expected_rows(srows, fit):
    for i, srow in enumerate(srows):
        assert [str(int(c)) for c in fit["pair"][i, 1]] == [srow[12], srow[14]]  # SNG.BEST.GUESS, SNG.NEXT.GUESS
    return table_rows.alpha_fit_rows([(i, srow[1:4]) for i, srow in enumerate(srows)], str, fit, freemuxlet.alpha_fit_summary(fit))


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_freemuxlet_cli_fit_alpha(tmp_path, devices):
    import pyplp

    K = 4
    p = synth.make_pileup(150, 1200, 6, seed=9, mean_entries=200, min_entries=30, with_gp=False)   # more donors than clusters
    prefix = str(tmp_path / "plp")
    plpio.write_plp(prefix, p, seed=9)
    d = pyplp.load(prefix)
    q = as_pileup(d)
    init = spread_init(q.C, K)
    initf = str(tmp_path / "init.txt")
    with open(initf, "w") as f:
        for i, bc in enumerate(d["bcs"]):
            f.write(f"{bc}\t{int(init[i])}\n")
    base = [BIN, "freemuxlet", "--plp", prefix, "--nsample", str(K), "--init-cluster", initf] + \
           (["--devices", devices] if devices else [])
    plain, out, capped = (str(tmp_path / n) for n in ("plain", "out", "capped"))
    run(base + ["--out", plain])
    err = run(base + ["--out", out, "--fit-alpha"])
    run(base + ["--out", capped, "--fit-alpha", "--alpha-fit-max", "0.0625"])
    assert "Mixing share: " in err and "droplets called SNG" in err
    assert not os.path.exists(plain + ".clust1.alphafit.gz")
    for suffix in (".lmix", ".clust1.samples.gz", ".clust1.vcf.gz"):              # every other output: byte-equal
        assert _read(plain + suffix) == _read(out + suffix) == _read(capped + suffix), suffix
    names = lambda pre: sorted(n[len(os.path.basename(pre)):] for n in os.listdir(tmp_path) if n.startswith(os.path.basename(pre) + "."))
    assert [n for n in names(out) if n != ".clust1.alphafit.gz"] == names(plain)
    got = gzip.open(out + ".clust1.alphafit.gz", "rt").read().splitlines()

    with gzip.open(out + ".clust1.samples.gz", "rt") as f:
        srows = [ln.rstrip("\n").split("\t") for ln in f.readlines()[1:]]
    assert len(srows) == q.C and [r[1] for r in srows] == list(d["bcs"])
    with prepared(q) as e:                                                        # the same job through the library
        recs, hist = freemuxlet.run_em(e, K, init)
        pair = freemuxlet.call_pairs(recs)
        assert (pair >= 0).all() and (pair < K).all()
        fit = e.fmx_alpha_fit(pair, 1.0)                                          # behind the last iteration, as the front end
        fit_capped = e.fmx_alpha_fit(pair, 0.0625)
    assert got[0] == HEADER and len(got) == 1 + 2 * q.C
    assert got[1:] == expected_rows(srows, fit)
    assert [r.split("\t")[3] for r in got[1:3]] == ["DBL", "SNG"]
    capped_rows = gzip.open(capped + ".clust1.alphafit.gz", "rt").read().splitlines()
    assert capped_rows[0] == HEADER and capped_rows[1:] == expected_rows(srows, fit_capped)
    on_bound = [r.split("\t") for r in capped_rows[1:] if r.split("\t")[12] in ("1", "2")]
    assert (fit_capped["alpha_hat"] <= 0.0625).all() and on_bound and all(r[9] == "NA" for r in on_bound)   # no standard error on a bound
    assert all(r.split("\t")[7] == "NA" for r in capped_rows[1:]) and all(r.split("\t")[7] != "NA" for r in got[1:])
    assert any(r.split("\t")[9] != "NA" for r in got[1:])
    sm = freemuxlet.alpha_fit_summary(fit)
    mixed = int(((recs["type"] == 0) & (fit["ll_hat"][:, 1] > np.maximum(fit["ll_zero"][:, 1], fit["ll_top"][:, 1]) + 2.0)).sum())
    assert f"Mixing share: {mixed} droplets" in err and sm["lrt"].shape == (q.C, 2)
