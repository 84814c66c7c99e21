"""`popscle-amd freemuxlet --fit-ambient` on a small file set: <out>.clust1.ambfit.gz has, per droplet of .clust1.samples.gz and
in its order, one row for SNG.BEST.GUESS and one for SNG.NEXT.GUESS with the columns of demuxlet's .ambfit.gz and CLUST in
place of SM_ID; the rows are Engine.fmx_ambient_fit of the last iteration with the same profile and candidates through the
format strings; the standard error is NA on a bound; --ambient-fit-max sets the upper bound; and the flag changes nothing
else: every other output is byte-equal with and without it, and there is no .clust1.ambfit.gz without it."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import table_rows
from popscle_amd import freemuxlet, muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup
from test_fmx_singlets_gpu import _read, prepared, spread_init

pytestmark = pytest.mark.gpu

HEADER = "BARCODE\tNUM.SNPS\tNUM.READS\tCLUST\tSNG.LLK\tAMB.RHO.MLE\tAMB.RHO.SE\tAMB.LLK.MLE\tAMB.LRT\tSTATUS"


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stderr


def expected_rows(srows, fit, cand):
    for i, srow in enumerate(srows):
        assert [str(int(c)) for c in cand[i]] == [srow[12], srow[14]]            # SNG.BEST.GUESS, SNG.NEXT.GUESS
    return table_rows.ambient_fit_rows([(i, srow[1:4]) for i, srow in enumerate(srows)], str, cand, fit,
                                       freemuxlet.ambient_fit_summary(fit))


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_freemuxlet_cli_fit_ambient(tmp_path, devices):
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
    plain, out, both, capped = (str(tmp_path / n) for n in ("plain", "out", "both", "capped"))
    run(base + ["--out", plain, "--write-ambient"])
    run(base + ["--out", out, "--fit-ambient"])
    run(base + ["--out", both, "--write-ambient", "--fit-ambient"])
    run(base + ["--out", capped, "--fit-ambient", "--ambient-fit-max", "0.0625"])
    assert not os.path.exists(plain + ".clust1.ambfit.gz") and not os.path.exists(out + ".clust1.amb.gz")
    for suffix in (".lmix", ".clust1.samples.gz", ".clust1.vcf.gz"):              # every other output: byte-equal
        assert _read(plain + suffix) == _read(out + suffix) == _read(both + suffix) == _read(capped + suffix), suffix
    assert _read(plain + ".clust1.amb.gz") == _read(both + ".clust1.amb.gz")
    got = gzip.open(out + ".clust1.ambfit.gz", "rt").read().splitlines()
    assert got == gzip.open(both + ".clust1.ambfit.gz", "rt").read().splitlines()

    with gzip.open(out + ".clust1.samples.gz", "rt") as f:
        srows = [ln.rstrip("\n").split("\t") for ln in f.readlines()[1:]]
    assert len(srows) == q.C and [r[1] for r in srows] == list(d["bcs"])
    with prepared(q) as e:                                                        # the same job through the library
        prof = muxgl.ambient_profile(*e.pileup_allele_counts(), q.af)
        recs, hist = freemuxlet.run_em(e, K, init)
        cand = np.stack([recs["sBest"], recs["sNext"]], axis=1).astype(np.int32)
        assert (cand >= 0).all() and (cand < K).all()
        fit = e.fmx_ambient_fit(prof, cand, 0.5)                                  # behind the last iteration, as the front end
        fit_capped = e.fmx_ambient_fit(prof, cand, 0.0625)
    assert got[0] == HEADER and len(got) == 1 + 2 * q.C
    assert got[1:] == expected_rows(srows, fit, cand)
    capped_rows = gzip.open(capped + ".clust1.ambfit.gz", "rt").read().splitlines()
    assert capped_rows[0] == HEADER and capped_rows[1:] == expected_rows(srows, fit_capped, cand)
    on_bound = [r.split("\t") for r in capped_rows[1:] if r.split("\t")[9] in ("1", "2")]
    assert (fit_capped["rho_hat"] <= 0.0625).all() and (fit_capped["status"] == 2).any()
    assert on_bound and all(r[6] == "NA" for r in on_bound)                       # no standard error on a bound
    assert any(r.split("\t")[6] != "NA" for r in got[1:])
