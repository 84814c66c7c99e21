"""`popscle-amd freemuxlet --write-ambient`: <out>.clust1.amb.gz has one row per droplet of .clust1.samples.gz, in its
order, and its rows are freemuxlet.ambient_summary on the table Engine.fmx_ambient gives for the same job and the same
profile, field by field to the printed digits (the table is bit-identical on one device and on a group, so the digits
are compared as strings); every other output is byte-equal to a run without the flag; one notice line counts the droplets
called DBL that one cell plus ambient RNA explains better by more than 2 than their best doublet.  The three ways to the
profile: the pileup's own reads, those of the droplets with at most N reads, a file."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from popscle_amd import freemuxlet, muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup
from test_fmx_singlets_gpu import _read, prepared, spread_init

pytestmark = pytest.mark.gpu

HEADER = ("BARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.LLK\tSNG.BEST.GUESS\tSNG.BEST.LLK\tAMB.GUESS\tAMB.RHO\tAMB.LLK\t"
          "DIFF.LLK.AMB.BEST")
DEFAULT_RHOS = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)
TYPES = ("SNG", "DBL", "AMB")


def _fmt(v):
    return "%.4f" % v   # (C's %.4lf: both round the exact binary value)


@pytest.mark.parametrize("K,devices,how", [(4, None, "own"), (4, "0,0", "few"), (300, None, "file")])
def test_freemuxlet_cli_write_ambient(tmp_path, K, devices, how):
    import pyplp

    if K == 300:
        p = synth.make_pileup(40, 1200, 24, seed=9, mean_entries=100, min_entries=20, max_entries=300, reads_lambda=0.8,
                              with_gp=False)
    else:
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
    rhos, extra = DEFAULT_RHOS, []
    if how == "few":
        rhos = (0.0, 0.25, 0.5, 1.0)
        extra = [x for r in rhos for x in ("--ambient-rho", repr(r))]
    af_file = None
    if how == "file":
        af_file = np.random.default_rng(4).random(q.S)
        af_file[::7] = 0.0
        af_file[3::7] = 1.0
        with open(str(tmp_path / "amb_af.txt"), "w") as f:
            f.write("".join(repr(float(x)) + "\n" for x in af_file))
        extra = ["--ambient-af", str(tmp_path / "amb_af.txt")]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = [BIN, "freemuxlet", "--plp", prefix, "--nsample", str(K), "--init-cluster", initf] + \
           (["--devices", devices] if devices else [])
    r = subprocess.run(base + ["--out", plain], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    log0 = r.stdout + r.stderr
    with gzip.open(plain + ".clust1.samples.gz", "rt") as f:
        nreads = np.array([int(ln.split("\t")[3]) for ln in f.readlines()[1:]])
    max_reads = int(np.median(nreads))
    if how == "few":
        extra += ["--ambient-max-reads", str(max_reads)]
    r = subprocess.run(base + ["--out", out, "--write-ambient"] + extra, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    log1 = r.stdout + r.stderr
    assert not os.path.exists(plain + ".clust1.amb.gz")
    for suffix in (".lmix", ".clust1.samples.gz", ".clust1.vcf.gz"):   # every other output: byte-equal
        assert _read(out + suffix) == _read(plain + suffix), suffix
    made = sorted(os.path.basename(x)[len("out"):] for x in os.listdir(tmp_path) if os.path.basename(x).startswith("out."))
    assert made == sorted([".lmix", ".clust1.samples.gz", ".clust1.vcf.gz", ".clust1.amb.gz"])

    with prepared(q) as e:   # the same job through the library
        if how == "file":
            prof = af_file
        else:
            mask = None
            if how == "few":
                mask = nreads <= max_reads
                assert 0 < mask.sum() < q.C
            prof = muxgl.ambient_profile(*e.pileup_allele_counts(mask), q.af)
        recs, hist, amb = freemuxlet.run_em(e, K, init, want_ambient=(prof, rhos))
    s = freemuxlet.ambient_summary(amb, rhos)
    with gzip.open(out + ".clust1.samples.gz", "rt") as f:
        srows = [ln.rstrip("\n").split("\t") for ln in f.readlines()[1:]]
    lines = gzip.open(out + ".clust1.amb.gz", "rt").read().splitlines()
    assert lines[0] == HEADER
    assert len(srows) == q.C and len(lines) == 1 + q.C
    for i, srow in enumerate(srows):       # droplets in the order of .clust1.samples.gz
        want = [srow[1], srow[2], srow[3], TYPES[int(recs["type"][i])], _fmt(recs["bestLLK"][i]), str(int(recs["sBest"][i])),
                _fmt(recs["sngBestLLK"][i]), str(int(s["amb_clust"][i])), "%.2f" % s["amb_rho"][i], _fmt(s["amb_llk"][i]),
                _fmt(s["amb_llk"][i] - recs["bestLLK"][i])]
        assert srow[1] == d["bcs"][i] and srow[4] == want[3] and lines[1 + i].split("\t") == want, (i, lines[1 + i], want)
    rescued = int(((recs["type"] == 1) & (s["amb_llk"] > recs["dblBestLLK"] + 2.0)).sum())
    m = [ln for ln in log1.splitlines() if "Ambient RNA:" in ln]
    assert len(m) == 1 and int(re.search(r"Ambient RNA: (\d+) droplets called DBL", m[0]).group(1)) == rescued, log1[-2000:]
    assert not any("Ambient RNA:" in ln for ln in log0.splitlines())
    few = [ln for ln in log1.splitlines() if "Ambient profile from the" in ln]
    assert len(few) == (1 if how == "few" else 0)
    print(f"CLI K={K} devices={devices} profile {how}: {rescued} droplets called DBL better explained by ambient RNA; "
          f"best rho histogram {np.bincount(s['amb_rho_idx'], minlength=len(rhos)).tolist()}")
