"""`popscle-amd freemuxlet --write-unknown`: <out>.clust1.unk.gz has one row per droplet of .clust1.samples.gz, in its
order, and its rows are freemuxlet.unknown_summary on the tables Engine.fmx_unknown gives for the same job, to the printed
digits (the tables are bit-identical on one device and on a group, so the digits are compared as strings); every other
output is byte-equal to a run without the flag; one notice line counts the droplets a donor outside the clusters explains
better by more than 2."""
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

HEADER = "BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.LLK\tHALF.CLUST\tHALF.LLK\tDIFF.LLK.CLUST.UNK"


def _fmt(v):
    return "%.4f" % v   # (C's %.4lf: both round the exact binary value; -inf prints as "-inf" in both)


@pytest.mark.parametrize("K,devices", [(4, None), (300, None), (4, "0,0")])
def test_freemuxlet_cli_write_unknown(tmp_path, K, devices):
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
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = [BIN, "freemuxlet", "--plp", prefix, "--nsample", str(K), "--init-cluster", initf] + \
           (["--devices", devices] if devices else [])
    logs = []
    for cmd in (base + ["--out", plain], base + ["--out", out, "--write-unknown"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
        logs.append(r.stdout + r.stderr)
    assert not os.path.exists(plain + ".clust1.unk.gz")
    for suffix in (".lmix", ".clust1.samples.gz", ".clust1.vcf.gz"):   # every other output: byte-equal
        assert _read(out + suffix) == _read(plain + suffix), suffix
    made = sorted(os.path.basename(x)[len("out"):] for x in os.listdir(tmp_path) if os.path.basename(x).startswith("out."))
    assert made == sorted([".lmix", ".clust1.samples.gz", ".clust1.vcf.gz", ".clust1.unk.gz"])

    with prepared(q) as e:   # the same job through the library
        recs, hist, unk = freemuxlet.run_em(e, K, init, want_unknown=True)
    s = freemuxlet.unknown_summary(unk, recs["bestLLK"])
    with gzip.open(out + ".clust1.samples.gz", "rt") as f:
        srows = [ln.rstrip("\n").split("\t") for ln in f.readlines()[1:]]
    lines = gzip.open(out + ".clust1.unk.gz", "rt").read().splitlines()
    assert lines[0] == HEADER
    assert len(srows) == q.C and len(lines) == 1 + q.C
    for i, srow in enumerate(srows):       # droplets in the order of .clust1.samples.gz
        want = [srow[1], srow[2], srow[3], _fmt(recs["bestLLK"][i]), _fmt(unk["ll_u"][i]), _fmt(unk["ll_uu"][i]),
                str(int(s["half_clust"][i])), _fmt(s["half_llk"][i]), _fmt(s["diff"][i])]
        assert srow[1] == d["bcs"][i] and lines[1 + i].split("\t") == want, (i, lines[1 + i], want)
    m = [ln for ln in logs[1].splitlines() if "donor that no cluster holds" in ln]
    assert len(m) == 1 and "--nsample" in m[0], logs[1][-2000:]
    assert int(re.search(r"(\d+) of (\d+) droplets", m[0]).group(1)) == s["n_better"]
    assert int(re.search(r"(\d+) of (\d+) droplets", m[0]).group(2)) == q.C
    assert not any("donor that no cluster holds" in ln for ln in logs[0].splitlines())
    print(f"CLI K={K} devices={devices}: {s['n_better']} of {q.C} droplets better explained by an unknown donor")
