"""`popscle-amd demuxlet --write-ambient` on a small synthetic pileup: <out>.amb.gz has one row per row of .best, in its
order; its AMB.* columns are muxgl.ambient_summary of the Python call with the same profile, to the printed digits; the
profile made from the pileup's own reads is muxgl.ambient_profile of the device counts and the AF column, so --ambient-af
with a file of that profile gives the same file; --ambient-max-reads builds it from the small droplets; and without the
flag nothing changes: no .amb.gz, and .best is the same bytes with and without it."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import ambient_ref as ar
from popscle_amd import muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup

pytestmark = pytest.mark.gpu

HEADER = ("BARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.LLK\tSNG.BEST.GUESS\tSNG.BEST.LLK\tAMB.GUESS\tAMB.RHO\tAMB.LLK\t"
          "DIFF.LLK.AMB.BEST")
DEFAULT_RHOS = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)
TOL = 0.5e-4 + 1e-9   # the printed digits of %.4lf


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stderr


def check_rows(lines, best_rows, index, ids, ll, rhos):
    sm = muxgl.ambient_summary(ll, rhos)
    assert lines[0] == HEADER and len(lines) == 1 + len(best_rows) and len(best_rows) > 0
    for n, brow in enumerate(best_rows):      # printed droplets in the order of .best
        i = index[brow[1]]
        f = lines[1 + n].split("\t")
        assert len(f) == 11 and f[:4] == brow[1:5] and f[5] == brow[12], (f, brow)
        assert abs(float(f[4]) - float(brow[6])) <= 0.5e-2 + 1e-9 and abs(float(f[6]) - float(brow[13])) <= 0.5e-2 + 1e-9
        assert f[7] == ids[int(sm["amb_sample"][i])] and f[8] == "%.2f" % sm["amb_rho"][i], (f, i)
        assert abs(float(f[9]) - sm["amb_llk"][i]) <= TOL
        assert abs(float(f[10]) - (float(f[9]) - float(f[4]))) <= 2 * TOL


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_demuxlet_cli_write_ambient(tmp_path, devices):
    import pyplp

    V, S = 8, 1200
    p = synth.make_pileup(60, S, V, seed=5, mean_entries=150, min_entries=20, doublet_frac=0.3, reads_lambda=1.0)
    prefix = str(tmp_path / "plp")
    plpio.write_plp(prefix, p, seed=5, extra_cells=1)
    vcf = str(tmp_path / "g.vcf.gz")
    plpio.write_vcf(vcf, p, p.truth["G"].astype(np.int64), field="GT", missing_frac=0.02, drop_snps=range(0, S, 37))
    alphas, rhos3 = (0.0, 0.25, 0.5), (0.0, 0.125, 0.4)
    base = ([BIN, "demuxlet", "--plp", prefix, "--vcf", vcf, "--field", "GT"] + [x for a in alphas for x in ("--alpha", str(a))]
            + (["--devices", devices] if devices else []))
    plain, out, out_af, out_few = (str(tmp_path / n) for n in ("plain", "out", "out_af", "out_few"))
    run(base + ["--out", plain])
    log = run(base + ["--out", out, "--write-ambient"])
    assert "Ambient RNA:" in log and not os.path.exists(plain + ".amb.gz")
    best = open(out + ".best", "rb").read()
    assert best == open(plain + ".best", "rb").read()

    d = pyplp.load(prefix, vcf=vcf, field="GT")
    assert d["nv"] == V
    q = as_pileup(d)
    ids = [f"S{v}" for v in range(V)]
    best_rows = [ln.split("\t") for ln in best.decode().splitlines()[1:]]
    index = {bc: i for i, bc in enumerate(d["bcs"])}
    reads_of_cell = np.diff(q.entry_rptr[q.cell_ptr])
    cut = int(np.median(reads_of_cell))
    few = reads_of_cell <= cut
    with muxgl.Engine(0) as e:
        e.set_pileup(q.S, q.cell_ptr, q.entry_snp, q.entry_rptr, q.reads)
        e.demux_set_gp(q.gp, q.has_gp)
        f_all = muxgl.ambient_profile(*e.pileup_allele_counts(), q.af)
        f_few = muxgl.ambient_profile(*e.pileup_allele_counts(few), q.af)
        ll_all = e.demux_ambient(alphas, f_all, DEFAULT_RHOS)["ll"]
        ll_few = e.demux_ambient(alphas, f_few, rhos3)["ll"]
    assert not np.array_equal(f_all, f_few)
    amb = gzip.open(out + ".amb.gz", "rb").read()
    check_rows(amb.decode().splitlines(), best_rows, index, ids, ll_all, DEFAULT_RHOS)

    # the same profile from a file: the same file
    af_file = str(tmp_path / "amb_af.txt")
    with open(af_file, "w") as fh:
        fh.writelines("%.17g\n" % x for x in f_all)
    run(base + ["--out", out_af, "--write-ambient", "--ambient-af", af_file])
    assert gzip.open(out_af + ".amb.gz", "rb").read() == amb and open(out_af + ".best", "rb").read() == best

    # the profile of the small droplets, on a grid of the caller's
    run(base + ["--out", out_few, "--write-ambient", "--ambient-max-reads", str(cut)] + [x for r in rhos3 for x in ("--ambient-rho", str(r))])
    check_rows(gzip.open(out_few + ".amb.gz", "rt").read().splitlines(), best_rows, index, ids, ll_few, rhos3)
