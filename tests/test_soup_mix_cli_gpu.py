"""`popscle-amd demuxlet --ambient-mix` on a written planted pool (tests/soup_mix_ref.planted_pool): <out>.soupmix.gz has one
row per component with the shares and gradients of Engine.demux_soup_mix on the loaded pileup, to the printed digits, and
<out>.soupmix.af.gz holds the fitted profile as doubles that read back exactly; fed back through --ambient-af the profile
gives the same .amb.gz bytes as the --ambient-mix run itself; --ambient-mix-unknown adds the UNKNOWN row; the flag is fatal
together with --ambient-af; and a run without the flag writes what a second run without it writes, and no .soupmix file."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import soup_mix_ref as sr
from popscle_amd import muxgl, plpio
from test_cli_gpu import BIN, as_pileup

pytestmark = pytest.mark.gpu


def run(cmd, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stderr


def test_demuxlet_cli_ambient_mix(tmp_path):
    import pyplp

    p, mask, pool, w = sr.planted_pool(C=200, S=1500, seed=8, n_empty=130, cell_markers=120)
    V = p.gp.shape[1]
    prefix, vcf = str(tmp_path / "plp"), str(tmp_path / "g.vcf.gz")
    plpio.write_plp(prefix, p, seed=8)
    G = np.argmax(p.gp, axis=2).astype(np.int64)
    plpio.write_vcf(vcf, p, G, field="GT", drop_snps=range(0, p.S, 41))
    base = [BIN, "demuxlet", "--plp", prefix, "--vcf", vcf, "--field", "GT", "--min-total", "0", "--min-umi", "0", "--min-snp", "0"]
    names = ("plain", "plain2", "mix", "fed", "unk")
    plain, plain2, mix, fed, unk = (str(tmp_path / n) for n in names)
    run(base + ["--out", plain, "--write-ambient", "--ambient-max-reads", "40"])
    run(base + ["--out", plain2, "--write-ambient", "--ambient-max-reads", "40"])
    log = run(base + ["--out", mix, "--write-ambient", "--ambient-max-reads", "40", "--ambient-mix", "--ambient-mix-iter", "60"])
    assert "Ambient mixture:" in log and "60 steps, status 1" in log

    # without the flag: the same files as a second run, and none of the new ones
    for sfx in (".best", ".amb.gz"):
        assert open(plain + sfx, "rb").read() == open(plain2 + sfx, "rb").read()
    assert not os.path.exists(plain + ".soupmix.gz") and not os.path.exists(plain + ".soupmix.af.gz")
    assert open(mix + ".best", "rb").read() == open(plain + ".best", "rb").read()
    assert gzip.open(mix + ".amb.gz", "rb").read() != gzip.open(plain + ".amb.gz", "rb").read()   # another profile

    # the rows, from the library on the pileup the front end loaded
    d = pyplp.load(prefix, vcf=vcf, field="GT")
    q = as_pileup(d)
    few = np.diff(q.entry_rptr[q.cell_ptr]) <= 40
    assert 0 < few.sum() < q.C
    with muxgl.Engine(0) as e:
        e.set_pileup(q.S, q.cell_ptr, q.entry_snp, q.entry_rptr, q.reads)
        e.demux_set_gp(q.gp, q.has_gp)
        got = e.demux_soup_mix(few, n_iter_max=60, tol=1e-8)
        got_u = e.demux_soup_mix(few, with_unknown=True, gp0=sr.hwe_prior(q.af), n_iter_max=60, tol=1e-8)
    assert f"{got['n_reads']} reads" in log
    ids = [f"S{v}" for v in range(V)]

    def rows_of(path, fit, names_):
        lines = gzip.open(path, "rt").read().splitlines()
        assert lines[0] == "SM_ID\tSHARE\tGRAD" and len(lines) == 1 + len(names_)
        for ln, n, s, g in zip(lines[1:], names_, fit["pi"], fit["grad"]):
            assert ln == "%s\t%.6f\t%.6f" % (n, s, g), (ln, n, s, g)

    rows_of(mix + ".soupmix.gz", got, ids)
    af = np.array([float(x) for x in gzip.open(mix + ".soupmix.af.gz", "rt").read().split()])
    assert np.array_equal(af, got["amb_af"])                                 # %.17g: the doubles themselves
    shares = np.array([float(ln.split("\t")[1]) for ln in gzip.open(mix + ".soupmix.gz", "rt").read().splitlines()[1:]])
    assert abs(shares.sum() - 1.0) < 1e-4 and np.argmax(shares) == int(np.argmax(w))

    # the fitted profile through --ambient-af: the same table, byte for byte
    run(base + ["--out", fed, "--write-ambient", "--ambient-af", mix + ".soupmix.af.gz"])
    assert gzip.open(fed + ".amb.gz", "rb").read() == gzip.open(mix + ".amb.gz", "rb").read()

    # the extra component, and the flag that excludes it
    run(base + ["--out", unk, "--ambient-max-reads", "40", "--ambient-mix", "--ambient-mix-iter", "60", "--ambient-mix-unknown"])
    rows_of(unk + ".soupmix.gz", got_u, ids + ["UNKNOWN"])
    err = run(base + ["--out", str(tmp_path / "no"), "--ambient-mix", "--ambient-af", mix + ".soupmix.af.gz"], ok=False)
    assert "--ambient-mix" in err and "--ambient-af" in err
