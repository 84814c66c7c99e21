"""GPU tests of the streamed demuxlet call (demux_stream.hip): more than 255 samples, MUXGL_FLAG_FORCE_STREAMED_CALL
against the existing paths, the slab budget (MUXGL_DEMUX_SLAB_MB), device groups, the sharded driver, the CLI, and the
refusal of full_ll on the streamed path.

Bar as everywhere (tests/parity.py): integer fields equal to the reference's after the exact-call pass, log-likelihoods
within LL_TOL.
"""
import os
import subprocess

import numpy as np
import pytest

import many_samples
import oracle_binding as ob
import parity
import ref_binding as rb
from popscle_amd import demuxlet, muxgl, plpio
from test_cli_gpu import BIN, TYPES, as_pileup, assert_rows_match

pytestmark = pytest.mark.gpu

G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
G03 = (0.0, 0.3)  # no symmetric alpha


def reference(p, alphas):
    """the reference's own demuxlet loop where it was built (oracle/_ref), else the oracle (bit-identical to it)"""
    if rb.available():
        return rb.RefScl.from_packed(p).demux(alphas, doublet_prior=0.5)[0]
    return ob.demux(p, alphas=alphas, nthreads=8)


def run(p, alphas, flags=0, devs=0):
    with muxgl.Engine(devs, flags) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        return e.demux_run(alphas, 0.5)


def small(V, seed, C=24, S=2000, mean_entries=50):
    return many_samples.pileup(C, S, V, seed=seed, mean_entries=mean_entries)


@pytest.mark.parametrize("V,alphas", [(256, G2), (256, G6), (256, G03), (300, G2), (300, G6), (300, G03), (513, G2),
                                      (513, G03), (700, G2)])
def test_against_the_reference(V, alphas):
    p = small(V, seed=400 + V, C=24 if V < 500 else 12)
    got = run(p, alphas)
    want = reference(p, alphas)
    rep = parity.compare_demux(got, want, alphas, p)
    assert rep["cells"] == p.C
    assert max(got["sBest"].max(), got["dBest1"].max(), got["dBest2"].max()) > 255 or V < 300


def test_ties_and_deep_bits_occur():
    """the duplicated samples of many_samples.pileup make the DEEP bits fire, and the exact pass settles them"""
    p = small(300, seed=777)
    got = run(p, G2)
    assert ((got["valid"] & (muxgl.CELL_DEEP_SNG | muxgl.CELL_DEEP_DBL)) != 0).any()
    rep = parity.compare_demux(got, reference(p, G2), G2, p)
    assert rep["exact_pass"]["deep"] > 0


def _same_after_exact(a, b, alphas, p, doublet_prior=0.5):
    ea, eb = parity.exact(a, alphas, p, doublet_prior), parity.exact(b, alphas, p, doublet_prior)
    for f in parity.DEMUX_INT_FIELDS:
        assert np.array_equal(ea[f], eb[f]), (f, np.flatnonzero(ea[f] != eb[f])[:5])
    for f in parity.DEMUX_LL_FIELDS:
        assert np.all(parity._close(ea[f], eb[f], parity.LL_TOL)), f


@pytest.mark.parametrize("V,alphas", [(40, G6), (64, G2), (130, G6), (200, G03), (255, G2)])
def test_forced_streamed_equals_existing_path(V, alphas):
    p = small(V, seed=500 + V, C=40, mean_entries=80)
    want = run(p, alphas)
    got = run(p, alphas, muxgl.FLAG_FORCE_STREAMED_CALL)
    _same_after_exact(got, want, alphas, p)


@pytest.mark.parametrize("V,alphas", [(300, G6), (130, G03)])
def test_budget_does_not_matter(monkeypatch, V, alphas):
    p = small(V, seed=600 + V, C=30)
    flags = muxgl.FLAG_FORCE_STREAMED_CALL
    monkeypatch.delenv("MUXGL_DEMUX_SLAB_MB", raising=False)
    one = run(p, alphas, flags)  # default budget: one group
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")  # a few cells x one block per group
    many = run(p, alphas, flags)
    assert one.tobytes() == many.tobytes()  # raw device records, before any exact pass


def test_device_group_and_sharded_driver():
    V, alphas = 300, G6
    p = small(V, seed=901, C=30)
    want = run(p, alphas)
    got = run(p, alphas, muxgl.FLAG_DEMUX_ONLY, devs=[0, 0])
    assert got.tobytes() == want.tobytes()
    sharded = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5)
    assert sharded.tobytes() == want.tobytes()


def test_full_ll_refused_on_streamed_path():
    p = small(300, seed=902, C=6)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        with pytest.raises(muxgl.MuxglError, match="full_ll"):
            e.demux_run(G2, 0.5, want_full_ll=True)
        ok = e.demux_run(G2, 0.5)  # the handle is still usable
        assert (ok["valid"] & 1).sum() == p.C


def test_demuxlet_cli_300_samples(tmp_path):
    import pyplp

    V = 300
    p = many_samples.pileup(30, 1200, V, seed=5, mean_entries=60)
    prefix = str(tmp_path / "plp")
    plpio.write_plp(prefix, p, seed=5, extra_cells=1)
    vcf = str(tmp_path / "g.vcf.gz")
    G = p.truth["G"].astype(np.int64)
    plpio.write_vcf(vcf, p, G, field="GT", missing_frac=0.02, drop_snps=range(0, 1200, 37))
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, "demuxlet", "--plp", prefix, "--vcf", vcf, "--field", "GT", "--out", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    d = pyplp.load(prefix, vcf=vcf, field="GT")
    assert d["nv"] == V
    q = as_pileup(d)
    al = G2
    cells = reference(q, al)
    ids = [f"S{v}" for v in range(V)]
    want = ["INT_ID\tBARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.GUESS\tBEST.LLK\tNEXT.GUESS\tNEXT.LLK\t"
            "DIFF.LLK.BEST.NEXT\tBEST.POSTERIOR\tSNG.POSTERIOR\tSNG.BEST.GUESS\tSNG.BEST.LLK\tSNG.NEXT.GUESS\t"
            "SNG.NEXT.LLK\tSNG.ONLY.POSTERIOR\tDBL.BEST.GUESS\tDBL.BEST.LLK\tDIFF.LLK.SNG.DBL\n"]
    order = sorted(range(d["C"]), key=lambda i: d["bcs"][i].encode())
    for rank, i in enumerate(order):
        c = cells[i]
        if not c["valid"]:
            continue
        want.append("%d\t%s\t%u\t%d\t%s\t%s,%s,%.2f\t%.2f\t%s,%s,%.2f\t%.2f\t%.2f\t%.2g\t%.2g\t%s\t%.2f\t%s\t%.2f\t%.5f\t"
                    "%s,%s,%.2f\t%.2f\t%.2f\n" % (
                        rank, d["bcs"][i], c["nsnps"], d["cell_uniq_reads"][i], TYPES[int(c["type"])],
                        ids[c["jBest"]], ids[c["kBest"]], al[c["aBest"]], c["bestLLK"], ids[c["jNext"]], ids[c["kNext"]],
                        al[c["aNext"]], c["nextLLK"], c["bestLLK"] - c["nextLLK"], c["bestPP"], c["sngPP"],
                        ids[c["sBest"]], c["sngBestLLK"], ids[c["sNext"]], c["sngNextLLK"], c["sngOnlyPP"],
                        ids[c["dBest1"]], ids[c["dBest2"]], al[c["dBestA"]], c["dblBestLLK"],
                        c["sngBestLLK"] - c["dblBestLLK"]))
    got = open(out + ".best").readlines()
    assert_rows_match(got, want)
    assert len(got) == 1 + int((cells["valid"] == 1).sum())
