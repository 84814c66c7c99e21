"""GPU tests of muxgl_demux_singlets (demux_singlets.hip): the [C][V] table of singlet log-likelihoods, llksAB[(j, 0, 0)] of
cmd_cram_demuxlet.cpp:733-747 for every droplet and sample, against the reference (its own loop where oracle/_ref is
built, else the oracle, bit-identical to it), against the records of the same handle on every path, bit for bit across
calls, budgets, device groups and the sharded driver, its error paths, and `popscle-amd demuxlet --write-singlets`.

Bar: parity.LL_TOL (1e-5 absolute) on every element; the observed deviation is ~1e-11.
"""
import ctypes
import gzip
import subprocess

import numpy as np
import pytest

import many_samples
import oracle_binding as ob
import parity
import ref_binding as rb
from popscle_amd import demuxlet, muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup
from test_demux_gpu import _truncate_cells, _with_empty_cells

pytestmark = pytest.mark.gpu

G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)


def reference_table(p, alphas):
    """full_ll[:, :, 0, 0] of the reference's own demuxlet loop where it was built, else of the oracle"""
    if rb.available():
        return rb.RefScl.from_packed(p).demux(alphas, doublet_prior=0.5, full_ll=True)[2][:, :, 0, 0]
    return ob.demux(p, alphas=alphas, full_ll=True, nthreads=8)[1][:, :, 0, 0]


def load(e, p):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)


def singlets(p, alphas, flags=0, devs=0):
    with muxgl.Engine(devs, flags) as e:
        load(e, p)
        return e.demux_singlets(alphas)


def assert_table(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.float64
    ok = parity._close(got, want, parity.LL_TOL)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
    d = d[np.isfinite(d)]
    worst = float(d.max()) if d.size else 0.0
    print(f"singlets {what}: {got.shape[0]} x {got.shape[1]}, max |dLL| = {worst:.3e}")
    assert ok.all(), f"{int((~ok).sum())} elements beyond {parity.LL_TOL}; worst {worst}"
    return worst


# ---- 1. against the reference, V <= 255 -------------------------------------------------------------------------------

@pytest.mark.parametrize("V,alphas,C,S,ment", [
    (1, G2, 20, 500, 100),
    (2, G2, 80, 1000, 200),
    (4, G2, 200, 2000, 300),
    (4, G6, 120, 2000, 300),
    (16, G2, 150, 5000, 600),
    (16, G6, 60, 5000, 600),
    (17, G2, 30, 3000, 400),
    (25, (0.2, 0.5), 24, 3000, 300),   # the slot is (j, 0, 0) whatever alpha[0] is: here a doublet of j with sample 0
    (32, G2, 24, 4000, 700),
    (33, G2, 30, 4000, 400),
    (64, G6, 12, 6000, 500),
    (64, G6, 6, 9000, 3000),           # cells walked in parts
    (65, G2, 10, 6000, 1500),
    (130, G2, 6, 8000, 2500),
    (200, G2, 4, 6000, 1200),
])
def test_random_vs_reference(V, alphas, C, S, ment):
    """the shapes of test_demux_gpu.py::test_random_vs_oracle (same seeds), 3 % of the markers without genotypes"""
    p = synth.make_pileup(C, S, V, seed=1000 + V * 7 + len(alphas), mean_entries=ment, min_entries=20,
                          missing_gp_frac=0.03)
    assert (p.has_gp == 0).any()
    assert_table(singlets(p, alphas), reference_table(p, alphas), f"V={V} A={len(alphas)}")


@pytest.mark.parametrize("V", [4, 16, 20, 28, 40])
def test_deep_pileups(V):
    p = synth.make_pileup(30, 600, V, seed=3000 + V, mean_entries=80, min_entries=10, reads_lambda=60.0, min_bq=2,
                          max_bq=93, cap_bq=127, other=0.03)
    assert np.diff(p.entry_rptr).max() > 80
    for alphas in [(0.0, 0.3, 0.5), G2]:
        assert_table(singlets(p, alphas), reference_table(p, alphas), f"deep V={V}")


@pytest.mark.parametrize("V", [5, 40, 100])
def test_empty_droplets_long_and_short_cells(V):
    base = synth.make_pileup(40, 9000, V, seed=5100 + V, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000,
                             missing_gp_frac=0.04)
    p = _with_empty_cells(_truncate_cells(base, {3: 1, 11: 2, 20: 7}), [0, 7, 39])
    lens = np.diff(p.cell_ptr)
    assert (lens == 0).sum() == 3 and lens.max() > 2048
    got = singlets(p, G6)
    assert_table(got, reference_table(p, G6), f"ragged V={V}")
    assert np.all(got[lens == 0] == 0.0)  # a droplet without entries: a row of zeros


def test_no_marker_has_genotypes():
    p = synth.make_pileup(20, 500, 12, seed=9, mean_entries=100, min_entries=10)
    p.has_gp = np.zeros_like(p.has_gp)
    got = singlets(p, G2)
    assert np.all(got == 0.0)
    assert_table(got, reference_table(p, G2), "no genotypes")


def test_zero_cells():
    p = synth.make_pileup(10, 300, 3, seed=8, mean_entries=50, min_entries=10)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8))
        e.demux_set_gp(p.gp, p.has_gp)
        assert e.demux_singlets(G2).shape == (0, 3)


# ---- 2. against the reference, V > 255: the value of sample j reads only columns 0 and j of gp ------------------------

@pytest.mark.parametrize("V,alphas", [(256, G2), (300, G6), (513, (0.2, 0.5)), (700, G2), (1024, G2)])
def test_many_samples_vs_reference_on_column_pairs(V, alphas):
    """the reference on the sub-tensors gp[:, [0] + chunk, :], chunks of 63 columns that together cover every sample
    (tests/test_demux_singlets.py restates the property the comparison rests on)"""
    p = many_samples.pileup(24 if V < 500 else 12, 2000, V, seed=400 + V, mean_entries=50)
    got = singlets(p, alphas)
    seen = np.zeros(V, dtype=bool)
    worst = 0.0
    for b in range(1, V, 63):
        cols = [0] + list(range(b, min(V, b + 63)))
        sub = synth.Pileup(p.C, p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads, p.af,
                           np.ascontiguousarray(p.gp[:, cols, :]), p.has_gp)
        worst = max(worst, assert_table(got[:, cols], reference_table(sub, alphas), f"V={V} columns {cols[1]}..{cols[-1]}"))
        seen[cols] = True
    assert seen.all()


# ---- 3. consistent with the records of the same handle, on every path ------------------------------------------------

@pytest.mark.parametrize("V,alphas,flags", [
    (8, G2, 0), (8, G6, muxgl.FLAG_FORCE_ROW_KERNEL), (16, G2, muxgl.FLAG_FORCE_WAVE_KERNEL),
    (16, G6, muxgl.FLAG_FORCE_TILE_SWEEP), (24, G2, 0), (24, G2, muxgl.FLAG_FORCE_ROW_KERNEL),
    (24, G6, muxgl.FLAG_FORCE_WAVE_KERNEL), (40, G6, 0), (40, G2, muxgl.FLAG_FORCE_TILE_SWEEP),
    (40, G6, muxgl.FLAG_FORCE_STREAMED_CALL), (100, (0.0, 0.3), 0), (130, G2, muxgl.FLAG_FORCE_STREAMED_CALL),
    (300, G2, 0), (300, G6, 0), (513, (0.0, 0.3), 0)])
def test_consistent_with_the_records(V, alphas, flags):
    dp = 0.5
    p = many_samples.pileup(30, 2000, V, seed=700 + V + len(alphas), mean_entries=80)
    with muxgl.Engine(0, flags) as e:
        load(e, p)
        raw = e.demux_run(alphas, dp)
        sng = e.demux_singlets(alphas)
    rec = parity.exact(raw, alphas, p, dp)
    valid = (rec["valid"] & 1) == 1
    assert valid.all()
    c = np.arange(p.C)
    tol = parity.LL_TOL
    assert np.all(parity._close(sng[c, rec["sBest"]], rec["sngBestLLK"], tol))
    assert np.all(parity._close(sng[c, rec["sNext"]], rec["sngNextLLK"], tol))
    assert np.all(sng.max(axis=1) - sng[c, rec["sBest"]] <= tol)
    # the reference's evidence chain restated on the table (it starts at -1e-300, sic, :791)
    chain = np.logaddexp(-1e-300, np.logaddexp.reduce(sng + np.log((1.0 - dp) / V), axis=1))
    print(f"V={V}: max |sngLLK - chain| = {np.max(np.abs(rec['sngLLK'] - chain)):.3e}")
    assert np.all(parity._close(rec["sngLLK"], chain, tol))


# ---- 4. bit-identical -------------------------------------------------------------------------------------------------

def _long_cells_pileup(V, seed, C=40):
    p = synth.make_pileup(C, 9000, V, seed=seed, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000,
                          missing_gp_frac=0.04)
    assert np.diff(p.cell_ptr).max() > 2048
    return p


def test_two_calls_on_one_handle():
    p = _long_cells_pileup(48, 4100)
    with muxgl.Engine(0) as e:
        load(e, p)
        a = e.demux_singlets(G6)
        assert e.timing()[muxgl.T_DEMUX_SINGLETS] > 0.0
        b = e.demux_singlets(G6)
    assert a.tobytes() == b.tobytes()


def test_budget_does_not_matter(monkeypatch):
    V = 300
    p = many_samples.pileup(1600, 6000, V, seed=611, mean_entries=150, sigma=1.2, min_entries=1, max_entries=5000)
    lens = np.diff(p.cell_ptr)
    rows = int(np.maximum(1, -(-lens // 2048)).sum())
    assert lens.max() > 2048 and rows * V * 8 > 3 * (1 << 20)  # several batches at 1 MB, cells in parts among them
    monkeypatch.delenv("MUXGL_DEMUX_SLAB_MB", raising=False)
    one = singlets(p, G6)
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
    many = singlets(p, G6)
    assert one.tobytes() == many.tobytes()


@pytest.mark.parametrize("V", [20, 300])
def test_device_group_and_sharded_driver(V):
    alphas = G6
    p = _long_cells_pileup(V, 4200 + V, C=30)
    want = singlets(p, alphas)
    assert singlets(p, alphas, muxgl.FLAG_DEMUX_ONLY, devs=[0, 0]).tobytes() == want.tobytes()
    assert singlets(p, alphas, muxgl.FLAG_DEMUX_ONLY, devs=[0, 0, 0]).tobytes() == want.tobytes()
    with muxgl.Engine(0) as e:
        load(e, p)
        records = e.demux_run(alphas, 0.5)
    rec, sng = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5, want_singlets=True)
    assert sng.tobytes() == want.tobytes() and rec.tobytes() == records.tobytes()
    assert demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5).tobytes() == records.tobytes()


@pytest.mark.parametrize("V,flags", [(40, 0), (40, muxgl.FLAG_FORCE_STREAMED_CALL), (12, 0), (300, 0)])
def test_the_call_leaves_the_demuxlet_state_alone(V, flags):
    p = many_samples.pileup(30, 2000, V, seed=800 + V, mean_entries=80)
    with muxgl.Engine(0, flags) as e:
        load(e, p)
        r0 = e.demux_run(G6, 0.5)
        s0 = e.demux_singlets(G6)
        view = e.demux_results_view().tobytes()
        r1 = e.demux_run(G6, 0.5)
        s1 = e.demux_singlets(G6)
        assert e.demux_results_view().tobytes() == view
        other = e.demux_singlets(G2)   # another grid between two runs
        r2 = e.demux_run(G6, 0.5)
    assert r0.tobytes() == r1.tobytes() == r2.tobytes() == view
    assert s0.tobytes() == s1.tobytes()
    assert not np.array_equal(other, s0)  # the normalisation is over the whole grid


# ---- 5. errors ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_error_paths(devs):
    p = synth.make_pileup(12, 300, 5, seed=1, mean_entries=40, min_entries=5)
    with muxgl.Engine(devs, muxgl.FLAG_DEMUX_ONLY) as e:
        with pytest.raises(muxgl.MuxglError, match="pileup"):
            e.demux_singlets(G2)
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        with pytest.raises(muxgl.MuxglError, match="GP tensor"):
            e.demux_singlets(G2)
        e.demux_set_gp(p.gp, p.has_gp)
        with pytest.raises(muxgl.MuxglError, match="n_alpha"):
            e.demux_singlets(())
        dp = muxgl._DemuxParams()
        dp.n_alpha = 2
        dp.alpha[1] = 0.5
        dp.doublet_prior = 0.5
        assert e.lib.muxgl_demux_singlets(e.h, ctypes.byref(dp), None) != 0
        assert b"NULL output" in e.lib.muxgl_last_error(e.h)
        dp.n_alpha = muxgl.MAX_ALPHA + 1
        out = np.zeros((p.C, 5))
        assert e.lib.muxgl_demux_singlets(e.h, ctypes.byref(dp), out.ctypes.data_as(ctypes.c_void_p)) != 0
        assert b"n_alpha" in e.lib.muxgl_last_error(e.h)
        assert_table(e.demux_singlets(G2), reference_table(p, G2), "after the errors")  # the handle is still usable


# ---- 6. front end ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,devices", [(300, None), (16, None), (16, "0,0")])
def test_demuxlet_cli_write_singlets(tmp_path, V, devices):
    import pyplp

    if V == 300:  # the case of test_demux_many_samples_gpu.py::test_demuxlet_cli_300_samples
        p = many_samples.pileup(30, 1200, V, seed=5, mean_entries=60)
    else:
        p = synth.make_pileup(60, 1200, V, seed=5, mean_entries=150, min_entries=20, doublet_frac=0.3)
    prefix = str(tmp_path / "plp")
    plpio.write_plp(prefix, p, seed=5, extra_cells=1)
    vcf = str(tmp_path / "g.vcf.gz")
    plpio.write_vcf(vcf, p, p.truth["G"].astype(np.int64), field="GT", missing_frac=0.02, drop_snps=range(0, 1200, 37))
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    base = [BIN, "demuxlet", "--plp", prefix, "--vcf", vcf, "--field", "GT"] + (["--devices", devices] if devices else [])
    for cmd in (base + ["--out", plain], base + ["--out", out, "--write-singlets"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    import os
    assert not os.path.exists(plain + ".sing2.gz")
    best = open(out + ".best", "rb").read()
    assert best == open(plain + ".best", "rb").read()

    d = pyplp.load(prefix, vcf=vcf, field="GT")
    assert d["nv"] == V
    q = as_pileup(d)
    want = reference_table(q, G2)
    post = muxgl.singlet_posteriors(want)
    ids = [f"S{v}" for v in range(V)]
    rows = [ln.split("\t") for ln in best.decode().splitlines()[1:]]
    index = {bc: i for i, bc in enumerate(d["bcs"])}
    lines = gzip.open(out + ".sing2.gz", "rt").read().splitlines()
    assert lines[0] == "BARCODE\tSM_ID\tNUM.SNPS\tNUM.READS\tLLK1\tPOSTPRB"
    assert len(lines) == 1 + len(rows) * V and len(rows) > 0
    tol = parity.LL_TOL
    for n, brow in enumerate(rows):      # printed droplets in the order of .best
        i = index[brow[1]]
        for j in range(V):               # samples in VCF column order
            f = lines[1 + n * V + j].split("\t")
            assert f[:4] == [brow[1], ids[j], brow[2], brow[3]], (f, brow[:4])
            assert abs(float(f[4]) - want[i, j]) <= 0.5e-4 + tol, (f, want[i, j])
            pp = float(f[5])
            assert abs(pp - post[i, j]) <= max(6e-3 * post[i, j], 1e-300), (f, post[i, j])
