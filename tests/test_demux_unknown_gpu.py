"""GPU tests of muxgl_demux_unknown (demux_unknown.hip): every droplet against a donor that is not in the panel -- ll_ju
(the reference's llksA0, cmd_cram_demuxlet.cpp:749-760), ll_uj (the other orientation) and ll_uu (llks00, :763-773) --
against the reference itself run on the panel with the unknown donor's prior appended as sample V (tests/unknown_ref.py;
tests/test_demux_unknown.py holds that premise bit for bit), bit for bit across calls, budgets, subsets of outputs, device
groups and the sharded driver, the state it must leave alone, its error paths, and `popscle-amd demuxlet --write-unknown`.

Bar: parity.LL_TOL (1e-5 absolute) on every element of every table; each comparison prints its worst deviation.
"""
import ctypes
import gzip
import itertools
import os
import subprocess

import numpy as np
import pytest

import many_samples
import parity
import unknown_ref as ur
from popscle_amd import demuxlet, muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup
from test_demux_gpu import _truncate_cells, _with_empty_cells

pytestmark = pytest.mark.gpu

G1 = (0.0,)
G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
G16 = tuple(i / 30.0 for i in range(16))   # 0 .. 0.5: six chunks of three alphas, the last of one
UNK_PART = 2048                            # entries per part of a long cell (demux_unknown.hip)


def load(e, p):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)


def unknown(p, alphas, gp0=None, flags=0, devs=0, want=ur.FIELDS):
    with muxgl.Engine(devs, flags) as e:
        load(e, p)
        return e.demux_unknown(alphas, gp0, want)


def assert_tables(got, want, what=""):
    worst = {}
    for k in ur.FIELDS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, (k, got[k].shape, want[k].shape)
        with np.errstate(invalid="ignore"):
            d = np.abs(got[k] - want[k])
        d = d[np.isfinite(d)]
        worst[k] = float(d.max()) if d.size else 0.0
    print(f"unknown {what}: C={got['uu'].shape[0]} V={got['ju'].shape[1]} A={got['uu'].shape[1]}, max |dLL| ju {worst['ju']:.3e} "
          f"uj {worst['uj']:.3e} uu {worst['uu']:.3e}, kernel {got.get('kernel_ms', 0.0):.3f} ms")
    for k in ur.FIELDS:
        ok = parity._close(got[k], want[k], parity.LL_TOL)
        assert ok.all(), f"{k}: {int((~ok).sum())} elements beyond {parity.LL_TOL}; worst {worst[k]}"
    return max(worst.values())


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ur.FIELDS)


def cell_bytes(p, A):
    """device bytes of every cell of a batch (demux_unknown.hip: weights, slab rows, table rows)"""
    lens = np.diff(p.cell_ptr)
    parts = np.maximum(1, -(-lens // UNK_PART))
    row = 8 * A * 2 * (p.gp.shape[1] + 1)
    return lens * A * 48 + parts * (row + 24) + row + 16


# ---- 1. against the reference, V <= 255 -------------------------------------------------------------------------------

@pytest.mark.parametrize("V,alphas,C,S,ment", [
    (1, G2, 20, 500, 100),             # one sample: both launches of the sweep at 64 entries per wave
    (2, G1, 40, 800, 150),             # a grid of one alpha
    (3, G6, 40, 1000, 200),            # two chunks of three alphas
    (16, G2, 60, 3000, 400),
    (16, G16, 16, 2000, 300),          # chunk remainder, 16 alphas
    (17, (0.2, 0.5), 30, 3000, 400),   # alpha[0] != 0
    (33, (0.0, 0.3), 20, 3000, 300),   # no 0.5
    (63, G16, 5, 2000, 300),           # 64 columns: one full block
    (64, G6, 8, 6000, 500),            # the unknown donor's column alone in a second block
    (64, G2, 5, 9000, 3000),           # cells walked in parts
    (65, G2, 8, 5000, 1200),
    (130, G2, 3, 6000, 2500),          # three blocks
])
def test_random_vs_reference(V, alphas, C, S, ment):
    p = synth.make_pileup(C, S, V, seed=1000 + V * 7 + len(alphas), mean_entries=ment, min_entries=20, missing_gp_frac=0.03)
    assert (p.has_gp == 0).any()
    got = unknown(p, alphas)
    assert got["kernel_ms"] > 0.0
    assert_tables(got, ur.tables(p, alphas, ur.panel_mean(p.gp, p.has_gp)), f"V={V} A={len(alphas)}")


@pytest.mark.parametrize("V", [4, 20])
def test_deep_pileups(V):
    p = synth.make_pileup(30, 600, V, seed=3000 + V, mean_entries=80, min_entries=10, reads_lambda=60.0, min_bq=2,
                          max_bq=93, cap_bq=127, other=0.03)
    assert np.diff(p.entry_rptr).max() > 80
    u = ur.panel_mean(p.gp, p.has_gp)
    for alphas in [(0.0, 0.3, 0.5), G2]:
        assert_tables(unknown(p, alphas), ur.tables(p, alphas, u), f"deep V={V}")


@pytest.mark.parametrize("V,alphas", [(5, G6), (40, G2)])
def test_empty_droplets_long_and_short_cells(V, alphas):
    base = synth.make_pileup(24, 9000, V, seed=5100 + V, mean_entries=500, sigma=1.2, min_entries=1, max_entries=6000,
                             missing_gp_frac=0.04)
    p = _with_empty_cells(_truncate_cells(base, {3: 1, 11: 2, 20: 7}), [0, 7, 23])
    lens = np.diff(p.cell_ptr)
    assert (lens == 0).sum() == 3 and lens.max() > UNK_PART and {1, 2, 7} <= set(lens.tolist())
    got = unknown(p, alphas)
    assert_tables(got, ur.tables(p, alphas, ur.panel_mean(p.gp, p.has_gp)), f"ragged V={V}")
    for k in ur.FIELDS:
        assert np.all(got[k][lens == 0] == 0.0)   # a droplet without entries: zeros


def test_no_marker_has_genotypes():
    p = synth.make_pileup(20, 500, 12, seed=9, mean_entries=100, min_entries=10)
    p.has_gp = np.zeros_like(p.has_gp)
    got = unknown(p, G6)
    assert all(np.all(got[k] == 0.0) for k in ur.FIELDS)   # every factor is exactly 1
    assert_tables(got, ur.tables(p, G6, ur.panel_mean(p.gp, p.has_gp)), "no genotypes")


def test_zero_cells():
    p = synth.make_pileup(10, 300, 3, seed=8, mean_entries=50, min_entries=10)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8))
        e.demux_set_gp(p.gp, p.has_gp)
        got = e.demux_unknown(G2)
    assert got["ju"].shape == (0, 3, 2) and got["uj"].shape == (0, 3, 2) and got["uu"].shape == (0, 2) and got["kernel_ms"] == 0.0


# ---- 2. an explicit prior ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,alphas", [(6, G6), (40, G2)])
def test_explicit_prior(V, alphas):
    p = synth.make_pileup(30, 2000, V, seed=6100 + V, mean_entries=200, min_entries=10, missing_gp_frac=0.05)
    miss = p.has_gp == 0
    assert miss.any()
    hw = ur.hwe(p.af)
    poisoned = hw.copy()
    poisoned[miss] = np.nan                 # rows of markers without genotypes do not matter
    got = unknown(p, alphas, gp0=poisoned)
    assert_tables(got, ur.tables(p, alphas, hw), f"HWE prior V={V}")
    plain = unknown(p, alphas)
    assert not np.array_equal(plain["uu"], got["uu"])
    mean = ur.panel_mean(p.gp, p.has_gp)    # added in sample order, one division: what the device forms for NULL
    mean[miss] = np.nan
    assert same_bytes(unknown(p, alphas, gp0=mean), plain)


# ---- 3. V > 255: ll_ju[:, j] and ll_uj[:, j] read only column j and u ----------------------------------------------------

@pytest.mark.parametrize("V,alphas", [(300, G6), (1024, G2)])
def test_many_samples_vs_reference_on_sub_panels(V, alphas):
    """the reference on `63 columns + [u]`, u from the full panel; every sample is covered (tests/test_demux_unknown.py
    restates the property the comparison rests on)"""
    p = many_samples.pileup(24 if V < 500 else 12, 2000, V, seed=400 + V, mean_entries=50)
    got = unknown(p, alphas)
    assert_tables(got, ur.tables_by_columns(p, alphas, ur.panel_mean(p.gp, p.has_gp), chunk=63), f"V={V} by columns")


# ---- 4. bit-identical ----------------------------------------------------------------------------------------------------

def _long_cells_pileup(V, seed, C=40):
    p = synth.make_pileup(C, 9000, V, seed=seed, mean_entries=700, sigma=1.0, min_entries=1, max_entries=6000,
                          missing_gp_frac=0.04)
    assert np.diff(p.cell_ptr).max() > UNK_PART
    return p


def test_two_calls_and_every_subset_of_outputs():
    p = _long_cells_pileup(48, 4100, C=20)
    with muxgl.Engine(0) as e:
        load(e, p)
        a = e.demux_unknown(G6)
        b = e.demux_unknown(G6)
        assert same_bytes(a, b) and a["kernel_ms"] > 0.0
        for r in (1, 2):
            for want in itertools.combinations(ur.FIELDS, r):
                only = e.demux_unknown(G6, want=want)
                assert set(only) == set(want) | {"kernel_ms"}
                assert all(only[k].tobytes() == a[k].tobytes() for k in want), want


def test_budget_does_not_matter(monkeypatch):
    V, alphas = 40, G2
    p = many_samples.pileup(200, 6000, V, seed=611, mean_entries=700, sigma=1.0, min_entries=1, max_entries=5000)
    lens, need = np.diff(p.cell_ptr), cell_bytes(p, len(alphas))
    # several batches at 1 MB, cells in parts among them, and no cell that exceeds the budget on its own
    assert lens.max() > UNK_PART and need.max() <= (1 << 20) and need.sum() > 8 * (1 << 20)
    monkeypatch.delenv("MUXGL_DEMUX_SLAB_MB", raising=False)
    one = unknown(p, alphas)
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
    many = unknown(p, alphas)
    assert same_bytes(one, many)
    # ... and one that does: the call fails, naming the reason, and the handle stays usable
    q = synth.make_pileup(6, 9000, 8, seed=612, mean_entries=5000, sigma=0.1, min_entries=4000, max_entries=8000)
    assert cell_bytes(q, 6).max() > (1 << 20)
    with muxgl.Engine(0) as e:
        load(e, q)
        with pytest.raises(muxgl.MuxglError, match="exceeds the budget"):
            e.demux_unknown(G6)
        monkeypatch.delenv("MUXGL_DEMUX_SLAB_MB")
        assert np.isfinite(e.demux_unknown(G6)["uu"]).all()


@pytest.mark.parametrize("V", [20, 300])
def test_device_group_and_sharded_driver(V):
    alphas = G6
    p = _long_cells_pileup(V, 4200 + V, C=30)
    want = unknown(p, alphas)
    for devs in ([0, 0], [0, 0, 0]):
        got = unknown(p, alphas, flags=muxgl.FLAG_DEMUX_ONLY, devs=devs)
        assert same_bytes(got, want) and got["kernel_ms"] > 0.0
    with muxgl.Engine(0) as e:
        load(e, p)
        records = e.demux_run(alphas, 0.5)
    rec, unk = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5, want_unknown=True)
    assert set(unk) == set(ur.FIELDS) and same_bytes(unk, want) and rec.tobytes() == records.tobytes()
    rec, sng, unk = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5, want_singlets=True, want_unknown=True)
    assert same_bytes(unk, want) and sng.shape == (p.C, V) and rec.tobytes() == records.tobytes()
    assert demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5).tobytes() == records.tobytes()


@pytest.mark.parametrize("V,flags", [(40, 0), (40, muxgl.FLAG_FORCE_STREAMED_CALL), (300, 0)])
def test_the_call_leaves_the_demuxlet_state_alone(V, flags):
    p = many_samples.pileup(30, 2000, V, seed=800 + V, mean_entries=80)
    with muxgl.Engine(0, flags) as e:
        load(e, p)
        r0 = e.demux_run(G6, 0.5)
        view, t0 = e.demux_results_view().tobytes(), e.timing().copy()
        u0 = e.demux_unknown(G6)
        assert e.demux_results_view().tobytes() == view and np.array_equal(e.timing(), t0)
        other = e.demux_unknown(G2)   # another grid between two runs
        assert e.demux_results_view().tobytes() == view and np.array_equal(e.timing(), t0)
        r1 = e.demux_run(G6, 0.5)
        u1 = e.demux_unknown(G6)
    assert r0.tobytes() == r1.tobytes() == view
    assert same_bytes(u0, u1)
    assert not np.array_equal(other["uu"][:, 0], u0["uu"][:, 0])  # the normalisation is over the whole grid


# ---- 5. errors ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_error_paths(devs):
    p = synth.make_pileup(12, 300, 5, seed=1, mean_entries=40, min_entries=5)
    with muxgl.Engine(devs, muxgl.FLAG_DEMUX_ONLY) as e:
        with pytest.raises(muxgl.MuxglError, match="pileup"):
            e.demux_unknown(G2)
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        with pytest.raises(muxgl.MuxglError, match="GP tensor"):
            e.demux_unknown(G2)
        e.demux_set_gp(p.gp, p.has_gp)
        with pytest.raises(muxgl.MuxglError, match="n_alpha"):
            e.demux_unknown(())
        dp = muxgl._DemuxParams()
        dp.n_alpha = 2
        dp.alpha[1] = 0.5
        dp.doublet_prior = 0.5
        ms = ctypes.c_float(-1.0)
        assert e.lib.muxgl_demux_unknown(e.h, ctypes.byref(dp), None, None, None, None, ctypes.byref(ms)) != 0
        assert b"all three outputs are NULL" in e.lib.muxgl_last_error(e.h)
        dp.n_alpha = muxgl.MAX_ALPHA + 1
        out = np.zeros((p.C, muxgl.MAX_ALPHA + 1))
        assert e.lib.muxgl_demux_unknown(e.h, ctypes.byref(dp), None, None, None, out.ctypes.data_as(ctypes.c_void_p), None) != 0
        assert b"n_alpha" in e.lib.muxgl_last_error(e.h)
        with pytest.raises(ValueError):
            e.demux_unknown(G2, want=("ju", "nope"))
        with pytest.raises(ValueError):
            e.demux_unknown(G2, gp0=np.zeros((p.S, 2)))
        # the handle is still usable
        assert_tables(e.demux_unknown(G2), ur.tables(p, G2, ur.panel_mean(p.gp, p.has_gp)), "after the errors")


# ---- 6. front end ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,devices", [(300, None), (16, None), (16, "0,0")])
def test_demuxlet_cli_write_unknown(tmp_path, V, devices):
    import pyplp

    if V == 300:
        p = many_samples.pileup(30, 1200, V, seed=5, mean_entries=60)
    else:
        p = synth.make_pileup(60, 1200, V, seed=5, mean_entries=150, min_entries=20, doublet_frac=0.3)
    prefix = str(tmp_path / "plp")
    plpio.write_plp(prefix, p, seed=5, extra_cells=1)
    vcf = str(tmp_path / "g.vcf.gz")
    plpio.write_vcf(vcf, p, p.truth["G"].astype(np.int64), field="GT", missing_frac=0.02, drop_snps=range(0, 1200, 37))
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    alphas = (0.0, 0.25, 0.5)
    base = ([BIN, "demuxlet", "--plp", prefix, "--vcf", vcf, "--field", "GT"] + [x for a in alphas for x in ("--alpha", str(a))]
            + (["--devices", devices] if devices else []))
    for cmd in (base + ["--out", plain], base + ["--out", out, "--write-unknown"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    assert not os.path.exists(plain + ".unk.gz")
    best = open(out + ".best", "rb").read()
    assert best == open(plain + ".best", "rb").read()

    d = pyplp.load(prefix, vcf=vcf, field="GT")
    assert d["nv"] == V
    q = as_pileup(d)
    u = ur.panel_mean(q.gp, q.has_gp)
    want = ur.tables(q, alphas, u) if V <= 255 else ur.tables_by_columns(q, alphas, u)
    sm = muxgl.unknown_summary(want, alphas)
    ids = [f"S{v}" for v in range(V)]
    rows = [ln.split("\t") for ln in best.decode().splitlines()[1:]]
    index = {bc: i for i, bc in enumerate(d["bcs"])}
    lines = gzip.open(out + ".unk.gz", "rt").read().splitlines()
    assert lines[0] == ("BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.ALPHA\tUNK.DBL.LLK\tHALF.GUESS\tHALF.LLK\t"
                        "DIFF.LLK.PANEL.UNK")
    assert len(lines) == 1 + len(rows) and len(rows) > 0
    tol = 0.5e-4 + parity.LL_TOL
    for n, brow in enumerate(rows):      # printed droplets in the order of .best
        i = index[brow[1]]
        f = lines[1 + n].split("\t")
        assert len(f) == 10 and f[:3] == [brow[1], brow[2], brow[3]], (f, brow[:4])
        assert abs(float(f[3]) - float(brow[6])) <= 0.5e-2 + 1e-9          # BEST.LLK of .best is printed %.2lf
        assert abs(float(f[4]) - sm["uu_sng"][i]) <= tol
        assert f[5] == "%.2f" % alphas[sm["uu_alpha_idx"][i]] and abs(float(f[6]) - sm["uu_dbl"][i]) <= tol
        assert abs(float(f[8]) - sm["half_llk"][i]) <= tol
        j, n_al = int(sm["half_sample"][i]), int(sm["half_alpha_idx"][i])
        guess = (ids[j], "*") if sm["half_known_major"][i] else ("*", ids[j])
        assert f[7] == "%s,%s,%.2f" % (guess + (alphas[n_al],)), (f, j, n_al)
        top = max(sm["uu_sng"][i], sm["uu_dbl"][i], sm["half_llk"][i])
        assert abs(float(f[9]) - (float(f[3]) - top)) <= 2 * tol
