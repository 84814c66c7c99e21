"""GPU tests of muxgl_demux_inclusion (demux_incl.hip): per droplet and sample, the evidence that the sample is in the
droplet and the doublet it pairs best in -- against the reference's full_ll through test_demux_inclusion.restate, against
the records and the singlet table of the same handle, bit for bit across calls, budgets, device groups and the sharded
driver, its error paths, and `popscle-amd demuxlet --write-inclusion`.

Bar: parity.LL_TOL (1e-5 absolute) on every element of incl, tot and dbl.  The integers: the reference's value of the
named hypothesis lies within 2 LL_TOL of the reference's maximum over H_s, and where the reference's best and runner-up
are more than 2 LL_TOL apart the three integers are the reference's (parity.compare_inclusion).  Where every hypothesis
ties, the integers are tested exactly against the documented order across several 64-sample blocks (section 1b).
Observed deviations: DESIGN.md 4.1d.
"""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import many_samples
import parity
from popscle_amd import demuxlet, muxgl, plpio, synth
from test_cli_gpu import BIN, as_pileup
from test_demux_gpu import _truncate_cells, _with_empty_cells
from test_demux_inclusion import G1, G2, G3, G6, reference_run, restate

pytestmark = pytest.mark.gpu

FIELDS = muxgl.Engine.INCLUSION_FIELDS if hasattr(muxgl.Engine, "INCLUSION_FIELDS") else ()
TOL = parity.LL_TOL


def load(e, p):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.demux_set_gp(p.gp, p.has_gp)


def inclusion(p, alphas, dp=0.5, flags=0, devs=0):
    with muxgl.Engine(devs, flags) as e:
        load(e, p)
        return e.demux_inclusion(alphas, dp)


def same_bits(a, b):
    return set(a) == set(b) == set(FIELDS) and all(a[k].tobytes() == b[k].tobytes() for k in FIELDS)


def case_pileup(V):
    """24 cells of ~150 entries (16 of ~100 at 130 samples, 12 of ~60 beyond: the reference's loop is O(V^2) per entry), 3 % of the markers without genotypes, droplets 2 and the last
    without entries; up to 65 samples cell 5 has ~3000 entries (the sweep renormalises its products many times over)"""
    if V > 130:
        return _with_empty_cells(many_samples.pileup(12, 3000, V, seed=60 + V, mean_entries=60, missing_gp_frac=0.03), [2, 11])
    if V > 65:
        return _with_empty_cells(many_samples.pileup(16, 3000, V, seed=60 + V, mean_entries=100, missing_gp_frac=0.03), [2, 15])
    big = synth.make_pileup(24, 20000, V, seed=60 + V, mean_entries=3000, sigma=0.05, min_entries=2800, max_entries=3200,
                            missing_gp_frac=0.03, doublet_frac=0.3)
    rng = np.random.default_rng(V)
    keep = {c: int(rng.integers(20, 300)) for c in range(24) if c != 5}
    p = _with_empty_cells(_truncate_cells(big, keep), [2, 23])
    lens = np.diff(p.cell_ptr)
    assert lens.max() > 2500 and (lens == 0).sum() == 2 and (p.has_gp == 0).any()
    return p


_REF = {}


def reference(V, alphas):
    """pileup, full_ll of the reference and its restatement: computed once per case and left unchanged"""
    key = (V, alphas)
    if key not in _REF:
        p = case_pileup(V)
        _, full = reference_run(p, alphas, 0.5)
        _REF[key] = (p, full, restate(full, alphas, 0.5))
    return _REF[key]


assert_against = parity.compare_inclusion


# ---- 1. against the reference ------------------------------------------------------------------------------------------

CASES = [(V, g) for g in (G2, G6, G3, G1) for V in (1, 2, 3, 16, 17, 33, 63, 64, 65, 130)] + [(256, G2), (300, G2)]
# grids the sweep and the fold treat differently: 0.5 not last (the symmetric alpha is tested per n, every block is swept),
# alpha[0] != 0 (the singlet slot is (j, 0, 0) whatever alpha[0] is), MUXGL_MAX_ALPHA alphas
G_MID = (0.0, 0.5, 0.2)
G_NZ = (0.2, 0.5)
G16 = (0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95)
assert len(G16) == muxgl.MAX_ALPHA
CASES += [(V, g) for g in (G_MID, G_NZ, G16) for V in (3, 65)]


@pytest.mark.parametrize("V,alphas", CASES)
def test_against_the_reference(V, alphas):
    p, full, want = reference(V, alphas)
    got = inclusion(p, alphas)
    assert_against(got, full, want, f"V={V} A={len(alphas)}")
    lens = np.diff(p.cell_ptr)
    e = lens == 0   # a droplet without entries: LL = 0 for every hypothesis, the priors alone
    if len(alphas) > 1 and V > 1:
        assert np.all(got["dbl"][e] == 0.0)
        assert np.allclose(got["tot"][e], 0.0, rtol=0, atol=1e-12)   # the priors sum to one
    else:
        assert np.all(got["dbl"] == -1e300) and np.all(got["partner"] == -1) and np.all(got["first"] == -1)


def test_doublet_prior_is_read():
    p, full, _ = reference(17, G6)
    want = restate(full, G6, 0.2)
    assert_against(inclusion(p, G6, dp=0.2), full, want, "V=17 doublet_prior=0.2")


def test_no_marker_has_genotypes():
    V = 12
    p = synth.make_pileup(20, 500, V, seed=9, mean_entries=100, min_entries=10)
    p.has_gp = np.zeros_like(p.has_gp)
    got = inclusion(p, G6)
    want = restate(np.zeros((p.C, V, V, 6)), G6, 0.5)
    assert np.all(got["dbl"] == 0.0)
    assert np.allclose(got["incl"], want["incl"], rtol=0, atol=1e-12) and np.allclose(got["tot"], 0.0, rtol=0, atol=1e-12)
    for k in ("partner", "alpha_idx", "first"):   # every hypothesis ties: the earliest scan position
        assert np.array_equal(got[k], want[k]), k


# ---- 1b. ties across blocks: the integers follow from the documented order alone (value descending, then scan position
# (j V + k) A + n ascending), whatever the blocks, waves, roles, groups and batches the hypotheses reach the state through

@pytest.mark.parametrize("alphas", [G2, G3, G_MID])
@pytest.mark.parametrize("V", [65, 130, 300])
def test_no_marker_has_genotypes_across_blocks(V, alphas, monkeypatch):
    """every LL is 0: every hypothesis of H_s ties, so the three integers are the earliest scan position of H_s.  The
    sums: n equal-magnitude terms, each within ~16 ulp (the exponent's argument is a difference of log priors of
    magnitude <= 14), so within 16 n 2^-53 <= 4.8e-10 at tot's n = V + V V (A - 1) <= 270 300; held to 1e-9."""
    monkeypatch.delenv("MUXGL_DEMUX_SLAB_MB", raising=False)
    A = len(alphas)
    p = synth.make_pileup(6, 400, V, seed=40 + V, mean_entries=60, min_entries=1, sigma=1.0)
    p.has_gp = np.zeros_like(p.has_gp)
    want = restate(np.zeros((p.C, V, V, A)), alphas, 0.5)
    runs = [inclusion(p, alphas)]
    if (V, alphas) == (130, G3):   # 1 MB: 130 * 60 + 56 B of state and 3 * 32 KB per block and cell: one batch of the six cells, nine groups of one block
        monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
        runs.append(inclusion(p, alphas))
        assert same_bits(*runs)
    for got in runs:
        assert np.all(got["dbl"] == 0.0)
        for k in ("partner", "alpha_idx", "first"):
            assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5])
        assert np.all(parity._close(got["incl"], want["incl"], 1e-9)) and np.all(parity._close(got["tot"], 0.0, 1e-9))


@pytest.mark.parametrize("alphas", [G2, G3, G_MID])
@pytest.mark.parametrize("V", [65, 130])
def test_every_sample_identical(V, alphas, monkeypatch):
    """for one n every (j, k) carries the same device value; which n wins is rounding, the rest is the order: sample 0
    pairs with 1 (as (0, 1, n), or as (1, 0, n) where alpha[n] = 0.5 keeps k < j only), every other sample with 0 (as
    (0, s, n), or as (s, 0, n) at 0.5)"""
    monkeypatch.delenv("MUXGL_DEMUX_SLAB_MB", raising=False)
    base = synth.make_pileup(14, 1500, V, seed=50 + V, mean_entries=40, sigma=1.3, min_entries=1, max_entries=200,
                             missing_gp_frac=0.03, doublet_frac=0.3)
    p = _truncate_cells(base, {0: 1, 1: 2, 2: 3, 13: 1})
    lens = np.diff(p.cell_ptr)
    assert lens.min() == 1 and lens.max() <= 200 and lens.max() > 60
    p.gp = np.ascontiguousarray(np.broadcast_to(p.gp[:, :1, :], p.gp.shape))
    got = inclusion(p, alphas)
    s = np.arange(V)
    assert np.all(got["partner"][:, 0] == 1) and np.all(got["partner"][:, 1:] == 0)
    sym = np.asarray(alphas)[got["alpha_idx"]] == 0.5
    assert np.array_equal(got["first"], np.where(sym, s[None] > 0, s[None] == 0).astype(np.int32))
    assert np.all(got["dbl"].view(np.int64) == got["dbl"].view(np.int64)[:, :1])
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
    assert same_bits(got, inclusion(p, alphas))


@pytest.mark.parametrize("alphas", [G2, G3, G_MID])
@pytest.mark.parametrize("V,pairs", [(130, ((3, 70), (64, 129), (10, 20), (100, 101))), (65, ((1, 64), (5, 6), (30, 63)))])
def test_duplicated_columns(V, pairs, alphas):
    """samples a < b with the same genotype rows, all others distinct: a hypothesis with b ties the one with a in b's
    place bit for bit, and that one scans first in either role, so no other sample s names b as its partner -- but for
    one hypothesis: at alpha = 0.5 only k < j carries prior mass, so for a < s < b the twin of (b, s) is the mirrored
    (s, a), whose sum is rounded in another order (in the reference's arithmetic too); it may win by rounding"""
    p = synth.make_pileup(12, 1500, V, seed=70 + V, mean_entries=80, min_entries=5, missing_gp_frac=0.03, doublet_frac=0.3)
    gp = np.array(p.gp, copy=True)
    for a, b in pairs:
        gp[:, b, :] = gp[:, a, :]
    p.gp = np.ascontiguousarray(gp)
    cols = np.unique(np.moveaxis(p.gp, 1, 0).reshape(V, -1), axis=0)
    assert cols.shape[0] == V - len(pairs)          # the premise: no other two samples alike
    with muxgl.Engine(0) as e:
        load(e, p)
        sng = e.demux_singlets(alphas)
        got = e.demux_inclusion(alphas)
    paired = {x for ab in pairs for x in ab}
    others = np.array([s for s in range(V) if s not in paired])
    sym = np.asarray(alphas)[got["alpha_idx"][:, others]] == 0.5
    for a, b in pairs:
        assert sng[:, a].tobytes() == sng[:, b].tobytes(), (a, b)
        if got["dbl"][:, a].tobytes() != got["dbl"][:, b].tobytes():   # the two copies' best values differ
            import warnings

            warnings.warn(f"V={V} alphas={alphas} pair ({a}, {b}): dbl differs between the two copies; partner check left "
                          "out for this pair")
            continue
        hit = got["partner"][:, others] == b
        mirrored = sym & (got["first"][:, others] == 0) & ((others > a) & (others < b))[None]   # (b, s, 0.5) against (s, a, 0.5)
        print(f"V={V} alphas={alphas} pair ({a}, {b}): {int((hit & mirrored).sum())} samples between them name {b} at alpha 0.5")
        assert not (hit & ~mirrored).any(), (a, b, others[np.argwhere(hit & ~mirrored)[:5, 1]].tolist())


def test_zero_cells():
    p = synth.make_pileup(10, 300, 3, seed=8, mean_entries=50, min_entries=10)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8))
        e.demux_set_gp(p.gp, p.has_gp)
        got = e.demux_inclusion(G2)
    assert got["incl"].shape == (0, 3) and got["tot"].shape == (0,) and got["partner"].shape == (0, 3)


# ---- 2. consistent with the records and the singlet table of the same handle -----------------------------------------

@pytest.mark.parametrize("V,alphas,flags", [(12, G2, 0), (12, G6, 0), (40, G6, 0), (40, G2, muxgl.FLAG_FORCE_STREAMED_CALL),
                                            (40, G6, muxgl.FLAG_FORCE_STREAMED_CALL), (300, G2, 0)])
def test_consistent_with_the_records(V, alphas, flags):
    dp = 0.5
    p = many_samples.pileup(30, 2000, V, seed=700 + V + len(alphas), mean_entries=80)
    with muxgl.Engine(0, flags) as e:
        load(e, p)
        raw = e.demux_run(alphas, dp)
        sng = e.demux_singlets(alphas)
        got = e.demux_inclusion(alphas, dp)
    rec = parity.exact(raw, alphas, p, dp)
    assert ((rec["valid"] & 1) == 1).all()
    c = np.arange(p.C)
    best = got["dbl"].max(axis=1)
    assert np.all(parity._close(best, rec["dblBestLLK"], TOL))
    for s_ in ("dBest1", "dBest2"):   # both samples of the record's best pair carry that value
        assert np.all(parity._close(got["dbl"][c, rec[s_]], rec["dblBestLLK"], TOL)), s_
    s = got["dbl"].argmax(axis=1)     # ... and the argmax names a pair at the maximum with the record's alpha
    pr, fi = got["partner"][c, s], got["first"][c, s]
    j, k = np.where(fi == 1, s, pr), np.where(fi == 1, pr, s)
    al = np.asarray(alphas)
    a_got, a_rec = al[got["alpha_idx"][c, s]], al[rec["dBestA"]]
    same = ((j == rec["dBest1"]) & (k == rec["dBest2"]) & (a_got == a_rec)) | \
           ((j == rec["dBest2"]) & (k == rec["dBest1"]) & (np.isclose(a_got, 1.0 - a_rec) | (a_got == 0.5)))
    others = (np.arange(V)[None] != s[:, None]) & (np.arange(V)[None] != pr[:, None])
    tied = got["dbl"][c, s] - np.where(others, got["dbl"], -np.inf).max(axis=1, initial=-np.inf) <= 2 * TOL  # a third sample reaches it
    assert np.all(same | tied), np.flatnonzero(~(same | tied))
    assert np.all(got["incl"] >= sng + np.log((1.0 - dp) / V))
    chain = np.logaddexp(-1e-300, got["tot"])
    print(f"V={V}: max |sumLLK - logadd(tot)| = {np.max(np.abs(rec['sumLLK'] - chain)):.3e}")
    assert np.all(parity._close(rec["sumLLK"], chain, TOL))


# ---- 3. bit-identical --------------------------------------------------------------------------------------------------

def test_two_calls_budgets_and_null_subsets(monkeypatch):
    V = 130
    p, _, _ = reference(V, G6)
    monkeypatch.delenv("MUXGL_DEMUX_SLAB_MB", raising=False)
    with muxgl.Engine(0) as e:
        load(e, p)
        a = e.demux_inclusion(G6)
        assert e.timing()[muxgl.T_DEMUX_INCLUSION] > 0.0
        b = e.demux_inclusion(G6)
        for want in (("incl",), ("tot",), ("partner", "first"), ("dbl", "alpha_idx"), ()):
            part = e.demux_inclusion(G6, want=want)
            assert set(part) == set(want) and all(part[k].tobytes() == a[k].tobytes() for k in want)
    assert same_bits(a, b)
    # 1 MB: a batch holds (1 MB) / (130 * 60 + 56 + 6 * 32 KB) = 5 of the 16 cells, a group one block: several batches, many groups
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
    assert same_bits(a, inclusion(p, G6))
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "3")
    assert same_bits(a, inclusion(p, G6))


@pytest.mark.parametrize("V,alphas", [(17, G3), (130, G2)])
def test_device_group_and_sharded_driver(V, alphas):
    p, _, _ = reference(V, alphas)
    want = inclusion(p, alphas)
    assert same_bits(want, inclusion(p, alphas, flags=muxgl.FLAG_DEMUX_ONLY, devs=[0, 0]))
    assert same_bits(want, inclusion(p, alphas, flags=muxgl.FLAG_DEMUX_ONLY, devs=[0, 0, 0]))
    with muxgl.Engine(0) as e:
        load(e, p)
        records = e.demux_run(alphas, 0.5)
        sng = e.demux_singlets(alphas)
    rec, inc = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5, want_inclusion=True)
    assert same_bits(want, inc) and rec.tobytes() == records.tobytes()
    rec, s2, inc = demuxlet.run_sharded(lambda: muxgl.Engine(0), p, alphas, 0.5, want_singlets=True, want_inclusion=True)
    assert same_bits(want, inc) and rec.tobytes() == records.tobytes() and s2.tobytes() == sng.tobytes()


@pytest.mark.parametrize("V,flags", [(12, 0), (40, 0), (40, muxgl.FLAG_FORCE_STREAMED_CALL), (300, 0)])
def test_the_call_leaves_the_demuxlet_state_alone(V, flags):
    p = many_samples.pileup(30, 2000, V, seed=800 + V, mean_entries=80)
    with muxgl.Engine(0, flags) as e:
        load(e, p)
        plain = e.demux_run(G6, 0.5)
    with muxgl.Engine(0, flags) as e:
        load(e, p)
        i0 = e.demux_inclusion(G6)           # without a previous run
        r0 = e.demux_run(G6, 0.5)
        t0 = e.timing()
        view = e.demux_results_view().tobytes()
        i1 = e.demux_inclusion(G6)
        t1 = e.timing()
        assert e.demux_results_view().tobytes() == view
        e.demux_inclusion(G2)                 # another grid between two runs
        r1 = e.demux_run(G6, 0.5)
    assert plain.tobytes() == r0.tobytes() == r1.tobytes() == view
    assert same_bits(i0, i1)
    for slot in (muxgl.T_DEMUX_SWEEP, muxgl.T_DEMUX_CALL):   # the run's timings keep their values
        assert t0[slot] == t1[slot]


# ---- 4. errors ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("devs", [0, [0, 0]])
def test_error_paths(devs):
    p = synth.make_pileup(12, 300, 5, seed=1, mean_entries=40, min_entries=5)
    with muxgl.Engine(devs, muxgl.FLAG_DEMUX_ONLY) as e:
        with pytest.raises(muxgl.MuxglError, match="pileup"):
            e.demux_inclusion(G2)
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        with pytest.raises(muxgl.MuxglError, match="GP tensor"):
            e.demux_inclusion(G2)
        e.demux_set_gp(p.gp, p.has_gp)
        with pytest.raises(muxgl.MuxglError, match="n_alpha"):
            e.demux_inclusion(())
        with pytest.raises(ValueError):
            e.demux_inclusion(G2, want=("incl", "nonsense"))
        dp = muxgl._DemuxParams()
        dp.n_alpha = muxgl.MAX_ALPHA + 1
        assert e.lib.muxgl_demux_inclusion(e.h, ctypes.byref(dp), None, None, None, None, None, None) != 0
        assert b"n_alpha" in e.lib.muxgl_last_error(e.h)
        assert e.lib.muxgl_demux_inclusion(e.h, None, None, None, None, None, None, None) != 0
        _, full = reference_run(p, G2)
        assert_against(e.demux_inclusion(G2), full, restate(full, G2, 0.5), "after the errors")  # the handle is still usable


# ---- 5. front end ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V,devices", [(300, None), (16, None), (16, "0,0")])
def test_demuxlet_cli_write_inclusion(tmp_path, V, devices):
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
    base = [BIN, "demuxlet", "--plp", prefix, "--vcf", vcf, "--field", "GT"] + (["--devices", devices] if devices else [])
    for cmd in (base + ["--out", plain], base + ["--out", out, "--write-inclusion"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    assert not os.path.exists(plain + ".incl.gz")
    best = open(out + ".best", "rb").read()
    assert best == open(plain + ".best", "rb").read()

    d = pyplp.load(prefix, vcf=vcf, field="GT")
    assert d["nv"] == V
    q = as_pileup(d)
    want = inclusion(q, G2)   # the table of the library on what the front end loaded (held to the reference above)
    ids = [f"S{v}" for v in range(V)]
    rows = [ln.split("\t") for ln in best.decode().splitlines()[1:]]
    index = {bc: i for i, bc in enumerate(d["bcs"])}
    lines = gzip.open(out + ".incl.gz", "rt").read().splitlines()
    assert lines[0] == "BARCODE\tSM_ID\tNUM.SNPS\tNUM.READS\tLLK.INCL\tPOSTPRB.INCL\tDBL.PARTNER\tDBL.ALPHA\tDBL.LLK"
    assert len(lines) == 1 + len(rows) * V and len(rows) > 0
    for n, brow in enumerate(rows):      # printed droplets in the order of .best
        i = index[brow[1]]
        for j in range(V):               # samples in VCF column order
            f = lines[1 + n * V + j].split("\t")
            assert f[:4] == [brow[1], ids[j], brow[2], brow[3]], (f, brow[:4])
            assert abs(float(f[4]) - want["incl"][i, j]) <= 0.5e-4 + 1e-9, (f, want["incl"][i, j])
            pp = float(np.exp(want["incl"][i, j] - want["tot"][i]))
            assert abs(float(f[5]) - pp) <= max(6e-3 * pp, 1e-300), (f, pp)
            assert f[6] == ids[want["partner"][i, j]], (f, want["partner"][i, j])
            a = 0.5   # the default grid's only doublet alpha: 1 - alpha = alpha
            assert abs(float(f[7]) - a) <= 0.5e-3
            assert abs(float(f[8]) - want["dbl"][i, j]) <= 0.5e-4 + 1e-9, (f, want["dbl"][i, j])
