"""CPU checks behind muxgl_demux_singlets: muxgl.singlet_posteriors against a plain softmax, and the property the
V > 255 comparison of tests/test_demux_singlets_gpu.py rests on -- the reference's singlet value of sample j,
llksAB[(j, 0, 0)] of cmd_cram_demuxlet.cpp:733-747, reads only columns 0 and j of the genotype tensor."""
import numpy as np
import pytest

import many_samples
import oracle_binding as ob
import ref_binding as rb
from popscle_amd import muxgl, synth

G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)


def plain_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def test_singlet_posteriors_is_a_softmax_over_the_row():
    rng = np.random.default_rng(1)
    sng = -rng.gamma(2.0, 40.0, size=(50, 37))
    got = muxgl.singlet_posteriors(sng)
    assert got.shape == sng.shape and got.dtype == np.float64
    assert np.allclose(got, plain_softmax(sng), rtol=1e-14, atol=0.0)
    assert np.allclose(got.sum(axis=1), 1.0, rtol=1e-13)
    # without the maximum subtracted these rows underflow to 0 / 0
    naive = np.exp(sng[:1] * 1000)
    assert naive.sum() == 0.0
    assert np.isfinite(muxgl.singlet_posteriors(sng[:1] * 1000)).all()


def test_singlet_posteriors_wide_and_flat_rows():
    wide = np.array([[-1e4, -5e3, -3.0, -2.0, 0.0], [1e4, 0.0, -1e4, 9999.0, 5e3]])
    got = muxgl.singlet_posteriors(wide)
    assert np.isfinite(got).all() and np.allclose(got.sum(axis=1), 1.0)
    assert np.allclose(got, plain_softmax(wide), rtol=1e-14, atol=0.0)
    assert got[0, 0] == 0.0 and got[0].argmax() == 4 and got[1].argmax() == 0
    assert np.isclose(got[1, 3], np.exp(-1.0) / (1.0 + np.exp(-1.0)))
    flat = muxgl.singlet_posteriors(np.zeros((3, 8)))   # droplets without entries
    assert np.array_equal(flat, np.full((3, 8), 0.125))
    assert muxgl.singlet_posteriors(np.zeros((0, 4))).shape == (0, 4)
    with pytest.raises(ValueError):
        muxgl.singlet_posteriors(np.zeros(5))


def _reference_table(p, alphas):
    if rb.available():
        return rb.RefScl.from_packed(p).demux(alphas, doublet_prior=0.5, full_ll=True)[2][:, :, 0, 0]
    return ob.demux(p, alphas=alphas, full_ll=True, nthreads=4)[1][:, :, 0, 0]


@pytest.mark.parametrize("alphas", [G2, (0.2, 0.5), G6])
def test_singlet_value_reads_only_columns_0_and_j(alphas):
    """V = 40, 12 cells, 3 % of the markers without genotypes: the reference run on gp[:, [0] + chunk, :] reproduces
    full_ll[:, [0] + chunk, 0, 0] of the run on the whole tensor bit for bit"""
    V = 40
    p = many_samples.pileup(12, 1500, V, seed=40, mean_entries=60, missing_gp_frac=0.03)
    whole = _reference_table(p, alphas)
    for chunk in (list(range(1, 14)), list(range(14, 40)), [39, 5, 17]):
        cols = [0] + chunk
        sub = synth.Pileup(p.C, p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads, p.af,
                           np.ascontiguousarray(p.gp[:, cols, :]), p.has_gp)
        assert np.array_equal(_reference_table(sub, alphas), whole[:, cols])
