"""CPU side of the anchored freemuxlet run (muxgl_fmx_set_anchors): the reference the GPU tests hold it to is sound -- the
panel rows tests/fmx_anchor_ref.py computes in numpy ARE the posterior rows the oracle forms from the diagonals it is given,
bit for bit -- and the driver refuses what the library cannot do, before it touches a device."""
import numpy as np
import pytest

import fmx_anchor_ref as ar
from popscle_amd import freemuxlet


@pytest.mark.parametrize("geno_error", [0.1, 0.0, 0.25])
def test_panel_rows_are_the_oracles_posterior_rows_bit_for_bit(geno_error):
    with_gp, S = ar.assert_rows_are_the_oracles(seed=5, geno_error=geno_error)
    assert 0 < with_gp < S   # both kinds of marker were in it


def test_diagonals_follow_the_genotypes():
    G = np.array([[0, 1, 2], [2, 2, 0]])
    d = ar.draw_diag(G, np.array([1, 0], dtype=np.uint8))
    assert d[0].tolist() == [[1.0, 1e-3, 1e-6], [1e-3, 1.0, 1e-3], [1e-6, 1e-3, 1.0]]
    assert np.all(d[1] == 1.0)
    rows = ar.panel_rows(d, np.array([0.3, 0.6]), 0.0)
    assert np.allclose(rows.sum(axis=2), 1.0, rtol=0, atol=1e-15)
    a = 0.6                                                  # no genotypes, no error: the Hardy-Weinberg triple itself
    assert np.allclose(rows[1, 0], [(1 - a) ** 2, 2 * a * (1 - a), a * a], rtol=1e-15)
    assert rows[0, 0].argmax() == 0 and rows[0, 1].argmax() == 1 and rows[0, 2].argmax() == 2


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"run_em touched the engine ({name}) before refusing")


def test_run_em_refuses_anchors_on_ranks():
    class Two(freemuxlet.NoExchange):
        world = 2

    class Always(freemuxlet.NoExchange):
        always = True

    for ex in (Two(), Always()):
        with pytest.raises(ValueError, match="anchors need one engine"):
            freemuxlet.run_em(_NoDevice(), 4, np.zeros(8, dtype=np.int32), exchange=ex, per=(4, 4), anchors=[0, 1])
