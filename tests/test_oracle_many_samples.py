"""CPU tests above 255 samples (no device): the checker and the host exact-call pass hold where the streamed demuxlet
call (demux_stream.hip) is the only device path.

  * the CPU oracle against the reference's own compiled demuxlet loop (oracle/_ref/libscdrop_ref.so) at V = 300, every
    field bit for bit, the full log-likelihood tensor included;
  * the host exact-call pass (muxgl_demux_exact_calls) at V = 300 on emulated device records (test_exact_calls.py's
    emulation), with duplicated samples so that a cell needs every hypothesis of a scan.
"""
import numpy as np
import pytest

import many_samples
import oracle_binding as ob
import ref_binding as rb
from popscle_amd import muxgl
from test_exact_calls import check_exact, emulate_device, reference_records

V = 300


@pytest.mark.skipif(not rb.available(), reason="oracle/_ref/libscdrop_ref.so not built (needs /root/reference)")
@pytest.mark.parametrize("alphas", [(0.0, 0.5), (0.0, 0.3)])
def test_oracle_is_the_reference_at_300_samples(alphas):
    p = many_samples.pileup(6, 1500, V, seed=301, mean_entries=60)
    want, _, want_ll = rb.RefScl.from_packed(p).demux(alphas, doublet_prior=0.5, full_ll=True)
    got, got_ll = ob.demux(p, alphas, doublet_prior=0.5, full_ll=True)
    assert (want["valid"] == 1).sum() == p.C
    for n in want.dtype.names:
        if n.startswith("_"):
            continue
        x, y = got[n], want[n]
        ok = np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
        assert ok, n
    assert np.array_equal(got_ll, want_ll, equal_nan=True)
    # sample indices beyond 255 occur in the calls (an 8-bit field anywhere would wrap them)
    assert max(want["sBest"].max(), want["dBest1"].max(), want["dBest2"].max()) > 255


def test_exact_pass_at_300_samples_with_every_hypothesis():
    alphas = (0.0, 0.5)
    p = many_samples.pileup(8, 1500, V, seed=302, mean_entries=60)
    # cell 0 made of sample 0 only: its copy (sample 1) ties it exactly in the singlet scan, and the doublets
    # (0, 1) / (1, 0) tie the best pair, so best, next and third of a scan are within reach of each other
    want, full = reference_records(p, alphas)
    got = emulate_device(want, full, alphas, 0.5, noise=1e-13, seed=7)
    deep = (got["valid"] & (muxgl.CELL_DEEP_SNG | muxgl.CELL_DEEP_DBL)) != 0
    st = muxgl.demux_exact_calls(p, alphas, got, 0.5, nthreads=2)
    check_exact(got, want, st)
    assert st["cells"] > 0
    assert deep.any() and st["deep"] > 0, st
