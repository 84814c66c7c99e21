"""muxgl_demux_unknown on the unfriendly pileups of tests/test_fuzz_gpu.py (demux_case: duplicated samples, rows normalised
in float, hard calls, markers without genotypes up to all of them, cells of a handful of entries, V from 1 to 255, device
groups): all three tables held to the reference on the panel with the mean row appended (tests/unknown_ref.py).  The
reference's tensor is [C][V + 1][V + 1][A], so a case keeps its first cells only, as many as RESTATE_BYTES of
test_fuzz_gpu.py allows (at least 16); no case is skipped.  Every fourth seed runs under MUXGL_DEMUX_SLAB_MB=1.

Bar: parity.LL_TOL on every element; each case prints its worst deviation."""
import numpy as np
import pytest

import parity
import test_fuzz_gpu as tf
import unknown_ref as ur
from popscle_amd import muxgl

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", tf.FUZZ_SEEDS)
def test_unknown_tables_fuzz(seed):
    info, p = tf.demux_case(seed)
    V, alphas = info["V"], info["alphas"]
    n = int(max(16, tf.RESTATE_BYTES // ((V + 1) * (V + 1) * len(alphas) * 8)))
    sub = ur.first_cells(p, n)
    want = ur.tables(sub, alphas, ur.panel_mean(sub.gp, sub.has_gp))
    slab = "1" if seed % 4 == 0 else None
    devs = [0, 0] if info["how"] == "group" else 0
    with tf.slab_env("MUXGL_DEMUX_SLAB_MB", slab), muxgl.Engine(devs, flags=info["flags"]) as e:
        e.set_pileup(sub.S, sub.cell_ptr, sub.entry_snp, sub.entry_rptr, sub.reads)
        e.demux_set_gp(sub.gp, sub.has_gp)
        got = e.demux_unknown(alphas)
        again = e.demux_unknown(alphas)
    worst = 0.0
    for k in ur.FIELDS:
        assert got[k].tobytes() == again[k].tobytes(), k
        worst = max(worst, parity.compare_singlet_table(got[k].reshape(sub.C, -1), want[k].reshape(sub.C, -1), parity.LL_TOL))
    print(f"unknown fuzz seed {seed}: V={V} A={len(alphas)} cells {sub.C} of {p.C}, gp mode {info['mode']}, {info['how']}, "
          f"slab {slab}: max |dLL| = {worst:.3e}")
