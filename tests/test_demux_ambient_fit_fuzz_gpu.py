"""muxgl_demux_ambient_fit on the unfriendly pileups of tests/test_fuzz_gpu.py (demux_case: duplicated samples, rows
normalised in float, hard calls, markers without genotypes up to all of them, cells of a handful of entries, V from 1 to
255, device groups), at a drawn ambient profile (uniform, with exact 0 and 1 on some markers), a drawn rho_max and drawn
candidates (-1 among them), under the bars of tests/test_demux_ambient_fit_gpu.check_fit against the restatement of
tests/ambient_fit_ref.py.  The restatement is Python, so a case keeps its first cells only: as many as hold 20 000 reads, at
least four, and twelve of their (droplet, slot) pairs are held to the restatement; status and step bounds and the bit
identity of a second call are checked on all.  No case is skipped.  Every fourth seed runs under MUXGL_DEMUX_SLAB_MB=1."""
import numpy as np
import pytest

import ambient_ref as ar
import test_demux_ambient_fit_gpu as tg
import test_fuzz_gpu as tf
import unknown_ref as ur
from popscle_amd import muxgl

pytestmark = pytest.mark.gpu

READS_CAP = 20000
PAIRS = 12


@pytest.mark.parametrize("seed", tf.FUZZ_SEEDS)
def test_ambient_fit_fuzz(seed):
    info, p = tf.demux_case(seed)
    V, alphas = info["V"], info["alphas"]
    reads_before = p.entry_rptr[p.cell_ptr]
    sub = ur.first_cells(p, max(4, int(np.searchsorted(reads_before, READS_CAP, side="right")) - 1))
    r = np.random.default_rng([seed, 89])
    n_cand = int(r.choice([1, 2, 3, 8, 16]))
    cand = r.integers(-1, V, size=(sub.C, n_cand)).astype(np.int32)
    rho_max = float(r.choice([0.05, 0.25, 0.5, 1.0, float(r.uniform(0.01, 1.0))]))
    f = ar.draw_af(sub.S, seed=2000 + seed, corners=0.15)
    slab = "1" if seed % 4 == 0 else None
    devs = [0, 0] if info["how"] == "group" else 0
    with tf.slab_env("MUXGL_DEMUX_SLAB_MB", slab), muxgl.Engine(devs, flags=info["flags"]) as e:
        e.set_pileup(sub.S, sub.cell_ptr, sub.entry_snp, sub.entry_rptr, sub.reads)
        e.demux_set_gp(sub.gp, sub.has_gp)
        got = e.demux_ambient_fit(alphas, f, cand, rho_max)
        again = e.demux_ambient_fit(alphas, f, cand, rho_max)
    assert tg.same(got, again)
    flat = r.permutation(sub.C * n_cand)[:PAIRS]
    pairs = [(int(x // n_cand), int(x % n_cand)) for x in flat]
    print(f"ambient fit fuzz seed {seed}: V={V} A={len(alphas)} n_cand={n_cand} rho_max={rho_max:.4f} cells {sub.C} of {p.C}, "
          f"gp mode {info['mode']}, {info['how']}, slab {slab}; status counts {np.bincount(got['status'].ravel(), minlength=6).tolist()}")
    with np.errstate(divide="ignore", invalid="ignore"):   # (a hard call against a read it excludes: the restatement's log(0))
        tg.check_fit(sub, alphas, f, cand, rho_max, got, f"fuzz seed {seed}", pairs=pairs)
