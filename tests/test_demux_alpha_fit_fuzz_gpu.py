"""muxgl_demux_alpha_fit on the unfriendly pileups of tests/test_fuzz_gpu.py (demux_case: duplicated samples, rows
normalised in float, hard calls, markers without genotypes up to all of them, cells of a handful of entries, V from 1 to
255, device groups), at drawn pairs ((-1, -1) and j == k among them) and a drawn alpha_max, under the bars of
tests/test_demux_alpha_fit_gpu.check_fit against the restatement of tests/alpha_fit_ref.py, and against the reference's own
slots: a second call with alpha_max = a drawn alpha[n] of the case's grid has ll_top = llksAB[j][k][n] and ll_zero = the
alpha = 0 slot within parity.LL_TOL (the oracle runs on the panel of the columns the checked pairs name: llksAB[j][k]
reads no other).  The restatement is Python, so a case keeps its first cells only: as many as hold 10 000 reads, at least
four, and twelve of their (droplet, slot) pairs are held to both; status and step bounds and the bit identity of a second
call are checked on all.  No case is skipped.  Every fourth seed runs under MUXGL_DEMUX_SLAB_MB=1."""
import numpy as np
import pytest

import parity
import test_demux_alpha_fit_gpu as tg
import test_fuzz_gpu as tf
import unknown_ref as ur
from popscle_amd import muxgl

pytestmark = pytest.mark.gpu

READS_CAP = 10000
PAIRS = 12


@pytest.mark.parametrize("seed", tf.FUZZ_SEEDS)
def test_alpha_fit_fuzz(seed):
    info, p = tf.demux_case(seed)
    V, alphas = info["V"], info["alphas"]
    reads_before = p.entry_rptr[p.cell_ptr]
    sub = ur.first_cells(p, max(4, int(np.searchsorted(reads_before, READS_CAP, side="right")) - 1))
    r = np.random.default_rng([seed, 97])
    n_cand = int(r.choice([1, 2, 3, 8, 16]))
    pairs = r.integers(0, V, size=(sub.C, n_cand, 2)).astype(np.int32)
    same_jk = r.random((sub.C, n_cand)) < 0.1
    pairs[same_jk, 1] = pairs[same_jk, 0]
    pairs[r.random((sub.C, n_cand)) < 0.1] = -1
    alpha_max = float(r.choice([0.05, 0.25, 0.5, 1.0, 1.0, float(r.uniform(0.01, 1.0))]))
    n = int(r.integers(1, len(alphas))) if len(alphas) > 1 else 0
    slab = "1" if seed % 4 == 0 else None
    devs = [0, 0] if info["how"] == "group" else 0
    with tf.slab_env("MUXGL_DEMUX_SLAB_MB", slab), muxgl.Engine(devs, flags=info["flags"]) as e:
        e.set_pileup(sub.S, sub.cell_ptr, sub.entry_snp, sub.entry_rptr, sub.reads)
        e.demux_set_gp(sub.gp, sub.has_gp)
        got = e.demux_alpha_fit(alphas, pairs, alpha_max)
        again = e.demux_alpha_fit(alphas, pairs, alpha_max)
        at_grid = e.demux_alpha_fit(alphas, pairs, alphas[n]) if n else None
    assert tg.same(got, again)
    flat = r.permutation(sub.C * n_cand)[:PAIRS]
    slots = [(int(x // n_cand), int(x % n_cand)) for x in flat]
    print(f"alpha fit fuzz seed {seed}: V={V} A={len(alphas)} n_cand={n_cand} alpha_max={alpha_max:.4f} cells {sub.C} of {p.C}, "
          f"gp mode {info['mode']}, {info['how']}, slab {slab}; status counts {np.bincount(got['status'].ravel(), minlength=6).tolist()}")
    with np.errstate(divide="ignore", invalid="ignore"):   # (a hard call against a read it excludes: the restatement's log(0))
        tg.check_fit(sub, alphas, pairs, alpha_max, got, f"fuzz seed {seed}", slots=slots)
    # the reference's own slots, on the panel of the columns the checked pairs name
    used = [(c, s) for c, s in slots if pairs[c, s, 0] >= 0]
    if not used:
        return
    cols = sorted({int(v) for c, s in used for v in pairs[c, s]})
    at = {v: i for i, v in enumerate(cols)}
    full = ur.full_ll(ur.with_panel(sub, sub.gp[:, cols, :]), alphas)                   # [C][len(cols)][len(cols)][A]
    worst = 0.0
    for c, s in used:
        j, k = at[int(pairs[c, s, 0])], at[int(pairs[c, s, 1])]
        d = abs(got["ll_zero"][c, s] - full[c, j, k, 0])
        if at_grid is not None:
            d = max(d, abs(at_grid["ll_top"][c, s] - full[c, j, k, n]), abs(at_grid["ll_zero"][c, s] - full[c, j, k, 0]))
            assert at_grid["status"][c, s] != 3
            if at_grid["status"][c, s] == 2:
                assert at_grid["ll_hat"][c, s].tobytes() == at_grid["ll_top"][c, s].tobytes()
        worst = max(worst, d)
        assert d <= parity.LL_TOL, (c, s, pairs[c, s], d)
    print(f"alpha fit fuzz seed {seed}: ll_top at alpha[{n}], ll_zero against the reference's slots: worst {worst:.3e} on {len(used)}")
