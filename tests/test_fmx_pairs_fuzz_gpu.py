"""muxgl_fmx_cluster_pairs on the unfriendly pileups of the fuzz (tests/test_fuzz_gpu.py fmx_case: tiny cells, entries
without reads, deep reads on the merge's clamp, doublets, 2 to 255 clusters, cells without a cluster): the twelve freemuxlet
seeds, each run on one handle from its own start through its iterations, the call after the last one, held to
tests/pairs_ref.py restate_pairs of the handle's own pileups.  The tile size and the slab budget are drawn per seed; the
bytes must be those of the default.  The bar stays parity.LL_TOL (DESIGN.md 4.2f has the worst deviation measured)."""
import numpy as np
import pytest

import parity
from pairs_ref import restate_pairs
from popscle_amd import muxgl
from test_fmx_pairs import TILES
from test_fuzz_gpu import FUZZ_SEEDS, fmx_case, slab_env, table_slab_mb

pytestmark = pytest.mark.gpu

ITERS = 3


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_cluster_pairs_on_fuzz_pileups(seed):
    info, p = fmx_case(seed)
    K = info["K"]
    tile = str(TILES[seed % len(TILES)])
    with muxgl.Engine(0, flags=info["flags"]) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        init = info["init"]
        if init is None:
            init = e.fmx_greedy_init(K, llk2 - llk0, info["frac"], info["thres"])
        e.fmx_set_clusters(K, init)
        for _ in range(ITERS):
            e.fmx_iterate(info["dp"], info["ge"])
        base = e.fmx_cluster_pairs()
        with slab_env("MUXGL_FMX_PAIRS_TILE", tile), slab_env("MUXGL_FMX_SLAB_MB", table_slab_mb(seed, "fmx")):
            got = e.fmx_cluster_pairs()
        gls, cnt = e.fmx_cluster_pileup()
    for n in ("llk2", "llk0", "nsnps"):
        assert got[n].tobytes() == base[n].tobytes(), (n, tile)
    w2, w0, wn = restate_pairs(gls, cnt, p.af)
    assert np.array_equal(got["nsnps"], wn)
    assert np.isfinite(got["llk2"]).all() and np.isfinite(got["llk0"]).all()
    worst = max(float(np.abs(got["llk2"] - w2).max()), float(np.abs(got["llk0"] - w0).max()))
    print(f"fmx pairs fuzz seed {seed}: K={K} C={p.C} S={p.S} tile {tile}, pairs with markers {int((wn > 0).sum())}/{wn.size}, "
          f"largest |sum| {max(np.abs(w2).max(), np.abs(w0).max()):.0f}, max |dLL| = {worst:.3e}")
    assert worst <= parity.LL_TOL
    assert not got["llk2"][wn == 0].any() and not got["llk0"][wn == 0].any()
