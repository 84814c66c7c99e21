"""muxgl_fmx_ambient on the unfriendly pileups of tests/test_fuzz_gpu.py (fmx_case: cells of a handful of entries, K from 2
to 255, more clusters than donors, greedy, partial and handed-in starts with cells left at -1, every E-step path by its
flag): the table after EVERY iteration, on one handle and on a [0, 0] device group, at a drawn ambient profile (uniform,
with exact 0 and 1 on some markers) and drawn rhos (0 and 1 among them), held to the restatement of
tests/fmx_ambient_ref.py with the posteriors made of the reference's cluster pileups of that iteration.  No cell is masked
and none is left out.  Every fourth seed makes the call under MUXGL_FMX_SLAB_MB=1.

Bar: 1e-7, the TABLE_TOL of the other tables in test_fuzz_gpu.py; each case prints its worst deviation."""
import numpy as np
import pytest

import ambient_ref as ar
import fmx_ambient_ref as fr
import oracle_binding as ob
import parity
import test_fuzz_gpu as tf
from popscle_amd import muxgl
from test_fmx_singlets import cluster_posteriors

pytestmark = pytest.mark.gpu

TOL = 1e-7
assert TOL == tf.TABLE_TOL["fmx_sng"]


@pytest.mark.parametrize("seed", tf.FUZZ_SEEDS)
def test_ambient_table_fuzz(seed):
    info, p = tf.fmx_case(seed)
    K, dp, ge = info["K"], info["dp"], info["ge"]
    ref = tf.fmx_reference(info, p)
    n = int(ref["n_iter"])
    clust0 = np.ascontiguousarray(ref["clust0"] if info["init"] is None else info["init"], dtype=np.int32)
    r = np.random.default_rng([seed, 89])
    n_rho = int(r.choice([1, 2, 3, 4, 5, 7, 8, 9, 16]))
    rhos = tuple(float(x) for x in np.where(r.random(n_rho) < 0.2, r.choice([0.0, 1.0], size=n_rho), r.random(n_rho)))
    f = ar.draw_af(p.S, seed=2000 + seed, corners=0.15)
    eplp = ob.fmx_entry_pileup(p)
    w, nine = fr.all_weights(p, f, rhos)
    assert nine.tobytes() == np.ascontiguousarray(eplp["gls"]).tobytes()
    want = []
    for it in range(n):   # the pileups the posteriors of iteration `it` are made of: the start's, then the M-step's of it - 1
        cplp = ob.fmx_build_cluster_pileup(p, eplp, K, clust0) if it == 0 else ref["cplp"][it - 1]
        want.append(fr.table_of_weights(p, cluster_posteriors(p.af, np.ascontiguousarray(cplp), ge), w, ordered=False))
    slab = "1" if seed % 4 == 0 else None
    worst = {}
    for how, devs in (("one", 0), ("group", [0, 0])):
        worst[how] = 0.0
        with muxgl.Engine(devs, flags=info["flags"]) as e:
            e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
            e.fmx_prepare(p.af)
            e.fmx_set_clusters(K, clust0)
            for it in range(n):
                cells, st = e.fmx_iterate(dp, ge)
                assert tuple(int(x) for x in st) == tuple(ref["counters"][it]), (how, it, st, ref["counters"][it])
                with tf.slab_env("MUXGL_FMX_SLAB_MB", slab):
                    got = e.fmx_ambient(f, rhos)["ll"]
                assert got.shape == want[it].shape                      # every cell, every cluster, every rho
                worst[how] = max(worst[how], parity.compare_singlet_table(got.reshape(p.C, -1), want[it].reshape(p.C, -1), TOL))
    print(f"fmx ambient fuzz seed {seed}: K={K} n_rho={n_rho} cells {p.C} ment {info['ment']} start {info['start']} "
          f"flags {info['flags']} iters {n} slab {slab}: max |dLL| one = {worst['one']:.3e}, group = {worst['group']:.3e}")
