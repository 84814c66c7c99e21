"""muxgl_fmx_unknown on the unfriendly pileups of tests/test_fuzz_gpu.py (fmx_case: cells of a handful of entries, K from 2
to 255, more clusters than donors, greedy, partial and handed-in starts with cells left at -1, every E-step path by its
flag): the three tables after EVERY iteration, on one handle and on a [0, 0] device group, held to the oracle's E-step
with two empty pileups appended (tests/fmx_unknown_ref.py), started from the reference's cluster pileups of that
iteration.  No cell is masked and none is left out; -inf equals -inf.  Every fourth seed makes the call under
MUXGL_FMX_SLAB_MB=1.

Bar: 1e-7, the TABLE_TOL of the other tables in test_fuzz_gpu.py; each case prints its worst deviation."""
import numpy as np
import pytest

import fmx_unknown_ref as fur
import oracle_binding as ob
import parity
import test_fuzz_gpu as tf
from popscle_amd import muxgl

pytestmark = pytest.mark.gpu

TOL = 1e-7
assert TOL == tf.TABLE_TOL["fmx_sng"]


@pytest.mark.parametrize("seed", tf.FUZZ_SEEDS)
def test_unknown_tables_fuzz(seed):
    info, p = tf.fmx_case(seed)
    K, dp, ge = info["K"], info["dp"], info["ge"]
    ref = tf.fmx_reference(info, p)
    n = int(ref["n_iter"])
    clust0 = np.ascontiguousarray(ref["clust0"] if info["init"] is None else info["init"], dtype=np.int32)
    eplp = ob.fmx_entry_pileup(p)
    cells0 = ob.fmx_init_cells(clust0)
    want = []
    for it in range(n):   # the pileups the posteriors of iteration `it` are made of: the start's, then the M-step's of it - 1
        cplp = ob.fmx_build_cluster_pileup(p, eplp, K, clust0) if it == 0 else ref["cplp"][it - 1]
        want.append(fur.oracle_tables(p, eplp, K, np.ascontiguousarray(cplp), cells0, ge, nthreads=16))
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
                    got = e.fmx_unknown()
                for name, w in zip(muxgl.FMX_UNKNOWN_FIELDS, want[it]):
                    assert got[name].shape == w.shape                      # every cell, every cluster
                    worst[how] = max(worst[how], parity.compare_singlet_table(got[name], w, TOL))
    print(f"fmx unknown fuzz seed {seed}: K={K} cells {p.C} ment {info['ment']} start {info['start']} flags {info['flags']} "
          f"iters {n} slab {slab}: max |dLL| one = {worst['one']:.3e}, group = {worst['group']:.3e}")
