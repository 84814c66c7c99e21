"""muxgl_fmx_ambient_fit on the unfriendly pileups of tests/test_fuzz_gpu.py (fmx_case: cells of a handful of entries, K from 2
to 255, more clusters than donors, greedy, partial and handed-in starts with cells left at -1, every E-step path by its
flag), after the first iteration, at a drawn ambient profile (uniform, with exact 0 and 1 on some markers), a drawn rho_max
and drawn candidates (-1 among them), under the bars of tests/test_fmx_ambient_fit_gpu.check_fit against the restatement of
tests/fmx_ambient_fit_ref.py with the posteriors made of the reference's cluster pileups of the start.  The restatement is
Python, so twelve (droplet, slot) pairs of a case are held to it; status and step bounds, the absence of NaN and the bit
identity of a second call and of a [0, 0] device group are checked on all.  No case is skipped.

Bar of ll_hat and ll_zero: 1e-7, the TABLE_TOL of the other freemuxlet tables in test_fuzz_gpu.py.

With a drawn candidate that does not fit the droplet, LL can rise a second time inside the coarse bracket (LL' jumps upward
where an element leaves the 1e-6 floor): on 6 of 443 pairs of these seeds the demuxlet fit's rules alone end on the local
maximum next to the best coarse point (seed 2, droplet 64, slot 6: the lower bound at LL -143.33483 where rho = 0.00567 has
-143.33337; seed 11, droplet 558, slot 0: -50.61449 against -50.07930 at 0.02051).  The kernel therefore scans a bracket in
which an element crosses the floor on 65 points before it iterates, and the bar "restated LL at the device's
rho_hat >= restated LL at the restatement's - 1e-9" holds on every seed."""
import numpy as np
import pytest

import ambient_ref as ar
import oracle_binding as ob
import test_fmx_ambient_fit_gpu as tg
import test_fuzz_gpu as tf
from popscle_amd import muxgl
from test_fmx_singlets import cluster_posteriors

pytestmark = pytest.mark.gpu

TOL = 1e-7
assert TOL == tf.TABLE_TOL["fmx_sng"]
PAIRS = 12


@pytest.mark.parametrize("seed", tf.FUZZ_SEEDS)
def test_ambient_fit_fuzz(seed):
    info, p = tf.fmx_case(seed)
    K, dp, ge = info["K"], info["dp"], info["ge"]
    ref = tf.fmx_reference(info, p)
    clust0 = np.ascontiguousarray(ref["clust0"] if info["init"] is None else info["init"], dtype=np.int32)
    r = np.random.default_rng([seed, 97])
    n_cand = int(r.choice([1, 2, 3, 8, 16]))
    cand = r.integers(-1, K, size=(p.C, n_cand)).astype(np.int32)
    rho_max = float(r.choice([0.05, 0.25, 0.5, 1.0, float(r.uniform(0.01, 1.0))]))
    f = ar.draw_af(p.S, seed=3000 + seed, corners=0.15)
    eplp = ob.fmx_entry_pileup(p)
    q = cluster_posteriors(p.af, np.ascontiguousarray(ob.fmx_build_cluster_pileup(p, eplp, K, clust0)), ge)
    got = {}
    for how, devs in (("one", 0), ("group", [0, 0])):
        with muxgl.Engine(devs, flags=info["flags"]) as e:
            e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
            e.fmx_prepare(p.af)
            e.fmx_set_clusters(K, clust0)
            cells, st = e.fmx_iterate(dp, ge)
            assert tuple(int(x) for x in st) == tuple(ref["counters"][0]), (how, st, ref["counters"][0])
            got[how] = e.fmx_ambient_fit(f, cand, rho_max)
            assert tg.same(e.fmx_ambient_fit(f, cand, rho_max), got[how])
    assert tg.same(got["one"], got["group"])
    got = got["one"]
    flat = r.permutation(p.C * n_cand)[:PAIRS]
    pairs = [(int(x // n_cand), int(x % n_cand)) for x in flat]
    print(f"fmx ambient fit fuzz seed {seed}: K={K} n_cand={n_cand} rho_max={rho_max:.4f} cells {p.C} ment {info['ment']} start "
          f"{info['start']} flags {info['flags']}; status counts {np.bincount(got['status'].ravel(), minlength=7).tolist()}")
    tg.check_fit(p, q, f, cand, rho_max, got, f"fuzz seed {seed}", pairs=pairs, ll_tol=TOL)
