"""GPU tests of muxgl_fmx_cluster_pairs (fmx_pairs.hip): every pair of a handle's cluster pileups scored as one donor
against two unrelated donors.  Everything goes through the C-ABI and is held to tests/pairs_ref.py restate_pairs, fed the
same handle's fmx_cluster_pileup() and the af that was handed in (the restatement itself is held to the reference's pair
loop in tests/test_fmx_pairs.py, the pileup to the reference in tests/test_fmx_gpu.py).

Bar: parity.LL_TOL (1e-5 absolute) on every element, nsnps equal, no NaN and no inf; every test prints the worst deviation
it saw (DESIGN.md 4.2f has the largest).

test_shapes_vs_restatement runs every instantiation of fcp_sweep_kernel (every lane width KH at every tile size T, the
grid that tests/test_fmx_pairs.py test_gpu_grid_reaches_every_variant counts without a GPU) and holds the tile sizes to
each other bit for bit."""
import gzip
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import parity
from pairs_ref import pair_index, restate_pairs
from popscle_amd import freemuxlet, muxgl, plpio, synth
from test_cli_gpu import BIN, tokens_match
from test_fmx_match_gpu import _clocks, _state, prepared, spread_init
from test_fmx_pairs import TILES, grid
from test_fuzz_gpu import slab_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (read from the header, not through the probe library: a library built by hipcc brings the system's HIP runtime with it, and
# loaded while the modules are imported it would come before the one the engine's process settles on)
P = int(re.search(r"constexpr int64_t PART = (\d+);", open(os.path.join(ROOT, "popscle_amd", "csrc", "pairs_plan.hpp")).read()).group(1))
FIELDS = ("llk2", "llk0", "nsnps")
TILE_ENV = "MUXGL_FMX_PAIRS_TILE"


def compare(got, want, what):
    """got: the call's dict; want: (llk2, llk0, nsnps) of the restatement.  nsnps equal, no NaN or inf, every element
    within parity.LL_TOL, a pair without a shared marker exactly 0, 0, 0.  Returns the worst deviation."""
    llk2, llk0, nsnps = want
    assert got["llk2"].shape == llk2.shape and got["llk0"].shape == llk0.shape and got["nsnps"].dtype == np.int32
    assert np.array_equal(got["nsnps"], nsnps)
    worst = 0.0
    for g, w in ((got["llk2"], llk2), (got["llk0"], llk0)):
        assert np.isfinite(g).all() and np.isfinite(w).all()
        if g.size:
            worst = max(worst, float(np.max(np.abs(g - w))))
    K = int(round((1 + np.sqrt(1 + 8 * llk2.size)) / 2))
    print(f"fmx pairs {what}: K={K}, pairs with markers {int((nsnps > 0).sum())}/{nsnps.size}, max |dLL| = {worst:.3e}, "
          f"kernel {got['kernel_ms']:.3f} ms")
    assert worst <= parity.LL_TOL
    assert np.all(got["llk2"][nsnps == 0] == 0.0) and np.all(got["llk0"][nsnps == 0] == 0.0)
    return worst


def assert_pairs(e, af, what, got=None):
    """the call against the restatement of the handle's own pileup; returns (got, worst deviation)"""
    got = got or e.fmx_cluster_pairs()
    gls, cnt = e.fmx_cluster_pileup()
    return got, compare(got, restate_pairs(gls, cnt, af), f"{what}, S={gls.shape[1]}")


def _same_bytes(a, b, what):
    for n in FIELDS:
        if n in a or n in b:
            assert a[n].tobytes() == b[n].tobytes(), f"{n} differs: {what}"


def _pairs_of(k, K):
    return [pair_index(max(k, j), min(k, j)) for j in range(K) if j != k]


# ---- 1. shapes: every lane width, partner block, tile remainder and cut of the markers, at every tile size ---------------

@pytest.mark.parametrize("K,S,what", grid(P))
def test_shapes_vs_restatement(K, S, what):
    """60 to 80 cells dealt round the clusters (the last of three or more clusters gets none: all its pairs 0, 0, 0), about a
    fifth of the markers per cell, so most markers of a pair have reads in one of its clusters alone"""
    p = synth.make_pileup(60 + (K + S) % 21, S, 4, seed=8200 + K + S, mean_entries=max(1, S // 5), min_entries=1, reads_lambda=0.6,
                          doublet_frac=0.1, with_gp=False)
    with prepared(p) as e:
        e.fmx_set_clusters(K, spread_init(p.C, K))
        for stage in ("initial pileups", "after an iteration"):
            with slab_env(TILE_ENV, None):
                base, _ = assert_pairs(e, p.af, f"{what}; {stage}")
            if K > 2 and stage == "initial pileups":   # (an iteration may hand the cluster cells)
                idx = _pairs_of(K - 1, K)
                assert not base["nsnps"][idx].any() and not base["llk2"][idx].any() and not base["llk0"][idx].any()
            if S > 100:   # a pair's count never exceeds either cluster's; from a dozen clusters on (six cells or fewer per
                # cluster, each at a fifth of the markers) there are markers where only one cluster of a pair has reads
                cover = (e.fmx_cluster_pileup()[1][:, :, 0] > 0).sum(axis=1)
                a, b = np.tril_indices(K, -1)
                live = (cover[a] > 0) & (cover[b] > 0)
                assert live.any() and (base["nsnps"] <= np.minimum(cover[a], cover[b])).all()
                if K >= 12:
                    assert (base["nsnps"][live] < np.minimum(cover[a], cover[b])[live]).any()
            for t in TILES:
                with slab_env(TILE_ENV, str(t)):
                    _same_bytes(e.fmx_cluster_pairs(), base, f"tile {t} against the default, K={K} S={S}")
            if stage == "initial pileups":
                e.fmx_iterate(0.5, 0.1)
        assert e.lib.muxgl_fmx_cluster_pairs(e.h, None, None, None, None) == 0   # all NULL: succeeds, writes nothing


def test_one_cluster_has_no_pair():
    p = synth.make_pileup(60, 300, 4, seed=8201, mean_entries=60, min_entries=5, with_gp=False)
    with prepared(p) as e:
        e.fmx_set_clusters(1, np.zeros(p.C, dtype=np.int32))
        got = e.fmx_cluster_pairs()
        assert all(got[n].size == 0 for n in FIELDS) and got["kernel_ms"] == 0.0
        e.fmx_iterate(0.5, 0.1)   # the handle goes on
        assert e.fmx_cluster_pairs()["llk2"].size == 0


def test_allele_frequencies_of_exactly_zero_and_one():
    """p = (1, 0, 0) and (0, 0, 1) at some markers: one term of weight 1 is left, every sum stays finite"""
    p = synth.make_pileup(70, P + 1, 4, seed=8202, mean_entries=400, min_entries=20, with_gp=False)
    af = p.af.copy()
    af[::7] = 0.0
    af[3::11] = 1.0
    for K in (5, 70):
        with muxgl.Engine(0) as e:
            e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
            e.fmx_prepare(af)
            e.fmx_set_clusters(K, ((np.arange(p.C) * 3) % K).astype(np.int32))   # (3: prime to both K, every cluster has a cell)
            got, _ = assert_pairs(e, af, f"af exactly 0 and 1, K={K}")
            assert (got["nsnps"] > 0).all() and np.isfinite(got["llk2"]).all() and np.isfinite(got["llk0"]).all()


# ---- 2. bytes -------------------------------------------------------------------------------------------------------------

def test_two_calls_and_every_subset_are_bit_identical():
    p = synth.make_pileup(80, 2 * P + 5, 4, seed=8300, mean_entries=800, min_entries=20, with_gp=False)
    for K in (9, 70):
        with prepared(p) as e:
            e.fmx_set_clusters(K, spread_init(p.C, K))
            e.fmx_iterate(0.5, 0.1)
            a, b = e.fmx_cluster_pairs(), e.fmx_cluster_pairs()
            assert a["kernel_ms"] > 0.0
            _same_bytes(a, b, "two calls")
            for t in (None, "8"):
                with slab_env(TILE_ENV, t):
                    for n in range(1, 4):
                        for want in itertools.combinations(FIELDS, n):
                            only = e.fmx_cluster_pairs(want=want)
                            assert set(only) == set(want) | {"kernel_ms"}
                            _same_bytes(only, {k: a[k] for k in want}, f"want={want}, tile {t}, K={K}")
            with pytest.raises(ValueError):
                e.fmx_cluster_pairs(want=("llk1",))


_CHILD = r"""
import os, sys, numpy as np
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
from pairs_ref import restate_pairs
from popscle_amd import muxgl, synth
from test_fmx_pairs import load_plan_probe, pairs_plan, plan_batches
K, S, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
mb = os.environ.get("MUXGL_FMX_SLAB_MB")
if mb:   # the cut the kernel's own byte count gives under this budget: two batches in block 0, the last one short
    lib = load_plan_probe()
    plan = pairs_plan(lib, S, K, budget=int(mb) << 20)
    assert plan["np"] == 3 and plan["rows"] == 272 and plan["blocks"] == 5, plan
    assert plan_batches(lib, K, 0, plan["rows"]) == [(0, 272), (272, 300)]
p = synth.make_pileup(70, S, 4, seed=8301, mean_entries=600, min_entries=300, max_entries=900, with_gp=False)
res = {}
with muxgl.Engine(0) as e:
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.fmx_prepare(p.af)
    e.fmx_set_clusters(K, ((np.arange(p.C) * 13) % K).astype(np.int32))   # spread over all five blocks: one cell or none
    for tile in ("4", "8"):
        os.environ["MUXGL_FMX_PAIRS_TILE"] = tile
        r = e.fmx_cluster_pairs()
        res.update({f"{n}_t{tile}": r[n] for n in ("llk2", "llk0", "nsnps")})
    if not mb:   # the restatement of the handle's own pileups, for the parent to hold the table to
        gls, cnt = e.fmx_cluster_pileup()
        res["want_llk2"], res["want_llk0"], res["want_nsnps"] = restate_pairs(gls, cnt, p.af)
np.savez(out, **res)
"""


def test_budget_and_tile_do_not_matter(tmp_path):
    """300 clusters, three parts: under MUXGL_FMX_SLAB_MB=1 partner block 0 is swept in batches of 272 and 28 row clusters
    (stated by the child from pairs_plan.hpp before it runs).  The bytes are those of the default budget at either tile,
    and that table is held to the restatement."""
    K, S = 300, 2 * P + 5
    outs = []
    for mb in (1, 0):
        env = dict(os.environ)
        env.pop("MUXGL_FMX_SLAB_MB", None)
        env.pop(TILE_ENV, None)
        if mb:
            env["MUXGL_FMX_SLAB_MB"] = str(mb)
        out = str(tmp_path / f"mb{mb}.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(K), str(S), out], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(np.load(out))
    small, full = outs
    for n in FIELDS:
        assert full[f"{n}_t4"].tobytes() == full[f"{n}_t8"].tobytes(), f"{n}: tiles 4 and 8 differ, one batch"
        for t in TILES:
            assert small[f"{n}_t{t}"].tobytes() == full[f"{n}_t4"].tobytes(), f"{n}: tile {t} under 1 MB differs from one batch"
    got = {n: full[f"{n}_t4"] for n in FIELDS}
    got["kernel_ms"] = 0.0
    compare(got, (full["want_llk2"], full["want_llk0"], full["want_nsnps"]), f"K={K} in two batches")
    live = np.zeros(K, dtype=bool)
    live[(np.arange(70) * 13) % K] = True
    a, b = np.tril_indices(K, -1)
    both = live[a] & live[b]               # pairs of two clusters with a cell; every other pair is 0, 0, 0
    assert (got["nsnps"][both] > 0).mean() > 0.9 and not got["nsnps"][~both].any()
    assert (got["nsnps"][both & (a >= 272)] > 0).any() and (got["nsnps"][both & (b >= 256)] > 0).any()


# ---- 3. labels ------------------------------------------------------------------------------------------------------------

def test_relabelling_the_clusters_permutes_the_table():
    """k -> K - 1 - k maps every pair (a, b), a > b, to (K - 1 - b, K - 1 - a): row cluster and partner change roles (the
    two roles round differently, so the sums are held to LL_TOL, not to equal bits; the counts are equal)"""
    K = 70
    p = synth.make_pileup(80, P + 1, 4, seed=8400, mean_entries=400, min_entries=20, with_gp=False)
    init = ((np.arange(p.C) * 3) % K).astype(np.int32)   # (3 is prime to 70: every cluster has a cell)
    outs = []
    for lab in (init, (K - 1 - init).astype(np.int32)):
        with prepared(p) as e:
            e.fmx_set_clusters(K, lab)
            outs.append(assert_pairs(e, p.af, "labels")[0])
    a, b = np.tril_indices(K, -1)
    j = pair_index(K - 1 - b, K - 1 - a)
    assert np.array_equal(outs[0]["nsnps"], outs[1]["nsnps"][j]) and (outs[0]["nsnps"] > 0).sum() > 1000
    worst = max(np.abs(outs[0][n] - outs[1][n][j]).max() for n in ("llk2", "llk0"))
    print(f"fmx pairs relabelled: max |dLL| = {worst:.3e}")
    assert worst <= parity.LL_TOL


# ---- 4. against the droplet call ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C_,S,kw", [(40, 500, {}), (30, 300, dict(reads_lambda=0.6))])
def test_one_cell_per_cluster_is_the_droplet_pair_distance(C_, S, kw):
    """K = C, cluster k = cell k: the cluster pileups are the droplets' after one merge, so nsnps is that of
    muxgl_fmxold_pair_dist and llk2 - llk0 agrees within LL_TOL (the reference's own merge moves that difference by up
    to 1.7e-9 at these two settings, by 1.1e-6 at reads_lambda = 4, which is left out)"""
    p = synth.make_pileup(C_, S, 4, seed=8100 + C_, mean_entries=max(1, S // 5), min_entries=1, with_gp=False, **kw)
    with prepared(p) as e:
        dd = e.fmxold_pair_dist(5.41, want_full=True)
        e.fmx_set_clusters(p.C, np.arange(p.C, dtype=np.int32))
        got, _ = assert_pairs(e, p.af, "one cell per cluster")
    assert np.array_equal(got["nsnps"], dd["nsnps"]) and got["nsnps"].max() > 3
    worst = float(np.abs((got["llk2"] - got["llk0"]) - (dd["llk2"] - dd["llk0"])).max())
    print(f"fmx pairs against muxgl_fmxold_pair_dist, {C_} x {S}: max |d(llk2 - llk0)| = {worst:.3e}")
    assert worst <= parity.LL_TOL


# ---- 5. state -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,flags", [(6, 0), (40, muxgl.FLAG_FORCE_STREAMED_ESTEP)])
def test_the_call_reads_state_and_changes_none(K, flags):
    # few reads per droplet: near-tie cells, so the exact path's bookkeeping is in play
    p = synth.make_pileup(300, 500, 4, seed=8500 + K, mean_entries=10, min_entries=2, reads_lambda=0.3, with_gp=False)
    init = (np.arange(p.C) % 3).astype(np.int32)

    def run(with_call):
        out, tables = [], []
        with prepared(p, 0, flags) as e:
            e.fmx_set_clusters(K, init)
            if with_call:
                with pytest.raises(muxgl.MuxglError, match="no E-step since muxgl_fmx_set_clusters"):
                    e.fmx_singlets()
                tables.append(assert_pairs(e, p.af, "state, initial")[0])
                with pytest.raises(muxgl.MuxglError, match="no E-step since muxgl_fmx_set_clusters"):
                    e.fmx_singlets()            # still refused, exactly as before
            for it in range(3):
                cells, st = e.fmx_iterate(0.5, 0.1)
                before = _state(e)              # records, cluster pileups, MUXGL_BUF_CGP, singlets, muxgl_fmx_exact_stats
                if with_call:
                    clocks = _clocks(e)         # every slot of muxgl_get_timing and muxgl_get_timing_sum, and the call count
                    got = e.fmx_cluster_pairs()
                    assert _clocks(e) == clocks
                    assert _state(e) == before  # (muxgl_fmx_singlets still runs after the call: _state calls it)
                    tables.append(assert_pairs(e, p.af, f"state, iteration {it + 1}", got)[0])
                out.append((cells.tobytes(), tuple(st), before))
            if with_call:   # the initial pileups and those of an iteration give different tables
                assert not np.array_equal(tables[0]["llk2"], tables[1]["llk2"])
        return out

    assert run(False) == run(True)   # and the following iterations are those of a run without the call


def test_asynchronous_phases_are_drained():
    p = synth.make_pileup(80, 300, 4, seed=8501, mean_entries=80, min_entries=5, with_gp=False)
    with prepared(p, 0, muxgl.FLAG_ASYNC_PHASES) as e:
        e.fmx_set_clusters(4, spread_init(p.C, 4))
        e.fmx_iter_gp(0.5, 0.1)
        e.fmx_iter_estep(0.5, 0.1)
        e.fmx_iter_fetch()
        e.fmx_iter_mstep()                      # enqueued, not waited for: the call scores what this M-step leaves
        got = e.fmx_cluster_pairs()
        assert_pairs(e, p.af, "asynchronous phases", got)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------

def test_missing_prerequisites_are_named_and_the_handle_stays_usable():
    K = 4
    p = synth.make_pileup(80, 300, 4, seed=8600, mean_entries=80, min_entries=5, with_gp=False)
    init = spread_init(p.C, K)
    with muxgl.Engine(0) as e:
        e.K = K   # (the binding sizes its outputs from it)
        with pytest.raises(muxgl.MuxglError, match=r"muxgl_fmx_cluster_pairs: no pileup set \(muxgl_set_pileup\)"):
            e.fmx_cluster_pairs()
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.K = K
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_cluster_pairs: call muxgl_fmx_prepare first"):
            e.fmx_cluster_pairs()
        e.fmx_prepare(p.af)
        e.K = K
        with pytest.raises(muxgl.MuxglError, match=r"muxgl_fmx_cluster_pairs: no clusters set \(muxgl_fmx_set_clusters\)"):
            e.fmx_cluster_pairs()
        e.fmx_set_clusters(K, init)
        first, _ = assert_pairs(e, p.af, "after the refusals, no GP tensor")
        e.fmx_set_shard(0, p.C, 0, p.S // 2)   # a partial range
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_cluster_pairs: not available on a sharded handle"):
            e.fmx_cluster_pairs()
        e.fmx_set_shard(0, p.C, 0, p.S)        # everything again: allowed, same table
        _same_bytes(e.fmx_cluster_pairs(), first, "after the shard range is everything again")


def test_device_groups_and_slabbed_handles_are_refused():
    K = 4
    p = synth.make_pileup(80, 300, 4, seed=8601, mean_entries=80, min_entries=5, with_gp=False)
    init = spread_init(p.C, K)
    with prepared(p, [0, 0]) as e:
        e.fmx_set_clusters(K, init)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_cluster_pairs: not available on a device group"):
            e.fmx_cluster_pairs()
        cells, st = e.fmx_iterate(0.5, 0.1)    # the group still works
        assert cells.shape == (p.C,)
    (c_ranges, _), (s_ranges, _) = freemuxlet.plan_ranges(p.C, p.S, 2)
    with muxgl.Engine(0) as e:
        freemuxlet.load_rank(e, p, c_ranges[0], s_ranges[0])
        e.fmx_set_clusters(K, init)
        with pytest.raises(muxgl.MuxglError, match="muxgl_fmx_cluster_pairs: not available on a slabbed handle"):
            e.fmx_cluster_pairs()
        e.fmx_iter_gp(0.5, 0.1)                # the handle still works
        gls, cnt = e.fmx_cluster_pileup()
        assert gls.shape == (K, p.S, 9)


# ---- 7. meaning: the halves of a donor belong together --------------------------------------------------------------------

def test_split_donors_are_found():
    V = 4
    p = synth.make_pileup(40, 500, V, seed=8100 + 40, mean_entries=100, min_entries=1, doublet_frac=0.0, with_gp=False)
    s1 = p.truth["s1"].astype(np.int64)
    half = np.zeros(p.C, dtype=np.int64)
    for v in range(V):
        m = np.flatnonzero(s1 == v)
        assert m.size >= 2
        half[m] = np.arange(m.size) % 2
    init = (2 * s1 + half).astype(np.int32)      # donor v is clusters 2 v and 2 v + 1
    with prepared(p) as e:
        e.fmx_set_clusters(2 * V, init)
        got, _ = assert_pairs(e, p.af, "split donors")
    t = freemuxlet.cluster_pair_table(got["llk2"], got["llk0"], got["nsnps"])
    a, b = np.tril_indices(2 * V, -1)
    same = (a // 2) == (b // 2)
    d = got["llk2"] - got["llk0"]
    print(f"  halves of one donor {d[same].min():+.1f} .. {d[same].max():+.1f}, every other pair {d[~same].min():+.1f} .. "
          f"{d[~same].max():+.1f}")
    assert (d[same] > 0).all() and (d[~same] < 0).all()
    assert t["groups"] == [[2 * v, 2 * v + 1] for v in range(V)]
    assert t["partner"].tolist() == [k ^ 1 for k in range(2 * V)]


# ---- 8. front end ---------------------------------------------------------------------------------------------------------

def test_freemuxlet_cli_write_cluster_pairs(tmp_path):
    K = 4
    p = synth.make_pileup(150, 1200, K, seed=8700, mean_entries=200, min_entries=30, with_gp=True)
    prefix, vcf = str(tmp_path / "plp"), str(tmp_path / "donors.vcf.gz")
    plpio.write_plp(prefix, p, seed=8)
    plpio.write_vcf(vcf, p, p.truth["G"].astype(np.int64))
    dump = str(tmp_path / "dump.bin")
    r = subprocess.run([BIN, "dump-plp", "--plp", prefix, "--vcf", vcf, "--field", "GT", "--out", dump], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    d = plpio.read_dump(dump)
    init = ((np.arange(d["C"]) * 7) % K).astype(np.int32)
    initf = str(tmp_path / "init.txt")
    with open(initf, "w") as f:
        for i, bc in enumerate(d["bcs"]):
            f.write(f"{bc}\t{int(init[i])}\n")
    out = str(tmp_path / "out")
    base = [BIN, "freemuxlet", "--plp", prefix, "--nsample", str(K), "--init-cluster", initf]
    r = subprocess.run(base + ["--out", out, "--write-cluster-pairs"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    with muxgl.Engine(0) as e:   # the Python route on the loader's arrays
        e.set_pileup(d["S"], d["cell_ptr"], d["entry_snp"], d["entry_rptr"], d["reads"])
        e.fmx_prepare(d["af"])
        freemuxlet.run_em(e, K, init)
        got, _ = assert_pairs(e, d["af"], "CLI arrays")
    lines = gzip.open(out + ".clust1.ldist.gz", "rt").read().splitlines()
    assert lines[0] == "ID1\tID2\tNSNP\tLLK0\tLLK2\tLDIFF\tDIFF.SNP" and len(lines) == 1 + K * (K - 1) // 2
    i = 0
    for a in range(1, K):
        for b in range(a):
            f = lines[1 + i].split("\t")
            assert f[:3] == [str(a), str(b), str(int(got["nsnps"][i]))]
            diff = got["llk2"][i] - got["llk0"][i]
            want = ["%.2f" % got["llk0"][i], "%.2f" % got["llk2"][i], "%.2f" % diff, "%.4f" % (diff / (got["nsnps"][i] + 1e-6))]
            for x, y in zip(f[3:], want):
                assert tokens_match(x, y), (f, want)
            i += 1
    r = subprocess.run(base + ["--out", str(tmp_path / "grp"), "--devices", "0,0", "--write-cluster-pairs"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "muxgl_fmx_cluster_pairs: not available on a device group" in r.stderr
    assert not os.path.exists(str(tmp_path / "grp") + ".clust1.ldist.gz")
