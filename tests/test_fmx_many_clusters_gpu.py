"""freemuxlet beyond 255 clusters: the streamed E-step (popscle_amd/csrc/fmx_stream.hip) against the reference library,
against the existing E-step paths (MUXGL_FLAG_FORCE_STREAMED_ESTEP), across slab budgets, on ties, at the limits and on a
device group."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
import ref_binding as rb
from popscle_amd import muxgl, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
needs_ref = pytest.mark.skipif(not rb.available(), reason="oracle/_ref/libscdrop_ref.so not built")


def _run(p, K, flags=0, clust=None, iters=4, doublet_prior=0.5):
    """greedy start (or the given clusters), then EM iterations: records, counters and cluster pileups per iteration"""
    with muxgl.Engine(0, flags) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        c0 = e.fmx_greedy_init(K, llk2 - llk0) if clust is None else clust
        e.fmx_set_clusters(K, c0)
        out = []
        for _ in range(iters):
            cells, st = e.fmx_iterate(doublet_prior, 0.1)
            out.append((cells, st, e.fmx_cluster_pileup()))
        return c0, out, e.fmx_exact_stats()


def _same_runs(a, b):
    assert np.array_equal(a[0], b[0])
    for (ca, sa, pa), (cb, sb, pb) in zip(a[1], b[1]):
        assert tuple(sa) == tuple(sb)
        parity.same_records(ca, cb)
        assert np.array_equal(pa[1], pb[1]) and np.array_equal(pa[0], pb[0])


def _check_vs_ref(p, K, ref, init=None):
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        if init is None:
            clust = e.fmx_greedy_init(K, llk2 - llk0)
            assert np.array_equal(clust, ref["clust0"]), "greedy initial clusters differ from the reference's"
        else:
            clust = init
        e.fmx_set_clusters(K, clust)
        top = -1
        for it in range(ref["n_iter"]):
            cells, st = e.fmx_iterate(0.5, 0.1)
            assert tuple(st) == tuple(ref["counters"][it]), (it, st, ref["counters"][it])
            parity.compare_fmx(cells, ref["cells"][it], resolved=True)
            g, c = e.fmx_cluster_pileup()
            w = ref["cplp"][it]
            assert np.array_equal(c, np.stack([w["nreads"], w["nref"], w["nalt"]], axis=-1))
            assert np.allclose(g, w["gls"], rtol=1e-11, atol=1e-300)
            for f in ("sBest", "sNext", "dBest1", "dNext1", "jBest", "jNext"):
                top = max(top, int(cells[f].max()))
        return top


@needs_ref
@pytest.mark.parametrize("K", [256, 300, 400])
def test_vs_reference_library(K):
    p = synth.make_pileup(40, 3000, 24, seed=1700 + K, mean_entries=100, min_entries=20, max_entries=300,
                          reads_lambda=0.8, other=0.02, doublet_frac=0.25, with_gp=False)
    ref = rb.RefScl.from_packed(p).freemux2(K, cluster_pileups=True)
    _check_vs_ref(p, K, ref)
    # clusters spread down from the top of the index range: the calls name the last clusters (beyond 255 for K > 256)
    init = ((K - 1 - np.arange(p.C) * 7) % K).astype(np.int32)
    ref = rb.RefScl.from_packed(p).freemux2(K, init_clust=init, cluster_pileups=True)
    top = _check_vs_ref(p, K, ref, init=init)
    assert top == K - 1 if K == 256 else top > 255


@pytest.mark.parametrize("K", [33, 64, 65, 200, 255])
def test_streamed_equals_default_path(K):
    p = synth.make_pileup(2500, 8000, min(K, 40), seed=1800 + K, mean_entries=300, min_entries=20, max_entries=5000,
                          reads_lambda=0.6, doublet_frac=0.15, with_gp=False)
    assert int(np.max(np.diff(p.cell_ptr))) > 2048  # long cells: the wave plan's parts
    _same_runs(_run(p, K), _run(p, K, XE))


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from popscle_amd import muxgl, synth
p = synth.make_pileup(300, 3000, 30, seed=1901, mean_entries=200, min_entries=20, max_entries=3000, reads_lambda=0.6,
                      with_gp=False)
with muxgl.Engine(0) as e:
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    llk0, llk2, _, _ = e.fmx_prepare(p.af)
    e.fmx_set_clusters(300, e.fmx_greedy_init(300, llk2 - llk0))
    recs = [e.fmx_iterate(0.5, 0.1)[0] for _ in range(3)]
np.save(sys.argv[2], np.stack(recs))
"""


def _child(tmp_path, name, slab_mb):
    env = dict(os.environ)
    env.pop("MUXGL_FMX_SLAB_MB", None)
    if slab_mb:
        env["MUXGL_FMX_SLAB_MB"] = str(slab_mb)
    out = str(tmp_path / (name + ".npy"))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


def test_budget_does_not_change_records(tmp_path):
    base = _child(tmp_path, "default", 0)
    # 1 MB: 32 (cell, block) slabs a group -- fewer than the 300 cells, so one block x 32 cells at a time
    # 40 MB: all cells x 4 of the 15 blocks a group
    for mb in (1, 40):
        got = _child(tmp_path, f"mb{mb}", mb)
        for a, b in zip(base, got):
            assert a.tobytes() == b.tobytes(), mb


@needs_ref
def test_ties_against_reference():
    # duplicated cells and clusters without cells score identically: deep ties in both scans
    p0 = synth.make_pileup(12, 2000, 6, seed=2001, mean_entries=100, min_entries=20, max_entries=200,
                           reads_lambda=0.8, with_gp=False)
    p = _duplicate(p0, 3)
    K = 280
    init = np.full(p.C, -1, dtype=np.int32)
    init[: p.C // 2] = (np.arange(p.C // 2) * 37) % K
    ref = rb.RefScl.from_packed(p).freemux2(K, init_clust=init, cluster_pileups=True)
    _check_vs_ref(p, K, ref, init=init)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.fmx_prepare(p.af)
        e.fmx_set_clusters(K, init)
        cells, _ = e.fmx_iterate(0.5, 0.1)
        near, _, _ = e.fmx_exact_stats()
    assert near > 0
    deep = (cells["sngNextLLK"] == cells["sngThirdLLK"]) | (cells["dblNextLLK"] == cells["dblThirdLLK"])
    assert deep.any()


def _duplicate(p, n):
    """the pileup with every cell repeated n times in a row"""
    lens = np.diff(p.cell_ptr)
    cell_ptr = [0]
    es, er_lens, reads = [], [], []
    rl = np.diff(p.entry_rptr)
    for c in range(p.C):
        e0, e1 = p.cell_ptr[c], p.cell_ptr[c + 1]
        for _ in range(n):
            es.append(p.entry_snp[e0:e1])
            er_lens.append(rl[e0:e1])
            reads.append(p.reads[p.entry_rptr[e0]:p.entry_rptr[e1]])
            cell_ptr.append(cell_ptr[-1] + lens[c])
    return synth.Pileup(C=p.C * n, S=p.S, cell_ptr=np.array(cell_ptr, dtype=np.int64),
                        entry_snp=np.concatenate(es).astype(np.int32),
                        entry_rptr=np.concatenate([[0], np.cumsum(np.concatenate(er_lens))]).astype(np.int64),
                        reads=np.concatenate(reads).astype(p.reads.dtype), af=p.af)


def test_limits():
    p = synth.make_pileup(60, 2000, 8, seed=2101, mean_entries=100, min_entries=20, max_entries=200, with_gp=False)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        clust = e.fmx_greedy_init(muxgl.MAX_CLUSTERS, llk2 - llk0)
        assert clust.max() < muxgl.MAX_CLUSTERS
        e.fmx_set_clusters(muxgl.MAX_CLUSTERS, clust)
        cells, _ = e.fmx_iterate(0.5, 0.1)
        assert (cells["type"] >= 0).all()
        with pytest.raises(muxgl.MuxglError, match="full_ll"):
            e.fmx_iterate(0.5, 0.1, want_full_ll=True)
        for call in (lambda: e.fmx_greedy_init(muxgl.MAX_CLUSTERS + 1, llk2 - llk0),
                     lambda: e.fmx_set_clusters(muxgl.MAX_CLUSTERS + 1, clust)):
            with pytest.raises(muxgl.MuxglError, match="MUXGL_MAX_CLUSTERS"):
                call()
    with muxgl.Engine(0, XE) as e:  # the flag at K <= 255: full_ll refused as well
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        e.fmx_set_clusters(40, e.fmx_greedy_init(40, llk2 - llk0))
        with pytest.raises(muxgl.MuxglError, match="full_ll"):
            e.fmx_iterate(0.5, 0.1, want_full_ll=True)


@pytest.mark.parametrize("flags", [0, muxgl.FLAG_ASYNC_PHASES])
def test_device_group_equals_one_handle(flags):
    K = 300
    p = synth.make_pileup(400, 4000, 30, seed=2201, mean_entries=150, min_entries=20, max_entries=1000,
                          reads_lambda=0.6, with_gp=False)
    c0, one, _ = _run(p, K, iters=3)
    with muxgl.Engine([0, 0], flags) as g:
        g.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        g.fmx_prepare(p.af)
        g.fmx_set_clusters(K, c0)
        for cells, st, (gls, cnt) in one:
            got, gst = g.fmx_iterate(0.5, 0.1)
            assert tuple(gst) == tuple(st)
            parity.same_records(got, cells)
            g2, c2 = g.fmx_cluster_pileup()
            assert np.array_equal(c2, cnt) and np.array_equal(g2, gls)
        with pytest.raises(muxgl.MuxglError, match="full_ll"):
            g.fmx_iterate(0.5, 0.1, want_full_ll=True)
