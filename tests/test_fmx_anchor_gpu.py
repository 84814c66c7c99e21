"""Anchored freemuxlet (muxgl_fmx_set_anchors): clusters 0 .. n-1 held to genotyped donors, the others learned, in one EM.

The reference is the oracle itself, unchanged (tests/fmx_anchor_ref.py): the panel's rows are the posterior rows the oracle
forms from diagonals written into the anchored clusters' pileups, bit for bit, so the bar is the one
tests/test_fmx_gpu.py::run_em sets for plain runs -- full_ll within 1e-7, every integer field of every record exact, the
three counters equal, the cluster pileups (the anchored clusters' droplet-derived ones included) allclose at rtol 1e-11,
over the whole trajectory, no cell left out.  One case per E-step path and edge of the kernel's lane mapping; then the
exact near-tie path, what needs no reference, the tables, determinism and the state rules, device groups, and the start
plan with the two drivers."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fmx_anchor_ref as ar
import oracle_binding as ob
import parity
from popscle_amd import freemuxlet, muxgl, plpio, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "popscle_amd", "bin", "popscle-amd")
XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
ITERS = 2


def make_case(C, S, ment, V, seed, hole_frac=0.2, n_true=None, min_entries=30):
    """droplets of n_true donors without a panel; a panel of V donors -- the true ones first, unrelated ones behind -- as
    diagonals d [S][V][3] (tests/fmx_anchor_ref.py), with a fraction of the markers without genotypes"""
    n_true = min(V, 8) if n_true is None else n_true
    p = synth.make_pileup(C, S, n_true, seed=seed, mean_entries=ment, min_entries=min_entries, with_gp=False)
    rng = np.random.default_rng([seed, 77])
    G = np.empty((S, V), dtype=np.int64)
    m = min(V, n_true)
    G[:, :m] = p.truth["G"][:, :m]
    G[:, m:] = rng.binomial(2, p.af[:, None], size=(S, V - m))
    has_gp = (rng.random(S) >= hole_frac).astype(np.uint8)
    return p, ar.draw_diag(G, has_gp), has_gp


def random_start(C, K, seed):
    rng = np.random.default_rng([seed, 3])
    c = rng.integers(0, K, C).astype(np.int32)
    c[rng.random(C) < 0.1] = -1
    return c


PERM39 = [int(x) for x in np.random.default_rng(39).permutation(40)[:39]]  # V = 40 > 32: other panel layouts on the device

#        name            K    n   C    S     ment V    donors            ge   holes flags full   pileups
TRAJ = [("k4",           4,   2,  200, 1001, 200, 2,   [0, 1],           0.1, 0.2,  0,    True,  True),   # 2002 lanes: no multiple of 256
        ("k5_twice",     5,   3,  150, 999,  150, 3,   [2, 0, 2],        0.1, 0.2,  0,    True,  True),   # one donor in two clusters
        ("k16_all",      16,  16, 120, 1500, 250, 16,  list(range(16)),  0.1, 0.2,  0,    True,  True),   # no free cluster
        ("k20_one",      20,  1,  100, 1203, 300, 3,   [1],              0.1, 0.2,  0,    True,  True),
        ("k20_blank",    20,  1,  100, 1203, 300, 1,   [0],              0.1, 1.0,  0,    True,  True),   # a donor without genotypes anywhere
        ("k27",          27,  26, 60,  2000, 300, 26,  list(range(26)),  0.0, 0.2,  0,    True,  True),   # geno_error 0
        ("k40",          40,  39, 40,  3001, 400, 40,  PERM39,           0.1, 0.2,  0,    True,  True),
        ("k40_streamed", 40,  39, 40,  3001, 400, 40,  PERM39,           0.1, 0.2,  XE,   False, True),   # full_ll is refused there
        ("k260",         260, 130, 24, 800,  100, 130, list(range(130)), 0.1, 0.2,  0,    False, False)]  # records only


@pytest.mark.parametrize("name,K,n,C,S,ment,V,donors,ge,holes,flags,full,pileups", TRAJ, ids=[t[0] for t in TRAJ])
def test_anchored_trajectory_vs_oracle(name, K, n, C, S, ment, V, donors, ge, holes, flags, full, pileups):
    assert len(donors) == n
    if name == "k4":
        assert (S * n) % 256 != 0   # the last block of the anchor kernel is a partial one
    p, d, has_gp = make_case(C, S, ment, V, seed=8100 + K + n, hole_frac=holes)
    with muxgl.Engine(0, flags) as e:
        worst, _, _ = ar.run_anchored_em(e, p, K, ITERS, donors, d, has_gp, clust=random_start(p.C, K, K), geno_error=ge,
                                         want_full=full, want_pileups=pileups)
    assert worst < 1e-7


@pytest.mark.parametrize("K,n,V", [(20, 7, 9), (40, 11, 40)])
@pytest.mark.parametrize("path", ["row", "wave", "pair"])
def test_anchored_trajectory_on_the_flag_engines(path, K, n, V):
    """the 'row', 'wave' and 'pair' engines of tests/test_fmx_gpu.py's fixture"""
    flags = {"row": muxgl.FLAG_FORCE_ROW_KERNEL, "wave": muxgl.FLAG_FORCE_WAVE_KERNEL, "pair": muxgl.FLAG_FORCE_TILE_SWEEP}[path]
    p, d, has_gp = make_case(60, 1501, 250, V, seed=8300 + K)
    donors = [int(x) for x in np.random.default_rng(K).permutation(V)[:n]]
    with muxgl.Engine(0, flags) as e:
        worst, _, _ = ar.run_anchored_em(e, p, K, ITERS, donors, d, has_gp, clust=random_start(p.C, K, K))
    assert worst < 1e-7


def test_near_ties_are_settled_as_the_reference_does():
    """the shape of test_fmx_gpu.py::test_near_tie_calls_are_settled_as_the_reference_does: droplets of a handful of entries,
    two anchors naming ONE donor (exact ties in the reference, the scan order decides), two free clusters without cells.
    Every integer field, the counters and the pileups equal the oracle's, and the exact path decided cells."""
    K = 6
    p, d, has_gp = make_case(300, 400, 8, 2, seed=906, n_true=3, min_entries=1)
    rng = np.random.default_rng(K)
    clust = rng.integers(0, 4, p.C).astype(np.int32)   # clusters 4 and 5 stay empty
    clust[rng.random(p.C) < 0.1] = -1
    with muxgl.Engine(0) as e:
        worst, _, _ = ar.run_anchored_em(e, p, K, 3, [1, 1], d, has_gp, clust=clust)
        near, changed, unresolved = e.fmx_exact_stats()
    print(f"{near} near-tie cell-iterations settled by the exact path, {changed} decided differently from the kernels")
    assert worst < 1e-7 and near > 0 and unresolved == 0


def test_without_genotypes_an_anchor_is_an_empty_cluster_bit_for_bit():
    """No reference needed: a panel without a single genotype, all cells unassigned, one iteration.  full_ll and the records
    are bit-identical to the same handle without anchors, and two clusters anchored to one donor have bit-equal columns."""
    K = 5
    p, d, has_gp = make_case(80, 700, 120, 2, seed=8501, hole_frac=1.0)
    assert not has_gp.any()
    none = np.full(p.C, -1, dtype=np.int32)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.fmx_prepare(p.af)
        e.demux_set_gp(ar.device_panel(ar.panel_rows(d, p.af, 0.1), has_gp), has_gp)
        e.fmx_set_clusters(K, none)
        plain, pst, pfull = e.fmx_iterate(0.5, 0.1, want_full_ll=True)
        psng = e.fmx_singlets()
        e.fmx_set_clusters(K, none)
        e.fmx_set_anchors([1, 1])
        got, gst, gfull = e.fmx_iterate(0.5, 0.1, want_full_ll=True)
        gsng = e.fmx_singlets()
    assert gfull.tobytes() == pfull.tobytes()
    assert got.tobytes() == plain.tobytes() and tuple(gst) == tuple(pst)
    assert gsng[:, 0].tobytes() == gsng[:, 1].tobytes() and gsng.tobytes() == psng.tobytes()


@pytest.mark.parametrize("K,n,V", [(4, 2, 2), (40, 12, 40)])
def test_tables_read_the_anchored_posteriors(K, n, V):
    """after an anchored E-step muxgl_fmx_singlets is "this droplet against donor j in freemuxlet's model": the diagonal
    slots of the oracle's full_ll, within 1e-7 (TABLE_TOL's value); the other two tables run on the same posteriors"""
    p, d, has_gp = make_case(60, 1200, 200, V, seed=8600 + K)
    donors = list(range(n))
    with muxgl.Engine(0) as e:
        _, cells, ofull = ar.run_anchored_em(e, p, K, 1, donors, d, has_gp, clust=random_start(p.C, K, K))
        sng = e.fmx_singlets()
        incl = e.fmx_inclusion(0.5)
        unk = e.fmx_unknown()
    j = np.arange(K)
    want = ofull[:, j * (j + 1) // 2 + j]
    dev = np.abs(sng - want)
    print(f"K={K}: fmx_singlets against the oracle's diagonal, max deviation {dev.max():.3e}")
    assert dev.max() < 1e-7
    assert incl["incl"].shape == (p.C, K) and np.isfinite(incl["tot"]).all() and unk["ll_ju"].shape == (p.C, K)


def _anchored(e, p, K, donors, d, has_gp, clust, iters=ITERS, ge=0.1):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.fmx_prepare(p.af)
    panel = ar.device_panel(ar.panel_rows(d, p.af, ge), has_gp)
    e.demux_set_gp(panel, has_gp)
    e.fmx_set_clusters(K, clust)
    e.fmx_set_anchors(donors)
    return [e.fmx_iterate(0.5, ge) for _ in range(iters)], panel


def _plain_from(e, p, K, clust, ge=0.1):
    e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    e.fmx_prepare(p.af)
    e.fmx_set_clusters(K, clust)
    return e.fmx_iterate(0.5, ge)


def test_two_handles_give_identical_records():
    K, donors = 20, [3, 0, 5, 1]
    p, d, has_gp = make_case(120, 1500, 200, 6, seed=8701)
    clust = random_start(p.C, K, 1)
    with muxgl.Engine(0) as a, muxgl.Engine(0) as b:
        ra, _ = _anchored(a, p, K, donors, d, has_gp, clust)
        rb, _ = _anchored(b, p, K, donors, d, has_gp, clust)
    for (ca, sa), (cb, sb) in zip(ra, rb):
        assert ca.tobytes() == cb.tobytes() and tuple(sa) == tuple(sb)


def test_removing_the_anchors_gives_a_plain_iteration():
    """fmx_set_anchors([]) after an anchored iteration, then an iteration: the records of a handle that never anchored and
    starts from the anchored iteration's assignments (the same cluster pileups, built in the same order)"""
    K, donors = 6, [2, 0]
    p, d, has_gp = make_case(200, 1200, 150, 3, seed=8702, min_entries=3)
    clust = random_start(p.C, K, 2)
    with muxgl.Engine(0) as a, muxgl.Engine(0) as b:
        (first, _), = _anchored(a, p, K, donors, d, has_gp, clust, iters=1)[0]
        a.fmx_set_anchors([])
        assert a.n_anchor == 0
        with pytest.raises(muxgl.MuxglError):
            a.fmx_singlets()                       # the tables are refused until the next E-step
        got, gst = a.fmx_iterate(0.5, 0.1)
        gsng = a.fmx_singlets()
        want, wst = _plain_from(b, p, K, first["clust"])
        wsng = b.fmx_singlets()
    assert got.tobytes() == want.tobytes() and tuple(gst[:2]) == tuple(wst[:2])
    assert gsng.tobytes() == wsng.tobytes()


def test_a_new_panel_drops_the_anchors():
    """set_clusters -> set_anchors -> iterate -> demux_set_gp, on a handle that has done other work and on a fresh one: no
    anchors afterwards, and the next iteration is a plain one"""
    K, donors = 6, [1, 2]
    p, d, has_gp = make_case(200, 1200, 150, 3, seed=8703, min_entries=3)
    q, dq, hq = make_case(50, 300, 40, 2, seed=8704)
    clust = random_start(p.C, K, 3)
    with muxgl.Engine(0) as used, muxgl.Engine(0) as fresh, muxgl.Engine(0) as b:
        _anchored(used, q, 4, [0], dq, hq, random_start(q.C, 4, 4))     # other work first
        outs = []
        for e in (used, fresh):
            ((first, _),), panel = _anchored(e, p, K, donors, d, has_gp, clust, iters=1)
            e.demux_set_gp(panel, has_gp)
            assert e.n_anchor == 0
            outs.append((first, e.fmx_iterate(0.5, 0.1)))
        assert outs[0][0].tobytes() == outs[1][0].tobytes()
        want, wst = _plain_from(b, p, K, outs[0][0]["clust"])
    for first, (got, gst) in outs:
        assert got.tobytes() == want.tobytes() and tuple(gst[:2]) == tuple(wst[:2])


def _refused(e, match, n, donors):
    """the C call itself: non-zero, the message names the cause"""
    arr = None if donors is None else np.ascontiguousarray(donors, dtype=np.int32)
    rc = e.lib.muxgl_fmx_set_anchors(e.h, n, None if arr is None else arr.ctypes.data_as(muxgl._VP))
    msg = e.lib.muxgl_last_error(e.h).decode()
    assert rc != 0 and match in msg, (rc, msg)


def test_refusals_leave_the_handle_usable():
    K = 4
    p, d, has_gp = make_case(60, 600, 100, 3, seed=8705)
    panel = ar.device_panel(ar.panel_rows(d, p.af, 0.1), has_gp)
    clust = random_start(p.C, K, 5)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.fmx_prepare(p.af)
        _refused(e, "no clusters set", 1, [0])
        e.fmx_set_clusters(K, clust)
        _refused(e, "no genotype panel", 1, [0])
        e.fmx_set_anchors([])                                  # removing nothing is fine without a panel
        e.demux_set_gp(panel, has_gp)
        _refused(e, "outside [0, K=4]", K + 1, [0] * (K + 1))
        _refused(e, "outside [0, K=4]", -1, None)
        _refused(e, "outside [0, V=3)", 2, [0, 3])
        _refused(e, "outside [0, V=3)", 1, [-1])
        _refused(e, "donor is NULL", 2, None)
        with pytest.raises(muxgl.MuxglError, match="outside"):
            e.fmx_set_anchors([0, 7])
        assert e.n_anchor == 0
        e.fmx_set_shard(0, p.C // 2, 0, p.S)
        _refused(e, "sharded", 1, [0])
        e.fmx_set_shard(0, p.C, 0, p.S)
        e.fmx_set_anchors([2, 0])                              # the next valid call succeeds
        assert e.n_anchor == 2
        got, _ = e.fmx_iterate(0.5, 0.1)
    with muxgl.Engine(0) as f:
        ((want, _), _), _ = _anchored(f, p, K, [2, 0], d, has_gp, clust)
    assert got.tobytes() == want.tobytes()
    with muxgl.Engine(0) as s:                                 # a caller's own slabs
        (c_ranges, _), (s_ranges, _) = freemuxlet.plan_ranges(p.C, p.S, 1)
        freemuxlet.load_rank(s, p, c_ranges[0], s_ranges[0])
        s.demux_set_gp(panel, has_gp)
        s.fmx_set_clusters(K, clust)
        _refused(s, "holds slabs", 1, [0])
        s.fmx_iter_gp(0.5, 0.1)                                # still works


@pytest.mark.parametrize("K,n,V", [(4, 2, 3), (40, 17, 40)])
def test_device_group_equals_one_device(K, n, V):
    p, d, has_gp = make_case(90, 1300, 200, V, seed=8800 + K)
    donors = [int(x) for x in np.random.default_rng(K + 1).permutation(V)[:n]]
    clust = random_start(p.C, K, 6)
    with muxgl.Engine(0) as one, muxgl.Engine([0, 0]) as grp:
        r1, _ = _anchored(one, p, K, donors, d, has_gp, clust)
        r2, _ = _anchored(grp, p, K, donors, d, has_gp, clust)
        assert grp.n_anchor == n
        g1, g2 = one.fmx_cluster_pileup(), grp.fmx_cluster_pileup()
    for (ca, sa), (cb, sb) in zip(r1, r2):
        assert ca.tobytes() == cb.tobytes() and tuple(sa) == tuple(sb)
    assert g1[0].tobytes() == g2[0].tobytes() and np.array_equal(g1[1], g2[1])


# ---- the start plan and the two drivers ----------------------------------------------------------------------------------

POOL = dict(C=400, S=1500, n_true=6, known=[4, 1, 0], K=6)


def _pool(seed=8900):
    p = synth.make_pileup(POOL["C"], POOL["S"], POOL["n_true"], seed=seed, mean_entries=200, min_entries=30, with_gp=False)
    G = p.truth["G"][:, POOL["known"]].astype(np.int64)
    return p, G


def test_run_em_from_the_default_start_follows_the_oracle():
    K, n = POOL["K"], len(POOL["known"])
    p, G = _pool()
    has_gp = (np.random.default_rng(1).random(p.S) >= 0.2).astype(np.uint8)
    d = ar.draw_diag(G, has_gp)
    donors = list(range(n))
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        greedy = e.fmx_greedy_init(K, llk2 - llk0)
        e.fmx_set_clusters(K, greedy)
        e.demux_set_gp(ar.device_panel(ar.panel_rows(d, p.af, 0.1), has_gp), has_gp)
        m = e.fmx_match_donors()
        plan = freemuxlet.anchor_start(m["ll"] - m["ll0"][:, None], m["nsnps"], np.bincount(greedy[greedy >= 0], minlength=K),
                                       donors, K)
        print("start plan:", plan)
        clust0 = np.where(greedy >= 0, plan["new_id"][np.clip(greedy, 0, K - 1)], -1).astype(np.int32)
        recs, hist = freemuxlet.run_em(e, K, clust0, max_iter=3, early_stop=False, anchors=donors)
        assert e.n_anchor == n
    eo = ob.fmx_entry_pileup(p)
    cplp = ob.fmx_build_cluster_pileup(p, eo, K, clust0)
    cells = ob.fmx_init_cells(clust0)
    for it in range(len(hist)):
        ar.write_diagonals(cplp, d, donors)
        ost = ob.fmx_iterate(p, eo, K, cplp, cells, 0.5, 0.1, nthreads=4)
        assert tuple(hist[it]) == tuple(ost[:3]), (it, hist[it], ost)
    rep = parity.compare_fmx(recs, cells)
    assert rep["max_abs_ll_diff"] < 1e-7


def test_freemuxlet_cli_anchor_vcf(tmp_path):
    """in the manner of tests/test_fmx_unknown_cli_gpu.py"""
    K, n = POOL["K"], len(POOL["known"])
    p, G = _pool()
    prefix, vcf = str(tmp_path / "plp"), str(tmp_path / "known.vcf.gz")
    plpio.write_plp(prefix, p, seed=9)
    plpio.write_vcf(vcf, p, G, missing_frac=0.02, drop_snps=range(0, p.S, 37))
    out = str(tmp_path / "out")
    base = [BIN, "freemuxlet", "--plp", prefix, "--nsample", str(K)]
    r = subprocess.run(base + ["--out", out, "--anchor-vcf", vcf, "--field", "GT"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    made = sorted(os.path.basename(x)[len("out"):] for x in os.listdir(tmp_path) if os.path.basename(x).startswith("out."))
    assert made == sorted([".lmix", ".clust1.samples.gz", ".clust1.vcf.gz", ".clust1.anchors.gz", ".clust1.match.gz",
                           ".clust1.match.best.gz"])
    lines = gzip.open(out + ".clust1.anchors.gz", "rt").read().splitlines()
    assert lines[0] == "CLUST\tSM_ID\tSTART.CLUST\tSTART.LLR\tN.SNG" and len(lines) == 1 + K
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [r_[0] for r_ in rows] == [str(k) for k in range(K)]
    assert [r_[1] for r_ in rows] == ["S0", "S1", "S2"] + ["NA"] * (K - n)     # the VCF's sample names, in its order
    assert all(r_[2] == "NA" and r_[3] == "NA" for r_ in rows[n:])
    starts = [r_[2] for r_ in rows[:n] if r_[2] != "NA"]
    assert len(set(starts)) == len(starts) and all(0 <= int(x) < K for x in starts)
    with gzip.open(out + ".clust1.samples.gz", "rt") as f:
        srows = [ln.rstrip("\n").split("\t") for ln in f.readlines()[1:]]
    for k in range(K):   # N.SNG: the droplets called singlets of the cluster
        assert int(rows[k][4]) == sum(1 for s in srows if s[4] == "SNG" and s[5] == f"{k},{k}")
    match = gzip.open(out + ".clust1.match.gz", "rt").read().splitlines()
    assert len(match) == 1 + K * n

    # --init-cluster: the file's ids as they are, no start match; one device and a group of two give the same files
    initf = str(tmp_path / "init.txt")
    with open(initf, "w") as f:
        for i, s in enumerate(srows):
            if i % 9:   # (some droplets start unassigned)
                f.write(f"{s[1]}\t{(i * 5) % K}\n")
    one, grp = str(tmp_path / "one"), str(tmp_path / "grp2")
    for o, extra in ((one, []), (grp, ["--devices", "0,0"])):
        r = subprocess.run(base + ["--out", o, "--anchor-vcf", vcf, "--field", "GT", "--init-cluster", initf] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
    for suffix in (".clust1.samples.gz", ".clust1.anchors.gz"):
        assert gzip.open(one + suffix, "rb").read() == gzip.open(grp + suffix, "rb").read(), suffix
    rows2 = [ln.split("\t") for ln in gzip.open(grp + ".clust1.anchors.gz", "rt").read().splitlines()[1:]]
    assert [r_[1] for r_ in rows2] == ["S0", "S1", "S2"] + ["NA"] * (K - n) and all(r_[2] == "NA" for r_ in rows2)
    assert os.path.exists(one + ".clust1.match.gz") and not os.path.exists(grp + ".clust1.match.gz")

    r = subprocess.run(base + ["--out", str(tmp_path / "both"), "--anchor-vcf", vcf, "--match-vcf", vcf], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "--match-vcf cannot be combined with --anchor-vcf" in r.stderr
    assert "against the anchor panel" in r.stderr
    r = subprocess.run(base + ["--out", str(tmp_path / "grp"), "--anchor-vcf", vcf, "--devices", "0,0"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "needs --init-cluster" in r.stderr
    r = subprocess.run([BIN, "freemuxlet", "--plp", prefix, "--nsample", "2", "--out", str(tmp_path / "few"), "--anchor-vcf", vcf,
                        "--field", "GT"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "must be at least that" in r.stderr
