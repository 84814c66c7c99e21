"""Reference values of muxgl_fmx_ambient (include/muxgl.h) for its tests.

entry_weights() / table(): a plain restatement.  The reference's per-read loop (sc_drop_seq.cpp:452-509 at alpha = 0.5)
runs with 3 * n_rho ambient elements carried along the entry's nine, one per (rho, l), whose expected ALT fraction is
p = 0.5 * l + (2 * f - l) * 0.5 * rho with f the ambient ALT fraction of the marker.  They are divided by the same
per-read sum t and the same final sum T as the nine and take part in neither; after the reads they are floored at 1e-6
like the nine.  Then ll_amb[c][j][r] = sum_e log((q[j][0] w[r][0] + q[j][1] w[r][1]) + q[j][2] w[r][2]), added in entry
order.  Elementwise numpy over the elements of one entry: every operation is the reference's, on IEEE doubles, in its
order (numpy fuses nothing), with the Phred tables of the oracle (pow(0.1, i * 0.1), 0.75 at i <= 1).  p is formed as
(2 f - l) * (0.5 rho) + 0.5 l; the device forms it with one fma -- the same number wherever the product is exact, which
covers the three identities, and within an ulp elsewhere.

oracle_slots(): identity 1 from the oracle itself.  With f in {0, 0.5, 1} per marker and rho = 0.5 the ambient RNA is a
donor of genotype 2 f: the oracle's E-step with one cluster appended whose pileup diagonal is one-hot at 2 f[s]
(fmx_anchor_ref.write_diagonals; at geno_error = 0 and af strictly inside (0, 1) its posterior row is exactly one-hot)
holds ll_amb[c][j] in slot (K, j) of its triangle."""
import numpy as np

import fmx_anchor_ref as far
import oracle_binding as ob
from popscle_amd import muxgl, synth

READ_OTHER = synth.READ_OTHER
ERR, MAT = ob.phred_tables()
MIN_NORM_GL = 1e-6                                                        # sc_drop_seq.h:14
FRAC_REF = np.array([1.0, .75, .5, .75, .5, .25, .5, .25, 0.0])           # :483-491 at alpha = 0.5, a REF read
FRAC_ALT = FRAC_REF[::-1].copy()                                          # ... an ALT read
DEFAULT_RHOS = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)                 # the front end's default grid


def ambient_p(f, rhos):
    """p of the 3 * n_rho ambient elements, order r * 3 + l"""
    return np.array([(2.0 * float(f) - l) * (0.5 * float(r)) + 0.5 * l for r in rhos for l in range(3)])


def entry_weights(reads, pa):
    """:452-509 for one entry with the ambient elements carried along: (w [n_rho][3], the entry's nine likelihoods)"""
    g = np.ones(9)
    a = np.ones(pa.size)
    qa = 1.0 - pa
    for b in reads:
        b = int(b)
        if b == READ_OTHER:                                   # :468
            continue
        al, bq = b >> 7, b & 0x7F
        mat, e4 = float(MAT[bq]), float(ERR[bq]) / 4.
        g *= (mat * (FRAC_ALT if al else FRAC_REF) + e4)      # :483-491
        a *= (mat * (pa if al else qa) + e4)
        t = 0.0
        for x in g:                                           # :493, in index order
            t += x
        g /= t                                                # :494
        a /= t
    g[g < MIN_NORM_GL] = MIN_NORM_GL                          # :498-501
    a[a < MIN_NORM_GL] = MIN_NORM_GL
    t = 0.0
    for x in g:
        t += x
    return (a / t).reshape(-1, 3), g / t                      # :502-504


def all_weights_plain(p, amb_af, rhos):
    """(w [nnz][n_rho][3], nine [nnz][9]) of every entry of pileup p, entry by entry through entry_weights()"""
    NR = len(rhos)
    w = np.zeros((p.nnz, NR, 3))
    nine = np.zeros((p.nnz, 9))
    for e in range(p.nnz):
        pa = ambient_p(amb_af[int(p.entry_snp[e])], rhos)
        w[e], nine[e] = entry_weights(p.reads[int(p.entry_rptr[e]):int(p.entry_rptr[e + 1])], pa)
    return w, nine


def all_weights(p, amb_af, rhos):
    """the same numbers as all_weights_plain(), bit for bit (tests/test_fmx_ambient.py), all entries at once: step k
    applies the k-th read of every entry that has one -- the operations of entry_weights() on rows instead of vectors"""
    rh = np.asarray(rhos, dtype=np.float64)
    f = np.asarray(amb_af, dtype=np.float64)[p.entry_snp]
    l = np.arange(3, dtype=np.float64)
    pa = ((2.0 * f[:, None, None] - l[None, None, :]) * (0.5 * rh[None, :, None]) + 0.5 * l[None, None, :]).reshape(p.nnz, -1)
    qa = 1.0 - pa
    g = np.ones((p.nnz, 9))
    a = np.ones_like(pa)
    n = np.diff(p.entry_rptr)
    for k in range(int(n.max()) if p.nnz else 0):
        ent = np.nonzero(n > k)[0]
        b = p.reads[p.entry_rptr[ent] + k]
        use = b != READ_OTHER                                 # :468
        ent, b = ent[use], b[use].astype(np.int64)
        al = (b >> 7).astype(bool)
        mat, e4 = MAT[b & 0x7F][:, None], (ERR[b & 0x7F] / 4.)[:, None]
        ge = g[ent] * (mat * np.where(al[:, None], FRAC_ALT[None, :], FRAC_REF[None, :]) + e4)
        ae = a[ent] * (mat * np.where(al[:, None], pa[ent], qa[ent]) + e4)
        t = np.zeros(ent.size)
        for i in range(9):                                    # :493, in index order
            t = t + ge[:, i]
        g[ent] = ge / t[:, None]
        a[ent] = ae / t[:, None]
    g[g < MIN_NORM_GL] = MIN_NORM_GL                          # :498-501
    a[a < MIN_NORM_GL] = MIN_NORM_GL
    t = np.zeros(p.nnz)
    for i in range(9):
        t = t + g[:, i]
    return (a / t[:, None]).reshape(p.nnz, rh.size, 3), g / t[:, None]


def table_of_weights(p, q, w, ordered=True):
    """ll_amb [C][K][n_rho] from the weights w [nnz][n_rho][3] and the posteriors q [S][K][3]; a factor of 0 gives -inf.
    ordered=False: the logs of a droplet are added by numpy's sum instead of one by one in entry order (the same to a few
    ulp of the sum; for the large cases of the fuzz)"""
    out = np.zeros((p.C, q.shape[1], w.shape[1]))
    for c in range(p.C):
        e0, e1 = int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])
        qe, we = q[p.entry_snp[e0:e1]], w[e0:e1]              # [e][K][3], [e][n_rho][3]
        f = (qe[:, :, None, 0] * we[:, None, :, 0] + qe[:, :, None, 1] * we[:, None, :, 1]) + qe[:, :, None, 2] * we[:, None, :, 2]
        with np.errstate(divide="ignore"):
            lf = np.log(f)                                    # [e][K][n_rho]
        if not ordered:
            out[c] = lf.sum(axis=0)
            continue
        for e in range(e1 - e0):                              # in entry order, as the reference accumulates
            out[c] += lf[e]
    return out


def table(p, q, amb_af, rhos):
    """ll_amb [C][K][n_rho] of pileup p with the cluster posteriors q [S][K][3]"""
    return table_of_weights(p, q, all_weights(p, amb_af, rhos)[0])


def onehot_diag(amb_af):
    """[S][1][3] one-hot at genotype 2 * f; f must be 0, 0.5 or 1 everywhere"""
    m = np.asarray(amb_af, dtype=np.float64) * 2.0
    assert np.isin(m, (0.0, 1.0, 2.0)).all()
    d = np.zeros((m.size, 1, 3))
    d[np.arange(m.size), 0, m.astype(np.int64)] = 1.0
    return d


def oracle_slots(p, eplp, K, cplp, cells, amb_af, nthreads=2):
    """[C][K]: the slots (K, j) of the oracle's E-step (geno_error = 0) on copies of cplp [K][S] with one cluster appended
    whose pileup diagonal is one-hot at 2 * amb_af[s].  cplp and cells stay as they are."""
    ext = np.ascontiguousarray(np.concatenate([cplp, ob.fmx_build_cluster_pileup(p, eplp, 1, np.full(p.C, -1, dtype=np.int32))]))
    far.write_diagonals(ext[K:], onehot_diag(amb_af), [0])
    assert np.array_equal(ext["gls"][K][:, [0, 4, 8]], onehot_diag(amb_af)[:, 0, :])
    *_, full = ob.fmx_iterate(p, eplp, K + 1, ext, cells.copy(), 0.5, 0.0, full_ll=True, nthreads=nthreads)
    rk = K * (K + 1) // 2
    return np.ascontiguousarray(full[:, rk:rk + K])


def draw_onehot_af(S, seed):
    return np.random.default_rng(seed).choice([0.0, 0.5, 1.0], size=S)


def draw_rhos(n, seed):
    """n off-grid rhos in (0, 1), none of them 0, 0.5 or 1"""
    return np.random.default_rng(seed).uniform(0.01, 0.99, size=n)


def assert_table(got, want, tol, what=""):
    """every element within tol; prints and returns the worst deviation"""
    assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape)
    d = np.abs(got - want)
    assert np.isfinite(d).all(), what
    worst = float(d.max()) if d.size else 0.0
    print(f"fmx ambient {what}: shape {got.shape}, max |dLL| {worst:.3e}")
    assert worst <= tol, f"{what}: {int((d > tol).sum())} elements beyond {tol}; worst {worst}"
    return worst


# the pileups of the sanity test (CPU: the restatement, tests/test_fmx_ambient.py; GPU: the device,
# tests/test_fmx_ambient_gpu.py): ambient_ref.soup_pileup with these arguments at soup 0.2 and at soup 0.  The clusters'
# genotypes are learned from the droplets themselves, soup included, so the share a droplet is given falls short of the
# truth until a cluster has many droplets.  Droplets per donor, at 6 donors x 300 markers, doubled from 24 until the
# restatement alone met check_soup_calls on the CPU -- every droplet to its own cluster at every size; droplets by best
# rho on the default grid at soup 0.2 (at soup 0: all at 0 but one droplet at most):
#    24: [92, 44, 8, 0, 0, 0, 0, 0]          median 0         48: [41, 117, 84, 39, 7, 0, 0, 0]        median 0.05
#    96: [17, 143, 226, 151, 36, 3, 0, 0]    median 0.1      192: [12, 146, 400, 406, 175, 13, 0, 0]   median 0.15
SOUP = dict(C=192 * 6, S=1500, V=6, markers=300, seed=11)


def check_soup_calls(ll, who, rhos, soup):
    """the checks of the sanity test on a table of a soup pileup whose clusters were handed in from the truth: every
    droplet's best cluster is its own, and the median best rho is 0 at soup 0, within one grid step of 0.2 at soup 0.2"""
    from popscle_amd import freemuxlet

    sm = freemuxlet.ambient_summary(ll, rhos)
    rh = np.asarray(rhos)
    hist = np.bincount(sm["amb_rho_idx"], minlength=rh.size)
    print(f"soup {soup}: best rho histogram {dict(zip(rh.tolist(), hist.tolist()))}")
    assert np.array_equal(sm["amb_clust"], who)
    med = float(np.median(rh[sm["amb_rho_idx"]]))
    if soup == 0.0:
        assert med == 0.0, med
    else:
        i = int(np.argmin(np.abs(rh - soup)))
        assert rh[max(i - 1, 0)] <= med <= rh[min(i + 1, rh.size - 1)], med
    return sm
