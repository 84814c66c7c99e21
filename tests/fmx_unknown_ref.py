"""What muxgl_fmx_unknown is held to (tests/test_fmx_unknown*.py): a numpy restatement of the three formulas of
include/muxgl.h, and the yardstick itself -- one E-step of the oracle on the cluster pileups with two EMPTY pileups
appended.  A cluster without cells has a pileup of ones, so its posterior row is the Hardy-Weinberg triple of
cmd_cram_freemux2.cpp:388-390, and the slots (K, j), (K, K), (K + 1, K) of the K + 2 cluster triangle are the tables."""
import numpy as np

import oracle_binding as ob


def hardy_weinberg(af):
    """u[S][3] with the expressions of :388-390"""
    af = np.asarray(af, dtype=np.float64)
    return np.ascontiguousarray(np.stack([(1.0 - af) * (1.0 - af), 2 * af * (1.0 - af), af * af], axis=-1))


def unknown_tables(p, egl, q, u):
    """the formulas of include/muxgl.h, entry by entry: (ll_ju [C][K], ll_u [C], ll_uu [C]).  egl [nnz][9], q [S][K][3],
    u [S][3].  A factor of 0 gives -inf."""
    s = p.entry_snp
    g = egl.reshape(-1, 3, 3)                                   # [e][g1][g2]
    ue = u[s]                                                   # [e][3]
    w = (ue[:, 0, None] * g[:, 0, :] + ue[:, 1, None] * g[:, 1, :]) + ue[:, 2, None] * g[:, 2, :]   # [e][g2], g1 ascending
    qe = q[s]                                                   # [e][K][3]
    f_ju = (w[:, None, 0] * qe[:, :, 0] + w[:, None, 1] * qe[:, :, 1]) + w[:, None, 2] * qe[:, :, 2]
    f_u = (g[:, 0, 0] * ue[:, 0] + g[:, 1, 1] * ue[:, 1]) + g[:, 2, 2] * ue[:, 2]
    f_uu = (w[:, 0] * ue[:, 0] + w[:, 1] * ue[:, 1]) + w[:, 2] * ue[:, 2]
    with np.errstate(divide="ignore"):
        l_ju, l_u, l_uu = np.log(f_ju), np.log(f_u), np.log(f_uu)
    K = q.shape[1]
    ju, lu, uu = np.zeros((p.C, K)), np.zeros(p.C), np.zeros(p.C)
    for c in range(p.C):
        for e in range(p.cell_ptr[c], p.cell_ptr[c + 1]):       # in entry order, as the reference accumulates (:454-455)
            ju[c] += l_ju[e]
            lu[c] += l_u[e]
            uu[c] += l_uu[e]
    return ju, lu, uu


def empty_pileup(p, eplp):
    """[1][S]: the pileup of a cluster without cells"""
    return ob.fmx_build_cluster_pileup(p, eplp, 1, np.full(p.C, -1, dtype=np.int32))


def slots(full, K):
    """(ll_ju, ll_u, ll_uu) out of a [C][(K + 2)(K + 3) / 2] triangle"""
    rk, rk1 = K * (K + 1) // 2, (K + 1) * (K + 2) // 2
    return full[:, rk:rk + K].copy(), full[:, rk + K].copy(), full[:, rk1 + K].copy()


def extended_estep(p, eplp, K, cplp, cells, geno_error, doublet_prior=0.5, nthreads=4):
    """the oracle's one E-step on copies of cplp [K][S] (the pileups the posteriors of the wanted iteration are made of)
    with two empty pileups appended: the whole [C][(K + 2)(K + 3) / 2] triangle.  cplp and cells stay as they are."""
    empty = empty_pileup(p, eplp)
    ext = np.ascontiguousarray(np.concatenate([cplp, empty, empty]))
    *_, full = ob.fmx_iterate(p, eplp, K + 2, ext, cells.copy(), doublet_prior, geno_error, full_ll=True, nthreads=nthreads)
    return full


def oracle_tables(p, eplp, K, cplp, cells, geno_error, nthreads=4):
    return slots(extended_estep(p, eplp, K, cplp, cells, geno_error, nthreads=nthreads), K)
