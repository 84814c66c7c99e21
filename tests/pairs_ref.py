"""Numpy restatement of muxgl_fmx_cluster_pairs (include/muxgl.h), the definition its GPU tests are held to.  Plain sums of
logs, one log per factor, every pair's sum with math.fsum (exactly rounded): nothing of the device's products, parts,
packed partner rows or butterflies.  llk0 is the double sum over (gi, gj) as the reference writes it
(cmd_cram_freemuxlet.cpp:208), not the product of two marginals the kernel forms."""
import math

import numpy as np


def pair_index(a, b):
    """position of the pair a > b in the triangle"""
    return a * (a - 1) // 2 + b


def restate_pairs(gls, counts, af):
    """gls [K][S][9], counts [K][S][3] as Engine.fmx_cluster_pileup() returns them; af [S].  Returns llk2, llk0 (float64)
    and nsnps (int32), each [K (K - 1) / 2] with the pair a > b at a (a - 1) / 2 + b."""
    gls = np.asarray(gls, dtype=np.float64)
    af = np.asarray(af, dtype=np.float64)
    K = gls.shape[0]
    n = K * (K - 1) // 2
    llk2, llk0, nsnps = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    member = np.asarray(counts)[:, :, 0] > 0                                              # [K][S]
    p = np.stack([(1.0 - af) * (1.0 - af), 2.0 * af * (1.0 - af), af * af], axis=-1)      # [S][3], gps of :200-203
    L = gls[:, :, (0, 4, 8)]                                                              # [K][S][3]
    for a in range(1, K):
        if not member[a].any():
            continue
        ua = np.flatnonzero(member[a])                                                    # (the markers of a: all b < a at once)
        la, lb, pu = L[a][ua], L[:a][:, ua], p[ua]                                        # [U][3], [a][U][3], [U][3]
        lk2 = np.zeros((a, ua.size))
        lk0 = np.zeros((a, ua.size))
        for gi in range(3):                                                               # the loop of :205-210, in its order
            lk2 += la[:, gi] * lb[:, :, gi] * pu[:, gi]
            for gj in range(3):
                lk0 += la[:, gi] * lb[:, :, gj] * pu[:, gi] * pu[:, gj]
        with np.errstate(divide="ignore", invalid="ignore"):
            f2, f0 = np.log(lk2), np.log(lk0)
        for b in range(a):
            u = member[b][ua]
            i = pair_index(a, b)
            nsnps[i] = int(u.sum())
            if nsnps[i] == 0:
                continue
            g2, g0 = f2[b][u], f0[b][u]
            llk2[i] = -math.inf if np.isneginf(g2).any() else math.fsum(g2)
            llk0[i] = -math.inf if np.isneginf(g0).any() else math.fsum(g0)
    return llk2, llk0, nsnps
