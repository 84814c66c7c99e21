"""Numpy restatement of muxgl_fmx_match_donors (include/muxgl.h), the definition its GPU tests are held to.  Plain sums
of logs, one log per factor, every (cluster, donor) sum with math.fsum (exactly rounded): nothing of the device's
products, parts or butterflies."""
import math

import numpy as np


def restate_match(gls, counts, gp, has_gp, af):
    """gls [K][S][9], counts [K][S][3] as Engine.fmx_cluster_pileup() returns them; gp [S][V][3], has_gp [S] as handed to
    demux_set_gp (rows of markers without genotypes are never read); af [S].  Returns ll [K][V], ll0 [K], nsnps [K]."""
    gls = np.asarray(gls, dtype=np.float64)
    gp = np.asarray(gp, dtype=np.float64)
    af = np.asarray(af, dtype=np.float64)
    K, S = gls.shape[:2]
    V = gp.shape[1]
    ll = np.zeros((K, V))
    ll0 = np.zeros(K)
    nsnps = np.zeros(K, dtype=np.int32)
    hwe = np.stack([(1.0 - af) * (1.0 - af), 2.0 * af * (1.0 - af), af * af], axis=-1)   # [S][3]
    for k in range(K):
        u = np.flatnonzero((np.asarray(has_gp) != 0) & (np.asarray(counts)[k, :, 0] > 0))
        nsnps[k] = u.size
        if u.size == 0:
            continue
        L = gls[k][u][:, (0, 4, 8)]                                # [U][3]
        with np.errstate(divide="ignore"):
            f = np.log(L[:, None, 0] * gp[u, :, 0] + L[:, None, 1] * gp[u, :, 1] + L[:, None, 2] * gp[u, :, 2])   # [U][V]
            f0 = np.log(L[:, 0] * hwe[u, 0] + L[:, 1] * hwe[u, 1] + L[:, 2] * hwe[u, 2])
        for v in range(V):
            ll[k, v] = -math.inf if np.isneginf(f[:, v]).any() else math.fsum(f[:, v])
        ll0[k] = -math.inf if np.isneginf(f0).any() else math.fsum(f0)
    return ll, ll0, nsnps
