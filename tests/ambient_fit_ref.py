"""Reference values of muxgl_demux_ambient_fit (include/muxgl.h) for its tests, on top of ambient_ref.py.

ll_d1_d2(): LL, LL' and LL'' of one (droplet, sample) at a share rho.  The per-read loop is that of
ambient_ref.entry_weights (multiply, then divide by the grid's maximum, after every read; + 1e-10 and the final maximum at
the end) with the three ambient elements of one rho and their first two derivatives carried along:
    t = pR * (1 - p) + pA * p,  p = 0.5 * l + (2 * f - l) * 0.5 * rho,  v = dt/drho = (pA - pR) * (2 * f - l) * 0.5
    a'' = a'' * t + 2 * a' * v;   a' = a' * t + a * v;   a = a * t
and the derivatives divided by whatever divides a (the 1e-10 is added to a alone: its derivative is 0).  Then
D = sum_l gp[j][l] * w[l], D', D'' likewise, and LL = sum log D, LL' = sum D'/D, LL'' = sum (D''/D - (D'/D)^2) over the
entries whose marker has genotypes.  It runs in float64 and in np.longdouble; the entries of a droplet are walked side by
side (numpy rows), every row in the per-read order above.

bracket(), maximise() (a 65-point scan in longdouble) and fit() are fit_ref_core.py's: they ask a cell for eval() only.

shaped_pileup(): the pileups of the shape tests, for this fit and, through its hook for the donor of a read, for
alpha_fit_ref.shaped_pileup."""
import numpy as np

import ambient_ref as ar
import fit_ref_core as core

READ_OTHER = ar.READ_OTHER


class Cell:
    """the entries of droplet c whose marker has genotypes, for candidate column j, as padded numpy rows"""

    def __init__(self, p, alphas, amb_af, c, j):
        es = [e for e in range(int(p.cell_ptr[c]), int(p.cell_ptr[c + 1])) if p.has_gp[int(p.entry_snp[e])]]
        self.n = len(es)
        self.alphas = [float(a) for a in alphas]
        snp = p.entry_snp[es].astype(np.int64) if es else np.zeros(0, dtype=np.int64)
        self.f = np.asarray(amb_af, dtype=np.float64)[snp]
        self.gp = np.asarray(p.gp, dtype=np.float64)[snp, j, :] if es else np.zeros((0, 3))
        lens = [int(p.entry_rptr[e + 1] - p.entry_rptr[e]) for e in es]
        self.maxr = max(lens, default=0)
        self.reads = np.full((self.n, self.maxr), READ_OTHER, dtype=np.int64)
        for i, e in enumerate(es):
            self.reads[i, :lens[i]] = p.reads[int(p.entry_rptr[e]):int(p.entry_rptr[e + 1])]
        self._grid = {}
        self._probs = {}

    def _read_probs(self, r, dtype):
        """the rows whose read r is usable (:664) and their pR, pA (:666-667), cached"""
        key = (r, dtype)
        if key not in self._probs:
            b = self.reads[:, r]
            idx = np.flatnonzero(b != READ_OTHER)
            al, bq = b[idx] >> 7, b[idx] & 0x7F
            mat, e3 = ar.MAT[bq].astype(dtype), ar.ERR[bq].astype(dtype) / dtype(3.0)
            self._probs[key] = (idx, np.where(al == 0, mat, e3), np.where(al == 1, mat, e3))
        return self._probs[key]

    def grid_maxima(self, dtype):
        """per entry: the grid's maximum after every read [n][maxr] (1 where the read is skipped) and the final one [n]"""
        if dtype not in self._grid:
            pg = ar.grid_p(self.alphas).astype(dtype)
            g = np.ones((self.n, pg.size), dtype=dtype)
            mxs = np.ones((self.n, self.maxr), dtype=dtype)
            for r in range(self.maxr):
                idx, pR, pA = self._read_probs(r, dtype)
                gn = g[idx] * (pR[:, None] * (dtype(1.0) - pg) + pA[:, None] * pg)   # :685
                mx = gn.max(axis=1)                                                   # :686-687
                g[idx] = gn / mx[:, None]                                             # :696
                mxs[idx, r] = mx
            g = g + dtype(1e-10)                                                      # :710
            self._grid[dtype] = (mxs, g.max(axis=1))                                  # :711-712
        return self._grid[dtype]

    def eval(self, rhos, dtype=np.float64):
        """(LL, LL', LL'', sum |log D|, sum |D'/D|, sum (|D''/D| + (D'/D)^2), sum A'/D, sum (A''/D + (A'/D)^2)), each
        [len(rhos)].  The fourth to sixth are the sums of absolute per-entry terms.  The last two are the same over absolute
        summands, A' = sum_l |gp[l] w'[l]| and A'' likewise: never smaller, and not 0 where the three l cancel exactly and
        the plain terms are (a one-read entry with gp[0] == gp[2] at f == 0.5: w'[0] == -w'[2], w'[1] == 0)"""
        rh = np.asarray(rhos, dtype=dtype).reshape(-1)
        R = rh.size
        if self.n == 0:
            return core.eval_empty(R, dtype)
        mxs, mxf = self.grid_maxima(dtype)
        l = np.arange(3).astype(dtype)
        tfl = dtype(2.0) * self.f.astype(dtype)[:, None] - l[None, :]              # 2 f - l, [n][3]
        p = dtype(0.5) * l[None, None, :] + tfl[:, None, :] * dtype(0.5) * rh[None, :, None]   # [n][R][3]
        a = np.ones((self.n, R, 3), dtype=dtype)
        a1 = np.zeros_like(a)
        a2 = np.zeros_like(a)
        for r in range(self.maxr):
            idx, pR, pA = self._read_probs(r, dtype)
            pi = p[idx]
            t = pR[:, None, None] * (dtype(1.0) - pi) + pA[:, None, None] * pi
            v = ((pA - pR)[:, None] * tfl[idx] * dtype(0.5))[:, None, :]
            m = mxs[idx, r][:, None, None]
            x0, x1, x2 = a[idx], a1[idx], a2[idx]
            a2[idx] = (x2 * t + dtype(2.0) * x1 * v) / m
            a1[idx] = (x1 * t + x0 * v) / m
            a[idx] = (x0 * t) / m
        a = a + dtype(1e-10)
        m = mxf[:, None, None]
        a, a1, a2 = a / m, a1 / m, a2 / m
        g = self.gp.astype(dtype)[:, None, :]
        D = np.zeros((self.n, R), dtype=dtype)
        D1 = np.zeros_like(D)
        D2 = np.zeros_like(D)
        A1 = np.zeros_like(D)
        A2 = np.zeros_like(D)
        for k in range(3):                                                         # :738-742, from 0 in the order l = 0, 1, 2
            D = D + g[:, :, k] * a[:, :, k]
            D1 = D1 + g[:, :, k] * a1[:, :, k]
            D2 = D2 + g[:, :, k] * a2[:, :, k]
            A1 = A1 + np.abs(g[:, :, k] * a1[:, :, k])
            A2 = A2 + np.abs(g[:, :, k] * a2[:, :, k])
        return core.eval_tail(D, D1, D2, A1, A2)


def ll_d1_d2(p, alphas, amb_af, c, j, rho, dtype=np.float64):
    """(LL, LL', LL'') of droplet c as one cell of sample j plus a share rho of ambient RNA, scalars of `dtype`"""
    L, d1, d2 = Cell(p, alphas, amb_af, c, j).eval([rho], dtype)[:3]
    return L[0], d1[0], d2[0]


coarse_points, bracket, maximise = core.coarse_points, core.bracket, core.maximise


def fit(p, alphas, amb_af, c, j, rho_max):
    """dict of the restated outputs of one (droplet, candidate): rho_hat, ll_hat, ll_zero, info, status (0, 1, 2 or 5)"""
    return core.fit(Cell(p, alphas, amb_af, c, j), "rho", rho_max, top=False, can_fail=False)


def shaped_pileup(cell_entries, S, V, seed, soup=0.2, depths=(1, 2, 33, 60), depth_p=(0.55, 0.35, 0.05, 0.05), other=0.03,
                  missing_gp_frac=0.03, min_bq=2, max_bq=93, p_alt_of=None):
    """A pileup whose droplets have exactly the given numbers of entries (0 allowed; each <= S): droplet c holds one cell of
    sample c % V, a read comes with probability `soup` from the pool and else from the cell (as ambient_ref.soup_pileup
    draws them) and is miscalled with the probability of its base quality, uniform in [min_bq, max_bq]; an entry has
    one of `depths` reads; a share `other` of the read bytes is READ_OTHER; a share `missing_gp_frac` of the markers has
    no genotypes (1.0: none has).  p_alt_of(G, s_of, cell_of, drawn): another donor rule -- the ALT probability of every
    read from the genotypes G [S][V], the read's marker and droplet and whether the share `soup` drew it (it takes no draw of
    its own, so the stream of draws is one for every rule).  Returns (pileup, sample of every droplet, the pool's fractions)."""
    rng = np.random.default_rng(seed)
    C = len(cell_entries)
    af = rng.uniform(0.1, 0.9, size=S)
    G = (rng.random((S, V)) < af[:, None]).astype(np.int64) + (rng.random((S, V)) < af[:, None]).astype(np.int64)
    pool = G.mean(axis=1) / 2.0
    who = np.arange(C) % V
    cell_ptr = np.concatenate([[0], np.cumsum(cell_entries)]).astype(np.int64)
    snp = np.concatenate([np.sort(rng.choice(S, size=n, replace=False)) for n in cell_entries] + [np.zeros(0, dtype=np.int64)])
    snp = snp.astype(np.int32)
    nreads = rng.choice(depths, size=snp.size, p=depth_p).astype(np.int64)
    rptr = np.concatenate([[0], np.cumsum(nreads)]).astype(np.int64)
    ent = np.repeat(np.arange(snp.size), nreads)
    cell_of = np.repeat(np.arange(C), cell_entries)[ent]
    s_of = snp[ent]
    from_soup = rng.random(ent.size) < soup
    p_alt = p_alt_of(G, s_of, cell_of, from_soup) if p_alt_of else np.where(from_soup, pool[s_of], G[s_of, who[cell_of]] / 2.0)
    bq = rng.integers(min_bq, max_bq + 1, size=ent.size)
    alt = (rng.random(ent.size) < p_alt) ^ (rng.random(ent.size) < 10.0 ** (-bq / 10.0))
    reads = ((alt.astype(np.uint8) << 7) | bq.astype(np.uint8)).astype(np.uint8)
    reads[rng.random(ent.size) < other] = READ_OTHER
    has_gp = (rng.random(S) >= missing_gp_frac).astype(np.uint8)
    gp = ar.synth.gt_to_gp(G, 0.01)
    gp[has_gp == 0] = (1.0, 0.0, 0.0)
    p = ar.synth.Pileup(C, S, cell_ptr, snp, rptr, reads, af, gp, has_gp)
    return p, who, pool
