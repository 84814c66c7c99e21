// pair_fit.hpp -- what the two mixing-share fits, muxgl_demux_alpha_fit (demux_alpha_fit.hip) and
// muxgl_fmx_alpha_fit (fmx_alpha_fit.hip), say alike: everything that depends only on "a pair of genotype rows
// (j, k) and a share alpha of the second".  The genotype pair (l, m), l from j and m from k, is element l * 3 + m and has
// the ALT-read probability p = 0.5 l + (m - l) 0.5 alpha (cmd_cram_demuxlet.cpp:673, sc_drop_seq.cpp:472-480).  The three
// diagonal elements do not depend on alpha and are the caller's walk's own; a lane carries the six others.
#pragma once
#include "ambient_fit_search.hpp"

namespace pair_fit {

// the six off-diagonal elements i <-> (l, m): (0,1) (0,2) (1,0) (1,2) (2,0) (2,1); p = P0[i] + P1[i] alpha, dp/dalpha = P1[i]
__device__ constexpr double P0[6] = {0.0, 0.0, 0.5, 0.5, 1.0, 1.0};
__device__ constexpr double P1[6] = {0.5, 1.0, -0.5, 0.5, -1.0, -0.5};

// p per (share, element) for the NS shares x[0..NS-1], at c * 6 + i: one fma from the reference's expression, exact at the
// ends (alpha = 0: p = 0.5 l, row j alone; alpha = 1: p = 0.5 m, row k alone) and at 0.5.  The same for every entry, and
// wave-uniform
template <int NS, class Keep>
__device__ __forceinline__ void p_of(const double (&x)[3], double* pv, Keep&& keep) {
#pragma unroll
  for (int c = 0; c < NS; ++c)
#pragma unroll
    for (int i = 0; i < 6; ++i) pv[c * 6 + i] = keep(fma(P1[i], x[c], P0[i]));
}

// gg[l * 3 + m] = row_j[l] * row_k[m]: the product of the two rows first (cmd_cram_demuxlet.cpp:740)
__device__ __forceinline__ void gg_of(const double* __restrict__ gj, const double* __restrict__ gk, double (&gg)[9]) {
  const double k0 = gk[0], k1 = gk[1], k2 = gk[2];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const double jl = gj[l];
    gg[l * 3 + 0] = jl * k0, gg[l * 3 + 1] = jl * k1, gg[l * 3 + 2] = jl * k2;
  }
}

// sum_l sum_m gg[l * 3 + m] * w_lm in the order l, then m: the diagonal's weights are wd, the others' w(a[i])
template <class W>
__device__ __forceinline__ double dot9(const double (&gg)[9], double wd0, double wd1, double wd2, const double* a, W&& w) {
  double D = gg[0] * wd0;
  D = fma(gg[1], w(a[0]), D);
  D = fma(gg[2], w(a[1]), D);
  D = fma(gg[3], w(a[2]), D);
  D = fma(gg[4], wd1, D);
  D = fma(gg[5], w(a[3]), D);
  D = fma(gg[6], w(a[4]), D);
  D = fma(gg[7], w(a[5]), D);
  return fma(gg[8], wd2, D);
}

// sum over the six off-diagonal elements of gg[l * 3 + m] * w_lm' for a derivative of D (the diagonal's is 0), w(a[i]) the others', (l, m) next to
// (m, l): six rounded products, no fused step.  Where the two rows are the same numbers (j == k, or a column that is a copy
// of another) gg is symmetric, and in a one-read entry w_lm' == -w_ml' exactly (v is +-0.5 d or +-d): the pairs then
// cancel to an exact 0, as they do in exact arithmetic, where a fused chain in the order l, m leaves a residue of rounding
// that an entry with a small D divides up.
template <class W>
__device__ __forceinline__ double dot6_paired(const double (&gg)[9], const double* a, W&& w) {
#pragma clang fp contract(off)
  const double p01 = gg[1] * w(a[0]), p10 = gg[3] * w(a[2]);
  const double p02 = gg[2] * w(a[1]), p20 = gg[6] * w(a[4]);
  const double p12 = gg[5] * w(a[3]), p21 = gg[7] * w(a[5]);
  return ((p01 + p10) + (p02 + p20)) + (p12 + p21);
}

}  // namespace pair_fit
