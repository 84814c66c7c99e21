// fmx_anchor_row.hpp -- the posterior row of an anchored cluster (muxgl_fmx_set_anchors), for its two writers:
// fmx_anchor_kernel (fmx_anchor.hip: the rows the E-step reads, d_cgp) and rows_kernel (fmx_exact.hip: the rows the
// exact path decides near ties from).
//
//   marker with genotypes     the panel row gp[s][donor] as muxgl_demux_set_gp took it: a copy, the same three doubles in
//                             both writers (the device copy of the panel holds neutral rows (1, 0, 0) where has_gp is 0,
//                             so the branch is on has_gp, never on the values)
//   marker without genotypes  the row a cluster without cells gets, in the arithmetic of the WRITER's own path.  Both are
//                             cmd_cram_freemux2.cpp:388-390,402-415 on the default-constructed pileup (1, ..., 1) in IEEE
//                             operations; they part in the last step only, the mix with geno_error:
//                               IEEE = true   rows_kernel's (the reference's): two products, one sum
//                               IEEE = false  fmx_cgp_kernel's as hipcc compiles it: (1 - e) * g rounded, e * p fused into
//                                             the sum.  (That kernel's products p * gls are fused into its sums too, but
//                                             with gls = 1 a fused and a rounded product are the same number.)
//                             The two differ in the last bit, as they do for every cluster; what holds on EACH path is
//                             that an anchored donor without genotypes is bit for bit a cluster without cells, so the ties
//                             between the two stay exact ties and the scan order decides them, as in the reference.
//                             tests/test_fmx_anchor_gpu.py holds the E-step's side to fmx_cgp_kernel on the device: a
//                             compiler that contracts that kernel differently shows up there.
#pragma once

template <bool IEEE>
__device__ __forceinline__ void fmx_anchor_row(bool has, const double* __restrict__ gprow, double a, double geno_error,
                                               double* __restrict__ o) {
#pragma clang fp contract(off)
  if (has) {
    o[0] = gprow[0], o[1] = gprow[1], o[2] = gprow[2];
    return;
  }
  const double p0 = (1.0 - a) * (1.0 - a), p1 = 2 * a * (1.0 - a), p2 = a * a;
  double g0 = p0, g1 = p1, g2 = p2;  // (x * 1.0 is x)
  const double sum = g0 + g1 + g2;
  g0 /= sum;
  g1 /= sum;
  g2 /= sum;
  if (geno_error > 0) {
    if constexpr (IEEE) {
      g0 = (1 - geno_error) * g0 + geno_error * p0;
      g1 = (1 - geno_error) * g1 + geno_error * p1;
      g2 = (1 - geno_error) * g2 + geno_error * p2;
    } else {
      g0 = fma(geno_error, p0, (1 - geno_error) * g0);
      g1 = fma(geno_error, p1, (1 - geno_error) * g1);
      g2 = fma(geno_error, p2, (1 - geno_error) * g2);
    }
  }
  o[0] = g0, o[1] = g1, o[2] = g2;
}

// The posterior row of a MUXGL_ANCHOR_PRIOR cluster (muxgl_fmx_set_anchors_mode), for its two writers: fmx_prior_kernel
// (fmx_anchor.hip) and rows_kernel.  It is the free cluster's row of cmd_cram_freemux2.cpp:402-415 on the cluster's own
// pileup diagonal d, with ONE change: at a marker with genotypes the Hardy-Weinberg triple p inside the product is the
// panel row w; the mix with geno_error keeps p.
//
//   marker with genotypes     q = w * d / sum(w * d), then (1 - e) q + e p.  A zero in w is a zero in q.  d is positive
//                             (sc_drop_seq.h:72-101: (1, .., 1) or floored at MIN_NORM_GL and renormalised, so >= ~1e-6 / 9),
//                             so the sum vanishes only where all of w does (or is no number): nothing muxgl_demux_set_gp
//                             refuses, so such a row is defined as the HELD row, the panel's as given
//   marker without genotypes  w := p, the free cluster's row, the same bits fmx_cgp_kernel / rows_kernel write
//
// Each side follows its writer's own arithmetic, so that with w == p (bit for bit) a PRIOR cluster IS a free one:
//   IEEE = true   rows_kernel's: rounded products, the left-to-right sum, the mix as two products and a sum
//   IEEE = false  fmx_cgp_kernel's as hipcc contracts it for gfx950 (read off its machine code): the three products that
//                 are divided are rounded; the sum is fma(p2, d2, fma(d0, p0, p1 * d1)); the mix is fma(e, p, (1 - e) * g).
//                 tests/test_fmx_prior_gpu.py holds this to fmx_cgp_kernel on the device, bit for bit.
template <bool IEEE>
__device__ __forceinline__ void fmx_prior_row(bool has, const double* __restrict__ gprow, double d0, double d1, double d2,
                                              double a, double geno_error, double* __restrict__ o) {
#pragma clang fp contract(off)
  const double p0 = (1.0 - a) * (1.0 - a), p1 = 2 * a * (1.0 - a), p2 = a * a;
  double w0 = p0, w1 = p1, w2 = p2;
  if (has) w0 = gprow[0], w1 = gprow[1], w2 = gprow[2];
  double g0 = w0 * d0, g1 = w1 * d1, g2 = w2 * d2;
  double sum;
  if constexpr (IEEE)
    sum = g0 + g1 + g2;
  else
    sum = fma(w2, d2, fma(d0, w0, g1));
  if (has && !(sum > 0.0)) {
    o[0] = w0, o[1] = w1, o[2] = w2;
    return;
  }
  g0 /= sum;
  g1 /= sum;
  g2 /= sum;
  if (geno_error > 0) {
    if constexpr (IEEE) {
      g0 = (1 - geno_error) * g0 + geno_error * p0;
      g1 = (1 - geno_error) * g1 + geno_error * p1;
      g2 = (1 - geno_error) * g2 + geno_error * p2;
    } else {
      g0 = fma(geno_error, p0, (1 - geno_error) * g0);
      g1 = fma(geno_error, p1, (1 - geno_error) * g1);
      g2 = fma(geno_error, p2, (1 - geno_error) * g2);
    }
  }
  o[0] = g0, o[1] = g1, o[2] = g2;
}
