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
