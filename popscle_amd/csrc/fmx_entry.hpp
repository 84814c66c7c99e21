// fmx_entry.hpp -- the per-entry genotype-pair likelihoods of freemuxlet (calculate_snp_droplet_pileup,
// sc_drop_seq.cpp:452-509, alpha = 0.5): the walk of the nine that fmx_entry_kernel (fmx_kernels.hip), fam_weight_kernel
// (fmx_ambient.hip) and fmx_fit_pass (fmx_fit.hpp: fmx_ambient_fit.hip, fmx_alpha_fit.hip) share, the counterpart of
// demux_entry.hpp's grid_walk.
#pragma once
#include "common.hpp"

// The nine start at 1.  Per usable read (a byte other than MUXGL_READ_OTHER, :468), in read order:
//   al = the byte's bit 7 (ALT read), mat = lut[128 + bq], e4 = lut[bq] / 4          lut: [0,128) phred2Err, [128,256) phred2Mat
//   gls[i] *= (mat * fr + e4), fr = fraction of REF reads of pair i, 1 - (g1 + g2) / 4, mirrored for an ALT read    :472-491
//   t = gls[0] + ... + gls[8], added in this order;  gls[i] *= 1 / t                                                :493-494
//   per_read(al, mat, e4, 1 / t)
// After the reads every element below MIN_NORM_GL becomes MIN_NORM_GL (:498-501) and T is their sum, added in the same
// order; the walk returns 1 / T and leaves the floored, not yet divided nine in gls (:502-504 is gls[i] * (1 / T)).
//
// A caller's companion products (the ambient tables' a[r][l], the mixing-share fit's a[l][m]) move in per_read alone: they
// see the read's al, mat, e4 and 1 / t and take part in neither t nor T.  Why the users form the same numbers: this is one
// text, inlined once per user, and every operation on the nine has its operands inside the walk -- a multiply-add the compiler fuses (or
// does not) in mat * fr + e4 is fused by a rule that sees this expression only, never a caller's.  So t, T and the nine
// of an entry are the numbers behind d_egls whichever kernel walks it, which is what puts the ambient table and the
// two fits on the scale of the records' log-likelihoods.
template <class PerRead>
__device__ __forceinline__ double fmx_nine_walk(const uint8_t* __restrict__ reads, int64_t r0, int64_t r1, const double* lut,
                                                double (&gls)[9], PerRead&& per_read) {
#pragma unroll
  for (int i = 0; i < 9; ++i) gls[i] = 1.0;
  for (int64_t r = r0; r < r1; ++r) {
    const uint32_t b = reads[r];
    if (b == MUXGL_READ_OTHER) continue;  // :468
    const uint32_t al = b >> 7, bq = b & 0x7f;
    const double mat = lut[128 + bq], e4 = lut[bq] / 4.;
    const double fr[9] = {1.0, .75, .5, .75, .5, .25, .5, .25, 0.0};
    double tmp = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double f = (al == 0) ? fr[i] : fr[8 - i];
      gls[i] *= (mat * f + e4);
      tmp += gls[i];
    }
    const double inv = 1.0 / tmp;
#pragma unroll
    for (int i = 0; i < 9; ++i) gls[i] *= inv;
    per_read(al, mat, e4, inv);
  }
  double tmp = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    if (gls[i] < kMinNormGL) gls[i] = kMinNormGL;  // :498-501
    tmp += gls[i];
  }
  return 1.0 / tmp;
}
