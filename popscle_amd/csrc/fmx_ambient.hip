// fmx_ambient.hip -- muxgl_fmx_ambient: every droplet scored as ONE cell of cluster j plus a share rho of ambient RNA, the
// freemuxlet counterpart of demux_ambient.hip.  The ambient RNA is no donor: where the second cluster's genotype stands in
// calculate_snp_droplet_pileup (sc_drop_seq.cpp:452-509, alpha = 0.5), its "genotype" at marker s is twice the pool's ALT
// fraction f[s], any number in [0, 2], and its share is rho instead of one half.  Per entry e, with the nine products of
// the reference carried along unchanged:
//
//   p(l, f, rho)    = 0.5 l + (2 f - l) 0.5 rho                 formed as fma(2 f - l, 0.5 rho, 0.5 l)
//   per usable read, in read order:
//       nine[i] *= mat frac_i + e4                              :483-491, as fmx_entry_kernel forms them
//       a[r][l] *= mat (ALT read ? p : 1 - p) + e4
//       t = nine[0] + ... + nine[8];  nine and a are all multiplied by 1 / t            :493-494
//   after the reads every element of nine and of a below 1e-6 becomes 1e-6 (:498-501, sc_drop_seq.h:14)
//       T = sum of the floored nine;  w_e[r][l] = a[r][l] (1 / T)                        :502-504
//   ll_amb[c][j][r] = sum over the entries e of droplet c of
//                     log( (q[s_e][j][0] w_e[r][0] + q[s_e][j][1] w_e[r][1]) + q[s_e][j][2] w_e[r][2] )
//
// q is d_cgp, the posteriors the last E-step read (muxgl_fmx_singlets' rule).  The ambient products take part in none of
// the sums t and T: those are the numbers behind d_egls, so the table is on the scale of the records' log-likelihoods.
// With f in {0, 1/2, 1} and rho = 0.5, p is (l + 2 f) / 4 exactly and w_e[l] is the entry's gls[3 l + 2 f]; with rho = 0
// w_e[l] is gls[4 l] (the singlet table); with rho = 1 p is f for every l.
//   * fam_weight_kernel, lane = entry: the nine through fmx_nine_walk (fmx_entry.hpp: the text fmx_entry_kernel walks, so
//     t and T are its numbers) and beside them 3 x RC ambient products through the same reads.  The rhos are swept in
//     passes of RC (4, 8 or 16); every pass repeats the nine identically and every ambient product belongs to one rho,
//     so the passes change no bit: 24 bytes per entry and rho.
//   * the sweep (lane = cluster of a 64-cluster block, one dot q_j . w_e[r] per (entry, cluster, rho)), the emit kernel,
//     and the host run (on table_call.hpp's batch loop) are ambient_table.hpp's, shared with demux_ambient.hip; what
//     they guarantee -- no bit depends on the chunking, the budget, the split of the rhos or the devices -- is written
//     there.  This unit cuts a long cell into the equal parts of the wave plan, as muxgl_fmx_singlets cuts a cell, and
//     sweeps inside the streamed E-step's budget (4 GiB or a third of the device, MUXGL_FMX_SLAB_MB).
#include <algorithm>
#include <cmath>
#include <vector>

#include "ambient_table.hpp"
#include "fmx_entry.hpp"

namespace {

// wt[(e - eb0)][r][0..2] = w_e[r][l], for the entries [eb0, eb1) of a batch
template <int RC>
__global__ void __launch_bounds__(256)
    fam_weight_kernel(int64_t eb0, int64_t eb1, int NR, const int32_t* __restrict__ entry_snp,
                      const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                      const double* __restrict__ lut_g, ambient_rhos rh, const double* __restrict__ af, double* __restrict__ wt) {
  __shared__ double lut[256];
  lut[threadIdx.x] = lut_g[threadIdx.x];
  __syncthreads();
  const int64_t e = eb0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= eb1) return;
  double* o = wt + (size_t)(e - eb0) * NR * 3;
  const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
  // p = fma(2 f - l, 0.5 rho, 0.5 l): exactly 0 at (l = 0, f = 0) and exactly 1 at (l = 2, f = 1), so those corners
  // carry e4 and mat + e4 themselves, as gls[0] and gls[8] do
  const double f = af[entry_snp[e]];
  const double tf = f + f;
  const double tf1 = tf - 1.0, tf2 = tf - 2.0;
  for (int rb = 0; rb < NR; rb += RC) {
    double gls[9], am[RC * 3];
#pragma unroll
    for (int i = 0; i < RC * 3; ++i) am[i] = 1.0;
    const double inv = fmx_nine_walk(reads, r0, r1, lut, gls, [&](uint32_t al, double mat, double e4, double inv_t) {
#pragma unroll
      for (int k = 0; k < RC; ++k) {
        const double hr = 0.5 * rh.a[rb + k];  // (rb + k < 16: a slot past the end holds the last rho again)
        const double p0 = tf * hr, p1 = fma(tf1, hr, 0.5), p2 = fma(tf2, hr, 1.0);
        const double x0 = (al == 0) ? 1.0 - p0 : p0;
        const double x1 = (al == 0) ? 1.0 - p1 : p1;
        const double x2 = (al == 0) ? 1.0 - p2 : p2;
        am[k * 3 + 0] *= (mat * x0 + e4);
        am[k * 3 + 1] *= (mat * x1 + e4);
        am[k * 3 + 2] *= (mat * x2 + e4);
      }
#pragma unroll
      for (int i = 0; i < RC * 3; ++i) am[i] *= inv_t;
    });
#pragma unroll
    for (int k = 0; k < RC; ++k)
      if (rb + k < NR) {
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          double a = am[k * 3 + l];
          if (a < kMinNormGL) a = kMinNormGL;
          o[(rb + k) * 3 + l] = a * inv;
        }
      }
  }
}

// Entries per lane between two renormalisations, all of their loads in flight.  The smallest factor this path can see:
// every weight w_e[r][l] is floored at MIN_NORM_GL = 1e-6 and divided by T, the sum of the nine floored likelihoods, which
// is <= 1 + 9e-6 (sc_drop_seq.cpp:498-504): w >= 9.9999e-7 > 2^-20.  A factor is a combination sum_l q_l w_l of the
// weights with a posterior triple that sums to 1 (within a few ulp, with or without the geno_error mixing of :402-415: a
// single q_l may be tiny or exactly 0 at geno_error = 0, their sum may not), so f >= min_l w_l > 2^-20.  A mantissa in
// [0.5, 1) times N such factors is >= 2^(-1 - 20 N): normal up to N = 51; eight leave 2^-161.  Upwards an
// ambient product can exceed the nine's maximum only by the modest factor by which the best p of the entry is off the
// reference's grid, per read, and an entry has at most a few hundred reads: no overflow of a double in eight factors.
// A factor of exactly 0 (posterior rows that were never filled) makes the product 0 and the log -inf; frexp(0) = 0, so
// no NaN on the way.
//
// As many entries as 128 VGPRs hold in flight: below 64 clusters the weights come through vector loads, and four rhos of
// four entries would take 134.
struct fam_sweep {
  static constexpr int unr(int KH, int CH) { return CH == 1 ? 8 : (CH == 4 && KH < 64) ? 3 : 4; }
};

template <int RC>
void launch_weights(muxgl_handle* h, int NR, const ambient_rhos& rh, const ambient_batch& b) {
  hipLaunchKernelGGL((fam_weight_kernel<RC>), dim3((unsigned)((b.eb1 - b.eb0 + 255) / 256)), dim3(256), 0, h->stream, b.eb0,
                     b.eb1, NR, h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, rh, b.d_af, b.d_wt);
}

// rhos per pass of the weight kernel: as many as the call has, rounded up to 4, 8 or 16
int weights_dispatch(muxgl_handle* h, int NR, const ambient_rhos& rh, const ambient_batch& b) {
  if (NR > 8)
    launch_weights<16>(h, NR, rh, b);
  else if (NR > 4)
    launch_weights<8>(h, NR, rh, b);
  else
    launch_weights<4>(h, NR, rh, b);
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // namespace

// the caller's arguments, on the host, before any device work: 0, or 1 with the reason in `why` (the handle's message is
// the caller's to set, so that a group's handle carries it)
int fmx_ambient_bad_args(const double* amb_af, int64_t S, int32_t n_rho, const double* rho, double* ll_amb, char* why,
                         size_t why_len) {
  if (!ll_amb) return snprintf(why, why_len, "muxgl_fmx_ambient: NULL output"), 1;
  if (n_rho < 1 || n_rho > AMBIENT_MAX_RHO)
    return snprintf(why, why_len, "muxgl_fmx_ambient: n_rho=%d outside [1,%d]", n_rho, AMBIENT_MAX_RHO), 1;
  if (!rho || !amb_af) return snprintf(why, why_len, "muxgl_fmx_ambient: %s is NULL", rho ? "amb_af" : "rho"), 1;
  for (int r = 0; r < n_rho; ++r)
    if (!(std::isfinite(rho[r]) && rho[r] >= 0.0 && rho[r] <= 1.0))
      return snprintf(why, why_len, "muxgl_fmx_ambient: rho[%d] (%g) is not a finite number in [0, 1]", r, rho[r]), 1;
  for (int64_t s = 0; s < S; ++s)
    if (!(std::isfinite(amb_af[s]) && amb_af[s] >= 0.0 && amb_af[s] <= 1.0))
      return snprintf(why, why_len, "muxgl_fmx_ambient: amb_af of marker %lld (%g) is not a finite number in [0, 1]",
                      (long long)s, amb_af[s]),
             1;
  return 0;
}

extern "C" int muxgl_fmx_ambient(muxgl_handle* h, const double* amb_af, int32_t n_rho, const double* rho, double* ll_amb,
                                 float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (h->group) return group_fmx_ambient(h, amb_af, n_rho, rho, ll_amb, kernel_ms);
  HIPCHK(h, hipSetDevice(h->device));
  if (fmx_refuse(h, h, "muxgl_fmx_ambient", "the table belongs")) return 1;
  char why[256];
  if (fmx_ambient_bad_args(amb_af, h->S, n_rho, rho, ll_amb, why, sizeof(why))) MUXGL_FAIL(h, "%s", why);
  if (h->C == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing, no timing slot: records, timings and every other state of the handle keep their values)
  const ambient_call call = {"muxgl_fmx_ambient", h->K, "clusters", h->d_cgp, "MUXGL_FMX_SLAB_MB", table_plan::equal_begin};
  return ambient_table_run<fam_sweep>(h, call, amb_af, n_rho, rho, ll_amb, kernel_ms,
                                      [&](const ambient_rhos& rh, const ambient_batch& b) {
                                        return weights_dispatch(h, n_rho, rh, b);
                                      });
}
