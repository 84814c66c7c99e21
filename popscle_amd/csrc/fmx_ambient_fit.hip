// fmx_ambient_fit.hip -- muxgl_fmx_ambient_fit: the ambient share rho of muxgl_fmx_ambient (fmx_ambient.hip) as a
// per-droplet maximum-likelihood estimate with its observed information, for a few candidate clusters per droplet: the
// freemuxlet counterpart of demux_ambient_fit.hip.  The model is fmx_ambient.hip's, unchanged.  Every read's ambient factor
// mat x + e4, x = ALT read ? p : 1 - p, p = fma(2 f - l, 0.5 rho, 0.5 l), is linear in rho with slope
// v = +-mat (2 f - l) 0.5 (+ for an ALT read), so an entry's product a_l(rho) is a polynomial and its first two derivatives
// follow from the product rule along the reads:
//
//   a'' = a'' fac + 2 a' v;   a' = a' fac + a v;   a = a fac;   all three times the read's 1 / t     (in this order, per usable read)
//   after the reads, where a_l < 1e-6:  a_l = 1e-6, a_l' = a_l'' = 0                     (the floor of sc_drop_seq.cpp:498-501)
//   w_l = a_l (1 / T),   w_l', w_l'' likewise
//   D = fma(q2, w2, fma(q1, w1, q0 w0)),   D', D'' likewise                              q = d_cgp[s_e][j]
//   LL = sum_e log D,   LL' = sum_e D' / D,   LL'' = sum_e (D'' / D - (D' / D)^2)         over ALL entries (no has_gp here)
//
// The nine, their per-read sum t, the reciprocal-multiply, the final floor and T are fmx_nine_walk's (fmx_entry.hpp), the
// text fam_weight_kernel and fmx_entry_kernel walk; the factor is fam_weight_kernel's expression.  The floor makes LL piecewise: on a floored element the derivative is that
// of the constant 1e-6, which is the derivative of the floored function on that piece.  LL is continuous; where an element
// crosses the floor LL' jumps, and always upward, because max(a, 1e-6) is convex in a.  So a maximum of LL cannot sit on
// such a kink, and a bracket with LL'(lo) > 0 > LL'(hi) narrowed by the sign of LL' closes on a smooth zero of LL'
// (DESIGN 4.2k).
// An upward jump can start a second rise inside the coarse bracket, so where an element crosses the floor between the
// bracket's three coarse points the bracket is first scanned on 65 points (ambient_fit::search_piecewise).
//
// fam_fit_kernel, one wave per (cell, candidate), four waves a workgroup, the candidate fastest: lane = entry index modulo
// 64, striding the cell's entries; each lane walks its entry's read bytes through the Phred table in LDS with the nine and
// nine more doubles (three shares' a_l in a coarse pass, (a, a', a'') in a derivative pass) and adds its share of the sums
// in entry order; a fixed xor butterfly adds the 64 shares, so every lane holds the same bits and every decision of the
// search (ambient_fit_search.hpp, three points per pass) is wave-uniform.  The nine are recomputed on every pass:
// nothing proportional to nnz is allocated, so no slab budget applies and MUXGL_FMX_SLAB_MB is not read.  One launch, no
// atomics; every reduction tree is fixed by the cell alone: the outputs are bit-identical from call to call, for any order,
// grouping or repetition of the candidates, on one device, on a group and through the sharded driver.
// A posterior row of exactly 0 at one of the cell's markers makes D = 0 and LL = -inf at every rho: status 6, found at the
// coarse points before any derivative is formed, so no NaN is written.
#include <cmath>
#include <vector>

#include "ambient_fit_search.hpp"
#include "fmx_entry.hpp"

namespace {

// One pass of a wave over the entries [e0, e1) of a cell for candidate cluster j (qj = cgp + j * 3, K3 = K * 3).
//   DERIV = false: out[k] = LL(x[k]) for the three shares x[0..2]
//   DERIV = true:  out = (LL, LL', LL'') at x[0]
// Returns in every lane the same bits.  crosses (coarse pass): whether an element of the cell is below the floor at one of
// the three shares and not at another.
template <bool DERIV>
__device__ __forceinline__ void fam_fit_pass(int64_t e0, int64_t e1, int lane, const int32_t* __restrict__ entry_snp,
                                             const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                                             const double* lut, const double* __restrict__ af, const double* __restrict__ qj,
                                             size_t K3, const double (&x)[3], double (&out)[3], bool* crosses) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  bool cr = false;  // (coarse pass) an element of one of the lane's entries is floored at one share and not at another
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int32_t s = entry_snp[e];
    const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
    const double f = af[s];
    const double tf = f + f;
    const double tf1 = tf - 1.0, tf2 = tf - 2.0;
    // p per (share, l) as fam_weight_kernel forms it; DERIV: the slope's (2 f - l) 0.5 per l in pv[3..5]
    double pv[9];
    if (DERIV) {
      const double hr = 0.5 * x[0];
      pv[0] = tf * hr, pv[1] = fma(tf1, hr, 0.5), pv[2] = fma(tf2, hr, 1.0);
      pv[3] = tf * 0.5, pv[4] = tf1 * 0.5, pv[5] = tf2 * 0.5;
      pv[6] = pv[7] = pv[8] = 0.0;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double hr = 0.5 * x[k];
        pv[k * 3 + 0] = tf * hr, pv[k * 3 + 1] = fma(tf1, hr, 0.5), pv[k * 3 + 2] = fma(tf2, hr, 1.0);
      }
    }
    // am: DERIV ? (a_0, a_1, a_2, a_0', a_1', a_2', a_0'', a_1'', a_2'') : a_l of share k at k * 3 + l
    double gls[9], am[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) am[i] = (DERIV && i >= 3) ? 0.0 : 1.0;
    const double inv = fmx_nine_walk(reads, r0, r1, lut, gls, [&](uint32_t al, double mat, double e4, double inv_t) {
      // (a 1 the compiler cannot see through: 1 - p stays in the read loop instead of nine more doubles held across it;
      // the same operations)
      double one = 1.0;
      asm volatile("" : "+v"(one));
      if (DERIV) {
        const double sm = (al == 0) ? -mat : mat;
        ambient_fit::product_rule<3>(am, [&](int l, double& fac, double& v) {
          const double xl = (al == 0) ? one - pv[l] : pv[l];
          fac = (mat * xl + e4);
          v = sm * pv[3 + l];
        });
      } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          const double xi = (al == 0) ? one - pv[i] : pv[i];
          am[i] *= (mat * xi + e4);
        }
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) am[i] *= inv_t;
    });
    const double* q = qj + (size_t)s * K3;
    const double q0 = q[0], q1 = q[1], q2 = q[2];
    if (DERIV) {
#pragma unroll
      for (int l = 0; l < 3; ++l)
        if (am[l] < kMinNormGL) am[l] = kMinNormGL, am[3 + l] = 0.0, am[6 + l] = 0.0;  // (the floored piece is constant)
      const double D = fma(q2, am[2] * inv, fma(q1, am[1] * inv, q0 * (am[0] * inv)));
      const double D1 = fma(q2, am[5] * inv, fma(q1, am[4] * inv, q0 * (am[3] * inv)));
      const double D2 = fma(q2, am[8] * inv, fma(q1, am[7] * inv, q0 * (am[6] * inv)));
      ambient_fit::add_entry(D, D1, D2, s0, s1, s2);
    } else {
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        const bool f0 = am[l] < kMinNormGL, f1 = am[3 + l] < kMinNormGL, f2 = am[6 + l] < kMinNormGL;
        cr = cr || f0 != f1 || f1 != f2;
      }
#pragma unroll
      for (int i = 0; i < 9; ++i)
        if (am[i] < kMinNormGL) am[i] = kMinNormGL;
      s0 += pos_log(fma(q2, am[2] * inv, fma(q1, am[1] * inv, q0 * (am[0] * inv))), 0.0);
      s1 += pos_log(fma(q2, am[5] * inv, fma(q1, am[4] * inv, q0 * (am[3] * inv))), 0.0);
      s2 += pos_log(fma(q2, am[8] * inv, fma(q1, am[7] * inv, q0 * (am[6] * inv))), 0.0);
    }
  }
  out[0] = ambient_fit::wave_sum(s0);
  out[1] = ambient_fit::wave_sum(s1);
  out[2] = ambient_fit::wave_sum(s2);
  if (crosses) *crosses = __any(cr) != 0;
}

// grid: ceil(C * n_cand / 4) workgroups of four waves; wave unit <-> (cell, candidate), the candidate fastest, so the
// waves of a workgroup walk the same entries.  dout: [4][n_units] rho_hat, ll_hat, ll_zero, info; iout: [2][n_units]
// status, n_steps
__global__ void __launch_bounds__(256)
    fam_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ cand, double rho_max,
                   const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                   const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                   const double* __restrict__ lut_g, const double* __restrict__ af, const double* __restrict__ cgp, int K,
                   double* __restrict__ dout, int32_t* __restrict__ iout) {
  __shared__ double lut[256];
  lut[threadIdx.x] = lut_g[threadIdx.x];
  __syncthreads();
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int lane = threadIdx.x & 63;
  const int64_t c = unit / n_cand;
  const int32_t j = cand[unit];
  ambient_fit::result res;  // (cand == -1: status 4, all outputs 0)
  if (j >= 0) {
    const int64_t e0 = cell_ptr[c], e1 = cell_ptr[c + 1];
    const size_t K3 = (size_t)K * 3;
    const double* qj = cgp + (size_t)j * 3;
    auto coarse = [&](const double (&x)[3], double (&o)[3], bool& crosses) {
      fam_fit_pass<false>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, af, qj, K3, x, o, &crosses);
    };
    auto deriv = [&](double x, double& L, double& d1, double& d2) {
      const double xs[3] = {x, 0.0, 0.0};
      double o[3];
      fam_fit_pass<true>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, af, qj, K3, xs, o, nullptr);
      L = o[0], d1 = o[1], d2 = o[2];
    };
    // (a droplet without entries: every coarse LL is 0, the first derivative pass finds nothing, status 5)
    res = ambient_fit::search_piecewise(rho_max, coarse, deriv, [&] { return e0 == e1; });
  }
  ambient_fit::store(res, lane, unit, n_units, dout, iout);
}

}  // namespace

// the caller's arguments, on the host, before any device work: 0, or 1 with the reason in `why`
int fmx_ambient_fit_bad_args(const double* amb_af, int64_t S, int32_t n_cand, const int32_t* cand, int64_t C, int K,
                             double rho_max, bool any_out, char* why, size_t n) {
  if (ambient_fit::bad_args("muxgl_fmx_ambient_fit", "cluster", amb_af, n_cand, cand, C, K, rho_max, any_out, why, n)) return 1;
  for (int64_t s = 0; s < S; ++s)
    if (!(std::isfinite(amb_af[s]) && amb_af[s] >= 0.0 && amb_af[s] <= 1.0))
      return snprintf(why, n, "muxgl_fmx_ambient_fit: amb_af of marker %lld (%g) is not a finite number in [0, 1]", (long long)s,
                      amb_af[s]),
             1;
  return 0;
}

extern "C" int muxgl_fmx_ambient_fit(muxgl_handle* h, const double* amb_af, int32_t n_cand, const int32_t* cand, double rho_max,
                                     double* rho_hat, double* ll_hat, double* ll_zero, double* info, int32_t* status,
                                     int32_t* n_steps, float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (h->group)
    return group_fmx_ambient_fit(h, amb_af, n_cand, cand, rho_max, rho_hat, ll_hat, ll_zero, info, status, n_steps, kernel_ms);
  HIPCHK(h, hipSetDevice(h->device));
  if (fmx_refuse(h, h, "muxgl_fmx_ambient_fit", "the fit belongs")) return 1;
  const ambient_fit::outputs out = {rho_hat, ll_hat, ll_zero, info, status, n_steps};
  char why[256];
  if (fmx_ambient_fit_bad_args(amb_af, h->S, n_cand, cand, h->C, h->K, rho_max, out.any(), why, sizeof(why)))
    MUXGL_FAIL(h, "%s", why);
  if (h->C == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing, no timing slot: records, timings and every other state of the handle keep their values)
  return ambient_fit::host_run(h, "muxgl_fmx_ambient_fit", amb_af, n_cand, 1, cand, 4, out, kernel_ms,
                               [&](int64_t n_units, const double* d_af, const int32_t* d_cand, double* d_dout, int32_t* d_iout) {
                                 hipLaunchKernelGGL(fam_fit_kernel, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream,
                                                    n_units, (int)n_cand, d_cand, rho_max, h->d_cell_ptr, h->d_entry_snp,
                                                    h->d_entry_rptr, h->d_reads, h->d_lut, d_af, h->d_cgp, h->K, d_dout, d_iout);
                                 HIPCHK(h, hipGetLastError());
                                 return 0;
                               });
}
