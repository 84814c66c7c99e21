// fmx_ambient_fit.hip -- muxgl_fmx_ambient_fit: the ambient share rho of muxgl_fmx_ambient (fmx_ambient.hip) as a
// per-droplet maximum-likelihood estimate with its observed information, for a few candidate clusters per droplet: the
// freemuxlet counterpart of demux_ambient_fit.hip.  The model is fmx_ambient.hip's, unchanged.  Every read's ambient factor
// mat x + e4, x = ALT read ? p : 1 - p, p = fma(2 f - l, 0.5 rho, 0.5 l), is linear in rho with slope
// v = +-mat (2 f - l) 0.5 (+ for an ALT read), so an entry's product a_l(rho) is a polynomial and its first two derivatives
// follow from the product rule along the reads (fmx_fit.hpp, where the pass, the floor and the kernel stand):
//
//   w_l = a_l (1 / T),   w_l', w_l'' likewise
//   D = fma(q2, w2, fma(q1, w1, q0 w0)),   D', D'' likewise                              q = d_cgp[s_e][j]
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
#include <cmath>
#include <vector>

#include "fmx_fit.hpp"

namespace {

// the model of fmx_fit.hpp: three elements a_l, one candidate cluster j (qj = cgp + j * 3, K3 = K * 3) per slot
struct fam_model {
  static constexpr int NE = 3, WIDTH = 1, ROWS = 4;
  const double* __restrict__ af;
  const double* __restrict__ qj;
  size_t K3;
  __device__ __forceinline__ fam_model(const double* af, const double* cgp, int K, int32_t j, int32_t)
      : af(af), qj(cgp + (size_t)j * 3), K3((size_t)K * 3) {}

  // p per (share, l) as fam_weight_kernel forms it, per entry from af[s]; DERIV: the slope's (2 f - l) 0.5 per l in v
  template <bool DERIV>
  struct shares {
    double p[DERIV ? 3 : 9], v[3];
    __device__ __forceinline__ void pass(const double (&)[3]) {}
    __device__ __forceinline__ void entry(const fam_model& m, int32_t s, const double (&x)[3]) {
      const double f = m.af[s];
      const double tf = f + f;
      const double tf1 = tf - 1.0, tf2 = tf - 2.0;
#pragma unroll
      for (int k = 0; k < (DERIV ? 1 : 3); ++k) {
        const double hr = 0.5 * x[k];
        p[k * 3 + 0] = tf * hr, p[k * 3 + 1] = fma(tf1, hr, 0.5), p[k * 3 + 2] = fma(tf2, hr, 1.0);
      }
      if (DERIV) v[0] = tf * 0.5, v[1] = tf1 * 0.5, v[2] = tf2 * 0.5;
    }
    __device__ __forceinline__ double slope(int l) const { return v[l]; }
  };

  // D, D' and D'' alike: the posterior row of cluster j at marker s over the three elements
  struct weights {
    double q0, q1, q2;
    __device__ __forceinline__ weights(const fam_model& m, int32_t s, const double (&)[9], double) {
      const double* q = m.qj + (size_t)s * m.K3;
      q0 = q[0], q1 = q[1], q2 = q[2];
    }
    __device__ __forceinline__ double D(const double* a, double inv) const {
      return fma(q2, a[2] * inv, fma(q1, a[1] * inv, q0 * (a[0] * inv)));
    }
    __device__ __forceinline__ double dD(const double* a, double inv) const { return D(a, inv); }
  };
};

__global__ void __launch_bounds__(256)
    fam_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ cand, double rho_max,
                   const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                   const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                   const double* __restrict__ lut_g, const double* __restrict__ af, const double* __restrict__ cgp, int K,
                   double* __restrict__ dout, int32_t* __restrict__ iout) {
  fmx_fit_frame<fam_model>(n_units, n_cand, cand, rho_max, cell_ptr, entry_snp, entry_rptr, reads, lut_g, af, cgp, K, dout,
                           iout);
}

}  // namespace

extern "C" int muxgl_fmx_ambient_fit(muxgl_handle* h, const double* amb_af, int32_t n_cand, const int32_t* cand, double rho_max,
                                     double* rho_hat, double* ll_hat, double* ll_zero, double* info, int32_t* status,
                                     int32_t* n_steps, float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (h->group)
    return group_fmx_ambient_fit(h, amb_af, n_cand, cand, rho_max, rho_hat, ll_hat, ll_zero, info, status, n_steps, kernel_ms);
  const ambient_fit::outputs out = {rho_hat, ll_hat, ll_zero, info, status, n_steps};
  return fmx_fit_call<fam_model>(h, "muxgl_fmx_ambient_fit", amb_af, n_cand, cand, rho_max, out, kernel_ms, fam_fit_kernel,
                                 [&](char* why, size_t n) {
                                   return fmx_ambient_fit_bad_args(amb_af, h->S, n_cand, cand, h->C, h->K, rho_max, out.any(), why, n);
                                 });
}
