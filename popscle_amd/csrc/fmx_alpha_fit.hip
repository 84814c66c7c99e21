// fmx_alpha_fit.hip -- muxgl_fmx_alpha_fit: the mixing share alpha of a freemuxlet doublet as a per-droplet
// maximum-likelihood estimate with its observed information, for a few pairs of clusters (j, k) per droplet: the
// freemuxlet counterpart of demux_alpha_fit.hip.  The reference fixes the share at one half
// (calculate_snp_droplet_pileup(..., 0.5), sc_drop_seq.cpp:452-509; the pair loop is cmd_cram_freemux2.cpp:394-455).  Here
// alpha is the share of k: the genotype pair (l, m), l from j and m from k, element l * 3 + m (sc_drop_seq.cpp:472-480), has
// the ALT-read probability p = 0.5 l + (m - l) 0.5 alpha, one fma, exact at alpha = 0, 0.5 and 1.  Every read's factor
// mat x + e4, x = ALT read ? p : 1 - p, is linear in alpha with slope v = +-mat (m - l) 0.5 (+ for an ALT read), so an
// entry's product a_lm(alpha) is a polynomial and its first two derivatives follow from the product rule along the reads
// (fmx_fit.hpp, where the pass, the floor and the kernel stand; the pair's p, its sums and ll_top are pair_fit.hpp's and
// ambient_fit_search.hpp's, shared with demux_alpha_fit.hip):
//
//   w_lm = a_lm (1 / T),   w_lm', w_lm'' likewise
//   D = sum_l sum_m (q[s_e][j][l] q[s_e][k][m]) w_lm      (the product of the two posteriors first; l, then m)   q = d_cgp
//   D', D'' the same sums over w', w'' (the diagonal's are 0), with (l, m) added next to (m, l): pair_fit::dot6_paired
//
// t and T are the sums of the REFERENCE nine, alpha = 0.5: the nine, their per-read sum t, the reciprocal-multiply, the
// final floor and T are fmx_nine_walk's (fmx_entry.hpp).  The reference renormalises its nine after every read by a sum
// that depends on alpha, so its function called with another alpha is on another scale per alpha and is no likelihood in
// alpha; the six off-diagonal elements therefore move in the walk's per_read hook alone, take the read's 1 / t and the final
// 1 / T and take part in neither sum, as the ambient elements of fmx_ambient.hip and fmx_ambient_fit.hip do.  The three
// diagonal elements do not depend on alpha: they are the walk's own gls[0], gls[4], gls[8].  At alpha = 0.5 LL is the
// reference's llks[j (j + 1) / 2 + k] of the last E-step; at alpha = 0 every element (l, m) is the diagonal element (l, l)
// and LL is cluster j's singlet log-likelihood (sum_m q_k[m] = 1 to rounding), at alpha = 1 cluster k's.
//
// The floor makes LL piecewise, as in fmx_ambient_fit.hip: each element is a product of positive linear factors in alpha,
// log-concave and above the floor on an interval; the coefficients q q are >= 0, so LL' jumps only upward at a crossing
// and a maximum never sits on a kink.  A bracket in which an element changes sides is first scanned on
// 65 points (ambient_fit::search_piecewise).
//
#include <cmath>
#include <vector>

#include "fmx_fit.hpp"
#include "pair_fit.hpp"

namespace {

// the model of fmx_fit.hpp: the six off-diagonal elements a_lm, one pair of clusters (j, k) (qj = cgp + j * 3, qk
// likewise, K3 = K * 3) per slot, ll_top as the fifth double row
struct fma_model {
  static constexpr int NE = 6, WIDTH = 2, ROWS = 5;
  const double* __restrict__ qj;
  const double* __restrict__ qk;
  size_t K3;
  __device__ __forceinline__ fma_model(const double*, const double* cgp, int K, int32_t j, int32_t k)
      : qj(cgp + (size_t)j * 3), qk(cgp + (size_t)k * 3), K3((size_t)K * 3) {}

  // p per (share, element): the same for every entry, formed once per pass and kept wave-uniform (in scalar registers:
  // what lets the eighteen products and the nine of a lane stay in vector registers)
  template <bool DERIV>
  struct shares {
    double p[DERIV ? 6 : 18];
    __device__ __forceinline__ void pass(const double (&x)[3]) {
      pair_fit::p_of<(DERIV ? 1 : 3)>(x, p, [](double v) { return ambient_fit::uniform(v); });
    }
    __device__ __forceinline__ void entry(const fma_model&, int32_t, const double (&)[3]) {}
    __device__ __forceinline__ double slope(int i) const { return pair_fit::P1[i]; }
  };

  // the diagonal: the walk's own elements (l, l), floored by the walk; gg: the products of the two posterior rows at s
  struct weights {
    double wd0, wd1, wd2, gg[9];
    __device__ __forceinline__ weights(const fma_model& m, int32_t s, const double (&gls)[9], double inv)
        : wd0(gls[0] * inv), wd1(gls[4] * inv), wd2(gls[8] * inv) {
      pair_fit::gg_of(m.qj + (size_t)s * m.K3, m.qk + (size_t)s * m.K3, gg);
    }
    __device__ __forceinline__ double D(const double* a, double inv) const {
      return pair_fit::dot9(gg, wd0, wd1, wd2, a, [&](double v) { return v * inv; });
    }
    __device__ __forceinline__ double dD(const double* a, double inv) const {
      return pair_fit::dot6_paired(gg, a, [&](double v) { return v * inv; });
    }
  };
};

// (af: none; the argument keeps the two fits' kernels one signature)
__global__ void __launch_bounds__(256)
    fma_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ pair, double alpha_max,
                   const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                   const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                   const double* __restrict__ lut_g, const double* __restrict__ af, const double* __restrict__ cgp, int K,
                   double* __restrict__ dout, int32_t* __restrict__ iout) {
  fmx_fit_frame<fma_model>(n_units, n_cand, pair, alpha_max, cell_ptr, entry_snp, entry_rptr, reads, lut_g, af, cgp, K, dout,
                           iout);
}

}  // namespace

extern "C" int muxgl_fmx_alpha_fit(muxgl_handle* h, int32_t n_cand, const int32_t* pair, double alpha_max, double* alpha_hat,
                                   double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status,
                                   int32_t* n_steps, float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (h->group)
    return group_fmx_alpha_fit(h, n_cand, pair, alpha_max, alpha_hat, ll_hat, ll_zero, ll_top, info, status, n_steps, kernel_ms);
  const ambient_fit::outputs out = {alpha_hat, ll_hat, ll_zero, info, status, n_steps, ll_top};
  return fmx_fit_call<fma_model>(h, "muxgl_fmx_alpha_fit", nullptr, n_cand, pair, alpha_max, out, kernel_ms, fma_fit_kernel,
                                 [&](char* why, size_t n) {
                                   return fmx_alpha_fit_bad_args(n_cand, pair, h->C, h->K, alpha_max, out.any(), why, n);
                                 });
}
