// fmx_alpha_fit.hip -- muxgl_fmx_alpha_fit: the mixing share alpha of a freemuxlet doublet as a per-droplet
// maximum-likelihood estimate with its observed information, for a few pairs of clusters (j, k) per droplet: the
// freemuxlet counterpart of demux_alpha_fit.hip.  The reference fixes the share at one half
// (calculate_snp_droplet_pileup(..., 0.5), sc_drop_seq.cpp:452-509; the pair loop is cmd_cram_freemux2.cpp:394-455).  Here
// alpha is the share of k: the genotype pair (l, m), l from j and m from k, element l * 3 + m (sc_drop_seq.cpp:472-480), has
// the ALT-read probability p = 0.5 l + (m - l) 0.5 alpha, one fma, exact at alpha = 0, 0.5 and 1.  Every read's factor
// mat x + e4, x = ALT read ? p : 1 - p, is linear in alpha with slope v = +-mat (m - l) 0.5 (+ for an ALT read), so an
// entry's product a_lm(alpha) is a polynomial and its first two derivatives follow from the product rule along the reads:
//
//   a'' = a'' fac + 2 a' v;   a' = a' fac + a v;   a = a fac;   all three times the read's 1 / t     (in this order, per usable read)
//   after the reads, where a_lm < 1e-6:  a_lm = 1e-6, a_lm' = a_lm'' = 0                 (the floor of sc_drop_seq.cpp:498-501)
//   w_lm = a_lm (1 / T),   w_lm', w_lm'' likewise
//   D = sum_l sum_m (q[s_e][j][l] q[s_e][k][m]) w_lm      (the product of the two posteriors first; l, then m)   q = d_cgp
//   D', D'' the same sums over w', w'' (the diagonal's are 0), with (l, m) added next to (m, l): dot6_paired below
//   LL = sum_e log D,   LL' = sum_e D' / D,   LL'' = sum_e (D'' / D - (D' / D)^2)         over ALL entries (no has_gp here)
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
// fma_fit_kernel, one wave per (cell, slot), four waves a workgroup, the slot fastest: lane = entry index modulo 64,
// striding the cell's entries; each lane walks its entry's read bytes through the Phred table in LDS with the nine and
// eighteen more doubles (three shares' six elements in a coarse pass, (a, a', a'') of the six in a derivative pass) and
// adds its share of the sums in entry order; a fixed xor butterfly adds the 64 shares, so every lane holds the same bits
// and every decision of the search is wave-uniform.  The nine are recomputed on every pass: nothing proportional to nnz is
// allocated, so no slab budget applies and MUXGL_FMX_SLAB_MB is not read.  One launch, no atomics; every reduction tree is
// fixed by the cell alone: the outputs are bit-identical from call to call, for any order, grouping or repetition of the
// slots, on one device, on a group and through the sharded driver.  The coarse callable keeps LL of coarse point 8,
// alpha_max: ll_top.  A coarse pass and a derivative pass form a and D by the same operations, so ll_hat on a bound is
// ll_zero resp. ll_top bit for bit.
// A posterior row of exactly 0 at one of the cell's markers makes D = 0 and LL = -inf at every alpha: status 6, found at
// the coarse points before any derivative is formed, so no NaN is written.
#include <cmath>
#include <vector>

#include "ambient_fit_search.hpp"
#include "fmx_entry.hpp"

namespace {

// the six off-diagonal elements i <-> (l, m): (0,1) (0,2) (1,0) (1,2) (2,0) (2,1); p = P0[i] + P1[i] alpha
__device__ constexpr double P0[6] = {0.0, 0.0, 0.5, 0.5, 1.0, 1.0};
__device__ constexpr double P1[6] = {0.5, 1.0, -0.5, 0.5, -1.0, -0.5};

// sum_l sum_m gg[l * 3 + m] * w_lm in the order l, then m: the diagonal from wd, the others from wo
__device__ __forceinline__ double dot9(const double (&gg)[9], double wd0, double wd1, double wd2, double wo0, double wo1,
                                       double wo2, double wo3, double wo4, double wo5) {
  double D = gg[0] * wd0;
  D = fma(gg[1], wo0, D);
  D = fma(gg[2], wo1, D);
  D = fma(gg[3], wo2, D);
  D = fma(gg[4], wd1, D);
  D = fma(gg[5], wo3, D);
  D = fma(gg[6], wo4, D);
  D = fma(gg[7], wo5, D);
  return fma(gg[8], wd2, D);
}

// sum over the six off-diagonal elements of gg[l * 3 + m] * w_lm' for a derivative of D (the diagonal's is 0), (l, m) next
// to (m, l): six rounded products, no fused step (demux_alpha_fit.hip's).  Where the two posterior rows hold
// the same numbers gg is symmetric and the pairs cancel to an exact 0.
__device__ __forceinline__ double dot6_paired(const double (&gg)[9], double wo0, double wo1, double wo2, double wo3, double wo4,
                                              double wo5) {
#pragma clang fp contract(off)
  const double p01 = gg[1] * wo0, p10 = gg[3] * wo2;
  const double p02 = gg[2] * wo1, p20 = gg[6] * wo4;
  const double p12 = gg[5] * wo3, p21 = gg[7] * wo5;
  return ((p01 + p10) + (p02 + p20)) + (p12 + p21);
}

// One pass of a wave over the entries [e0, e1) of a cell for the pair of clusters (j, k) (qj = cgp + j * 3, qk likewise,
// K3 = K * 3).
//   DERIV = false: out[c] = LL(x[c]) for the three shares x[0..2]
//   DERIV = true:  out = (LL, LL', LL'') at x[0]
// Returns in every lane the same bits.  crosses (coarse pass): whether an element of the cell is below the floor at one of
// the three shares and not at another.
template <bool DERIV>
__device__ __forceinline__ void fma_fit_pass(int64_t e0, int64_t e1, int lane, const int32_t* __restrict__ entry_snp,
                                             const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                                             const double* lut, const double* __restrict__ qj, const double* __restrict__ qk,
                                             size_t K3, const double (&x)[3], double (&out)[3], bool* crosses) {
  // p per (share, element); the same for every entry, and wave-uniform
  constexpr int NM = DERIV ? 6 : 18;
  double pv[NM];
#pragma unroll
  for (int c = 0; c < (DERIV ? 1 : 3); ++c)
#pragma unroll
    for (int i = 0; i < 6; ++i) pv[c * 6 + i] = ambient_fit::uniform(fma(P1[i], x[c], P0[i]));
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  bool cr = false;  // (coarse pass) an element of one of the lane's entries is floored at one share and not at another
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int32_t s = entry_snp[e];
    const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
    // am: DERIV ? (a_i, a_i', a_i'') at i, 6 + i, 12 + i : a_i of share c at c * 6 + i
    double gls[9], am[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) am[i] = (DERIV && i >= 6) ? 0.0 : 1.0;
    const double inv = fmx_nine_walk(reads, r0, r1, lut, gls, [&](uint32_t al, double mat, double e4, double inv_t) {
      // (a 1 the compiler cannot see through: 1 - p stays in the read loop instead of eighteen more doubles held across
      // it; the same operations)
      double one = 1.0;
      asm volatile("" : "+v"(one));
      if (DERIV) {
        const double sm = (al == 0) ? -mat : mat;
        ambient_fit::product_rule<6>(am, [&](int i, double& fac, double& v) {
          const double xi = (al == 0) ? one - pv[i] : pv[i];
          fac = (mat * xi + e4);
          v = sm * P1[i];
        });
      } else {
#pragma unroll
        for (int i = 0; i < 18; ++i) {
          const double xi = (al == 0) ? one - pv[i] : pv[i];
          am[i] *= (mat * xi + e4);
        }
      }
#pragma unroll
      for (int i = 0; i < 18; ++i) am[i] *= inv_t;
    });
    // the diagonal: the walk's own elements (l, l), floored by the walk
    const double wd0 = gls[0] * inv, wd1 = gls[4] * inv, wd2 = gls[8] * inv;
    const double* gj = qj + (size_t)s * K3;
    const double* gk = qk + (size_t)s * K3;
    const double k0 = gk[0], k1 = gk[1], k2 = gk[2];
    double gg[9];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const double jl = gj[l];
      gg[l * 3 + 0] = jl * k0, gg[l * 3 + 1] = jl * k1, gg[l * 3 + 2] = jl * k2;
    }
    auto D_of = [&](const double* a) {
      return dot9(gg, wd0, wd1, wd2, a[0] * inv, a[1] * inv, a[2] * inv, a[3] * inv, a[4] * inv, a[5] * inv);
    };
    if (DERIV) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (am[i] < kMinNormGL) am[i] = kMinNormGL, am[6 + i] = 0.0, am[12 + i] = 0.0;  // (the floored piece is constant)
      const double D1 = dot6_paired(gg, am[6] * inv, am[7] * inv, am[8] * inv, am[9] * inv, am[10] * inv, am[11] * inv);
      const double D2 = dot6_paired(gg, am[12] * inv, am[13] * inv, am[14] * inv, am[15] * inv, am[16] * inv, am[17] * inv);
      ambient_fit::add_entry(D_of(&am[0]), D1, D2, s0, s1, s2);
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const bool f0 = am[i] < kMinNormGL, f1 = am[6 + i] < kMinNormGL, f2 = am[12 + i] < kMinNormGL;
        cr = cr || f0 != f1 || f1 != f2;
      }
#pragma unroll
      for (int i = 0; i < 18; ++i)
        if (am[i] < kMinNormGL) am[i] = kMinNormGL;
      s0 += pos_log(D_of(&am[0]), 0.0);
      s1 += pos_log(D_of(&am[6]), 0.0);
      s2 += pos_log(D_of(&am[12]), 0.0);
    }
  }
  out[0] = ambient_fit::wave_sum(s0);
  out[1] = ambient_fit::wave_sum(s1);
  out[2] = ambient_fit::wave_sum(s2);
  if (crosses) *crosses = __any(cr) != 0;
}

// grid: ceil(C * n_cand / 4) workgroups of four waves; wave unit <-> (cell, slot), the slot fastest, so the waves of a
// workgroup walk the same entries.  dout: [5][n_units] alpha_hat, ll_hat, ll_zero, info, ll_top; iout: [2][n_units] status,
// n_steps
__global__ void __launch_bounds__(256)
    fma_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ pair, double alpha_max,
                   const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                   const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                   const double* __restrict__ lut_g, const double* __restrict__ cgp, int K, double* __restrict__ dout,
                   int32_t* __restrict__ iout) {
  __shared__ double lut[256];
  lut[threadIdx.x] = lut_g[threadIdx.x];
  __syncthreads();
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int lane = threadIdx.x & 63;
  const int64_t c = unit / n_cand;
  const int32_t j = pair[2 * unit], k = pair[2 * unit + 1];
  ambient_fit::result res;  // (a negative index: status 4, all outputs 0)
  double ll_top = 0.0;      // (its own variable: the coarse callable writes it while the search runs)
  bool have_top = false;
  if (j >= 0 && k >= 0) {
    const int64_t e0 = cell_ptr[c], e1 = cell_ptr[c + 1];
    const size_t K3 = (size_t)K * 3;
    const double* qj = cgp + (size_t)j * 3;
    const double* qk = cgp + (size_t)k * 3;
    auto coarse = [&](const double (&x)[3], double (&o)[3], bool& crosses) {
      fma_fit_pass<false>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, qj, qk, K3, x, o, &crosses);
      // (coarse point 8 is alpha_max bit for bit: the third share of the third pass; later passes that end on alpha_max,
      // the bracket's and the scan's, repeat it)
      if (!have_top && x[2] == alpha_max) ll_top = ambient_fit::uniform(o[2]), have_top = true;
    };
    auto deriv = [&](double x, double& L, double& d1, double& d2) {
      const double xs[3] = {x, 0.0, 0.0};
      double o[3];
      fma_fit_pass<true>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, qj, qk, K3, xs, o, nullptr);
      L = o[0], d1 = o[1], d2 = o[2];
    };
    // (a droplet without entries: every coarse LL is 0, the first derivative pass finds nothing, status 5)
    res = ambient_fit::search_piecewise(alpha_max, coarse, deriv, [&] { return e0 == e1; });
    res.ll_top = res.status == ambient_fit::NO_ENTRY ? 0.0 : res.status == ambient_fit::NOT_FINITE ? res.ll_zero : ll_top;
  }
  ambient_fit::store<5>(res, lane, unit, n_units, dout, iout);
}

}  // namespace

// the caller's arguments, on the host, before any device work: 0, or 1 with the reason in `why`
int fmx_alpha_fit_bad_args(int32_t n_cand, const int32_t* pair, int64_t C, int K, double alpha_max, bool any_out, char* why,
                           size_t n) {
  const char* who = "muxgl_fmx_alpha_fit";
  if (ambient_fit::bad_head(who, n_cand, pair ? nullptr : "pair", "alpha_max", alpha_max, any_out, why, n)) return 1;
  for (int64_t i = 0; i < C * n_cand; ++i) {
    const int32_t j = pair[2 * i], k = pair[2 * i + 1];
    for (int t = 0; t < 2; ++t)
      if (pair[2 * i + t] < -1 || pair[2 * i + t] >= K)
        return snprintf(why, n, "%s: pair[%lld][%d][%d] (%d) is neither -1 nor a cluster in [0,%d)", who,
                        (long long)(i / n_cand), (int)(i % n_cand), t, pair[2 * i + t], K), 1;
    if ((j < 0) != (k < 0))
      return snprintf(why, n, "%s: pair[%lld][%d] (%d, %d) has exactly one negative index", who, (long long)(i / n_cand),
                      (int)(i % n_cand), j, k), 1;
  }
  return 0;
}

extern "C" int muxgl_fmx_alpha_fit(muxgl_handle* h, int32_t n_cand, const int32_t* pair, double alpha_max, double* alpha_hat,
                                   double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status,
                                   int32_t* n_steps, float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (h->group)
    return group_fmx_alpha_fit(h, n_cand, pair, alpha_max, alpha_hat, ll_hat, ll_zero, ll_top, info, status, n_steps, kernel_ms);
  HIPCHK(h, hipSetDevice(h->device));
  if (fmx_refuse(h, h, "muxgl_fmx_alpha_fit", "the fit belongs")) return 1;
  const ambient_fit::outputs out = {alpha_hat, ll_hat, ll_zero, info, status, n_steps, ll_top};
  char why[256];
  if (fmx_alpha_fit_bad_args(n_cand, pair, h->C, h->K, alpha_max, out.any(), why, sizeof(why))) MUXGL_FAIL(h, "%s", why);
  if (h->C == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing, no timing slot: records, timings and every other state of the handle keep their values)
  return ambient_fit::host_run(h, "muxgl_fmx_alpha_fit", nullptr, n_cand, 2, pair, 5, out, kernel_ms,
                               [&](int64_t n_units, const double*, const int32_t* d_pair, double* d_dout, int32_t* d_iout) {
                                 hipLaunchKernelGGL(fma_fit_kernel, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream,
                                                    n_units, (int)n_cand, d_pair, alpha_max, h->d_cell_ptr, h->d_entry_snp,
                                                    h->d_entry_rptr, h->d_reads, h->d_lut, h->d_cgp, h->K, d_dout, d_iout);
                                 HIPCHK(h, hipGetLastError());
                                 return 0;
                               });
}
