// demux_alpha_fit.hip -- muxgl_demux_alpha_fit: the mixing share alpha of a demuxlet doublet as a per-droplet
// maximum-likelihood estimate with its observed information, for a few pairs of samples (j, k) per droplet.  Every read's
// factor pR (1 - p) + pA p of the reference's doublet term is linear in alpha, because p = 0.5 l + (m - l) 0.5 alpha is
// (cmd_cram_demuxlet.cpp:673): t = u + v alpha with v = (pA - pR) (m - l) 0.5, exactly 0 on the diagonal l == m.  The
// product a_lm(alpha) of an entry is therefore a polynomial, and its first two derivatives follow from the product rule
// along the reads, as in demux_ambient_fit.hip:
//
//   a'' = a'' t + 2 a' v;   a' = a' t + a v;   a = a t                                  (in this order, per usable read)
//   w_lm = (a_lm / q_max_e + 1e-10) / (1 + 1e-10),   w_lm' = a_lm' / q_max_e / (1 + 1e-10),   w_lm'' likewise
//   D = sum_l sum_m (gp[s_e][j][l] gp[s_e][k][m]) w_lm   (:740: the product of the two GPs first; l, then m)
//   D', D'' the same sums over w', w'' (the diagonal's are 0), with (l, m) added next to (m, l): dot6_paired below
//   LL = sum_e log D,   LL' = sum_e D' / D,   LL'' = sum_e (D'' / D - (D' / D)^2)       over entries whose marker has genotypes
//
// The three diagonal elements do not depend on alpha: they are the grid's own elements (l, l) of alpha[0], which the pass
// forms anyway, so a lane carries the six off-diagonal ones only: (a, a', a'') of one share, 18 doubles, or a of three
// shares, 18 doubles.  The grid's NA x 9 products are formed by grid_walk (demux_entry.hpp, where the argument that
// q_max_e is the same number stands), and the pair's elements are rescaled with them every 32 reads, by the grid's maximum
// only.  The product rule, the step from (D, D', D'') to the three sums, the end of a pass and the host side of the call
// are ambient_fit_search.hpp's, shared with demux_ambient_fit.hip.
// p is formed by one fma from the reference's expression and is exact at the ends: at alpha = 0 every element (l, m) has
// p = 0.5 l (sample j alone), at alpha = 1 p = 0.5 m (sample k alone).
//
// alpha_fit_kernel, one wave per (cell, slot): the lanes stride the cell's entries, each lane walks its entry's read bytes
// through the Phred table in LDS, dots the nine elements with the nine GP products and adds its share of (LL, LL', LL'') in
// entry order; a fixed xor butterfly adds the 64 shares, so every lane holds the same bits and every decision of the
// search (ambient_fit_search.hpp, shared with the two ambient fits) is wave-uniform.  The whole fit runs in this one
// launch.  The coarse callable keeps LL of coarse point 8, alpha_max: ll_top.  A coarse pass and a derivative pass form
// a and D by the same operations, so ll_hat on a bound is ll_zero resp. ll_top bit for bit.
// Every reduction tree is fixed by the cell alone (lane = entry index modulo 64, then the butterfly), there is no atomic
// and nothing depends on the batch, the device or the other slots: the outputs are bit-identical from call to call, for
// any order or grouping of the slots, on one device, on a group and through the sharded driver.
//
// Memory: the inputs, pair and the seven output arrays.  Nothing proportional to nnz is allocated, so no slab budget applies.
#include <cmath>
#include <vector>

#include "ambient_fit_search.hpp"
#include "demux_entry.hpp"

namespace {

// the six off-diagonal elements i <-> (l, m): (0,1) (0,2) (1,0) (1,2) (2,0) (2,1); p = P0[i] + P1[i] alpha (:673)
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

// sum over the six off-diagonal elements of gg[l * 3 + m] * w_lm' for a derivative of D (the diagonal's is 0), (l, m) next to
// (m, l): six rounded products, no fused step.  Where the two GP rows are the same numbers (j == k, or a sample that is
// a copy of another) gg is symmetric, and in a one-read entry w_lm' == -w_ml' exactly (v is +-0.5 d or +-d): the pairs
// then cancel to an exact 0, as they do in exact arithmetic, where a fused chain in the order l, m leaves a residue of
// rounding that an entry with a small D divides up.
__device__ __forceinline__ double dot6_paired(const double (&gg)[9], double wo0, double wo1, double wo2, double wo3, double wo4,
                                              double wo5) {
#pragma clang fp contract(off)
  const double p01 = gg[1] * wo0, p10 = gg[3] * wo2;
  const double p02 = gg[2] * wo1, p20 = gg[6] * wo4;
  const double p12 = gg[5] * wo3, p21 = gg[7] * wo5;
  return ((p01 + p10) + (p02 + p20)) + (p12 + p21);
}

// One pass of a wave over the entries [e0, e1) of a cell for the pair of columns (j, k).
//   DERIV = false: out[c] = LL(x[c]) for the NC <= 3 shares x[0..NC-1]
//   DERIV = true:  out = (LL, LL', LL'') at x[0]
// Returns in every lane the same bits.  n_scored (DERIV only): the entries whose marker has genotypes.
template <int NA, bool DERIV, int NC>
__device__ __forceinline__ void fit_pass(int64_t e0, int64_t e1, int lane, const int32_t* __restrict__ entry_snp,
                                         const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                                         const double* lut, const demux_grid& al, const uint8_t* __restrict__ has_gp,
                                         const double* __restrict__ gpj, const double* __restrict__ gpk, size_t V3,
                                         const double (&x)[3], double (&out)[3], int* n_scored) {
  // p per (share, element); the same for every entry, and wave-uniform
  constexpr int NM = DERIV ? 6 : NC * 6;
  double pv[NM];
#pragma unroll
  for (int c = 0; c < (DERIV ? 1 : NC); ++c)
#pragma unroll
    for (int i = 0; i < 6; ++i) pv[c * 6 + i] = fma(P1[i], x[c], P0[i]);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int ns = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int32_t s = entry_snp[e];
    if (!has_gp[s]) continue;  // (no genotypes: the reference skips the marker, :733)
    ++ns;
    // am: DERIV ? (a_i, a_i', a_i'') at i, 6 + i, 12 + i : a_i of share c at c * 6 + i
    double pG[NA * 9], am[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) am[i] = (DERIV && i >= 6) ? 0.0 : 1.0;
    // the grid's walk (demux_entry.hpp); the wide grids with the hoist barrier.  The pair's elements follow the grid's
    // rescale, all together.
    const double mx = grid_walk<NA, (DERIV ? 18 : NM), (NA > 8)>(
        reads, entry_rptr[e], entry_rptr[e + 1], al.a, lut, pG, am, [&](double pR, double pA, double d) {
          if (DERIV) {
            ambient_fit::product_rule<6>(am, [&](int i, double& t, double& v) {
              t = fma(pA, pv[i], pR * (1.0 - pv[i]));
              v = d * P1[i];
            });
          } else {
#pragma unroll
            for (int i = 0; i < NM; ++i) am[i] *= fma(pA, pv[i], pR * (1.0 - pv[i]));
          }
        });
    const double c1 = 1.0 / (1.0 + 1e-10);
    const double sc = c1 / mx, t10 = 1e-10 * c1;
    // the diagonal: the grid's elements (l, l) of alpha[0]
    const double wd0 = fma(pG[0], sc, t10), wd1 = fma(pG[4], sc, t10), wd2 = fma(pG[8], sc, t10);
    const double* gj = gpj + (size_t)s * V3;
    const double* gk = gpk + (size_t)s * V3;
    const double k0 = gk[0], k1 = gk[1], k2 = gk[2];
    double gg[9];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const double jl = gj[l];
      gg[l * 3 + 0] = jl * k0, gg[l * 3 + 1] = jl * k1, gg[l * 3 + 2] = jl * k2;  // :740
    }
    auto D_of = [&](const double* a) {
      return dot9(gg, wd0, wd1, wd2, fma(a[0], sc, t10), fma(a[1], sc, t10), fma(a[2], sc, t10), fma(a[3], sc, t10),
                  fma(a[4], sc, t10), fma(a[5], sc, t10));
    };
    if (DERIV) {
      // (the offset's derivative is 0, and so is the diagonal's)
      const double D1 = dot6_paired(gg, am[6] * sc, am[7] * sc, am[8] * sc, am[9] * sc, am[10] * sc, am[11] * sc);
      const double D2 = dot6_paired(gg, am[12] * sc, am[13] * sc, am[14] * sc, am[15] * sc, am[16] * sc, am[17] * sc);
      ambient_fit::add_entry(D_of(&am[0]), D1, D2, s0, s1, s2);
    } else {
      s0 += pos_log(D_of(&am[0]), 0.0);
      if (NC > 1) s1 += pos_log(D_of(&am[6]), 0.0);
      if (NC > 2) s2 += pos_log(D_of(&am[12]), 0.0);
    }
  }
  ambient_fit::pass_sums<DERIV ? 3 : NC>(s0, s1, s2, ns, out, n_scored);
}

// coarse shares per pass, 1 or 3 (ambient_fit::search): three where the NA * 9 + 18 products of a lane stay in registers
template <int NA>
constexpr int coarse_shares() {
  return NA > 12 ? 1 : 3;
}

// grid: ceil(C * n_cand / 4) workgroups of four waves; wave unit <-> (cell, slot), the slot fastest, so the waves of a
// workgroup walk the same entries.  dout: [5][n_units] alpha_hat, ll_hat, ll_zero, info, ll_top; iout: [2][n_units] status,
// n_steps
template <int NA>
__global__ void __launch_bounds__(256)
    alpha_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ pair, double alpha_max,
                     const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                     const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                     const double* __restrict__ lut_g, demux_grid al, const uint8_t* __restrict__ has_gp,
                     const double* __restrict__ gp, int V, double* __restrict__ dout, int32_t* __restrict__ iout) {
  __shared__ double lut[384];
  for (int i = threadIdx.x; i < 384; i += 256) lut[i] = lut_g[i];
  __syncthreads();
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int lane = threadIdx.x & 63;
  const int64_t c = unit / n_cand;
  const int32_t j = pair[2 * unit], k = pair[2 * unit + 1];
  ambient_fit::result res;  // (a negative index: status 4, all outputs 0)
  double ll_top = 0.0;  // (its own variable: the coarse callable writes it while the search runs)
  if (j >= 0 && k >= 0) {
    const int64_t e0 = cell_ptr[c], e1 = cell_ptr[c + 1];
    const size_t V3 = (size_t)V * 3;
    const double* gpj = gp + (size_t)j * 3;
    const double* gpk = gp + (size_t)k * 3;
    constexpr int NC = coarse_shares<NA>();
    auto coarse = [&](const double (&x)[3], double (&o)[3]) {
      fit_pass<NA, false, NC>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, has_gp, gpj, gpk, V3, x, o, nullptr);
      if (x[NC - 1] == alpha_max) ll_top = o[NC - 1];  // (coarse point 8 is alpha_max bit for bit, and the only one)
    };
    int n_scored = 0;
    auto deriv = [&](double x, double& L, double& d1, double& d2) {
      const double xs[3] = {ambient_fit::uniform(x), 0.0, 0.0};  // (the same bits in every lane)
      double o[3];
      fit_pass<NA, true, 1>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, has_gp, gpj, gpk, V3, xs, o, &n_scored);
      L = o[0], d1 = o[1], d2 = o[2];
    };
    res = ambient_fit::search<NC, false>(alpha_max, coarse, deriv, [&] { return n_scored == 0; });
    res.ll_top = res.status == ambient_fit::NO_ENTRY ? 0.0 : ll_top;
  }
  ambient_fit::store<5>(res, lane, unit, n_units, dout, iout);
}

template <int NA>
int launch_fit(muxgl_handle* h, int64_t n_units, int n_cand, const int32_t* d_pair, double alpha_max, const demux_grid& al,
               double* d_dout, int32_t* d_iout) {
  hipLaunchKernelGGL((alpha_fit_kernel<NA>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, n_cand,
                     d_pair, alpha_max, h->d_cell_ptr, h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, al,
                     h->d_has_gp, h->d_gp, h->V, d_dout, d_iout);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int fit_dispatch(muxgl_handle* h, int A, int64_t n_units, int n_cand, const int32_t* d_pair, double alpha_max,
                 const demux_grid& al, double* d_dout, int32_t* d_iout) {
#define CALL_F(N) launch_fit<N>(h, n_units, n_cand, d_pair, alpha_max, al, d_dout, d_iout)
  DISPATCH_NA(A, CALL_F);
#undef CALL_F
}

}  // namespace

// the arguments checked on the host: 0, or 1 with the reason in `why`
int demux_alpha_fit_bad_args(int32_t n_cand, const int32_t* pair, int64_t C, int V, double alpha_max, bool any_out, char* why,
                             size_t n) {
  const char* who = "muxgl_demux_alpha_fit";
  if (ambient_fit::bad_head(who, n_cand, pair ? nullptr : "pair", "alpha_max", alpha_max, any_out, why, n)) return 1;
  for (int64_t i = 0; i < C * n_cand; ++i) {
    const int32_t j = pair[2 * i], k = pair[2 * i + 1];
    for (int t = 0; t < 2; ++t)
      if (pair[2 * i + t] < -1 || pair[2 * i + t] >= V)
        return snprintf(why, n, "%s: pair[%lld][%d][%d] (%d) is neither -1 nor a sample in [0,%d)", who,
                        (long long)(i / n_cand), (int)(i % n_cand), t, pair[2 * i + t], V), 1;
    if ((j < 0) != (k < 0))
      return snprintf(why, n, "%s: pair[%lld][%d] (%d, %d) has exactly one negative index", who, (long long)(i / n_cand),
                      (int)(i % n_cand), j, k), 1;
  }
  return 0;
}

// ambient_fit::host_run without an amb_af, with two indices per slot and ll_top as the fifth double row
int demux_alpha_fit_run(muxgl_handle* h, const muxgl_demux_params* p, int n_cand, const int32_t* pair, double alpha_max,
                        double* alpha_hat, double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status,
                        int32_t* n_steps, float* kernel_ms) {
  const demux_grid al = demux_grid_of(p);
  const ambient_fit::outputs out = {alpha_hat, ll_hat, ll_zero, info, status, n_steps, ll_top};
  return ambient_fit::host_run(h, "muxgl_demux_alpha_fit", nullptr, n_cand, 2, pair, 5, out, kernel_ms,
                               [&](int64_t n_units, const double*, const int32_t* d_pair, double* d_dout, int32_t* d_iout) {
                                 return fit_dispatch(h, p->n_alpha, n_units, n_cand, d_pair, alpha_max, al, d_dout, d_iout);
                               });
}
