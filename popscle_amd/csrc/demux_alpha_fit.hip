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
//   D', D'' the same sums over w', w'' (the diagonal's are 0), with (l, m) added next to (m, l): pair_fit::dot6_paired
//   LL = sum_e log D,   LL' = sum_e D' / D,   LL'' = sum_e (D'' / D - (D' / D)^2)       over entries whose marker has genotypes
//
// The three diagonal elements do not depend on alpha: they are the grid's own elements (l, l) of alpha[0], which the pass
// forms anyway, so a lane carries the six off-diagonal ones only: (a, a', a'') of one share, 18 doubles, or a of three
// shares, 18 doubles.  The grid's NA x 9 products are formed by grid_walk (demux_entry.hpp, where the argument that
// q_max_e is the same number stands), and the pair's elements are rescaled with them every 32 reads, by the grid's maximum
// only.  The pair's p, the GP products and the two sums are pair_fit.hpp's, shared with fmx_alpha_fit.hip; the product rule,
// the step from (D, D', D'') to the three sums, the end of a pass, the kernel's frame, ll_top and the host side of the call
// are ambient_fit_search.hpp's, shared with all the fits.
//
// alpha_fit_kernel, one wave per (cell, slot) in ambient_fit::frame: the lanes stride the cell's entries, each lane walks
// its entry's read bytes through the Phred table in LDS, dots the nine elements with the nine GP products and adds its
// share of (LL, LL', LL'') in entry order, and the search is ambient_fit::search.
//
// Memory: the inputs, pair and the seven output arrays.  Nothing proportional to nnz is allocated, so no slab budget applies.
#include <cmath>
#include <vector>

#include "ambient_fit_search.hpp"
#include "demux_entry.hpp"
#include "pair_fit.hpp"

namespace {

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
  pair_fit::p_of<(DERIV ? 1 : NC)>(x, pv, [](double v) { return v; });
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
              v = d * pair_fit::P1[i];
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
    double gg[9];
    pair_fit::gg_of(gpj + (size_t)s * V3, gpk + (size_t)s * V3, gg);
    auto D_of = [&](const double* a) {
      return pair_fit::dot9(gg, wd0, wd1, wd2, a, [&](double v) { return fma(v, sc, t10); });
    };
    auto dD_of = [&](const double* a) { return pair_fit::dot6_paired(gg, a, [&](double v) { return v * sc; }); };
    if (DERIV) {
      // (the offset's derivative is 0, and so is the diagonal's)
      const double D1 = dD_of(&am[6]), D2 = dD_of(&am[12]);
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

// dout: [5][n_units] alpha_hat, ll_hat, ll_zero, info, ll_top; iout: [2][n_units] status, n_steps
template <int NA>
__global__ void __launch_bounds__(256)
    alpha_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ pair, double alpha_max,
                     const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                     const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                     const double* __restrict__ lut_g, demux_grid al, const uint8_t* __restrict__ has_gp,
                     const double* __restrict__ gp, int V, double* __restrict__ dout, int32_t* __restrict__ iout) {
  ambient_fit::frame<384, 2, 5>(
      n_units, n_cand, pair, cell_ptr, lut_g, dout, iout,
      [&](const double* lut, int lane, int64_t e0, int64_t e1, int32_t j, int32_t k) {
        const size_t V3 = (size_t)V * 3;
        const double* gpj = gp + (size_t)j * 3;
        const double* gpk = gp + (size_t)k * 3;
        constexpr int NC = coarse_shares<NA>();
        double ll_top = 0.0;  // (its own variable: the coarse callable writes it while the search runs)
        auto coarse = [&](const double (&x)[3], double (&o)[3]) {
          fit_pass<NA, false, NC>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, has_gp, gpj, gpk, V3, x, o, nullptr);
          ambient_fit::keep_top<NC>(x, o, alpha_max, ll_top);
        };
        int n_scored = 0;
        auto deriv = [&](double x, double& L, double& d1, double& d2) {
          const double xs[3] = {ambient_fit::uniform(x), 0.0, 0.0};  // (the same bits in every lane)
          double o[3];
          fit_pass<NA, true, 1>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, has_gp, gpj, gpk, V3, xs, o, &n_scored);
          L = o[0], d1 = o[1], d2 = o[2];
        };
        ambient_fit::result res = ambient_fit::search<NC, false>(alpha_max, coarse, deriv, [&] { return n_scored == 0; });
        res.ll_top = ambient_fit::top_of(res, ll_top);
        return res;
      });
}

}  // namespace

// ambient_fit::host_run without an amb_af, with two indices per slot and ll_top as the fifth double row
int demux_alpha_fit_run(muxgl_handle* h, const muxgl_demux_params* p, int n_cand, const int32_t* pair, double alpha_max,
                        double* alpha_hat, double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status,
                        int32_t* n_steps, float* kernel_ms) {
  const demux_grid al = demux_grid_of(p);
  const ambient_fit::outputs out = {alpha_hat, ll_hat, ll_zero, info, status, n_steps, ll_top};
  return ambient_fit::host_run(h, "muxgl_demux_alpha_fit", nullptr, n_cand, 2, pair, 5, out, kernel_ms,
                               [&](int64_t n_units, const double*, const int32_t* d_pair, double* d_dout, int32_t* d_iout) {
#define CALL_F(N)                                                                                                    \
  ambient_fit::launch(h, alpha_fit_kernel<N>, n_units, n_cand, d_pair, alpha_max, h->d_cell_ptr, h->d_entry_snp,    \
                      h->d_entry_rptr, h->d_reads, h->d_lut, al, h->d_has_gp, h->d_gp, h->V, d_dout, d_iout)
                                 DISPATCH_NA(p->n_alpha, CALL_F);
#undef CALL_F
                               });
}
