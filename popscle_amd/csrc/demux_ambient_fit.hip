// demux_ambient_fit.hip -- muxgl_demux_ambient_fit: the ambient share rho of muxgl_demux_ambient (demux_ambient.hip) as a
// per-droplet maximum-likelihood estimate with its observed information, for a few candidate samples per droplet.  Every
// read's factor pR (1 - p) + pA p is linear in rho, because p = 0.5 l + (2 f - l) 0.5 rho (the reference's own
// expression, cmd_cram_demuxlet.cpp:673, with the second donor's genotype replaced by 2 f): t = u + v rho with
// v = (pA - pR) (2 f - l) 0.5.  An entry's product a_l(rho) is therefore a polynomial, and its first two derivatives
// follow from the product rule along the reads, with no division and no finite difference:
//
//   a'' = a'' t + 2 a' v;   a' = a' t + a v;   a = a t                                  (in this order, per usable read)
//   w_l = (a_l / q_max_e + 1e-10) / (1 + 1e-10),   w_l' = a_l' / q_max_e / (1 + 1e-10),   w_l'' likewise
//   D = sum_l gp[s_e][j][l] w_l,   D', D'' likewise
//   LL = sum_e log D,   LL' = sum_e D' / D,   LL'' = sum_e (D'' / D - (D' / D)^2)       over entries whose marker has genotypes
//
// t is formed exactly as amb_weight_kernel forms it (p is exactly 0 at (l = 0, f = 0) and exactly 1 at (l = 2, f = 1),
// where v is exactly 0); the grid's NA x 9 products run beside the triples in grid_walk (demux_entry.hpp, where the
// argument that q_max_e is the same number stands), and all nine of (a, a', a'') are rescaled together every 32 reads by
// the grid's maximum only.  The product rule, the step from (D, D', D'') to the three sums, the end of a pass, the
// kernel's frame and the host side of the call are ambient_fit_search.hpp's, shared with all the fits.
//
// amb_fit_kernel, one wave per (cell, candidate) in ambient_fit::frame: the lanes stride the cell's entries, each lane
// walks its entry's read bytes through the Phred table in LDS, dots the three triples with the candidate's gp row and adds
// its share of (LL, LL', LL'') in entry order, and the search is ambient_fit::search, three coarse points per pass (nine
// products per lane, as in a derivative pass).
//
// Memory: the inputs, cand and the six output arrays.  Nothing proportional to nnz is allocated, so no slab budget applies.
#include <cmath>
#include <vector>

#include "ambient_fit_search.hpp"
#include "demux_entry.hpp"

namespace {

// One pass of a wave over the entries [e0, e1) of a cell for candidate column j.
//   DERIV = false: out[k] = LL(x[k]) for the NC <= 3 shares x[0..NC-1]
//   DERIV = true:  out = (LL, LL', LL'') at x[0]
// Returns in every lane the same bits.  n_scored (DERIV only): the entries whose marker has genotypes.
template <int NA, bool DERIV, int NC>
__device__ __forceinline__ void fit_pass(int64_t e0, int64_t e1, int lane, const int32_t* __restrict__ entry_snp,
                                         const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                                         const double* lut, const demux_grid& al, const double* __restrict__ af,
                                         const uint8_t* __restrict__ has_gp, const double* __restrict__ gpj, size_t V3,
                                         const double (&x)[3], double (&out)[3], int* n_scored) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int ns = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int32_t s = entry_snp[e];
    if (!has_gp[s]) continue;  // (no genotypes: the reference skips the marker, :733)
    ++ns;
    const double tf = af[s] + af[s];
    const double tf1 = tf - 1.0, tf2 = tf - 2.0;
    // p per (share, l) as amb_weight_kernel forms it; DERIV: dp/drho per l in pv[3..5]
    double pv[9];
    if (DERIV) {
      const double hr = 0.5 * x[0];
      pv[0] = tf * hr, pv[1] = fma(tf1, hr, 0.5), pv[2] = fma(tf2, hr, 1.0);
      pv[3] = 0.5 * tf, pv[4] = 0.5 * tf1, pv[5] = 0.5 * tf2;
      pv[6] = pv[7] = pv[8] = 0.0;
    } else {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const double hr = 0.5 * x[k];
        pv[k * 3 + 0] = tf * hr, pv[k * 3 + 1] = fma(tf1, hr, 0.5), pv[k * 3 + 2] = fma(tf2, hr, 1.0);
      }
    }
    // am: DERIV ? (a_0, a_1, a_2, a_0', a_1', a_2', a_0'', a_1'', a_2'') : a_l of share k at k * 3 + l
    constexpr int NM = DERIV ? 9 : NC * 3;
    double pG[NA * 9], am[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) am[i] = (DERIV && i >= 3) ? 0.0 : 1.0;
    // the grid's walk (demux_entry.hpp); the widest grid with the hoist barrier.  All of am follows the grid's rescale.
    const double mx = grid_walk<NA, NM, (NA > 12)>(
        reads, entry_rptr[e], entry_rptr[e + 1], al.a, lut, pG, am, [&](double pR, double pA, double d) {
          if (DERIV) {
            ambient_fit::product_rule<3>(am, [&](int l, double& t, double& v) {
              t = fma(pA, pv[l], pR * (1.0 - pv[l]));
              v = d * pv[3 + l];
            });
          } else {
#pragma unroll
            for (int i = 0; i < NM; ++i) am[i] *= fma(pA, pv[i], pR * (1.0 - pv[i]));
          }
        });
    const double c = 1.0 / (1.0 + 1e-10);
    const double sc = c / mx, t10 = 1e-10 * c;
    const double* g = gpj + (size_t)s * V3;
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    auto D_of = [&](const double* a) { return fma(g2, fma(a[2], sc, t10), fma(g1, fma(a[1], sc, t10), g0 * fma(a[0], sc, t10))); };
    if (DERIV) {
      const double D1 = fma(g2, am[5] * sc, fma(g1, am[4] * sc, g0 * (am[3] * sc)));  // (the offset's derivative is 0)
      const double D2 = fma(g2, am[8] * sc, fma(g1, am[7] * sc, g0 * (am[6] * sc)));
      ambient_fit::add_entry(D_of(&am[0]), D1, D2, s0, s1, s2);
    } else {
      s0 += pos_log(D_of(&am[0]), 0.0);
      if (NC > 1) s1 += pos_log(D_of(&am[3]), 0.0);
      if (NC > 2) s2 += pos_log(D_of(&am[6]), 0.0);
    }
  }
  ambient_fit::pass_sums<DERIV ? 3 : NC>(s0, s1, s2, ns, out, n_scored);
}

// dout: [4][n_units] rho_hat, ll_hat, ll_zero, info; iout: [2][n_units] status, n_steps
template <int NA>
__global__ void __launch_bounds__(256)
    amb_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ cand, double rho_max,
                   const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                   const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                   const double* __restrict__ lut_g, demux_grid al, const double* __restrict__ af,
                   const uint8_t* __restrict__ has_gp, const double* __restrict__ gp, int V, double* __restrict__ dout,
                   int32_t* __restrict__ iout) {
  ambient_fit::frame<384, 1, 4>(
      n_units, n_cand, cand, cell_ptr, lut_g, dout, iout,
      [&](const double* lut, int lane, int64_t e0, int64_t e1, int32_t j, int32_t) {
        const size_t V3 = (size_t)V * 3;
        const double* gpj = gp + (size_t)j * 3;
        // shares per coarse pass: three (nine products per lane, as in a derivative pass); one at the widest grid, whose
        // 144 products leave a lane no room for more.  Every sum belongs to one share, so the chunking changes no bit.
        constexpr int NC = NA > 12 ? 1 : 3;
        auto coarse = [&](const double (&x)[3], double (&o)[3]) {
          fit_pass<NA, false, NC>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, af, has_gp, gpj, V3, x, o, nullptr);
        };
        int n_scored = 0;
        auto deriv = [&](double x, double& L, double& d1, double& d2) {
          const double xs[3] = {x, 0.0, 0.0};
          double o[3];
          fit_pass<NA, true, 1>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, af, has_gp, gpj, V3, xs, o, &n_scored);
          L = o[0], d1 = o[1], d2 = o[2];
        };
        return ambient_fit::search<NC, false>(rho_max, coarse, deriv, [&] { return n_scored == 0; });
      });
}

}  // namespace

int demux_ambient_fit_run(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int n_cand,
                          const int32_t* cand, double rho_max, double* rho_hat, double* ll_hat, double* ll_zero,
                          double* info, int32_t* status, int32_t* n_steps, float* kernel_ms) {
  if (demux_ambient_check_af(h, amb_af, "muxgl_demux_ambient_fit")) return 1;
  const demux_grid al = demux_grid_of(p);
  const ambient_fit::outputs out = {rho_hat, ll_hat, ll_zero, info, status, n_steps};
  return ambient_fit::host_run(h, "muxgl_demux_ambient_fit", amb_af, n_cand, 1, cand, 4, out, kernel_ms,
                               [&](int64_t n_units, const double* d_af, const int32_t* d_cand, double* d_dout, int32_t* d_iout) {
#define CALL_F(N)                                                                                                \
  ambient_fit::launch(h, amb_fit_kernel<N>, n_units, n_cand, d_cand, rho_max, h->d_cell_ptr, h->d_entry_snp,    \
                      h->d_entry_rptr, h->d_reads, h->d_lut, al, d_af, h->d_has_gp, h->d_gp, h->V, d_dout, d_iout)
                                 DISPATCH_NA(p->n_alpha, CALL_F);
#undef CALL_F
                               });
}
