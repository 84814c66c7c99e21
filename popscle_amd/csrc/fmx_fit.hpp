// fmx_fit.hpp -- what the two freemuxlet fits, muxgl_fmx_ambient_fit (fmx_ambient_fit.hip) and
// muxgl_fmx_alpha_fit (fmx_alpha_fit.hip), say alike: one pass of a wave over a cell's entries and the kernel
// around it.  Beside the reference's nine (fmx_nine_walk, fmx_entry.hpp) an entry carries NE elements a_i(x), each a
// product over the reads of a factor mat xi + e4, xi = ALT read ? p_i : 1 - p_i, that is linear in the share x:
//
//   a'' = a'' fac + 2 a' v;   a' = a' fac + a v;   a = a fac;   all three times the read's 1 / t     (in this order, per usable read)
//   after the reads, where a_i < 1e-6:  a_i = 1e-6, a_i' = a_i'' = 0                     (the floor of sc_drop_seq.cpp:498-501)
//   LL = sum_e log D,   LL' = sum_e D' / D,   LL'' = sum_e (D'' / D - (D' / D)^2)         over ALL entries (no has_gp here)
//
// A Model states what differs:
//   NE, WIDTH, ROWS           elements per entry (3 or 6), indices per slot (1 or 2), double rows of the result (4 or 5)
//   Model(af, cgp, K, j, k)   the slot's posterior rows (k == j where WIDTH is 1)
//   shares<DERIV>             p[share * NE + i] of the pass's shares (one in a derivative pass, three in a coarse pass) and
//                             slope(i) = dp_i/dx; formed in pass(x), once per pass and wave-uniform, or in entry(m, s, x),
//                             per entry from the marker's numbers
//   weights(m, s, gls, inv)   what an entry's sums take from the posteriors of marker s and from the walk's nine;
//                             D(a, inv) from the floored elements a[0..NE) and 1 / T, dD(a, inv) from their derivatives
//
// The kernel: one wave per (cell, slot) in ambient_fit::frame; lane = entry index modulo 64, striding the cell's entries;
// each lane walks its entry's read bytes through the Phred table in LDS with the nine and 3 NE more doubles (three shares'
// elements in a coarse pass, (a, a', a'') in a derivative pass) and adds its share of the sums in entry order; a fixed xor
// butterfly adds the 64 shares, so every lane holds the same bits and every decision of the search
// (ambient_fit::search_piecewise, three points per pass) is wave-uniform.  The nine are recomputed on every pass: nothing
// proportional to nnz is allocated, so no slab budget applies and MUXGL_FMX_SLAB_MB is not read.
// A posterior row of exactly 0 at one of the cell's markers makes D = 0 and LL = -inf at every share: status 6, found at
// the coarse points before any derivative is formed, so no NaN is written.
#pragma once
#include "ambient_fit_search.hpp"
#include "fmx_entry.hpp"

// One pass of a wave over the entries [e0, e1) of a cell.
//   DERIV = false: out[c] = LL(x[c]) for the three shares x[0..2]
//   DERIV = true:  out = (LL, LL', LL'') at x[0]
// Returns in every lane the same bits.  crosses (coarse pass): whether an element of the cell is below the floor at one of
// the three shares and not at another.
template <class Model, bool DERIV>
__device__ __forceinline__ void fmx_fit_pass(const Model& m, int64_t e0, int64_t e1, int lane,
                                             const int32_t* __restrict__ entry_snp, const int64_t* __restrict__ entry_rptr,
                                             const uint8_t* __restrict__ reads, const double* lut, const double (&x)[3],
                                             double (&out)[3], bool* crosses) {
  constexpr int NE = Model::NE, NM = 3 * NE;
  typename Model::template shares<DERIV> sh;
  sh.pass(x);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  bool cr = false;  // (coarse pass) an element of one of the lane's entries is floored at one share and not at another
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int32_t s = entry_snp[e];
    const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
    sh.entry(m, s, x);
    // am: DERIV ? (a_i, a_i', a_i'') at i, NE + i, 2 NE + i : a_i of share c at c * NE + i
    double gls[9], am[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) am[i] = (DERIV && i >= NE) ? 0.0 : 1.0;
    const double inv = fmx_nine_walk(reads, r0, r1, lut, gls, [&](uint32_t al, double mat, double e4, double inv_t) {
      // (a 1 the compiler cannot see through: 1 - p stays in the read loop instead of 3 NE more doubles held across it;
      // the same operations)
      double one = 1.0;
      asm volatile("" : "+v"(one));
      if (DERIV) {
        const double sm = (al == 0) ? -mat : mat;
        ambient_fit::product_rule<NE>(am, [&](int i, double& fac, double& v) {
          const double xi = (al == 0) ? one - sh.p[i] : sh.p[i];
          fac = (mat * xi + e4);
          v = sm * sh.slope(i);
        });
      } else {
#pragma unroll
        for (int i = 0; i < NM; ++i) {
          const double xi = (al == 0) ? one - sh.p[i] : sh.p[i];
          am[i] *= (mat * xi + e4);
        }
      }
#pragma unroll
      for (int i = 0; i < NM; ++i) am[i] *= inv_t;
    });
    const typename Model::weights w(m, s, gls, inv);
    if (DERIV) {
#pragma unroll
      for (int i = 0; i < NE; ++i)
        if (am[i] < kMinNormGL) am[i] = kMinNormGL, am[NE + i] = 0.0, am[2 * NE + i] = 0.0;  // (the floored piece is constant)
      const double D1 = w.dD(&am[NE], inv), D2 = w.dD(&am[2 * NE], inv);
      ambient_fit::add_entry(w.D(&am[0], inv), D1, D2, s0, s1, s2);
    } else {
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const bool f0 = am[i] < kMinNormGL, f1 = am[NE + i] < kMinNormGL, f2 = am[2 * NE + i] < kMinNormGL;
        cr = cr || f0 != f1 || f1 != f2;
      }
#pragma unroll
      for (int i = 0; i < NM; ++i)
        if (am[i] < kMinNormGL) am[i] = kMinNormGL;
      s0 += pos_log(w.D(&am[0], inv), 0.0);
      s1 += pos_log(w.D(&am[NE], inv), 0.0);
      s2 += pos_log(w.D(&am[2 * NE], inv), 0.0);
    }
  }
  out[0] = ambient_fit::wave_sum(s0);
  out[1] = ambient_fit::wave_sum(s1);
  out[2] = ambient_fit::wave_sum(s2);
  if (crosses) *crosses = __any(cr) != 0;
}

// The body of a kernel (ambient_fit::frame): dout [ROWS][n_units] x_hat, ll_hat, ll_zero, info and, with five rows,
// ll_top; iout [2][n_units] status, n_steps.  af: the model's, or NULL.
template <class Model>
__device__ __forceinline__ void fmx_fit_frame(int64_t n_units, int n_cand, const int32_t* __restrict__ slot, double x_max,
                                              const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                                              const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                                              const double* __restrict__ lut_g, const double* __restrict__ af,
                                              const double* __restrict__ cgp, int K, double* __restrict__ dout,
                                              int32_t* __restrict__ iout) {
  ambient_fit::frame<256, Model::WIDTH, Model::ROWS>(
      n_units, n_cand, slot, cell_ptr, lut_g, dout, iout,
      [&](const double* lut, int lane, int64_t e0, int64_t e1, int32_t j, int32_t k) {
        const Model m(af, cgp, K, j, k);
        double ll_top = 0.0;  // (its own variable: the coarse callable writes it while the search runs)
        auto coarse = [&](const double (&x)[3], double (&o)[3], bool& crosses) {
          fmx_fit_pass<Model, false>(m, e0, e1, lane, entry_snp, entry_rptr, reads, lut, x, o, &crosses);
          // (kept in scalar registers across the passes that follow)
          if (Model::ROWS > 4) ambient_fit::keep_top<3>(x, o, x_max, ll_top), ll_top = ambient_fit::uniform(ll_top);
        };
        auto deriv = [&](double x, double& L, double& d1, double& d2) {
          const double xs[3] = {x, 0.0, 0.0};
          double o[3];
          fmx_fit_pass<Model, true>(m, e0, e1, lane, entry_snp, entry_rptr, reads, lut, xs, o, nullptr);
          L = o[0], d1 = o[1], d2 = o[2];
        };
        // (a droplet without entries: every coarse LL is 0, the first derivative pass finds nothing, status 5)
        ambient_fit::result res = ambient_fit::search_piecewise(x_max, coarse, deriv, [&] { return e0 == e1; });
        if (Model::ROWS > 4) res.ll_top = ambient_fit::top_of(res, ll_top);
        return res;
      });
}

// The host side of the two calls on one device: fmx_refusal.hpp's rule, the call's own rule for its arguments
// (bad(why, n), fit_args.hpp), then ambient_fit::host_run around the call's kernel.  amb_af: the model's, or NULL.
template <class Model, class Kernel, class Bad>
int fmx_fit_call(muxgl_handle* h, const char* who, const double* amb_af, int32_t n_cand, const int32_t* slot, double x_max,
                 const ambient_fit::outputs& out, float* kernel_ms, Kernel* kernel, Bad&& bad) {
  HIPCHK(h, hipSetDevice(h->device));
  if (fmx_refuse(h, h, who, "the fit belongs")) return 1;
  char why[256];
  if (bad(why, sizeof(why))) MUXGL_FAIL(h, "%s", why);
  if (h->C == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing, no timing slot: records, timings and every other state of the handle keep their values)
  return ambient_fit::host_run(h, who, amb_af, n_cand, Model::WIDTH, slot, Model::ROWS, out, kernel_ms,
                               [&](int64_t n_units, const double* d_af, const int32_t* d_slot, double* d_dout, int32_t* d_iout) {
                                 return ambient_fit::launch(h, kernel, n_units, (int)n_cand, d_slot, x_max, h->d_cell_ptr,
                                                            h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, d_af,
                                                            h->d_cgp, h->K, d_dout, d_iout);
                               });
}
