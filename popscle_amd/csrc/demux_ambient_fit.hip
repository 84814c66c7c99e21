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
// where v is exactly 0), the grid's NA x 9 products run beside the triples operation for operation as row_entry_pg forms
// them, so q_max_e is the same number, and all nine of (a, a', a'') are rescaled together every 32 reads by the grid's
// maximum only.
//
// amb_fit_kernel, one wave per (cell, candidate): the lanes stride the cell's entries, each lane walks its entry's read
// bytes through the Phred table in LDS, dots the three triples with the candidate's gp row and adds its share of
// (LL, LL', LL'') in entry order; a fixed xor butterfly adds the 64 shares (a + b commutes, so every lane holds the same
// bits and every decision below is wave-uniform).  The whole fit runs in this one launch:
//   * LL on the nine coarse points i rho_max / 8, three per pass (nine products per lane, as in a derivative pass); the best
//     point, ties to the lowest index; the bracket is its two neighbours, clipped to [0, rho_max];
//   * (LL, LL', LL'') at the best point x.  LL'(x) <= 0 at x = 0 is the lower bound (status 1), LL'(x) >= 0 at x = rho_max the
//     upper (status 2); otherwise the sign of LL'(x) keeps the half of the bracket that holds the maximum;
//   * safeguarded Newton on LL': x - LL' / LL'' when LL'' < 0 and the point lies strictly inside the bracket, the
//     bracket's midpoint otherwise; the bracket shrinks by the sign of LL' after every evaluation.  It stops (status 0)
//     when LL' is 0 or so small that the Newton step no longer moves x, after a Newton step <= 1e-9, or when the bracket or a bisection step is <= 1e-9 and no Newton step
//     is possible from there: where one is, it is taken first (it stays inside the bracket, so it is <= 1e-9 too), which
//     leaves LL' at rounding level, not at up to 1e-9 info.  After 48 steps it gives up (status 3) and returns the best
//     point evaluated, by LL.  n_steps counts the evaluations after the one at the coarse best point.
// Every reduction tree is fixed by the cell alone (lane = entry index modulo 64, then the butterfly), there is no atomic
// and nothing depends on the batch, the device or the other candidates: the outputs are bit-identical from call to call,
// for any budget, any order or grouping of the candidates, on one device, on a group and through the sharded driver.
//
// Memory: the inputs, cand and the six output arrays.  Nothing proportional to nnz is allocated, so no slab budget applies.
#include <cmath>
#include <vector>

#include "demux_entry.hpp"

namespace {

struct fit_grid {
  double a[MUXGL_MAX_ALPHA];
};

constexpr int FIT_MAX_STEPS = 48;
constexpr double FIT_STOP = 1e-9;

__device__ __forceinline__ double fit_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// One pass of a wave over the entries [e0, e1) of a cell for candidate column j.
//   DERIV = false: out[k] = LL(x[k]) for the NC <= 3 shares x[0..NC-1]
//   DERIV = true:  out = (LL, LL', LL'') at x[0]
// Returns in every lane the same bits.  n_scored (DERIV only): the entries whose marker has genotypes.
template <int NA, bool DERIV, int NC>
__device__ __forceinline__ void fit_pass(int64_t e0, int64_t e1, int lane, const int32_t* __restrict__ entry_snp,
                                         const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                                         const double* lut, const fit_grid& al, const double* __restrict__ af,
                                         const uint8_t* __restrict__ has_gp, const double* __restrict__ gpj, size_t V3,
                                         const double (&x)[3], double (&out)[3], int* n_scored) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int ns = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int32_t s = entry_snp[e];
    if (!has_gp[s]) continue;  // (no genotypes: the reference skips the marker, :733)
    ++ns;
    const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
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
    for (int i = 0; i < NA * 9; ++i) pG[i] = 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) am[i] = (DERIV && i >= 3) ? 0.0 : 1.0;
    int since_norm = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const uint32_t b = (uint32_t)reads[r];
      if (b == MUXGL_READ_OTHER) continue;  // :664
      const uint32_t alt = b >> 7, bq = b & 0x7f;
      const double e3 = lut[256 + bq], mt = lut[128 + bq];  // Err/3.0, Mat
      const double pR = (alt == 0) ? mt : e3;  // :666
      const double pA = (alt == 0) ? e3 : mt;  // :667
      const double d = pA - pR;
#pragma unroll
      for (int n = 0; n < NA; ++n) {  // the grid's products, operation for operation those of row_entry_pg
        double an = al.a[n];
        // (the widest grid: kept from being hoisted out of the read loop as 48 registers of ha, hb, 2 ha; same operations)
        if (NA > 12) asm volatile("" : "+v"(an));
        const double ha = 0.5 * an, hb = 0.5 - ha;
        const double A1 = fma(d, hb, pR);
        const double B1 = d * ha, B2 = d * (ha + ha);
        double* q = &pG[n * 9];
        q[0] *= pR;
        q[1] *= pR + B1;
        q[2] *= pR + B2;
        q[3] *= A1;
        q[4] *= A1 + B1;
        q[5] *= A1 + B2;
        q[6] *= pA - B2;
        q[7] *= pA - B1;
        q[8] *= pA;
      }
      if (DERIV) {
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          const double t = fma(pA, pv[l], pR * (1.0 - pv[l]));
          const double v = d * pv[3 + l];
          am[6 + l] = fma(am[6 + l], t, (am[3 + l] + am[3 + l]) * v);
          am[3 + l] = fma(am[3 + l], t, am[l] * v);
          am[l] *= t;
        }
      } else {
#pragma unroll
        for (int i = 0; i < NM; ++i) am[i] *= fma(pA, pv[i], pR * (1.0 - pv[i]));
      }
      if (++since_norm == 32) {  // the grid's maximum only: the triples follow it, all nine together
        since_norm = 0;
        double mx = 0.0;
#pragma unroll
        for (int i = 0; i < NA * 9; ++i) mx = fmax(mx, pG[i]);
        const double inv = 1.0 / mx;
#pragma unroll
        for (int i = 0; i < NA * 9; ++i) pG[i] *= inv;
#pragma unroll
        for (int i = 0; i < NM; ++i) am[i] *= inv;
      }
    }
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i < NA * 9; ++i) mx = fmax(mx, pG[i]);
    const double c = 1.0 / (1.0 + 1e-10);
    const double sc = c / mx, t10 = 1e-10 * c;
    const double* g = gpj + (size_t)s * V3;
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    if (DERIV) {
      const double D = fma(g2, fma(am[2], sc, t10), fma(g1, fma(am[1], sc, t10), g0 * fma(am[0], sc, t10)));
      const double D1 = fma(g2, am[5] * sc, fma(g1, am[4] * sc, g0 * (am[3] * sc)));  // (the offset's derivative is 0)
      const double D2 = fma(g2, am[8] * sc, fma(g1, am[7] * sc, g0 * (am[6] * sc)));
      const double iD = 1.0 / D;
      const double q1 = D1 * iD;
      s0 += pos_log(D, 0.0);
      s1 += q1;
      s2 += fma(-q1, q1, D2 * iD);
    } else {
      s0 += pos_log(fma(g2, fma(am[2], sc, t10), fma(g1, fma(am[1], sc, t10), g0 * fma(am[0], sc, t10))), 0.0);
      if (NC > 1) s1 += pos_log(fma(g2, fma(am[5], sc, t10), fma(g1, fma(am[4], sc, t10), g0 * fma(am[3], sc, t10))), 0.0);
      if (NC > 2) s2 += pos_log(fma(g2, fma(am[8], sc, t10), fma(g1, fma(am[7], sc, t10), g0 * fma(am[6], sc, t10))), 0.0);
    }
  }
  out[0] = fit_wave_sum(s0);
  out[1] = (DERIV || NC > 1) ? fit_wave_sum(s1) : 0.0;
  out[2] = (DERIV || NC > 2) ? fit_wave_sum(s2) : 0.0;
  if (n_scored) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ns += __shfl_xor(ns, off, 64);
    *n_scored = ns;
  }
}

// grid: ceil(C * n_cand / 4) workgroups of four waves; wave unit <-> (cell, candidate), the candidate fastest, so the
// waves of a workgroup walk the same entries.  dout: [4][n_units] rho_hat, ll_hat, ll_zero, info; iout: [2][n_units]
// status, n_steps
template <int NA>
__global__ void __launch_bounds__(256)
    amb_fit_kernel(int64_t n_units, int n_cand, const int32_t* __restrict__ cand, double rho_max,
                   const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                   const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                   const double* __restrict__ lut_g, fit_grid al, const double* __restrict__ af,
                   const uint8_t* __restrict__ has_gp, const double* __restrict__ gp, int V, double* __restrict__ dout,
                   int32_t* __restrict__ iout) {
  __shared__ double lut[384];
  for (int i = threadIdx.x; i < 384; i += 256) lut[i] = lut_g[i];
  __syncthreads();
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int lane = threadIdx.x & 63;
  const int64_t c = unit / n_cand;
  const int32_t j = cand[unit];
  double rho_hat = 0.0, ll_hat = 0.0, ll_zero = 0.0, info = 0.0;
  int32_t status = 4, steps = 0;
  if (j >= 0) {
    const int64_t e0 = cell_ptr[c], e1 = cell_ptr[c + 1];
    const size_t V3 = (size_t)V * 3;
    const double* gpj = gp + (size_t)j * 3;
    // shares per coarse pass: three (nine products per lane, as in a derivative pass); one at the widest grid, whose 144
    // products leave a lane no room for more.  Every sum belongs to one share, so the chunking changes no bit.
    constexpr int NC = NA > 12 ? 1 : 3;
    auto coarse = [&](const double (&x)[3], double (&o)[3]) {
      fit_pass<NA, false, NC>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, af, has_gp, gpj, V3, x, o, nullptr);
    };
    int n_scored = 0;
    double L = 0.0, d1 = 0.0, d2 = 0.0;
    auto deriv = [&](double x) {
      const double xs[3] = {x, 0.0, 0.0};
      double o[3];
      fit_pass<NA, true, 1>(e0, e1, lane, entry_snp, entry_rptr, reads, lut, al, af, has_gp, gpj, V3, xs, o, &n_scored);
      L = o[0], d1 = o[1], d2 = o[2];
    };
    // the nine coarse points i * rho_max / 8 (the division by 8 is exact: point 8 is rho_max bit for bit)
    double best_ll = 0.0;
    int best = 0;
    for (int i0 = 0; i0 < 9; i0 += NC) {
      const double xs[3] = {(double)i0 * rho_max / 8.0, (double)(i0 + 1) * rho_max / 8.0, (double)(i0 + 2) * rho_max / 8.0};
      double o[3];
      coarse(xs, o);
      if (i0 == 0) ll_zero = o[0];
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if ((i0 == 0 && k == 0) || o[k] > best_ll) best_ll = o[k], best = i0 + k;  // (ties to the lowest index)
    }
    double a = (double)(best > 0 ? best - 1 : 0) * rho_max / 8.0;
    double b = (double)(best < 8 ? best + 1 : 8) * rho_max / 8.0;
    double x = (double)best * rho_max / 8.0;
    // the best point evaluated, by LL: what a fit that runs into the step cap returns
    double xb = x, Lb = 0.0, d2b = 0.0;
    double step = 1.0;
    bool newton = false;  // the last move was a Newton step
    status = 3;
    for (bool first = true;; first = false) {  // (one evaluation site: the pass is inlined once)
      deriv(x);
      if (first || L > Lb) xb = x, Lb = L, d2b = d2;
      if (first) {
        if (n_scored == 0) status = 5;
        else if (best == 0 && d1 <= 0.0) status = 1;
        else if (best == 8 && d1 >= 0.0) status = 2;
        if (status != 3) break;
      } else {
        ++steps;
      }
      if (d1 > 0.0) a = x; else if (d1 < 0.0) b = x;
      if (d1 == 0.0 || (newton && step <= FIT_STOP)) {  // a Newton step within the stop: x is converged quadratically
        status = 0;
        break;
      }
      if (steps == FIT_MAX_STEPS) break;
      double xn = x - d1 / d2;
      if (d2 < 0.0 && xn == x) {  // LL' is at rounding level: the Newton step no longer moves x
        status = 0;
        break;
      }
      newton = d2 < 0.0 && xn > a && xn < b;
      if (!newton) {
        // the bracket, or the bisection step that led here, is within the stop.  (Where a Newton step is possible it was
        // taken above: it lies inside the bracket, so it is within the stop too, and the fit ends after it with LL' at
        // rounding level instead of up to 1e-9 info.)
        if (b - a <= FIT_STOP || (!first && step <= FIT_STOP)) {
          status = 0;
          break;
        }
        xn = 0.5 * (a + b);
      }
      step = fabs(xn - x);
      x = xn;
    }
    if (status == 3) x = xb, L = Lb, d2 = d2b;
    if (status == 5) ll_zero = 0.0;
    if (status != 5) rho_hat = x, ll_hat = L, info = -d2;
  }
  if (lane == 0) {
    dout[unit] = rho_hat;
    dout[n_units + unit] = ll_hat;
    dout[2 * n_units + unit] = ll_zero;
    dout[3 * n_units + unit] = info;
    iout[unit] = status;
    iout[n_units + unit] = steps;
  }
}

template <int NA>
int launch_fit(muxgl_handle* h, int64_t n_units, int n_cand, const int32_t* d_cand, double rho_max, const fit_grid& al,
               const double* d_af, double* d_dout, int32_t* d_iout) {
  hipLaunchKernelGGL((amb_fit_kernel<NA>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, n_cand,
                     d_cand, rho_max, h->d_cell_ptr, h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, al, d_af,
                     h->d_has_gp, h->d_gp, h->V, d_dout, d_iout);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int fit_dispatch(muxgl_handle* h, int A, int64_t n_units, int n_cand, const int32_t* d_cand, double rho_max,
                 const fit_grid& al, const double* d_af, double* d_dout, int32_t* d_iout) {
#define CALL_F(N) launch_fit<N>(h, n_units, n_cand, d_cand, rho_max, al, d_af, d_dout, d_iout)
  DISPATCH_NA(A, CALL_F);
#undef CALL_F
}

}  // namespace

int demux_ambient_fit_bad_args(const double* amb_af, int32_t n_cand, const int32_t* cand,
                               int64_t C, int V, double rho_max, bool any_out, char* why, size_t n) {
  const char* who = "muxgl_demux_ambient_fit";
  if (!any_out) return snprintf(why, n, "%s: every output is NULL", who), 1;
  if (n_cand < 1 || n_cand > MUXGL_MAX_FIT_CAND)
    return snprintf(why, n, "%s: n_cand=%d outside [1,%d]", who, n_cand, MUXGL_MAX_FIT_CAND), 1;
  if (!cand || !amb_af) return snprintf(why, n, "%s: %s is NULL", who, cand ? "amb_af" : "cand"), 1;
  if (!(std::isfinite(rho_max) && rho_max > 0.0 && rho_max <= 1.0))
    return snprintf(why, n, "%s: rho_max (%g) is not a finite number in (0, 1]", who, rho_max), 1;
  for (int64_t i = 0; i < C * n_cand; ++i)
    if (cand[i] < -1 || cand[i] >= V)
      return snprintf(why, n, "%s: cand[%lld][%d] (%d) is neither -1 nor a sample in [0,%d)", who, (long long)(i / n_cand),
                      (int)(i % n_cand), cand[i], V), 1;
  return 0;
}

int demux_ambient_fit_run(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int n_cand,
                          const int32_t* cand, double rho_max, double* rho_hat, double* ll_hat, double* ll_zero,
                          double* info, int32_t* status, int32_t* n_steps, float* kernel_ms) {
  if (demux_ambient_check_af(h, amb_af, "muxgl_demux_ambient_fit")) return 1;
  const int64_t C = h->C, S = h->S, n_units = C * n_cand;
  if (n_units == 0) return 0;
  if ((n_units + 3) / 4 > 0x7fffffffLL)
    MUXGL_FAIL(h, "muxgl_demux_ambient_fit: %lld droplets x %d candidates exceed one launch", (long long)C, n_cand);
  const int A = p->n_alpha;
  fit_grid al;
  for (int i = 0; i < MUXGL_MAX_ALPHA; ++i) al.a[i] = i < A ? p->alpha[i] : p->alpha[0];  // (repeats of alpha[0] change no maximum)

  dev_tmp<double> d_af, d_dout;
  dev_tmp<int32_t> d_cand, d_iout;
  if (dev_alloc(h, &d_af.p, (size_t)S)) return 1;
  if (dev_alloc(h, &d_cand.p, (size_t)n_units)) return 1;
  if (dev_alloc(h, &d_dout.p, (size_t)n_units * 4)) return 1;
  if (dev_alloc(h, &d_iout.p, (size_t)n_units * 2)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, "muxgl_demux_ambient_fit")) return 1;
  if (S > 0) HIPCHK(h, hipMemcpyAsync(d_af.p, amb_af, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_cand.p, cand, sizeof(int32_t) * (size_t)n_units, hipMemcpyHostToDevice, h->stream));
  if (ev.start(h)) return 1;
  if (fit_dispatch(h, A, n_units, n_cand, d_cand.p, rho_max, al, d_af.p, d_dout.p, d_iout.p)) return 1;
  if (ev.stop(h)) return 1;
  double* const dst[4] = {rho_hat, ll_hat, ll_zero, info};
  for (int k = 0; k < 4; ++k)
    if (dst[k])
      HIPCHK(h, hipMemcpyAsync(dst[k], d_dout.p + (size_t)k * n_units, sizeof(double) * (size_t)n_units, hipMemcpyDeviceToHost,
                               h->stream));
  int32_t* const idst[2] = {status, n_steps};
  for (int k = 0; k < 2; ++k)
    if (idst[k])
      HIPCHK(h, hipMemcpyAsync(idst[k], d_iout.p + (size_t)k * n_units, sizeof(int32_t) * (size_t)n_units, hipMemcpyDeviceToHost,
                               h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ev.add();
  return 0;
}
