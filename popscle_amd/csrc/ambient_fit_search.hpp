// ambient_fit_search.hpp -- what the per-droplet fits share: muxgl_demux_ambient_fit (demux_ambient_fit.hip),
// muxgl_fmx_ambient_fit (fmx_ambient_fit.hip), muxgl_demux_alpha_fit (demux_alpha_fit.hip) and
// muxgl_fmx_alpha_fit (fmx_alpha_fit.hip), where rho reads alpha: the search, the pieces of a pass that do not
// depend on the model, the ll_top rule, the kernel's frame with the store of a result, and the host side of the call (its
// argument rules: fit_args.hpp).  The search: one wave maximises LL(rho) on [0, rho_max] for one (droplet, candidate).  The model
// is the caller's: two callables that return, in every lane the same bits,
//   coarse(x[3], o[3])   o[k] = LL(x[k]) for k < NC
//   deriv(x, L, d1, d2)  (LL, LL', LL'') at x
// so every decision below is wave-uniform.  The rules:
//   * LL on the nine coarse points i rho_max / 8, NC per pass; the best point, ties to the lowest index; the bracket is its
//     two neighbours, clipped to [0, rho_max];
//   * (LL, LL', LL'') at the best point x.  LL'(x) <= 0 at x = 0 is the lower bound (status 1), LL'(x) >= 0 at x = rho_max the
//     upper (status 2); otherwise the sign of LL'(x) keeps the half of the bracket that holds the maximum;
//   * safeguarded Newton on LL': x - LL' / LL'' when LL'' < 0 and the point lies strictly inside the bracket, the
//     bracket's midpoint otherwise; the bracket shrinks by the sign of LL' after every evaluation.  It stops (status 0)
//     when LL' is 0 or so small that the Newton step no longer moves x, after a Newton step <= 1e-9, or when the bracket or
//     a bisection step is <= 1e-9 and no Newton step is possible from there: where one is, it is taken first (it stays
//     inside the bracket, so it is <= 1e-9 too), which leaves LL' at rounding level, not at up to 1e-9 info.  After 48
//     steps it gives up (status 3) and returns the best point evaluated, by LL.  n_steps counts the evaluations after the
//     one at the coarse best point.
// Only the sign of LL' narrows the bracket, so an LL' that jumps upward inside it (a floored element of the freemuxlet
// model) cannot trap the search: from LL'(a) > 0 > LL'(b) it closes on a zero that LL' crosses downward.
#pragma once
#include <cmath>

#include "common.hpp"

namespace ambient_fit {

constexpr int MAX_STEPS = 48;
constexpr double STOP = 1e-9;

enum : int32_t {
  INTERIOR = 0,
  LOWER = 1,
  UPPER = 2,
  STEP_CAP = 3,
  SKIPPED = 4,    // cand == -1
  NO_ENTRY = 5,   // no scored entry
  NOT_FINITE = 6  // LL at a coarse point is not finite (freemuxlet: a posterior row of exactly 0)
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// v, of which every lane holds the same bits, as a value the compiler knows to be wave-uniform: it may then live in scalar
// registers across a pass instead of taking two vector registers of every lane.  Changes no bit.
__device__ __forceinline__ double uniform(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

struct result {
  double rho_hat = 0.0, ll_hat = 0.0, ll_zero = 0.0, info = 0.0;
  double ll_top = 0.0;  // LL at the upper bound: the caller's, for a call with five double rows (muxgl_demux_alpha_fit)
  int32_t status = SKIPPED, steps = 0;
};

// ---- what the passes of the fits share ----
// The product rule along the reads for NE elements, am = (a[NE], a'[NE], a''[NE]): tv(i, t, v) gives element i's factor t
// of this read and its slope v; a'' = a'' t + 2 a' v; a' = a' t + a v; a = a t, in this order.
template <int NE, class TV>
__device__ __forceinline__ void product_rule(double* am, TV&& tv) {
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    double t, v;
    tv(i, t, v);
    am[2 * NE + i] = fma(am[2 * NE + i], t, (am[NE + i] + am[NE + i]) * v);
    am[NE + i] = fma(am[NE + i], t, am[i] * v);
    am[i] *= t;
  }
}

// an entry's (D, D', D'') added to the lane's (LL, LL', LL''): log D, D' / D, D'' / D - (D' / D)^2
__device__ __forceinline__ void add_entry(double D, double D1, double D2, double& s0, double& s1, double& s2) {
  const double iD = 1.0 / D;
  const double q1 = D1 * iD;
  s0 += pos_log(D, 0.0);
  s1 += q1;
  s2 += fma(-q1, q1, D2 * iD);
}

// the end of a pass: the lanes' sums added over the wave, the N that the pass formed (the others are 0), and the lanes'
// counts of scored entries where the caller asks for them
template <int N>
__device__ __forceinline__ void pass_sums(double s0, double s1, double s2, int ns, double (&out)[3], int* n_scored) {
  out[0] = wave_sum(s0);
  out[1] = N > 1 ? wave_sum(s1) : 0.0;
  out[2] = N > 2 ? wave_sum(s2) : 0.0;
  if (n_scored) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ns += __shfl_xor(ns, off, 64);
    *n_scored = ns;
  }
}

// NC: coarse points per pass (1 or 3).  FINITE: end with NOT_FINITE when LL at a coarse point is not finite (rho_hat = 0,
// ll_hat = ll_zero = -inf, info = 0, no step).  empty(): after the first derivative pass, whether the droplet has no scored
// entry (NO_ENTRY: all outputs 0).  UNIFORM_STATE (newton): the doubles the search carries across a derivative pass go
// through uniform() before it (fam_fit_kernel needs the sixteen vector registers to stay within 128; amb_fit_kernel keeps
// the code it had).
__device__ __forceinline__ result not_finite() {
  result res;
  res.ll_hat = -__builtin_huge_val();
  res.ll_zero = -__builtin_huge_val();
  res.status = NOT_FINITE;
  return res;
}

// The second half of the search: from the bracket [a, b] around the best point x (at_lo: x is 0 and the best point is the
// bracket's lower end; at_hi likewise with rho_max), the bound tests and the safeguarded Newton iteration.
template <bool UNIFORM_STATE, class Deriv, class Empty>
__device__ __forceinline__ result newton(double a, double x, double b, bool at_lo, bool at_hi, double ll_zero, Deriv&& deriv,
                                         Empty&& empty) {
  result res;
  int32_t status, steps = 0;
  double L = 0.0, d1 = 0.0, d2 = 0.0;
  // the best point evaluated, by LL: what a fit that runs into the step cap returns
  double xb = x, Lb = 0.0, d2b = 0.0;
  double step = 1.0;
  bool newton = false;  // the last move was a Newton step
  status = STEP_CAP;
  for (bool first = true;; first = false) {  // (one evaluation site: the pass is inlined once)
    if (UNIFORM_STATE) {  // what the search carries across the pass
      a = uniform(a), b = uniform(b), x = uniform(x), xb = uniform(xb), Lb = uniform(Lb), d2b = uniform(d2b);
      step = uniform(step), ll_zero = uniform(ll_zero);
    }
    deriv(x, L, d1, d2);
    if (first || L > Lb) xb = x, Lb = L, d2b = d2;
    if (first) {
      if (empty()) status = NO_ENTRY;
      else if (at_lo && d1 <= 0.0) status = LOWER;
      else if (at_hi && d1 >= 0.0) status = UPPER;
      if (status != STEP_CAP) break;
    } else {
      ++steps;
    }
    if (d1 > 0.0) a = x; else if (d1 < 0.0) b = x;
    if (d1 == 0.0 || (newton && step <= STOP)) {  // a Newton step within the stop: x is converged quadratically
      status = INTERIOR;
      break;
    }
    if (steps == MAX_STEPS) break;
    double xn = x - d1 / d2;
    if (d2 < 0.0 && xn == x) {  // LL' is at rounding level: the Newton step no longer moves x
      status = INTERIOR;
      break;
    }
    newton = d2 < 0.0 && xn > a && xn < b;
    if (!newton) {
      // the bracket, or the bisection step that led here, is within the stop.  (Where a Newton step is possible it was
      // taken above: it lies inside the bracket, so it is within the stop too, and the fit ends after it with LL' at
      // rounding level instead of up to 1e-9 info.)
      if (b - a <= STOP || (!first && step <= STOP)) {
        status = INTERIOR;
        break;
      }
      xn = 0.5 * (a + b);
    }
    step = fabs(xn - x);
    x = xn;
  }
  if (status == STEP_CAP) x = xb, L = Lb, d2 = d2b;
  if (status == NO_ENTRY) ll_zero = 0.0;
  if (status != NO_ENTRY) res.rho_hat = x, res.ll_hat = L, res.info = -d2;
  res.ll_zero = ll_zero;
  res.status = status, res.steps = steps;
  return res;
}

template <int NC, bool FINITE, class Coarse, class Deriv, class Empty>
__device__ __forceinline__ result search(double rho_max, Coarse&& coarse, Deriv&& deriv, Empty&& empty) {
  double ll_zero = 0.0;
  // the nine coarse points i * rho_max / 8 (the division by 8 is exact: point 8 is rho_max bit for bit)
  double best_ll = 0.0;
  int best = 0;
  bool finite = true;
  for (int i0 = 0; i0 < 9; i0 += NC) {
    const double xs[3] = {(double)i0 * rho_max / 8.0, (double)(i0 + 1) * rho_max / 8.0, (double)(i0 + 2) * rho_max / 8.0};
    double o[3];
    coarse(xs, o);
    if (i0 == 0) ll_zero = o[0];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (FINITE) finite = finite && (o[k] - o[k] == 0.0);
      if ((i0 == 0 && k == 0) || o[k] > best_ll) best_ll = o[k], best = i0 + k;  // (ties to the lowest index)
    }
  }
  if (FINITE && !finite) return not_finite();
  double a = (double)(best > 0 ? best - 1 : 0) * rho_max / 8.0;
  double b = (double)(best < 8 ? best + 1 : 8) * rho_max / 8.0;
  double x = (double)best * rho_max / 8.0;
  return newton<false>(a, x, b, best == 0, best == 8, ll_zero, deriv, empty);
}

// The search for a model whose LL is piecewise: freemuxlet's 1e-6 floor.  LL' jumps upward where an element
// leaves or reaches the floor, so LL can rise a second time inside the bracket and the rules above would then end on the
// local maximum next to the best coarse point.  coarse(x[3], o[3], crosses) also says whether any element is below the
// floor at one of its three points and not at another.  After the nine coarse points one more pass takes the bracket's
// three points (lo, best, hi): where no element crosses the floor between them LL is smooth there and the search goes
// on as above.  Where one does, LL is taken on the 65 points lo + (hi - lo) i / 64; the best of them (ties to the lowest
// index) with its two neighbours is the bracket, and the bound tests and the Newton iteration run from there.  An element
// is a product of positive linear factors, so it is above the floor on an interval: one that is above it at lo and at hi
// is above it in between.  Every pass goes through one call site (the pass is inlined once); every decision is
// wave-uniform.
template <class Coarse, class Deriv, class Empty>
__device__ __forceinline__ result search_piecewise(double rho_max, Coarse&& coarse, Deriv&& deriv, Empty&& empty) {
  constexpr int FINE = 64, T_BRACKET = 3, T_FINE = 4, T_END = T_FINE + (FINE + 3) / 3;
  double ll_zero = 0.0, best_ll = 0.0, lo = 0.0, hi = 0.0, mid = 0.0;
  int best = 0;
  bool finite = true, fine = false;
  for (int t = 0; t < T_END; ++t) {
    ll_zero = uniform(ll_zero), best_ll = uniform(best_ll), lo = uniform(lo), hi = uniform(hi), mid = uniform(mid);
    best = __builtin_amdgcn_readfirstlane(best);
    finite = __builtin_amdgcn_readfirstlane((int)finite) != 0;
    if (t == T_BRACKET) {
      if (!finite) return not_finite();
      lo = (double)(best > 0 ? best - 1 : 0) * rho_max / 8.0;
      hi = (double)(best < 8 ? best + 1 : 8) * rho_max / 8.0;
      mid = (double)best * rho_max / 8.0;
    }
    double xs[3], o[3];
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      idx[k] = (t < T_BRACKET ? t : t - T_FINE) * 3 + k;
      if (t < T_BRACKET) xs[k] = (double)idx[k] * rho_max / 8.0;  // (the division by 8 is exact: point 8 is rho_max bit for bit)
      else if (t == T_BRACKET) xs[k] = k == 0 ? lo : k == 1 ? mid : hi;
      else xs[k] = idx[k] >= FINE ? hi : lo + (hi - lo) * (double)idx[k] / (double)FINE;
    }
    bool crosses = false;
    coarse(xs, o, crosses);
    if (t == T_BRACKET) {
      if (!crosses) break;
      fine = true;
      continue;
    }
    if (t == 0) ll_zero = o[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (t < T_BRACKET) finite = finite && (o[k] - o[k] == 0.0);
      if (idx[k] > FINE) continue;  // (the last fine pass repeats hi)
      if (idx[k] == 0 || o[k] > best_ll) best_ll = o[k], best = idx[k];  // (ties to the lowest index)
    }
  }
  if (!fine) return newton<true>(lo, mid, hi, best == 0, best == 8, ll_zero, deriv, empty);
  auto pt = [&](int i) { return i >= FINE ? hi : lo + (hi - lo) * (double)i / (double)FINE; };
  const double x = pt(best);
  return newton<true>(pt(best > 0 ? best - 1 : 0), x, pt(best < FINE ? best + 1 : FINE), best == 0 && x == 0.0,
                      best == FINE && x == rho_max, ll_zero, deriv, empty);
}

// lane 0 of the wave of `unit` writes its row: dout [ROWS][n_units] rho_hat, ll_hat, ll_zero, info and, with five rows,
// ll_top; iout [2][n_units] status, n_steps
template <int ROWS = 4>
__device__ __forceinline__ void store(const result& r, int lane, int64_t unit, int64_t n_units, double* __restrict__ dout,
                                      int32_t* __restrict__ iout) {
  if (lane == 0) {
    dout[unit] = r.rho_hat;
    dout[n_units + unit] = r.ll_hat;
    dout[2 * n_units + unit] = r.ll_zero;
    dout[3 * n_units + unit] = r.info;
    if (ROWS > 4) dout[4 * n_units + unit] = r.ll_top;
    iout[unit] = r.status;
    iout[n_units + unit] = r.steps;
  }
}

// ---- ll_top, LL at the upper bound: the fifth double row of the two mixing-share fits ----
// Coarse point 8 is x_max bit for bit, the last of the NC shares of the coarse pass that ends on it, and the coarse
// callable keeps its LL while the search runs.  (A later pass that ends on x_max, the bracket's or the scan's of
// search_piecewise, goes through the same inlined text and writes the same bits again.)  A coarse pass and a derivative
// pass form a and D by the same operations, so ll_hat on a bound is ll_zero resp. ll_top bit for bit.
template <int NC>
__device__ __forceinline__ void keep_top(const double (&x)[3], const double (&o)[3], double x_max, double& ll_top) {
  if (x[NC - 1] == x_max) ll_top = o[NC - 1];
}

// what the call reports: 0 for a droplet without a scored entry, as every output; ll_zero (-inf) where LL is not finite
__device__ __forceinline__ double top_of(const result& res, double ll_top) {
  return res.status == NO_ENTRY ? 0.0 : res.status == NOT_FINITE ? res.ll_zero : ll_top;
}

// ---- the kernel frame of the four fits ----
// grid: ceil(C * n_cand / 4) workgroups of four waves of one launch; wave unit <-> (cell, slot), the slot fastest, so the
// waves of a workgroup walk the same entries.  A slot is WIDTH indices (a candidate, or a pair); one that is negative skips
// the unit (status 4, all outputs 0).  The Phred table, LUT doubles, goes to LDS; fit(lut, lane, e0, e1, j, k) is the
// model's search over the cell's entries [e0, e1) and returns in every lane the same result, of which lane 0 stores ROWS
// double rows.  Every reduction tree under `fit` is fixed by the cell alone (lane = entry index modulo 64, then
// wave_sum's butterfly), there is no atomic and nothing depends on the batch, the device or the other slots: the outputs
// are bit-identical from call to call, for any order, grouping or repetition of the slots, on one device, on a group and
// through the sharded driver.
template <int LUT, int WIDTH, int ROWS, class Fit>
__device__ __forceinline__ void frame(int64_t n_units, int n_cand, const int32_t* __restrict__ slot,
                                      const int64_t* __restrict__ cell_ptr, const double* __restrict__ lut_g,
                                      double* __restrict__ dout, int32_t* __restrict__ iout, Fit&& fit) {
  __shared__ double lut[LUT];
  for (int i = threadIdx.x; i < LUT; i += 256) lut[i] = lut_g[i];
  __syncthreads();
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int lane = threadIdx.x & 63;
  const int64_t c = unit / n_cand;
  const int32_t j = slot[WIDTH * unit], k = slot[WIDTH * unit + WIDTH - 1];
  result res;
  if (j >= 0 && k >= 0) res = fit(lut, lane, cell_ptr[c], cell_ptr[c + 1], j, k);
  store<ROWS>(res, lane, unit, n_units, dout, iout);
}

// ---- the host side of a fit call ----
struct outputs {  // each host [C][n_cand] or NULL; ll_top: the calls with five double rows only
  double *rho_hat, *ll_hat, *ll_zero, *info;
  int32_t *status, *n_steps;
  double* ll_top = nullptr;
  bool any() const { return rho_hat || ll_hat || ll_zero || info || ll_top || status || n_steps; }
};

// amb_af (NULL: the call has none, and nothing is copied) and the slots' indices (`width` per slot: a candidate, or a pair)
// to the device, launch(n_units, d_af, d_slot, d_dout, d_iout) between the call's own events, the wanted ones of the `rows`
// (4, or 5 with ll_top) double rows and the two int rows to the host.  Nothing proportional to nnz is allocated; the
// handle's timing slots keep their values.
template <class Launch>
int host_run(muxgl_handle* h, const char* who, const double* amb_af, int n_cand, int width, const int32_t* slot, int rows,
             const outputs& o, float* kernel_ms, Launch&& launch) {
  const int64_t C = h->C, S = h->S, n_units = C * n_cand;
  if (n_units == 0) return 0;
  if ((n_units + 3) / 4 > 0x7fffffffLL)
    MUXGL_FAIL(h, "%s: %lld droplets x %d %s exceed one launch", who, (long long)C, n_cand, width == 2 ? "slots" : "candidates");
  dev_tmp<double> d_af, d_dout;
  dev_tmp<int32_t> d_slot, d_iout;
  if (amb_af && dev_alloc(h, &d_af.p, (size_t)S)) return 1;
  if (dev_alloc(h, &d_slot.p, (size_t)n_units * width)) return 1;
  if (dev_alloc(h, &d_dout.p, (size_t)n_units * rows)) return 1;
  if (dev_alloc(h, &d_iout.p, (size_t)n_units * 2)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, who)) return 1;
  if (amb_af && S > 0) HIPCHK(h, hipMemcpyAsync(d_af.p, amb_af, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_slot.p, slot, sizeof(int32_t) * (size_t)n_units * width, hipMemcpyHostToDevice, h->stream));
  if (ev.start(h)) return 1;
  if (launch(n_units, d_af.p, d_slot.p, d_dout.p, d_iout.p)) return 1;
  if (ev.stop(h)) return 1;
  double* const dst[5] = {o.rho_hat, o.ll_hat, o.ll_zero, o.info, o.ll_top};
  for (int k = 0; k < rows; ++k)
    if (dst[k])
      HIPCHK(h, hipMemcpyAsync(dst[k], d_dout.p + (size_t)k * n_units, sizeof(double) * (size_t)n_units, hipMemcpyDeviceToHost,
                               h->stream));
  int32_t* const idst[2] = {o.status, o.n_steps};
  for (int k = 0; k < 2; ++k)
    if (idst[k])
      HIPCHK(h, hipMemcpyAsync(idst[k], d_iout.p + (size_t)k * n_units, sizeof(int32_t) * (size_t)n_units, hipMemcpyDeviceToHost,
                               h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ev.add();
  return 0;
}

// a fit kernel on the frame's grid, on the handle's stream; its first argument is n_units
template <class... P, class... A>
int launch(muxgl_handle* h, void (*kernel)(int64_t, P...), int64_t n_units, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, args...);
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // namespace ambient_fit
