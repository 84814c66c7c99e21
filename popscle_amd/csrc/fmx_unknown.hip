// fmx_unknown.hip -- muxgl_fmx_unknown: every droplet scored against a donor that no cluster holds.  A cluster without
// cells has a pileup of ones and its posterior row at a marker is the Hardy-Weinberg triple gp0s of
// cmd_cram_freemux2.cpp:388-390; the reference run with K + 2 clusters, two of them empty, holds these numbers in its
// llks[] triangle.  With g = egl_e[9] the entry likelihoods of muxgl_fmx_prepare (d_egls), q the cluster posteriors the
// last E-step read (d_cgp, [S][K][3], geno_error mixed in) and u[s] the unknown donor's genotype prior at marker s (gp0s,
// or the caller's row), over the entries e of droplet c:
//
//   ll_ju[c][j] = sum_e log( sum_g1 sum_g2 g[3 g1 + g2] u[s_e][g1] q[s_e][j][g2] )     slot (K, j),     :440-446
//   ll_u[c]     = sum_e log( sum_g g[4 g] u[s_e][g] )                                  slot (K, K),     :448-452
//   ll_uu[c]    = sum_e log( sum_g1 sum_g2 g[3 g1 + g2] u[s_e][g1] u[s_e][g2] )        slot (K + 1, K)
//
// The design is demux_unknown.hip's with one alpha and one orientation, on fmx_singlets.hip's state rules:
//   * fun_prior_kernel, lane = marker: u from af with the expressions of :388-390, every product rounded on its own
//     (nothing to contract), so the caller's Hardy-Weinberg rows formed the same way give the same bits.
//   * fun_weight_kernel, lane = entry: w[g2] = sum_g1 u[g1] g[3 g1 + g2], g1 ascending, and the entry's two scalars
//     f_u = sum_g g[4 g] u[g] and f_uu = sum_g2 w[g2] u[g2]: [entries of the batch][5], 40 bytes per entry.
//   * fun_sweep_kernel, lane = cluster: f = w[0] q[0] + w[1] q[1] + w[2] q[2] per (entry, cluster), three FMAs in this
//     order, multiplied into a product kept as mantissa x 2^exponent (prodacc), one log per (cell part, cluster).  A wave
//     is one work unit: a part of a cell x a block of 64 clusters, the entry wave-uniform.  Below 64 clusters a wave
//     holds G = 64 / KH entries side by side (KH = K rounded up to a power of two) and the G partial products of a
//     cluster are multiplied in fsg_sweep_kernel's fixed xor butterfly.
//   * fun_scalar_kernel: the two per-cell scalars, a wave per cell part, 64 entries side by side, the same butterfly.
//   * table_join_kernel (table_call.hpp): the logs of the parts of a long cell, added in entry order, over the K + 2
//     columns of a slab row (the clusters, then u, then uu).
//   * fun_split_kernel: the cells' rows into the three tables of the caller's layout.
// Which cell goes into which batch, its cut into parts (the equal parts of the wave plan, as muxgl_fmx_singlets cuts a
// cell) and the order of the work items are table_plan.hpp's; the host body that drives the plan is table_call.hpp's
// table_batches, whose customer this unit is.  The cut of a cell depends on the cell alone and every
// reduction tree is fixed: the tables are bit-identical from call to call, for any budget, for any subset of outputs,
// on one device, on a group and through the sharded driver.
//
// Memory: nothing proportional to nnz is held for the whole pileup beyond what the handle already has.  Cells are swept
// in batches of whole cells whose weights, slab rows and table rows (table_plan::fmx_unknown_bytes) fit the streamed
// E-step's budget (4 GiB or a third of the device, MUXGL_FMX_SLAB_MB); table_call.hpp has the protocol of the batches.
// The call caches nothing on the handle.
#include <algorithm>
#include <cmath>
#include <vector>

#include "table_call.hpp"

namespace {

// Entries per lane between two renormalisations, all of their loads in flight.  The smallest factor this path can see:
// every row of u is a probability triple (gp0s of an af in [0, 1], or a caller's row that muxgl_fmx_unknown has checked:
// entries in [0, 1], sum within 1e-6 of 1), so a weight w[g2] = sum_g1 u[g1] g[3 g1 + g2] is a convex combination (to
// 1e-6) of entry likelihoods, and those leave calculate_snp_droplet_pileup clamped to MIN_NORM_GL = 1e-6 and divided by
// a sum <= 1 + 9e-6 (sc_drop_seq.cpp:498-504): w >= 9.9999e-7 (1 - 1e-6) > 2^-20; f_u likewise.  A factor is a
// combination of the weights with a posterior triple that sums to 1 within a few ulp (fmx_singlets.hip), or with u
// again: f >= min w > 2^-20.  A mantissa in [0.5, 1) times eight such factors is >= 2^-161: normal.  A factor of
// exactly 0 (posterior rows that were never filled) makes the product 0 and the log -inf; frexp(0) = 0, so no NaN.
constexpr int FUN_UNR = 8;
constexpr int FUN_W = 5;  // doubles per entry: w[0..2], f_u, f_uu

using fun_item = table_plan::item;  // the entries [e0, e1) of one cell, result row `row` of the slab

// u[s] = ((1 - af)(1 - af), 2 af (1 - af), af af), :388-390 (fmx_cgp_kernel's p0, p1, p2)
__global__ void __launch_bounds__(256) fun_prior_kernel(int64_t S, const double* __restrict__ af, double* __restrict__ u) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double a = af[s];
  u[3 * s] = (1.0 - a) * (1.0 - a);
  u[3 * s + 1] = 2 * a * (1.0 - a);
  u[3 * s + 2] = a * a;
}

// wt[e - eb0][0..2] = w, [3] = f_u, [4] = f_uu, for the entries [eb0, eb1) of a batch
__global__ void __launch_bounds__(256)
    fun_weight_kernel(int64_t eb0, int64_t eb1, const int32_t* __restrict__ entry_snp, const double* __restrict__ egls,
                      const double* __restrict__ u, double* __restrict__ wt) {
  const int64_t e = eb0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= eb1) return;
  const double* g = egls + (size_t)e * 9;
  const double* us = u + (size_t)entry_snp[e] * 3;
  const double u0 = us[0], u1 = us[1], u2 = us[2];
  const double w0 = fma(u2, g[6], fma(u1, g[3], u0 * g[0]));
  const double w1 = fma(u2, g[7], fma(u1, g[4], u0 * g[1]));
  const double w2 = fma(u2, g[8], fma(u1, g[5], u0 * g[2]));
  double* o = wt + (size_t)(e - eb0) * FUN_W;
  o[0] = w0;
  o[1] = w1;
  o[2] = w2;
  o[3] = fma(u2, g[8], fma(u1, g[4], u0 * g[0]));
  o[4] = fma(u2, w2, fma(u1, w1, u0 * w0));
}

// grid: ceil(n_items * nblk / 4) workgroups of four waves; wave x <-> (item x / nblk, cluster block x % nblk), so the
// waves of a workgroup walk the same entries and read neighbouring pieces of the same posterior rows.
// slab is [rows][K + 2]; this kernel writes the columns [0, K).
template <int KH>
__global__ void __launch_bounds__(256)
    fun_sweep_kernel(int64_t n_units, int nblk, const fun_item* __restrict__ items, const int32_t* __restrict__ entry_snp,
                     int64_t eb0, const double* __restrict__ wt, const double* __restrict__ cgp, int K,
                     double* __restrict__ slab) {
  constexpr int G = 64 / KH;  // entries side by side in a wave
  const int64_t x = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (x >= n_units) return;
  const int64_t it = x / nblk;
  const int blk = (int)(x - it * nblk);
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / KH;  // entry slot of the lane
  const int j = G == 1 ? blk * 64 + lane : lane % KH;
  const bool jl = j < K;
  const size_t jo = (size_t)(jl ? j : K - 1) * 3;
  const int64_t e0 = items[it].e0, e1 = items[it].e1;
  const size_t K3 = (size_t)K * 3;

  double acc = 1.0;
  int32_t ex = 0;
  for (int64_t eb = e0; eb < e1; eb += (int64_t)FUN_UNR * G) {
    double f[FUN_UNR];
#pragma unroll
    for (int i = 0; i < FUN_UNR; ++i) {
      const int64_t e = eb + (int64_t)i * G + sub;
      const bool ok = e < e1;
      const int64_t ec = ok ? e : e1 - 1;  // (a slot past the end reads the last entry again and counts as 1)
      const double* w = wt + (size_t)(ec - eb0) * FUN_W;
      const double* q = cgp + (size_t)entry_snp[ec] * K3 + jo;
      const double v = fma(w[2], q[2], fma(w[1], q[1], w[0] * q[0]));  // :440-446 with g1 summed into w
      f[i] = ok ? v : 1.0;
    }
#pragma unroll
    for (int i = 0; i < FUN_UNR; ++i) acc *= f[i];
    prodacc_renorm(acc, ex);
  }
  if (G > 1) {  // the G partial products of a cluster, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
    for (int off = KH; off < 64; off <<= 1) {
      acc *= __shfl_xor(acc, off, 64);
      ex += __shfl_xor(ex, off, 64);
    }
  }
  if (jl && sub == 0) slab[(size_t)items[it].row * (K + 2) + j] = prodacc_log(acc, ex);
}

// grid: ceil(n_items / 4) workgroups of four waves; wave <-> item, lane = entry slot: the columns K (u) and K + 1 (uu)
__global__ void __launch_bounds__(256)
    fun_scalar_kernel(int64_t n_items, const fun_item* __restrict__ items, int64_t eb0, const double* __restrict__ wt, int K,
                      double* __restrict__ slab) {
  const int64_t it = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (it >= n_items) return;
  const int lane = threadIdx.x & 63;
  const int64_t e0 = items[it].e0, e1 = items[it].e1;
  double a1 = 1.0, a2 = 1.0;
  int32_t x1 = 0, x2 = 0;
  for (int64_t eb = e0; eb < e1; eb += (int64_t)FUN_UNR * 64) {
    double f1[FUN_UNR], f2[FUN_UNR];
#pragma unroll
    for (int i = 0; i < FUN_UNR; ++i) {
      const int64_t e = eb + (int64_t)i * 64 + lane;
      const bool ok = e < e1;
      const double* w = wt + (size_t)((ok ? e : e1 - 1) - eb0) * FUN_W;
      f1[i] = ok ? w[3] : 1.0;
      f2[i] = ok ? w[4] : 1.0;
    }
#pragma unroll
    for (int i = 0; i < FUN_UNR; ++i) {
      a1 *= f1[i];
      a2 *= f2[i];
    }
    prodacc_renorm(a1, x1);
    prodacc_renorm(a2, x2);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    a1 *= __shfl_xor(a1, off, 64);
    x1 += __shfl_xor(x1, off, 64);
    a2 *= __shfl_xor(a2, off, 64);
    x2 += __shfl_xor(x2, off, 64);
  }
  if (lane == 0) {
    double* o = slab + (size_t)items[it].row * (K + 2) + K;
    o[0] = prodacc_log(a1, x1);
    o[1] = prodacc_log(a2, x2);
  }
}

// lane = (cell, column) of the first nc slab rows: ju [nc][K], lu [nc], uu [nc]
__global__ void __launch_bounds__(256)
    fun_split_kernel(int64_t nc, int K, const double* __restrict__ slab, double* __restrict__ ju, double* __restrict__ lu,
                     double* __restrict__ uu) {
  const int KC = K + 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc * KC) return;
  const int64_t c = i / KC;
  const int j = (int)(i - c * KC);
  const double v = slab[i];
  if (j < K)
    ju[(size_t)c * K + j] = v;
  else if (j == K)
    lu[c] = v;
  else
    uu[c] = v;
}

template <int KH>
void launch_sweep(muxgl_handle* h, int64_t n_items, int nblk, const fun_item* d_items, int64_t eb0, const double* d_wt,
                  double* d_slab) {
  const int64_t n_units = n_items * nblk;
  hipLaunchKernelGGL((fun_sweep_kernel<KH>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, nblk,
                     d_items, h->d_entry_snp, eb0, d_wt, h->d_cgp, h->K, d_slab);
}

int fmx_unknown_run(muxgl_handle* h, const double* gp0, double* ll_ju, double* ll_u, double* ll_uu, float* kernel_ms) {
  const int K = h->K, KC = K + 2, nblk = (K + 63) / 64, KH = lane_width(K);
  const int64_t S = h->S;
  const table_call call = {"muxgl_fmx_unknown", "MUXGL_FMX_SLAB_MB", table_plan::equal_begin, (double)nblk, (double)KC, 0.0,
                           table_plan::shape(K, "clusters"), table_plan::shape(K, "clusters")};
  table_batches<table_plan::cut> tb;
  if (tb.plan(h, call, [K](int64_t len, int64_t np) { return table_plan::fmx_unknown_bytes(len, np, K); })) return 1;

  dev_tmp<double> d_u, d_wt, d_slab, d_ju, d_lu, d_uu;
  if (dev_alloc(h, &d_u.p, (size_t)S * 3)) return 1;
  if (dev_alloc(h, &d_wt.p, (size_t)tb.bt.max_entries * FUN_W)) return 1;
  if (dev_alloc(h, &d_slab.p, (size_t)tb.bt.max_rows * KC)) return 1;
  if (dev_alloc(h, &d_ju.p, (size_t)tb.bt.max_cells * K)) return 1;
  if (dev_alloc(h, &d_lu.p, (size_t)tb.bt.max_cells)) return 1;
  if (dev_alloc(h, &d_uu.p, (size_t)tb.bt.max_cells)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, call.who)) return 1;
  if (gp0 && S > 0) HIPCHK(h, hipMemcpyAsync(d_u.p, gp0, sizeof(double) * (size_t)S * 3, hipMemcpyHostToDevice, h->stream));
  return tb.run(h, ev,
      [&](const table_batch<table_plan::cut>& b) {
        if (b.c0 == 0 && !gp0 && S > 0) {  // the unknown donor's prior, once per call
          hipLaunchKernelGGL(fun_prior_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, S, h->d_af, d_u.p);
          HIPCHK(h, hipGetLastError());
        }
        if (b.eb1 > b.eb0) {
          hipLaunchKernelGGL(fun_weight_kernel, dim3((unsigned)((b.eb1 - b.eb0 + 255) / 256)), dim3(256), 0, h->stream, b.eb0,
                             b.eb1, h->d_entry_snp, h->d_egls, d_u.p, d_wt.p);
          HIPCHK(h, hipGetLastError());
        }
#define CALL_S(W) launch_sweep<W>(h, b.n_items, nblk, b.d_items, b.eb0, d_wt.p, d_slab.p)
        DISPATCH_WIDTH(KH, CALL_S);
#undef CALL_S
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(fun_scalar_kernel, dim3((unsigned)((b.n_items + 3) / 4)), dim3(256), 0, h->stream, b.n_items, b.d_items,
                           b.eb0, d_wt.p, K, d_slab.p);
        HIPCHK(h, hipGetLastError());
        if (table_join(h, b, KC, d_slab.p)) return 1;
        const int64_t n = b.nc() * KC;
        hipLaunchKernelGGL(fun_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, b.nc(), K, d_slab.p,
                           d_ju.p, d_lu.p, d_uu.p);
        HIPCHK(h, hipGetLastError());
        return 0;
      },
      [&](const table_batch<table_plan::cut>& b) {
        const size_t nc = (size_t)b.nc();
        if (ll_ju) HIPCHK(h, hipMemcpyAsync(ll_ju + (size_t)b.c0 * K, d_ju.p, sizeof(double) * nc * K, hipMemcpyDeviceToHost, h->stream));
        if (ll_u) HIPCHK(h, hipMemcpyAsync(ll_u + b.c0, d_lu.p, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        if (ll_uu) HIPCHK(h, hipMemcpyAsync(ll_uu + b.c0, d_uu.p, sizeof(double) * nc, hipMemcpyDeviceToHost, h->stream));
        return 0;
      });
}

}  // namespace

// the caller's prior, on the host: every row a probability triple (entries in [0, 1], sum within 1e-6 of 1), which is
// what the renormalisation bound above rests on; the first offending marker, or -1
int64_t fmx_unknown_bad_prior(const double* gp0, int64_t S) {
  for (int64_t s = 0; s < S; ++s) {
    const double a = gp0[3 * s], b = gp0[3 * s + 1], c = gp0[3 * s + 2];
    if (!(a >= 0.0 && a <= 1.0 && b >= 0.0 && b <= 1.0 && c >= 0.0 && c <= 1.0 && std::fabs(a + b + c - 1.0) <= 1e-6)) return s;
  }
  return -1;
}

extern "C" int muxgl_fmx_unknown(muxgl_handle* h, const double* gp0, double* ll_ju, double* ll_u, double* ll_uu,
                                 float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (h->group) return group_fmx_unknown(h, gp0, ll_ju, ll_u, ll_uu, kernel_ms);
  HIPCHK(h, hipSetDevice(h->device));
  if (fmx_refuse(h, h, "muxgl_fmx_unknown", "the tables belong")) return 1;
  if (!ll_ju && !ll_u && !ll_uu) MUXGL_FAIL(h, "muxgl_fmx_unknown: all three outputs are NULL");
  if (gp0) {
    const int64_t bad = fmx_unknown_bad_prior(gp0, h->S);
    if (bad >= 0)
      MUXGL_FAIL(h, "muxgl_fmx_unknown: gp0 row of marker %lld (%g, %g, %g) is not a probability triple (entries in [0, 1], "
                    "sum within 1e-6 of 1)",
                 (long long)bad, gp0[3 * bad], gp0[3 * bad + 1], gp0[3 * bad + 2]);
  }
  if (h->C == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  return fmx_unknown_run(h, gp0, ll_ju, ll_u, ll_uu, kernel_ms);
}
