// ambient_table.hpp -- what the two ambient tables share (muxgl_demux_ambient in demux_ambient.hip, muxgl_fmx_ambient in
// fmx_ambient.hip): the sweep and emit kernels, the batch, the width and chunk dispatch and the host run, itself a
// customer of table_call.hpp's table_batches like the singlet and unknown-donor tables.  A unit brings its weight kernel
// -- the only place where the two models differ -- and a description of the call.
//
// What the skeleton guarantees to both callers:
//   * wt[(e - eb0)][r][0..2], the unit's weight triple of entry e at rho r, is read and never rescaled; the table is
//     out[c][j][r] = sum over the entries e of cell c of log( (p_j0 w_e[r][0] + p_j1 w_e[r][1]) + p_j2 w_e[r][2] ), p_j
//     the row [s_e][j][0..2] of the unit's posterior array, the dot formed as fma(p2, w2, fma(p1, w1, p0 w0)).
//   * A wave is one work unit: a part of a cell (at most table_plan::PART entries) x a block of 64 columns x a chunk of
//     CH <= 4 rhos.  Every accumulator belongs to one (column, rho); every lane walks the entries sub, sub + G, ... of
//     its part whatever UNR is, and a renormalisation moves powers of two only: neither the chunk, the block width nor
//     UNR changes a bit.  Below 64 columns a wave holds G = 64 / WH entries side by side, multiplied in a fixed xor
//     butterfly at the end; the logs of the parts of a cell are added in entry order.
//   * Which cell goes into which batch and its cut into parts are table_plan.hpp's, under the unit's cut policy.  The
//     cut of a cell depends on the cell alone and every reduction tree is fixed: the table is bit-identical from call to
//     call, for any budget, for any split of the rhos over calls, on one device, on a group and through the sharded
//     driver.
//   * Nothing proportional to nnz x n_rho is held for the whole pileup: cells are swept in batches of whole cells whose
//     device bytes (table_plan::ambient_bytes) fit the unit's budget.  The call caches nothing on the handle and leaves
//     its timing slots alone.
//   * The order of the run is table_call.hpp's protocol; here the rho grid, four buffers (af, wt, slab, out), the event
//     pair and the profile's copy to the device, per batch weights, sweep and emit inside the bracket, then the copy-out.
// UNR, the entries per lane between two renormalisations, is the unit's: how many factors a product can take without
// leaving the normal range depends on the smallest factor its weights allow (Tool::unr(WH, CH), see each unit).
#pragma once
#include <vector>

#include "table_call.hpp"

constexpr int AMBIENT_MAX_RHO = 16;  // rhos of one call (MUXGL_MAX_ALPHA)

// the call's rhos as a kernel argument; the slots past the end repeat the last rho (they are computed and not written)
struct ambient_rhos {
  double a[AMBIENT_MAX_RHO];
};
using ambient_item = table_plan::item;  // the entries [e0, e1) of one cell, result row `row` of the slab
// the further parts of a cell: its value = slab[cell row] + slab[first] + ... + slab[first + count - 1], in this order
using ambient_cell = table_plan::cell;

// grid: ceil(n_units / 4) workgroups of four waves; wave unit <-> (item, column block, rho chunk), the chunk fastest,
// so the waves of a workgroup walk the same entries and read the same or neighbouring pieces of the posterior rows.
// lane = column of a 64-column block; post: [S][W][3]; slab[row][r][W].  Tool: the unit's tag, with its UNR rule.
template <class Tool, int WH, int CH>
__global__ void __launch_bounds__(256)
    ambient_sweep_kernel(int64_t n_units, int nblk, int nch, int NR, const ambient_item* __restrict__ items,
                         const int32_t* __restrict__ entry_snp, int64_t eb0, const double* __restrict__ wt,
                         const double* __restrict__ post, int W, double* __restrict__ slab) {
  constexpr int G = 64 / WH;  // entries side by side in a wave
  constexpr int UNR = Tool::unr(WH, CH);  // entries per lane between two renormalisations, all of their loads in flight
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int ch = (int)(unit % nch);
  const int64_t rest = unit / nch;
  const int blk = (int)(rest % nblk);
  const int64_t it = rest / nblk;
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / WH;  // entry slot of the lane
  const int j = G == 1 ? blk * 64 + lane : lane % WH;
  const bool jl = j < W;
  const size_t jo = (size_t)(jl ? j : W - 1) * 3;
  const size_t W3 = (size_t)W * 3;
  const int64_t e0 = items[it].e0, e1 = items[it].e1;
  int rr[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) rr[c] = ch * CH + c < NR ? ch * CH + c : NR - 1;  // (a slot past the end repeats the last rho)

  double acc[CH];
  int32_t ex[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    acc[c] = 1.0;
    ex[c] = 0;
  }
  for (int64_t eb = e0; eb < e1; eb += (int64_t)UNR * G) {
    double f[UNR][CH];
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      const int64_t e = eb + (int64_t)i * G + sub;
      const bool ok = e < e1;
      const int64_t ec = ok ? e : e1 - 1;  // (a slot past the end reads the last entry again and counts as 1)
      const double* q = post + (size_t)entry_snp[ec] * W3 + jo;
      const double q0 = q[0], q1 = q[1], q2 = q[2];
      const double* we = wt + (size_t)(ec - eb0) * NR * 3;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const double* w = we + rr[c] * 3;
        const double v = fma(q2, w[2], fma(q1, w[1], q0 * w[0]));
        f[i][c] = ok ? v : 1.0;
      }
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i)
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] *= f[i][c];
#pragma unroll
    for (int c = 0; c < CH; ++c) prodacc_renorm(acc[c], ex[c]);
  }
  if (G > 1) {  // the G partial products of a column, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
    for (int off = WH; off < 64; off <<= 1)
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        acc[c] *= __shfl_xor(acc[c], off, 64);
        ex[c] += __shfl_xor(ex[c], off, 64);
      }
  }
  if (jl && sub == 0) {
    double* out = slab + (size_t)items[it].row * NR * W + j;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (ch * CH + c < NR) out[(size_t)rr[c] * W] = prodacc_log(acc[c], ex[c]);
  }
}

// lane = (cell, column, rho), rho fastest: out[nc][W][NR], the logs of the parts of a cell added in entry order
template <class Tool>
__global__ void __launch_bounds__(256)
    ambient_emit_kernel(int64_t nc, const ambient_cell* __restrict__ cells, int W, int NR, const double* __restrict__ slab,
                        double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc * W * NR) return;
  const int r = (int)(i % NR);
  const int j = (int)((i / NR) % W);
  const int64_t c = i / ((int64_t)NR * W);
  const size_t rs = (size_t)NR * W, off = (size_t)r * W + j;
  const ambient_cell ct = cells[c];
  double s = slab[(size_t)c * rs + off];
  for (int64_t k = 0; k < ct.count; ++k) s += slab[(size_t)(ct.first + k) * rs + off];
  out[i] = s;
}

struct ambient_batch {  // what one launch of the three kernels needs
  int64_t eb0, eb1, n_items, nc;
  const ambient_item* d_items;
  const ambient_cell* d_cells;
  double *d_wt, *d_slab, *d_out;
  const double* d_af;
};

// what a unit says about its call
struct ambient_call {
  const char* who;             // the call's name, for the messages and the event pair
  int W;                       // columns of the table: samples or clusters
  const char* noun;            // ... and what the messages call them
  const double* d_post;        // the posterior array [S][W][3] the sweep reads (d_gp, d_cgp)
  const char* budget_env;      // the variable that sets the budget, named in the messages
  table_plan::begin_fn begin;  // the cut policy of a long cell
};

template <class Tool, int WH, int CH>
void ambient_launch_sweep(muxgl_handle* h, const ambient_call& call, int NR, int nch, const ambient_batch& b) {
  const int nblk = (call.W + 63) / 64;
  const int64_t n_units = b.n_items * nblk * nch;
  hipLaunchKernelGGL((ambient_sweep_kernel<Tool, WH, CH>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream,
                     n_units, nblk, nch, NR, b.d_items, h->d_entry_snp, b.eb0, b.d_wt, call.d_post, call.W, b.d_slab);
}

template <class Tool, int CH>
void ambient_sweep_width(muxgl_handle* h, const ambient_call& call, int NR, int nch, const ambient_batch& b) {
#define CALL_S(N) ambient_launch_sweep<Tool, N, CH>(h, call, NR, nch, b)
  DISPATCH_WIDTH(lane_width(call.W), CALL_S);
#undef CALL_S
}

template <class Tool>
int ambient_sweep_dispatch(muxgl_handle* h, const ambient_call& call, int CH, int NR, int nch, const ambient_batch& b) {
  switch (CH) {
    case 1: ambient_sweep_width<Tool, 1>(h, call, NR, nch, b); break;
    case 2: ambient_sweep_width<Tool, 2>(h, call, NR, nch, b); break;
    case 3: ambient_sweep_width<Tool, 3>(h, call, NR, nch, b); break;
    default: ambient_sweep_width<Tool, 4>(h, call, NR, nch, b); break;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The table of the handle's own cells to the host, ll_amb[C][W][NR].  weights(rh, b) launches the unit's weight kernel
// for the entries [b.eb0, b.eb1) of a batch (it is not called for a batch without entries) and returns 0, or 1 with the
// handle's message set.  The arguments are the caller's to check.
template <class Tool, class Weights>
int ambient_table_run(muxgl_handle* h, const ambient_call& call, const double* amb_af, int NR, const double* rho,
                      double* ll_amb, float* kernel_ms, Weights&& weights) {
  const int W = call.W;
  const int64_t S = h->S;
  const int nblk = (W + 63) / 64;
  const int nch = (NR + 3) / 4, CH = (NR + nch - 1) / nch;  // chunks of the rhos, rhos per chunk (1..4)
  const table_call tc = {call.who, call.budget_env, call.begin, (double)nblk * nch, 0.0, (double)W * NR,
                         table_plan::shape(W, call.noun, NR, "rhos"), table_plan::shape(NR, "rhos", W, call.noun)};
  table_batches<ambient_cell> tb;
  if (tb.plan(h, tc, [=](int64_t len, int64_t np) { return table_plan::ambient_bytes(len, np, NR, W); })) return 1;
  ambient_rhos rh;
  for (int i = 0; i < AMBIENT_MAX_RHO; ++i) rh.a[i] = i < NR ? rho[i] : rho[NR - 1];  // (a slot past the end is not written)

  dev_tmp<double> d_af, d_wt, d_slab, d_out;
  if (dev_alloc(h, &d_af.p, (size_t)S)) return 1;
  if (dev_alloc(h, &d_wt.p, (size_t)tb.bt.max_entries * NR * 3)) return 1;
  if (dev_alloc(h, &d_slab.p, (size_t)tb.bt.max_rows * NR * W)) return 1;
  if (dev_alloc(h, &d_out.p, (size_t)tb.bt.max_cells * W * NR)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, call.who)) return 1;
  if (S > 0) HIPCHK(h, hipMemcpyAsync(d_af.p, amb_af, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, h->stream));
  return tb.run(h, ev,
      [&](const table_batch<ambient_cell>& t) {
        const ambient_batch b = {t.eb0, t.eb1, t.n_items, t.nc(), t.d_items, t.d_recs, d_wt.p, d_slab.p, d_out.p, d_af.p};
        if (b.eb1 > b.eb0 && weights(rh, b)) return 1;
        if (ambient_sweep_dispatch<Tool>(h, call, CH, NR, nch, b)) return 1;
        const int64_t n = b.nc * W * NR;
        hipLaunchKernelGGL(ambient_emit_kernel<Tool>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, b.nc, b.d_cells, W,
                           NR, d_slab.p, d_out.p);
        HIPCHK(h, hipGetLastError());
        return 0;
      },
      [&](const table_batch<ambient_cell>& t) {
        HIPCHK(h, hipMemcpyAsync(ll_amb + (size_t)t.c0 * W * NR, d_out.p, sizeof(double) * (size_t)t.nc() * W * NR,
                                 hipMemcpyDeviceToHost, h->stream));
        return 0;
      });
}
