// demux_unknown.hip -- muxgl_demux_unknown: every droplet scored against a donor that is not in the panel, the
// llksA0 / llks00 accumulation of cmd_cram_demuxlet.cpp:749-773 (which the reference computes and never prints) and
// the other orientation of the half-known doublet.  With u[s] the unknown donor's genotype prior at marker s (the panel
// mean of :428-440, or the caller's), over the entries e of droplet c whose marker has genotypes:
//
//   ll_ju[c][j][n] = sum_e log( sum_l sum_m gp[s_e][j][l] * u[s_e][m]     * pG_e[n][l][m] )     (llksA0)
//   ll_uj[c][k][n] = sum_e log( sum_l sum_m u[s_e][l]     * gp[s_e][k][m] * pG_e[n][l][m] )
//   ll_uu[c][n]    = sum_e log( sum_l sum_m u[s_e][l]     * u[s_e][m]     * pG_e[n][l][m] )     (llks00)
//
// The design is that of demux_singlets.hip with 2 x n_alpha weight triples per entry instead of one:
//   * unk_mean_kernel, lane = marker: u = (gp[s][0] + ... + gp[s][V-1]) / V, added in sample order.  (1, 0, 0) for a
//     marker without genotypes, which is also what unk_neutral_kernel writes into the caller's prior.
//   * unk_weight_kernel, lane = entry: the per-entry likelihoods of the whole grid (row_entry_pg), then per alpha
//     wju[n][l] = sum_m u[m] pG[n][l][m] and wuj[n][m] = sum_l u[l] pG[n][l][m].  A marker without genotypes gets ones:
//     its rows of gp and u are (1, 0, 0), so its factor is exactly 1 everywhere and the sweep has no branch.
//   * unk_sweep_kernel, lane = column of the slab: the V samples and, as column V, u itself (its "ju" dot is ll_uu).
//     Two dots per (entry, column, alpha), multiplied into products kept as mantissa x 2^exponent, one log per (cell
//     part, column, alpha, orientation).  A wave is one work unit: a part of a cell (at most 2048 entries) x a block
//     of 64 columns x a chunk of CH <= 3 alphas -- the accumulators of a whole 16-alpha grid do not fit a lane beside
//     the loads in flight.  Every accumulator belongs to one (alpha, orientation), so the chunking changes no bit.
//     Below 64 columns a wave holds G = 64 / VH entries side by side, multiplied in a fixed butterfly at the end.
//     Two launches per batch: the samples (VH = V rounded up to a power of two, as the singlet sweep) and column V alone
//     (VH = 1, 64 entries side by side) -- one launch over V + 1 columns would idle half the lanes at 8, 16 or 32
//     samples and spend a whole second block on one column at 64.
//   * unk_emit_kernel: the logs of the parts of a cell added in entry order and written in the caller's layout.
// Which cell goes into which batch, its cut into parts (fixed parts of 2048 entries) and the order of the work items
// are table_plan.hpp's; the host body that drives the plan is table_call.hpp's table_batches, whose customer this unit
// is.  The cut of a cell depends on the cell alone and every reduction tree is fixed: the tables are
// bit-identical from call to call, for any budget, for any subset of outputs, on one device, on a group and through the
// sharded driver.
//
// Memory: nothing proportional to nnz x n_alpha is held for the whole pileup.  Cells are swept in batches of whole cells
// whose weights ([entries][n_alpha][6]), slab rows and output rows (table_plan::unknown_bytes) fit the streamed call's
// budget (4 GiB or a third of the device, MUXGL_DEMUX_SLAB_MB); table_call.hpp has the protocol of the batches.
#include <algorithm>
#include <vector>

#include "demux_entry.hpp"
#include "table_call.hpp"

namespace {

using unk_item = table_plan::item;  // the entries [e0, e1) of one cell, result row `row` of the slab
// the further parts of a cell: its value = slab[cell row] + slab[first] + ... + slab[first + count - 1], in this order
using unk_cell = table_plan::cell;

__global__ void __launch_bounds__(256)
    unk_mean_kernel(int64_t S, const double* __restrict__ gp, const uint8_t* __restrict__ has_gp, int V, double* __restrict__ u) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  double a0 = 1.0, a1 = 0.0, a2 = 0.0;
  if (has_gp[s]) {  // :428-440: the rows added in sample order, one division
    const double* g = gp + (size_t)s * V * 3;
    a0 = a1 = a2 = 0.0;
    for (int j = 0; j < V; ++j) {
      a0 += g[3 * j];
      a1 += g[3 * j + 1];
      a2 += g[3 * j + 2];
    }
    const double nv = (double)V;
    a0 /= nv;
    a1 /= nv;
    a2 /= nv;
  }
  u[3 * s] = a0;
  u[3 * s + 1] = a1;
  u[3 * s + 2] = a2;
}

__global__ void __launch_bounds__(256) unk_neutral_kernel(int64_t S, const uint8_t* __restrict__ has_gp, double* __restrict__ u) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S || has_gp[s]) return;
  u[3 * s] = 1.0;
  u[3 * s + 1] = 0.0;
  u[3 * s + 2] = 0.0;
}

// wt[(e - eb0)][n][0..2] = wju[n][l], [3..5] = wuj[n][m], for the entries [eb0, eb1) of a batch
template <int NA>
__global__ void __launch_bounds__(256)
    unk_weight_kernel(int64_t eb0, int64_t eb1, int A, const int32_t* __restrict__ entry_snp, const int64_t* __restrict__ entry_rptr,
                      const uint8_t* __restrict__ reads, const double* __restrict__ lut_g, demux_grid al,
                      const double* __restrict__ u, const uint8_t* __restrict__ has_gp, double* __restrict__ wt) {
  __shared__ double lut[384];
  for (int i = threadIdx.x; i < 384; i += 256) lut[i] = lut_g[i];
  __syncthreads();
  const int64_t e = eb0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= eb1) return;
  const int32_t s = entry_snp[e];
  double* o = wt + (size_t)(e - eb0) * A * 6;
  if (!has_gp[s]) {  // (no genotypes: the reference skips the marker, :733)
    for (int i = 0; i < A * 6; ++i) o[i] = 1.0;
    return;
  }
  const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
  uint32_t first4 = 0;
  for (int64_t k = 0; k < 4 && r0 + k < r1; ++k) first4 |= (uint32_t)reads[r0 + k] << (8 * (int)k);
  double pG[NA * 9];
  row_entry_pg<NA>(reads, r0, r1, first4, al.a, lut, pG);
  const double u0 = u[3 * (size_t)s], u1 = u[3 * (size_t)s + 1], u2 = u[3 * (size_t)s + 2];
#pragma unroll
  for (int n = 0; n < NA; ++n) {
    if (n >= A) break;
    const double* q = &pG[n * 9];
    o[n * 6 + 0] = fma(u2, q[2], fma(u1, q[1], u0 * q[0]));
    o[n * 6 + 1] = fma(u2, q[5], fma(u1, q[4], u0 * q[3]));
    o[n * 6 + 2] = fma(u2, q[8], fma(u1, q[7], u0 * q[6]));
    o[n * 6 + 3] = fma(u2, q[6], fma(u1, q[3], u0 * q[0]));
    o[n * 6 + 4] = fma(u2, q[7], fma(u1, q[4], u0 * q[1]));
    o[n * 6 + 5] = fma(u2, q[8], fma(u1, q[5], u0 * q[2]));
  }
}

// grid: ceil(n_units / 4) workgroups of four waves; wave unit <-> (item, column block, alpha chunk), the chunk fastest,
// so the waves of a workgroup walk the same entries and read the same or neighbouring pieces of the genotype rows.
// slab[row][n][orientation][V + 1]
template <int VH, int CH>
__global__ void __launch_bounds__(256)
    unk_sweep_kernel(int64_t n_units, int nblk, int nch, int A, const unk_item* __restrict__ items,
                     const int32_t* __restrict__ entry_snp, int64_t eb0, const double* __restrict__ wt,
                     const double* __restrict__ gp, const double* __restrict__ u, int V, int j0, int ncol,
                     double* __restrict__ slab) {
  constexpr int G = 64 / VH;              // entries side by side in a wave
  constexpr int UNR = CH == 1 ? 8 : 4;    // entries per lane between two renormalisations, their loads in flight: a factor
                                          // is >= ~1e-11 for triples that sum to ~1, eight cannot underflow
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int ch = (int)(unit % nch);
  const int64_t rest = unit / nch;
  const int blk = (int)(rest % nblk);
  const int64_t it = rest / nblk;
  const int VC = V + 1;  // columns of the slab: the samples, then u; this launch sweeps [j0, j0 + ncol)
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / VH;  // entry slot of the lane
  const int jj = G == 1 ? blk * 64 + lane : lane % VH;
  const bool jl = jj < ncol;
  const int j = j0 + (jl ? jj : ncol - 1);
  const double* colp = j < V ? gp + (size_t)j * 3 : u;  // column V reads u in place of a panel row
  const size_t cstride = j < V ? (size_t)V * 3 : 3;
  const int64_t e0 = items[it].e0, e1 = items[it].e1;
  int nn[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) nn[c] = ch * CH + c < A ? ch * CH + c : A - 1;  // (a slot past the grid repeats the last alpha)

  double acc[CH][2];
  int32_t ex[CH][2];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    acc[c][0] = acc[c][1] = 1.0;
    ex[c][0] = ex[c][1] = 0;
  }
  for (int64_t eb = e0; eb < e1; eb += (int64_t)UNR * G) {
    double f[UNR][CH][2];
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      const int64_t e = eb + (int64_t)i * G + sub;
      const bool ok = e < e1;
      const int64_t ec = ok ? e : e1 - 1;  // (a slot past the end reads the last entry again and counts as 1)
      const double* g = colp + (size_t)entry_snp[ec] * cstride;
      const double g0 = g[0], g1 = g[1], g2 = g[2];
      const double* we = wt + (size_t)(ec - eb0) * A * 6;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const double* w = we + nn[c] * 6;
        const double v0 = fma(g2, w[2], fma(g1, w[1], g0 * w[0]));
        const double v1 = fma(g2, w[5], fma(g1, w[4], g0 * w[3]));
        f[i][c][0] = ok ? v0 : 1.0;
        f[i][c][1] = ok ? v1 : 1.0;
      }
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i)
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        acc[c][0] *= f[i][c][0];
        acc[c][1] *= f[i][c][1];
      }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      prodacc_renorm(acc[c][0], ex[c][0]);
      prodacc_renorm(acc[c][1], ex[c][1]);
    }
  }
  if (G > 1) {  // the G partial products of a column, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
    for (int off = VH; off < 64; off <<= 1)
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          acc[c][o] *= __shfl_xor(acc[c][o], off, 64);
          ex[c][o] += __shfl_xor(ex[c][o], off, 64);
        }
  }
  if (jl && sub == 0) {
    double* out = slab + (size_t)items[it].row * A * 2 * VC + j;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (ch * CH + c < A) {
        out[((size_t)nn[c] * 2 + 0) * VC] = prodacc_log(acc[c][0], ex[c][0]);
        out[((size_t)nn[c] * 2 + 1) * VC] = prodacc_log(acc[c][1], ex[c][1]);
      }
  }
}

// lane = (cell, column, alpha), alpha fastest: ju / uj [nc][V][A], uu [nc][A]
__global__ void __launch_bounds__(256)
    unk_emit_kernel(int64_t nc, const unk_cell* __restrict__ cells, int V, int A, const double* __restrict__ slab,
                    double* __restrict__ ju, double* __restrict__ uj, double* __restrict__ uu) {
  const int VC = V + 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc * VC * A) return;
  const int n = (int)(i % A);
  const int j = (int)((i / A) % VC);
  const int64_t c = i / ((int64_t)A * VC);
  const size_t rs = (size_t)A * 2 * VC, off = (size_t)n * 2 * VC + j;
  const unk_cell ct = cells[c];
  double s0 = slab[(size_t)c * rs + off], s1 = slab[(size_t)c * rs + off + VC];
  for (int64_t k = 0; k < ct.count; ++k) {
    s0 += slab[(size_t)(ct.first + k) * rs + off];
    s1 += slab[(size_t)(ct.first + k) * rs + off + VC];
  }
  if (j < V) {
    ju[((size_t)c * V + j) * A + n] = s0;
    uj[((size_t)c * V + j) * A + n] = s1;
  } else {
    uu[(size_t)c * A + n] = s0;
  }
}

struct unk_batch {  // what one launch of the three kernels needs
  int64_t eb0, eb1, n_items, nc;
  const unk_item* d_items;
  const unk_cell* d_cells;
  double *d_wt, *d_slab, *d_ju, *d_uj, *d_uu;
  const double* d_u;
};

template <int NA>
int launch_weights(muxgl_handle* h, int A, const demux_grid& al, const unk_batch& b) {
  hipLaunchKernelGGL((unk_weight_kernel<NA>), dim3((unsigned)((b.eb1 - b.eb0 + 255) / 256)), dim3(256), 0, h->stream, b.eb0,
                     b.eb1, A, h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, al, b.d_u, h->d_has_gp, b.d_wt);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int weights_dispatch(muxgl_handle* h, int A, const demux_grid& al, const unk_batch& b) {
#define CALL_W(N) launch_weights<N>(h, A, al, b)
  DISPATCH_NA(A, CALL_W);
#undef CALL_W
}

// the columns [j0, j0 + ncol) of the slab
template <int VH, int CH>
void launch_sweep(muxgl_handle* h, int A, int nch, int j0, int ncol, const unk_batch& b) {
  const int nblk = (ncol + 63) / 64;
  const int64_t n_units = b.n_items * nblk * nch;
  hipLaunchKernelGGL((unk_sweep_kernel<VH, CH>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, nblk,
                     nch, A, b.d_items, h->d_entry_snp, b.eb0, b.d_wt, h->d_gp, b.d_u, h->V, j0, ncol, b.d_slab);
}

template <int CH>
void sweep_dispatch_vh(muxgl_handle* h, int A, int nch, int j0, int ncol, const unk_batch& b) {
#define CALL_S(W) launch_sweep<W, CH>(h, A, nch, j0, ncol, b)
  DISPATCH_WIDTH(lane_width(ncol), CALL_S);
#undef CALL_S
}

int sweep_dispatch(muxgl_handle* h, int CH, int A, int nch, int j0, int ncol, const unk_batch& b) {
  switch (CH) {
    case 1: sweep_dispatch_vh<1>(h, A, nch, j0, ncol, b); break;
    case 2: sweep_dispatch_vh<2>(h, A, nch, j0, ncol, b); break;
    default: sweep_dispatch_vh<3>(h, A, nch, j0, ncol, b); break;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // namespace

int demux_unknown_run(muxgl_handle* h, const muxgl_demux_params* p, const double* gp0, double* ll_ju, double* ll_uj,
                      double* ll_uu, float* kernel_ms) {
  const int V = h->V, A = p->n_alpha, VC = V + 1;
  const int64_t S = h->S;
  const int nblk = (V + 63) / 64;
  const int nch = (A + 2) / 3, CH = (A + nch - 1) / nch;  // chunks of the grid, alphas per chunk (1..3)
  const table_call call = {"muxgl_demux_unknown", "MUXGL_DEMUX_SLAB_MB", table_plan::fixed_begin, (double)nblk * nch, 0.0,
                           (double)VC * A, table_plan::shape(V, "samples", A, "alphas"), table_plan::shape(A, "alphas", V, "samples")};
  table_batches<unk_cell> tb;
  if (tb.plan(h, call, [=](int64_t len, int64_t np) { return table_plan::unknown_bytes(len, np, A, VC); })) return 1;
  const demux_grid al = demux_grid_of(p);

  dev_tmp<double> d_u, d_wt, d_slab, d_ju, d_uj, d_uu;
  if (dev_alloc(h, &d_u.p, (size_t)S * 3)) return 1;
  if (dev_alloc(h, &d_wt.p, (size_t)tb.bt.max_entries * A * 6)) return 1;
  if (dev_alloc(h, &d_slab.p, (size_t)tb.bt.max_rows * A * 2 * VC)) return 1;
  if (dev_alloc(h, &d_ju.p, (size_t)tb.bt.max_cells * V * A)) return 1;
  if (dev_alloc(h, &d_uj.p, (size_t)tb.bt.max_cells * V * A)) return 1;
  if (dev_alloc(h, &d_uu.p, (size_t)tb.bt.max_cells * A)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, call.who)) return 1;
  if (gp0 && S > 0) HIPCHK(h, hipMemcpyAsync(d_u.p, gp0, sizeof(double) * (size_t)S * 3, hipMemcpyHostToDevice, h->stream));
  return tb.run(h, ev,
      [&](const table_batch<unk_cell>& t) {
        const unk_batch b = {t.eb0, t.eb1, t.n_items, t.nc(), t.d_items, t.d_recs, d_wt.p, d_slab.p, d_ju.p, d_uj.p, d_uu.p, d_u.p};
        if (t.c0 == 0 && S > 0) {  // the unknown donor's prior, once per call
          if (gp0)
            hipLaunchKernelGGL(unk_neutral_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, S, h->d_has_gp, d_u.p);
          else
            hipLaunchKernelGGL(unk_mean_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, S, h->d_gp, h->d_has_gp,
                               V, d_u.p);
          HIPCHK(h, hipGetLastError());
        }
        if (b.eb1 > b.eb0 && weights_dispatch(h, A, al, b)) return 1;
        if (sweep_dispatch(h, CH, A, nch, 0, V, b)) return 1;  // the samples
        if (sweep_dispatch(h, CH, A, nch, V, 1, b)) return 1;  // the unknown donor's own column
        const int64_t n = b.nc * VC * A;
        hipLaunchKernelGGL(unk_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, b.nc, b.d_cells, V, A,
                           d_slab.p, d_ju.p, d_uj.p, d_uu.p);
        HIPCHK(h, hipGetLastError());
        return 0;
      },
      [&](const table_batch<unk_cell>& t) {
        const size_t nva = sizeof(double) * (size_t)t.nc() * V * A;
        if (ll_ju) HIPCHK(h, hipMemcpyAsync(ll_ju + (size_t)t.c0 * V * A, d_ju.p, nva, hipMemcpyDeviceToHost, h->stream));
        if (ll_uj) HIPCHK(h, hipMemcpyAsync(ll_uj + (size_t)t.c0 * V * A, d_uj.p, nva, hipMemcpyDeviceToHost, h->stream));
        if (ll_uu)
          HIPCHK(h, hipMemcpyAsync(ll_uu + (size_t)t.c0 * A, d_uu.p, sizeof(double) * (size_t)t.nc() * A, hipMemcpyDeviceToHost, h->stream));
        return 0;
      });
}
