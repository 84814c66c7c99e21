// demux_singlets.hip -- muxgl_demux_singlets: the [C][V] table of singlet log-likelihoods, llksAB[(j, 0, 0)] of
// cmd_cram_demuxlet.cpp:733-747 for every droplet and every sample (what the reference's disabled .single / .sing2 writers
// print, :580, :839-848).
//
//   sng[c][j] = sum over the entries e of c whose marker has genotypes of
//               log( sum_l sum_m gp[snp_e][j][l] * gp[snp_e][0][m] * pG_e[0][l][m] )
//
// Two kernels and a small one for long cells:
//   * sng_weight_kernel, lane = entry: the per-entry likelihoods of the whole grid (row_entry_pg: their normalisation is
//     over all alphas, :686-725), then w_l = sum_m gp[snp][0][m] pG[0][l][m], three numbers per entry.  A marker without
//     genotypes gets w = (1, 1, 1): its row in the device copy of gp is (1, 0, 0) (demux_gp_neutral_rows), so its factor is
//     exactly 1 for every sample and the sweep has no branch.
//   * sng_sweep_kernel, lane = sample: f = g_0 w_0 + g_1 w_1 + g_2 w_2 per (entry, sample), multiplied into a product kept
//     as mantissa x 2^exponent (prodacc), one log per (cell part, sample).  A wave is one work unit: a part of a cell
//     (at most 2048 entries) x a block of 64 samples, the entry wave-uniform.  Below 64 samples a wave holds
//     G = 64 / VH entries side by side (VH = V rounded up to a power of two, lane = (entry slot, sample)) and the G partial
//     products of a sample are multiplied in a fixed butterfly at the end.
//   * table_join_kernel (table_call.hpp): the logs of the parts of a long cell, added in entry order.
// Which cell goes into which batch, its cut into parts (fixed parts of 2048 entries) and the order of the work items
// are table_plan.hpp's; the host body that drives the plan is table_call.hpp's table_batches, whose customer this unit
// is (its cost: the slab rows of a cell; one bracket in its timing slot, open from the weight kernel on).  The cut of a cell depends on the cell alone and every reduction tree is fixed: the table is
// bit-identical from run to run, for any slab budget, on one device, on a group and through the sharded driver.
//
// Memory: [nnz][3] weights and a slab of the table.  When the table exceeds the budget (the streamed call's: 4 GiB or a
// third of the device, MUXGL_DEMUX_SLAB_MB) the cells are swept in batches (table_call.hpp has the protocol).
#include <algorithm>
#include <vector>

#include "demux_entry.hpp"
#include "table_call.hpp"

namespace {

constexpr int SNG_UNR = 8;          // entries per lane between two renormalisations, all of their loads in flight: a
                                    // factor is >= ~1e-11 (pG >= 1e-10 / (1 + 1e-10)), eight cannot underflow

using sng_item = table_plan::item;  // the entries [e0, e1) of one cell, result row `row` of the slab

template <int NA>
__global__ void __launch_bounds__(256)
    sng_weight_kernel(int64_t nnz, const int32_t* __restrict__ entry_snp, const int64_t* __restrict__ entry_rptr,
                      const uint8_t* __restrict__ reads, const double* __restrict__ lut_g, demux_grid al,
                      const double* __restrict__ gp, const uint8_t* __restrict__ has_gp, int V, double* __restrict__ wt) {
  __shared__ double lut[384];
  for (int i = threadIdx.x; i < 384; i += 256) lut[i] = lut_g[i];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const int32_t s = entry_snp[e];
  double w0 = 1.0, w1 = 1.0, w2 = 1.0;
  if (has_gp[s]) {  // (no genotypes: the reference skips the marker, :733)
    const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
    uint32_t first4 = 0;
    for (int64_t k = 0; k < 4 && r0 + k < r1; ++k) first4 |= (uint32_t)reads[r0 + k] << (8 * (int)k);
    double pG[NA * 9];
    row_entry_pg<NA>(reads, r0, r1, first4, al.a, lut, pG);
    const double* g = gp + (size_t)s * V * 3;  // sample 0's triple
    const double h0 = g[0], h1 = g[1], h2 = g[2];
    w0 = fma(h2, pG[2], fma(h1, pG[1], h0 * pG[0]));
    w1 = fma(h2, pG[5], fma(h1, pG[4], h0 * pG[3]));
    w2 = fma(h2, pG[8], fma(h1, pG[7], h0 * pG[6]));
  }
  double* o = wt + (size_t)e * 3;
  o[0] = w0;
  o[1] = w1;
  o[2] = w2;
}

// grid: ceil(n_items * nblk / 4) workgroups of four waves; wave u <-> (item u / nblk, sample block u % nblk), so the
// waves of a workgroup walk the same entries and read neighbouring pieces of the same genotype rows.
template <int VH>
__global__ void __launch_bounds__(256)
    sng_sweep_kernel(int64_t n_units, int nblk, const sng_item* __restrict__ items, const int32_t* __restrict__ entry_snp,
                     const double* __restrict__ wt, const double* __restrict__ gp, int V, double* __restrict__ slab) {
  constexpr int G = 64 / VH;  // entries side by side in a wave
  const int64_t u = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (u >= n_units) return;
  const int64_t it = u / nblk;
  const int blk = (int)(u - it * nblk);
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / VH;  // entry slot of the lane
  const int j = G == 1 ? blk * 64 + lane : lane % VH;
  const bool jl = j < V;
  const size_t jo = (size_t)(jl ? j : V - 1) * 3;
  const int64_t e0 = items[it].e0, e1 = items[it].e1;
  const size_t V3 = (size_t)V * 3;

  double acc = 1.0;
  int32_t ex = 0;
  for (int64_t eb = e0; eb < e1; eb += (int64_t)SNG_UNR * G) {
    double f[SNG_UNR];
#pragma unroll
    for (int i = 0; i < SNG_UNR; ++i) {
      const int64_t e = eb + (int64_t)i * G + sub;
      const bool ok = e < e1;
      const int64_t ec = ok ? e : e1 - 1;  // (a slot past the end reads the last entry again and counts as 1)
      const double* w = wt + (size_t)ec * 3;
      const double* g = gp + (size_t)entry_snp[ec] * V3 + jo;
      const double v = fma(g[2], w[2], fma(g[1], w[1], g[0] * w[0]));
      f[i] = ok ? v : 1.0;
    }
#pragma unroll
    for (int i = 0; i < SNG_UNR; ++i) acc *= f[i];
    prodacc_renorm(acc, ex);
  }
  if (G > 1) {  // the G partial products of a sample, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
    for (int off = VH; off < 64; off <<= 1) {
      acc *= __shfl_xor(acc, off, 64);
      ex += __shfl_xor(ex, off, 64);
    }
  }
  if (jl && sub == 0) slab[(size_t)items[it].row * V + j] = prodacc_log(acc, ex);
}

template <int NA>
int launch_weights(muxgl_handle* h, const demux_grid& al, double* d_wt) {
  hipLaunchKernelGGL((sng_weight_kernel<NA>), dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, h->stream, h->nnz,
                     h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, al, h->d_gp, h->d_has_gp, h->V, d_wt);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int weights_dispatch(muxgl_handle* h, int A, const demux_grid& al, double* d_wt) {
#define CALL_W(N) launch_weights<N>(h, al, d_wt)
  DISPATCH_NA(A, CALL_W);
#undef CALL_W
}

template <int VH>
void launch_sweep(muxgl_handle* h, int64_t n_items, int nblk, const sng_item* d_items, const double* d_wt, double* d_slab) {
  const int64_t n_units = n_items * nblk;
  hipLaunchKernelGGL((sng_sweep_kernel<VH>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, nblk,
                     d_items, h->d_entry_snp, d_wt, h->d_gp, h->V, d_slab);
}

}  // namespace

int demux_singlets_run(muxgl_handle* h, const muxgl_demux_params* p, double* sng) {
  const int V = h->V, A = p->n_alpha, nblk = (V + 63) / 64, VH = lane_width(V);
  const table_call call = {"muxgl_demux_singlets", "MUXGL_DEMUX_SLAB_MB", table_plan::fixed_begin, (double)nblk, 0.0, 0.0,
                           table_plan::shape(V, "samples"), ""};
  table_batches<table_plan::cut> tb;
  if (tb.plan(h, call, [V](int64_t, int64_t np) { return table_plan::singlet_bytes(np, V); })) return 1;
  const demux_grid al = demux_grid_of(p);

  dev_tmp<double> d_wt, d_slab;
  if (dev_alloc(h, &d_wt.p, (size_t)h->nnz * 3)) return 1;
  if (dev_alloc(h, &d_slab.p, (size_t)tb.bt.max_rows * V)) return 1;
  tic(h, MUXGL_T_DEMUX_SINGLETS);
  if (h->nnz > 0 && weights_dispatch(h, A, al, d_wt.p)) return 1;  // the whole pileup's, once per call
  return tb.run(h, table_slot_timer{MUXGL_T_DEMUX_SINGLETS},
      [&](const table_batch<table_plan::cut>& b) {
#define CALL_S(W) launch_sweep<W>(h, b.n_items, nblk, b.d_items, d_wt.p, d_slab.p)
        DISPATCH_WIDTH(VH, CALL_S);
#undef CALL_S
        HIPCHK(h, hipGetLastError());
        return table_join(h, b, V, d_slab.p);
      },
      [&](const table_batch<table_plan::cut>& b) {
        HIPCHK(h, hipMemcpyAsync(sng + (size_t)b.c0 * V, d_slab.p, sizeof(double) * (size_t)b.nc() * V, hipMemcpyDeviceToHost, h->stream));
        return 0;
      });
}
