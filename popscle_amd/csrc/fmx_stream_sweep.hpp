// fmx_stream_sweep.hpp -- the sweep of the streamed freemuxlet paths: one group of (cells x 64 x 64 blocks of clusters,
// X >= Y) into slab[cell][block][slot][lane], the launch that picks its flags, and the walk over a block's valid
// hypotheses.  Shared by fmx_stream.hip (the E-step and call) and fmx_incl.hip (the per-cluster marginals); each includes it
// into its own anonymous namespace, so each translation unit keeps its own copy of the kernels.  Arithmetic, the mapping of
// lanes and slots and the cut of long cells: fmx_stream.hip's header.
#pragma once
#include <vector>

#include "common.hpp"
#include "stream_plan.hpp"

namespace {

constexpr int CB = 64;              // clusters per side of a block
constexpr int SLAB = CB * CB;       // doubles per (cell, block) of the slab: [slot][lane]
constexpr int64_t PART = 2048;      // entries per part of a long cell (demux_wave_plan's WAVE_ITEM)

__device__ __forceinline__ bool lin_bit(const uint32_t* __restrict__ lin, int64_t e) { return (lin[e >> 5] >> (e & 31)) & 1u; }

// products of one part [e0, e1) for the lane's NS slots; DIAG: partner pk[i] per lane (rotations), else wave-uniform
template <int NS, bool DIAG, bool LIN, bool PIV>
__device__ __forceinline__ void sweep_part(int64_t e0, int64_t e1, const int32_t* __restrict__ entry_snp,
                                           const double* __restrict__ egls, const uint32_t* __restrict__ lin,
                                           const double* __restrict__ cgp, int K3, int jo, const int (&ko)[NS], bool live,
                                           const bool (&live2)[NS], double (&acc)[NS], int32_t (&ex)[NS], double& accS,
                                           int32_t& exS) {
  int cnt = 0;
  auto renorm = [&]() {
    if (++cnt == 16) {  // a factor is >= ~1e-13 (clamped likelihoods, mixed posteriors): sixteen cannot underflow
      cnt = 0;
#pragma unroll
      for (int i = 0; i < NS; ++i) prodacc_renorm(acc[i], ex[i]);
      prodacc_renorm(accS, exS);
    }
  };
  if (DIAG && LIN) {  // linear entries first (fw_walk_lin)
    for (int64_t e = e0; e < e1; ++e) {
      if (!lin_bit(lin, e)) continue;
      const double* q = egls + (size_t)e * 9;
      const double rc0 = q[0], u1 = q[1] - q[0];
      const double* row = cgp + (size_t)entry_snp[e] * K3;
      const double c0r = live ? fma(2.0, row[jo + 2], row[jo + 1]) : 0.0;  // E of the lane's cluster (fw_ce_kernel)
      const double u0 = fma(u1, c0r, rc0);
      accS *= fma(2.0 * u1, c0r, rc0);
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const double r0 = live2[i] ? fma(2.0, row[ko[i] + 2], row[ko[i] + 1]) : 0.0;
        acc[i] *= fma(u1, r0, u0);
      }
      renorm();
    }
  }
  for (int64_t e = e0; e < e1; ++e) {  // the others (fw_walk_gen)
    if (DIAG && LIN && lin_bit(lin, e)) continue;
    const double* q = egls + (size_t)e * 9;
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5], q6 = q[6], q7 = q[7], q8 = q[8];
    const double* row = cgp + (size_t)entry_snp[e] * K3;
    const double g0 = live ? row[jo] : 1.0, g1 = live ? row[jo + 1] : 0.0, g2 = live ? row[jo + 2] : 0.0;
    const double u0 = fma(g2, q6, fma(g1, q3, g0 * q0));
    const double u1 = fma(g2, q7, fma(g1, q4, g0 * q1));
    const double u2 = fma(g2, q8, fma(g1, q5, g0 * q2));
    if (DIAG) accS *= fma(g2, q8, fma(g1, q4, g0 * q0));
    if (DIAG && PIV) {
      const bool p0 = u0 <= u1 && u0 <= u2, p1 = !p0 && u1 <= u2;
      const double up = p0 ? u0 : (p1 ? u1 : u2);
      const double da = (p0 ? u1 : u0) - up;
      const double db = ((p0 || p1) ? u2 : u1) - up;
      const int ca = p0 ? 1 : 0, cb = (p0 || p1) ? 2 : 1;
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const double ra = live2[i] ? row[ko[i] + ca] : (ca == 0 ? 1.0 : 0.0);
        const double rb = live2[i] ? row[ko[i] + cb] : 0.0;
        acc[i] *= fma(rb, db, fma(ra, da, up));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NS; ++i) {
        const double r0 = live2[i] ? row[ko[i]] : 1.0, r1 = live2[i] ? row[ko[i] + 1] : 0.0,
                     r2 = live2[i] ? row[ko[i] + 2] : 0.0;
        acc[i] *= fma(r2, u2, fma(r1, u1, r0 * u0));
      }
    }
    renorm();
  }
}

// the lane's NS slots of one (cell, block) over the cell's parts, written to the slab
template <int NS, bool DIAG, bool LIN, bool PIV>
__device__ __forceinline__ void sweep_block(int64_t b, int64_t n, int X, int Y, int w, int j,
                                            const int32_t* __restrict__ entry_snp, const double* __restrict__ egls,
                                            const uint32_t* __restrict__ lin, const double* __restrict__ cgp, int K,
                                            double* __restrict__ out) {
  const int sj = CB * X + j;
  const bool live = sj < K;
  const int jo = (live ? sj : K - 1) * 3;
  int ko[NS];
  bool live2[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int sk = DIAG ? CB * X + ((j - (NS * w + i + 1)) & 63) : CB * Y + NS * w + i;
    live2[i] = sk < K;
    ko[i] = (live2[i] ? sk : K - 1) * 3;
  }
  double sum[NS], sumS = 0.0;
#pragma unroll
  for (int i = 0; i < NS; ++i) sum[i] = 0.0;
  const int64_t parts = n > PART ? (n + PART - 1) / PART : 1;
  for (int64_t q = 0; q < parts; ++q) {
    double acc[NS], accS = 1.0;
    int32_t ex[NS], exS = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 1.0, ex[i] = 0;
    sweep_part<NS, DIAG, LIN, PIV>(b + n * q / parts, b + n * (q + 1) / parts, entry_snp, egls, lin, cgp, K * 3, jo, ko,
                                   live, live2, acc, ex, accS, exS);
    if (q == 0) {
#pragma unroll
      for (int i = 0; i < NS; ++i) sum[i] = prodacc_log(acc[i], ex[i]);
      sumS = prodacc_log(accS, exS);
    } else {  // (fmx_wave_combine_kernel: the parts' rows added in entry order)
#pragma unroll
      for (int i = 0; i < NS; ++i) sum[i] += prodacc_log(acc[i], ex[i]);
      sumS += prodacc_log(accS, exS);
    }
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) out[(NS * w + i) * CB + j] = sum[i];
  if (DIAG && w == 0) out[32 * CB + j] = sumS;
}

// Sweep of one group: grid = (cells of the group, blocks of the group), 4 waves.  Cell = cells[c0 + x] when a cell list
// is given (the rows of the exact pass), else c0 + x.  slab[x][z][slot][lane].
template <bool LIN, bool PIV>
__global__ void __launch_bounds__(256)
    fmx_stream_sweep_kernel(int64_t c0, const int32_t* __restrict__ cells, int32_t b0, const int32_t* __restrict__ blocks,
                            const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                            const double* __restrict__ egls, const uint32_t* __restrict__ lin,
                            const double* __restrict__ cgp, int K, double* __restrict__ slab) {
  const int64_t c = cells ? (int64_t)cells[c0 + blockIdx.x] : c0 + blockIdx.x;
  const int64_t e0 = cell_ptr[c], n = cell_ptr[c + 1] - e0;
  const int bz = blocks[b0 + (int)blockIdx.y];
  const int X = bz >> 16, Y = bz & 0xffff;
  const int j = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* out = slab + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * SLAB;
  if (X == Y)
    sweep_block<8, true, LIN, PIV>(e0, n, X, Y, w, j, entry_snp, egls, lin, cgp, K, out);
  else
    sweep_block<16, false, false, false>(e0, n, X, Y, w, j, entry_snp, egls, lin, cgp, K, out);
}

// the valid hypotheses of thread (w, j) in block (X, Y): f(position, value, singlet)
template <typename F>
__device__ __forceinline__ void block_hyps(int X, int Y, int w, int j, int K, const double* __restrict__ in, F&& f) {
  const int sj = CB * X + j;
  if (sj >= K) return;
  if (X == Y) {
    for (int i = 0; i < 8; ++i) {
      const int t = 8 * w + i + 1, kk = (j - t) & 63, sk = CB * X + kk;
      if (sk >= K || (t == 32 && j < kk)) continue;  // rotation 32 meets every pair twice: the higher lane writes
      const int hi = sj > sk ? sj : sk, lo = sj > sk ? sk : sj;
      f(hi * (hi + 1) / 2 + lo, in[(t - 1) * CB + j], false);
    }
    if (w == 0) f(sj * (sj + 1) / 2 + sj, in[32 * CB + j], true);
  } else {
    for (int i = 0; i < 16; ++i) {
      const int sk = CB * Y + 16 * w + i;
      if (sk >= K) break;
      f(sj * (sj + 1) / 2 + sk, in[(16 * w + i) * CB + j], false);
    }
  }
}

// the blocks (X, Y), X >= Y, in sweep order, as X << 16 | Y
std::vector<int32_t> block_list(int K) { return stream_plan::block_list((K + CB - 1) / CB, true, 1 << 16); }

int sweep_launch(muxgl_handle* h, int64_t c0, const int32_t* d_cells, int64_t nc, int32_t b0, int32_t nb,
                 const int32_t* d_blocks, double* d_slab) {
  const bool lin = h->d_flin && !(h->flags & MUXGL_FLAG_NO_LINEAR_ENTRIES);
  const bool piv = !(h->flags & MUXGL_FLAG_NO_PIVOT_SUMS);
#define SW(L, P)                                                                                                       \
  hipLaunchKernelGGL((fmx_stream_sweep_kernel<L, P>), dim3((unsigned)nc, (unsigned)nb), dim3(256), 0, h->stream, c0,    \
                     d_cells, b0, d_blocks, h->d_cell_ptr, h->d_entry_snp, h->d_egls, h->d_flin, h->d_cgp, h->K, d_slab)
  if (lin && piv) SW(true, true);
  else if (lin) SW(true, false);
  else if (piv) SW(false, true);
  else SW(false, false);
#undef SW
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // namespace
