// demux_stream_sweep.hpp -- the sweep of the streamed demuxlet paths: one group of (cells x 64 x 64 blocks of the pair
// matrix) into slab[cell][block][n][k][j].  Shared by demux_stream.hip (the call) and demux_incl.hip (the per-sample
// marginals); each includes it into its own anonymous namespace, so each translation unit keeps its own copy of the kernels.
// Arithmetic, mapping and why these are not the wave kernels of demux_wave.hip: demux_stream.hip's header.
#pragma once
#include "common.hpp"

namespace {

constexpr int SBLK = 64;                     // samples per side of a block of the pair matrix
constexpr int SLAB_DOUBLES = SBLK * SBLK;    // per alpha and block: [k][j]

// Sweep of one group: grid = (cells of the group, 64 / (4 KT) sub-tiles, blocks of the group).  Lane j of wave w owns
// sample jbase + j and the KT partners kbase + 4 KT y + KT w + i; NA >= A - 1 accumulators per pair (alphas 1 .. A - 1),
// and lanes of the sub-tile holding k = 0 also the singlet slot (j, 0, alpha 0) (:806,828).
// slab[cell - c0][block of group][n][k][j].  Markers without genotypes are skipped (:733), wave-uniformly.
template <int NA, int KT>
__global__ void __launch_bounds__(256)
    stream_sweep_kernel(int64_t c0, int32_t b0, const int32_t* __restrict__ blocks, int nblk,
                        const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                        const double* __restrict__ pg, const uint8_t* __restrict__ has_gp, const double* __restrict__ gp,
                        int V, int nAlpha, double* __restrict__ slab) {
  const int64_t c = c0 + blockIdx.x;
  const int64_t e0 = cell_ptr[c], e1 = cell_ptr[c + 1];
  if (e0 == e1) return;
  const int b = blocks[b0 + (int)blockIdx.z];
  const int X = b / nblk, Y = b - X * nblk;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = SBLK * X + lane;
  const int kk0 = 4 * KT * (int)blockIdx.y + KT * w;  // first partner of the wave, inside the block
  const int kb = SBLK * Y + kk0;
  const bool jl = j < V;
  const bool with_singlet = kb == 0;  // wave-uniform
  const int V3 = V * 3;
  const int PG = nAlpha * 9;
  const int jo = (jl ? j : V - 1) * 3;
  int ko[KT];  // (no sample: any valid row; the fold never reads those slots)
#pragma unroll
  for (int i = 0; i < KT; ++i) ko[i] = (kb + i < V ? kb + i : V - 1) * 3;

  double acc[KT][NA], accS = 1.0;
  int32_t ex[KT][NA], exS = 0;
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[i][a] = 1.0, ex[i][a] = 0;

  int cnt = 0;
  for (int64_t e = e0; e < e1; ++e) {
    const int32_t s = entry_snp[e];
    if (!has_gp[s]) continue;
    const double* row = gp + (size_t)s * V3;
    const double* q = pg + (size_t)e * PG;
    const double g0 = jl ? row[jo] : 1.0, g1 = jl ? row[jo + 1] : 0.0, g2 = jl ? row[jo + 2] : 0.0;
    double u[NA][3];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const double* qa = q + (size_t)(a + 1 < nAlpha ? a + 1 : 0) * 9;
#pragma unroll
      for (int m = 0; m < 3; ++m) u[a][m] = fma(g2, qa[6 + m], fma(g1, qa[3 + m], g0 * qa[m]));
    }
    if (with_singlet) {  // llksAB[j][0][0]: alpha 0 against sample 0's triple
      const double v0 = fma(g2, q[6], fma(g1, q[3], g0 * q[0]));
      const double v1 = fma(g2, q[7], fma(g1, q[4], g0 * q[1]));
      const double v2 = fma(g2, q[8], fma(g1, q[5], g0 * q[2]));
      accS *= fma(row[2], v2, fma(row[1], v1, row[0] * v0));
    }
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      const double h0 = row[ko[i]], h1 = row[ko[i] + 1], h2 = row[ko[i] + 2];
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[i][a] *= fma(h2, u[a][2], fma(h1, u[a][1], h0 * u[a][0]));  // :738-746
    }
    if (++cnt == 16) {  // every factor is >= ~1e-11: sixteen of them cannot underflow
      cnt = 0;
#pragma unroll
      for (int i = 0; i < KT; ++i)
#pragma unroll
        for (int a = 0; a < NA; ++a) prodacc_renorm(acc[i][a], ex[i][a]);
      prodacc_renorm(accS, exS);
    }
  }

  double* out = slab + ((size_t)blockIdx.x * gridDim.z + blockIdx.z) * nAlpha * SLAB_DOUBLES;
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int a = 0; a < NA; ++a)
      if (a + 1 < nAlpha) out[((size_t)(a + 1) * SBLK + kk0 + i) * SBLK + lane] = prodacc_log(acc[i][a], ex[i][a]);
  if (with_singlet) out[lane] = prodacc_log(accS, exS);  // slot (n = 0, k = 0)
}

template <int NA, int KT>
void launch_sweep(muxgl_handle* h, int64_t c0, int64_t nc, int32_t b0, int32_t nb, const int32_t* d_blocks, int nblk,
                  const double* d_pg, int A, double* d_slab) {
  hipLaunchKernelGGL((stream_sweep_kernel<NA, KT>), dim3((unsigned)nc, (unsigned)(SBLK / (4 * KT)), (unsigned)nb),
                     dim3(256), 0, h->stream, c0, b0, d_blocks, nblk, h->d_cell_ptr, h->d_entry_snp, d_pg, h->d_has_gp,
                     h->d_gp, h->V, A, d_slab);
}

int sweep_dispatch(muxgl_handle* h, int64_t c0, int64_t nc, int32_t b0, int32_t nb, const int32_t* d_blocks, int nblk,
                   const double* d_pg, int A, double* d_slab) {
  const int na = A - 1;  // alphas 1 .. A - 1; none: the singlet slots alone (the kernel writes no pair slot)
#define SW(NA, KT) launch_sweep<NA, KT>(h, c0, nc, b0, nb, d_blocks, nblk, d_pg, A, d_slab)
  if (na <= 1) SW(1, 16);
  else if (na <= 2) SW(2, 8);
  else if (na <= 4) SW(4, 8);
  else if (na <= 6) SW(6, 4);
  else if (na <= 8) SW(8, 4);
  else if (na <= 12) SW(12, 2);
  else SW(15, 2);
#undef SW
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // namespace
