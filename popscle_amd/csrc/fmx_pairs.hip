// fmx_pairs.hip -- muxgl_fmx_cluster_pairs: every pair of freemuxlet's cluster pileups scored as one donor against two
// unrelated donors, the pairwise Bayes factor of freemuxlet-old (cmd_cram_freemuxlet.cpp:186-221) with clusters in the place
// of droplets.  It is muxgl_fmx_match_donors (fmx_match.hip) with a second cluster in the donor's place.
//
//   U(k)       = { s : the cluster has reads at s },  L_k,g = cgls[k][s][4 g],  p = ((1-af)^2, 2 af (1-af), af^2)   (:200-203)
//   nsnps[a,b] = |U(a) n U(b)|
//   llk2[a,b]  = sum over s in U(a) n U(b) of log( sum_g p_g L_a,g L_b,g )                                   (lk2, :206)
//   llk0[a,b]  = sum over the same s of log( (sum_g p_g L_a,g) (sum_g p_g L_b,g) )                            (lk0, :208)
// for a > b, stored at a (a - 1) / 2 + b.
//
// Inputs, all resident: d_cgls [K][S][9], d_af, and the entries with their cells' clusters.  The read counts of the cluster
// pileups are not kept current by every M-step path (muxgl_fmx_get_cluster_pileup recounts them), so membership in U is
// taken from the entries, by fmm_count_kernel's rule, as one bit per (SNP, cluster).
//
// Kernels:
//   * fcp_member_kernel, lane = entry: the bit of (entry_snp, cluster of the entry's cell) in memb [S][W] 64-bit words
//     (W = ceil(K / 64)) where the entry has reads, by a 64-bit atomic OR (order-independent).
//   * fcp_pack_kernel: the partner rows of a block Y of 64 clusters, w_g = p_g L_b,g, as [S][64][3]: a SNP's rows are one
//     contiguous 1536-byte stretch.  d_cgls is cluster-major, so the kernel reads it along S (32 consecutive SNPs of a
//     cluster per half wave) and transposes a 32 x 64 x 3 tile through LDS; what that buys is coalesced reads AND
//     coalesced writes, where lane = cluster alone would read at a stride of 72 S bytes.  A lane at or beyond K packs the
//     last cluster again: finite, never stored by the sweep.
//   * fcp_sweep_kernel<KH, T>, lane = partner b.  A wave is one work unit: a part of PART consecutive SNPs x a tile of T
//     row clusters a x the partner block.  The SNP is wave-uniform (KH = 64), so the three L_a,g, both membership words
//     and af[s] come through uniform loads.  Per (SNP, a, b): lk2 = w_0 L_a,0 + w_1 L_a,1 + w_2 L_a,2 and lk0 = m_a (w_0 +
//     w_1 + w_2), m_a = sum_g p_g L_a,g once per (SNP, a); each multiplied into a product kept as mantissa x 2^exponent
//     (prodacc), a SNP outside U(a) n U(b) a factor of exactly 1 by a select (no branch), an integer count beside them,
//     one log per (a, part, lane) and product.  Below 64 clusters a wave holds G = 64 / KH SNPs side by side (KH = K
//     rounded up to a power of two) and the G partial products of a pair meet in fmm_sweep_kernel's fixed butterfly.
//     No LDS.
//   * fcp_join_kernel: the logs of the parts of a pair, added in ascending SNP order, into the triangle on the device.
// Only units that hold a pair b < a are launched (pairs_plan.hpp); lanes with b >= a or b >= K compute and do not store.
// The cut into parts depends on S alone, a pair's products do not depend on its tile mates or the batch, the butterfly
// and the join are fixed: all three outputs are bit-identical from call to call, for any slab budget and any tile size.
//
// Memory beyond the inputs.  Fixed: memb (8 W S bytes), one packed partner block (1536 S bytes), the triangle (20 bytes
// per pair).  Inside the streamed E-step's budget (MUXGL_FMX_SLAB_MB): per row cluster of a batch, parts x 64 lanes x (two
// logs, a count).  Nothing proportional to K^2 S.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "pairs_plan.hpp"

namespace {

constexpr int64_t FCP_PART = pairs_plan::PART;
// SNPs per lane between two renormalisations, their loads in flight.  A factor is a combination, with weights p_g that
// sum to 1, of products of two diagonal elements of cluster pileups, which leave the merge clamped to 1e-6 and divided by
// a sum <= 1 + 9e-6 (sc_drop_seq.h:92-100): every lk2 and lk0 is >= (9.9999e-7)^2 > 2^-40 and <= 1, for any af in [0, 1]
// (af = 0 or 1 leaves one term of weight 1).  A mantissa in [0.5, 1) times eight factors is >= 2^-321: normal, a long way
// above 2^-1022.  A factor of exactly 0 would make the product 0 and the log -inf; frexp(0) = 0, so no NaN on the way.
constexpr int FCP_UNR = 8;

typedef unsigned long long u64;

__global__ void __launch_bounds__(256)
    fcp_member_kernel(int64_t nnz, int K, int W, const int32_t* __restrict__ entry_snp, const int32_t* __restrict__ entry_cell,
                      const int32_t* __restrict__ clust, const int32_t* __restrict__ ecnt, u64* __restrict__ memb) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t k = clust[entry_cell[e]];
    if (k < 0 || k >= K || ecnt[(size_t)e * 3] <= 0) continue;
    atomicOr(memb + (size_t)entry_snp[e] * W + (k >> 6), (u64)1 << (k & 63));
  }
}

// grid: ceil(S / 32) workgroups; packed[s][j][g] = p_g(s) cgls[min(64 Y + j, K - 1)][s][4 g]
constexpr int FCP_PS = 32;          // SNPs of a pack tile
constexpr int FCP_PROW = 192 + 1;   // doubles of a SNP's row in LDS (+1: the 32 SNPs of a half wave on 32 banks)
__global__ void __launch_bounds__(256)
    fcp_pack_kernel(int64_t S, int K, int Y, const double* __restrict__ cgls, const double* __restrict__ af,
                    double* __restrict__ packed) {
  __shared__ double tile[FCP_PS * FCP_PROW];
  const int64_t s0 = (int64_t)blockIdx.x * FCP_PS;
  const int sl = threadIdx.x & (FCP_PS - 1);
  const int64_t s = s0 + sl < S ? s0 + sl : S - 1;
  const double a = af[s], b = 1.0 - a;
  const double p0 = b * b, p1 = 2.0 * a * b, p2 = a * a;  // gps of :200-203
  for (int j = threadIdx.x / FCP_PS; j < 64; j += 256 / FCP_PS) {
    const int k = 64 * Y + j < K ? 64 * Y + j : K - 1;
    const double* L = cgls + ((size_t)k * S + (size_t)s) * 9;
    double* t = tile + sl * FCP_PROW + j * 3;
    t[0] = p0 * L[0];
    t[1] = p1 * L[4];
    t[2] = p2 * L[8];
  }
  __syncthreads();
  const int64_t ns = S - s0 < FCP_PS ? S - s0 : FCP_PS;
  double* out = packed + (size_t)s0 * 192;
  for (int i = threadIdx.x; i < (int)ns * 192; i += 256) out[i] = tile[(i / 192) * FCP_PROW + i % 192];
}

// grid: ceil(n_units / 4) workgroups of four waves; wave u <-> (part, tile) = (u / ntile, tile_lo + u % ntile), part-major
// so that the waves resident at one time walk the same stretch of SNPs.  Tile i holds the row clusters i T .. i T + T - 1;
// r0 is the first row cluster of the batch, whose part logs are part2 / part0 / partn [row - r0][NP][64].
template <int KH, int T>
__global__ void __launch_bounds__(256)
    fcp_sweep_kernel(int64_t n_units, int ntile, int tile_lo, int Y, int r0, int64_t S, int K, int W, int NP,
                     const double* __restrict__ cgls, const u64* __restrict__ memb, const double* __restrict__ packed,
                     const double* __restrict__ af, double* __restrict__ part2, double* __restrict__ part0,
                     int32_t* __restrict__ partn) {
  constexpr int G = 64 / KH;  // SNPs side by side in a wave
  const int64_t u = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (u >= n_units) return;
  const int tile = tile_lo + (int)(u % ntile);
  const int64_t p = u / ntile;
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / KH;  // SNP slot of the lane
  const int j = G == 1 ? lane : lane % KH;  // partner lane within the block
  const int64_t s0 = p * FCP_PART, s1 = s0 + FCP_PART < S ? s0 + FCP_PART : S;

  const double* cg[T];
  int aw[T], ab[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int a = tile * T + t < K ? tile * T + t : K - 1;  // (a slot past K reads the last cluster again)
    cg[t] = cgls + (size_t)a * S * 9;
    aw[t] = a >> 6;
    ab[t] = a & 63;
  }
  double acc2[T], acc0[T];
  int32_t ex2[T], ex0[T], cnt[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc2[t] = 1.0, acc0[t] = 1.0, ex2[t] = 0, ex0[t] = 0, cnt[t] = 0;

  for (int64_t sb = s0; sb < s1; sb += (int64_t)FCP_UNR * G) {
    double w0[FCP_UNR], w1[FCP_UNR], w2[FCP_UNR], ws[FCP_UNR], q0[FCP_UNR], q1[FCP_UNR], q2[FCP_UNR];
    int64_t sc[FCP_UNR];
    bool okb[FCP_UNR];
#pragma unroll
    for (int i = 0; i < FCP_UNR; ++i) {
      const int64_t s = sb + (int64_t)i * G + sub;
      const bool ok = s < s1;
      sc[i] = ok ? s : s1 - 1;  // (a slot past the end reads the last SNP again and counts as 1)
      okb[i] = ok & (((memb[(size_t)sc[i] * W + Y] >> j) & 1) != 0);  // (& not &&: the load is issued, nothing branches)
      const double* w = packed + (size_t)sc[i] * 192 + j * 3;
      w0[i] = w[0];
      w1[i] = w[1];
      w2[i] = w[2];
      ws[i] = w0[i] + w1[i] + w2[i];
      const double a = af[sc[i]], b = 1.0 - a;
      q0[i] = b * b;
      q1[i] = 2.0 * a * b;
      q2[i] = a * a;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int i = 0; i < FCP_UNR; ++i) {
        const double* L = cg[t] + (size_t)sc[i] * 9;
        const double l0 = L[0], l1 = L[4], l2 = L[8];
        const double ma = fma(q2[i], l2, fma(q1[i], l1, q0[i] * l0));
        const double lk2 = fma(w2[i], l2, fma(w1[i], l1, w0[i] * l0));
        const double lk0 = ma * ws[i];
        const bool in = okb[i] & (((memb[(size_t)sc[i] * W + aw[t]] >> ab[t]) & 1) != 0);
        acc2[t] *= in ? lk2 : 1.0;
        acc0[t] *= in ? lk0 : 1.0;
        cnt[t] += in ? 1 : 0;
      }
      prodacc_renorm(acc2[t], ex2[t]);
      prodacc_renorm(acc0[t], ex0[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (G > 1) {  // the G partial products of a pair, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
      for (int off = KH; off < 64; off <<= 1) {
        acc2[t] *= __shfl_xor(acc2[t], off, 64);
        ex2[t] += __shfl_xor(ex2[t], off, 64);
        acc0[t] *= __shfl_xor(acc0[t], off, 64);
        ex0[t] += __shfl_xor(ex0[t], off, 64);
        cnt[t] += __shfl_xor(cnt[t], off, 64);
      }
    }
    const int a = tile * T + t, b = 64 * Y + j;
    if (a < K && b < a && sub == 0) {  // (b < a < K)
      const size_t o = ((size_t)(a - r0) * NP + (size_t)p) * 64 + j;
      part2[o] = prodacc_log(acc2[t], ex2[t]);
      part0[o] = prodacc_log(acc0[t], ex0[t]);
      partn[o] = cnt[t];
    }
  }
}

// lane i <-> (row, j) = (i / 64, i % 64), the pair (a, b) = (r0 + row, 64 Y + j): tri[a (a - 1) / 2 + b] = part[row][0][j] +
// part[row][1][j] + ..., in this order
__global__ void __launch_bounds__(256)
    fcp_join_kernel(int64_t n, int Y, int r0, int K, int NP, const double* __restrict__ part2, const double* __restrict__ part0,
                    const int32_t* __restrict__ partn, double* __restrict__ tri2, double* __restrict__ tri0,
                    int32_t* __restrict__ trin) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t row = i >> 6;
  const int j = (int)(i & 63);
  const int64_t a = r0 + row, b = 64 * (int64_t)Y + j;
  if (a >= K || b >= a) return;
  const size_t q = (size_t)row * NP * 64 + j;
  double s2 = part2[q], s0 = part0[q];
  int32_t c = partn[q];
  for (int p = 1; p < NP; ++p) {
    s2 += part2[q + (size_t)p * 64];
    s0 += part0[q + (size_t)p * 64];
    c += partn[q + (size_t)p * 64];
  }
  const size_t o = (size_t)(a * (a - 1) / 2 + b);
  tri2[o] = s2;
  tri0[o] = s0;
  trin[o] = c;
}

struct fcp_args {
  int64_t n_units;
  int ntile, tile_lo, Y, r0;
  int64_t S;
  int K, W, NP;
  const double* cgls;
  const u64* memb;
  const double *packed, *af;
  double *part2, *part0;
  int32_t* partn;
};

template <int KH, int T>
void launch_sweep(muxgl_handle* h, const fcp_args& a) {
  hipLaunchKernelGGL((fcp_sweep_kernel<KH, T>), dim3((unsigned)((a.n_units + 3) / 4)), dim3(256), 0, h->stream, a.n_units,
                     a.ntile, a.tile_lo, a.Y, a.r0, a.S, a.K, a.W, a.NP, a.cgls, a.memb, a.packed, a.af, a.part2, a.part0,
                     a.partn);
}

template <int T>
void launch_width(muxgl_handle* h, int KH, const fcp_args& a) {
  switch (KH) {  // (no width 1, pairs_plan::lane_width: not common.hpp's DISPATCH_WIDTH)
    case 2: launch_sweep<2, T>(h, a); break;
    case 4: launch_sweep<4, T>(h, a); break;
    case 8: launch_sweep<8, T>(h, a); break;
    case 16: launch_sweep<16, T>(h, a); break;
    case 32: launch_sweep<32, T>(h, a); break;
    default: launch_sweep<64, T>(h, a); break;
  }
}

// row clusters per wave (DESIGN.md 4.2f has the measurement behind the default); MUXGL_FMX_PAIRS_TILE=4|8 for the probe,
// read at each call.  The outputs do not depend on it.
int pairs_tile() {
  const char* s = getenv("MUXGL_FMX_PAIRS_TILE");
  const int t = s ? atoi(s) : 0;
  return t == 4 || t == 8 ? t : 4;
}

int fmx_pairs_run(muxgl_handle* h, double* llk2, double* llk0, int32_t* nsnps, float* kernel_ms) {
  const int K = h->K;
  const int64_t S = h->S;
  const size_t npair = (size_t)K * (size_t)(K - 1) / 2;
  if (kernel_ms) *kernel_ms = 0.f;
  if ((!llk2 && !llk0 && !nsnps) || npair == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  if (S == 0) {  // no SNPs: U is empty for every cluster
    if (llk2) memset(llk2, 0, sizeof(double) * npair);
    if (llk0) memset(llk0, 0, sizeof(double) * npair);
    if (nsnps) memset(nsnps, 0, sizeof(int32_t) * npair);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // the cut of the call (pairs_plan.hpp): parts, lane width, partner blocks, row clusters of a batch
  const int NP = pairs_plan::parts(S);
  const int KH = pairs_plan::lane_width(K);
  const int NY = pairs_plan::blocks(K);
  const int W = (K + 63) / 64;
  const int rb_cap = pairs_plan::rows_per_batch(K, pairs_plan::bytes_per_row(NP), dev_slab_budget("MUXGL_FMX_SLAB_MB"));
  const int T = pairs_tile();
  if ((double)NP * ((rb_cap + T - 1) / T) / 4.0 >= 2147483647.0 || (double)rb_cap * 64.0 / 256.0 >= 2147483647.0)
    MUXGL_FAIL(h, "muxgl_fmx_cluster_pairs: a batch of %d row clusters exceeds one launch (lower MUXGL_FMX_SLAB_MB)", rb_cap);

  dev_tmp<u64> d_memb;
  dev_tmp<double> d_packed, d_part2, d_part0, d_tri2, d_tri0;
  dev_tmp<int32_t> d_partn, d_trin;
  const size_t part_n = (size_t)rb_cap * NP * 64;
  if (dev_alloc(h, &d_memb.p, (size_t)S * W) || dev_alloc(h, &d_packed.p, (size_t)S * 192) ||
      dev_alloc(h, &d_part2.p, part_n) || dev_alloc(h, &d_part0.p, part_n) || dev_alloc(h, &d_partn.p, part_n) ||
      dev_alloc(h, &d_tri2.p, npair) || dev_alloc(h, &d_tri0.p, npair) || dev_alloc(h, &d_trin.p, npair))
    return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, "muxgl_fmx_cluster_pairs")) return 1;

  if (ev.start(h)) return 1;
  HIPCHK(h, hipMemsetAsync(d_memb.p, 0, sizeof(u64) * (size_t)S * W, h->stream));
  if (h->nnz) {
    const int64_t blocks = std::min<int64_t>((h->nnz + 255) / 256, 16384);
    hipLaunchKernelGGL(fcp_member_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, h->nnz, K, W, h->d_entry_snp,
                       h->d_entry_cell, h->d_clust, h->d_ecnt, d_memb.p);
    HIPCHK(h, hipGetLastError());
  }
  for (int Y = 0; Y < NY; ++Y) {
    hipLaunchKernelGGL(fcp_pack_kernel, dim3((unsigned)((S + FCP_PS - 1) / FCP_PS)), dim3(256), 0, h->stream, S, K, Y, h->d_cgls,
                       h->d_af, d_packed.p);
    HIPCHK(h, hipGetLastError());
    for (int r0 = pairs_plan::first_row(Y); r0 < K; r0 += rb_cap) {
      const int r1 = std::min(K, r0 + rb_cap);
      const int tile_lo = std::max(pairs_plan::first_tile(Y, T), r0 / T), tile_hi = (r1 + T - 1) / T;
      fcp_args a = {(int64_t)NP * (tile_hi - tile_lo), tile_hi - tile_lo, tile_lo, Y, r0, S, K, W, NP, h->d_cgls, d_memb.p,
                    d_packed.p, h->d_af, d_part2.p, d_part0.p, d_partn.p};
      if (T == 8)
        launch_width<8>(h, KH, a);
      else
        launch_width<4>(h, KH, a);
      HIPCHK(h, hipGetLastError());
      const int64_t n = (int64_t)(r1 - r0) * 64;
      hipLaunchKernelGGL(fcp_join_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, Y, r0, K, NP, d_part2.p,
                         d_part0.p, d_partn.p, d_tri2.p, d_tri0.p, d_trin.p);
      HIPCHK(h, hipGetLastError());
    }
  }
  if (ev.stop(h)) return 1;
  if (llk2) HIPCHK(h, hipMemcpyAsync(llk2, d_tri2.p, sizeof(double) * npair, hipMemcpyDeviceToHost, h->stream));
  if (llk0) HIPCHK(h, hipMemcpyAsync(llk0, d_tri0.p, sizeof(double) * npair, hipMemcpyDeviceToHost, h->stream));
  if (nsnps) HIPCHK(h, hipMemcpyAsync(nsnps, d_trin.p, sizeof(int32_t) * npair, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ev.add();  // (*kernel_ms is 0 so far)
  return 0;
}

}  // namespace

extern "C" int muxgl_fmx_cluster_pairs(muxgl_handle* h, double* llk2, double* llk0, int32_t* nsnps, float* kernel_ms) {
  if (!h) return 1;
  MUXGL_NOT_FOR_GROUPS(h, "muxgl_fmx_cluster_pairs");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->col || h->role != MUXGL_ROLE_FULL)
    MUXGL_FAIL(h, "muxgl_fmx_cluster_pairs: not available on a slabbed handle (muxgl_fmx_set_column_slab): its cluster pileups "
                  "cover a SNP range only");
  if (!h->d_cell_ptr) MUXGL_FAIL(h, "muxgl_fmx_cluster_pairs: no pileup set (muxgl_set_pileup)");
  if (!h->fmx_prepared) MUXGL_FAIL(h, "muxgl_fmx_cluster_pairs: call muxgl_fmx_prepare first");
  if (h->K < 1 || !h->d_cgls) MUXGL_FAIL(h, "muxgl_fmx_cluster_pairs: no clusters set (muxgl_fmx_set_clusters)");
  if (h->fc0 != 0 || h->fc1 != h->C || h->fs0 != 0 || h->fs1 != h->S)
    MUXGL_FAIL(h, "muxgl_fmx_cluster_pairs: not available on a sharded handle (muxgl_fmx_set_shard): its cluster pileups "
                  "cover a SNP range only");
  return fmx_pairs_run(h, llk2, llk0, nsnps, kernel_ms);
}
