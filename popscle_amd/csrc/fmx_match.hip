// fmx_match.hip -- muxgl_fmx_match_donors: the cluster pileups of freemuxlet scored against the donors' genotypes, the
// singlet likelihood of demuxlet with a cluster in the place of a droplet.
//
//   U(k)      = { s : has_gp[s] != 0 and the cluster has reads at s }
//   ll [k][v] = sum over s in U(k) of log( L_0 gp[s][v][0] + L_1 gp[s][v][1] + L_2 gp[s][v][2] ),  L_g = cgls[k][s][4 g]
//   ll0[k]    = the same with the triple of an unrelated individual, ((1-af)^2, 2 af (1-af), af^2)   (gp0s, :388-390)
//   nsnps[k]  = |U(k)|
//
// Inputs, all resident: d_cgls [K][S][9] (the diagonal is what the E-step reads, cmd_cram_freemux2.cpp:402-404), d_gp
// [S][V][3] and d_has_gp of muxgl_demux_set_gp, d_af.  The read counts of the cluster pileups are not kept current by
// every M-step path (muxgl_fmx_get_cluster_pileup recounts them), so the call counts nreads of its batch of clusters
// into scratch of its own, with integer atomics (order-independent), and leaves d_ccnt alone.
//
// Kernels:
//   * fmm_count_kernel, lane = entry: nreads[k][s] of the clusters of the batch.
//   * fmm_sweep_kernel<VH, T, HWE>, lane = donor.  A wave is one work unit: a PART of FMM_PART consecutive SNPs x a tile of
//     T clusters x a block of 64 donors.  The SNP is wave-uniform, so the three L_g, the read count and has_gp[s] come
//     through uniform loads, and the donors' triples of a SNP are one contiguous 1536-byte stretch, read once for the T
//     clusters of the tile.  f = g_0 L_0 + g_1 L_1 + g_2 L_2 per (SNP, cluster, donor), multiplied into a product kept as
//     mantissa x 2^exponent (prodacc), a SNP outside U(k) a factor of exactly 1 by a select (no branch), one log per
//     (cluster, part, donor).  Below 64 donors a wave holds G = 64 / VH SNPs side by side (VH = V rounded up to a power of
//     two, lane = (SNP slot, donor)) and the G partial products of a donor are multiplied in a fixed butterfly.
//     HWE = true is the same sweep with the one "donor" of the unrelated individual, 64 SNPs side by side: ll0, and
//     nsnps as an integer sum beside it.
//   * fmm_join_kernel: the logs of the parts of a cluster, added in ascending SNP order.
// The cut into parts depends on S and FMM_PART alone, a cluster's products do not depend on its tile mates and every
// reduction tree is fixed: the outputs are bit-identical from call to call, for any slab budget and any tile size.
// Work units are ordered part-major (then donor block, then tile) so that the waves resident at one time walk the same
// stretch of SNPs: the four waves of a workgroup are four neighbouring tiles reading the same donor rows.
//
// Memory beyond the inputs, per cluster of a batch: parts x V logs, parts x (log, count) of the HWE sweep, S read counts
// and the V + 2 results; batches of clusters are sized to the streamed E-step's budget (4 GiB or a third of the device,
// MUXGL_FMX_SLAB_MB) and each is copied out before the next.  Nothing proportional to K x S x V.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "match_plan.hpp"

namespace {

constexpr int64_t FMM_PART = 2048;  // SNPs per part (the wave kernels' cut of a long cell)
// SNPs per lane between two renormalisations, their loads in flight.  A factor is a combination of a donor triple with
// the diagonal of a cluster pileup, whose elements leave the merge clamped to 1e-6 and divided by a sum <= 1 + 9e-6
// (sc_drop_seq.h:92-100): f >= 9.9999e-7 x (g_0 + g_1 + g_2).  A mantissa in [0.5, 1) times eight factors stays normal
// while every factor is >= 2^-127 = 5.9e-39, i.e. for triple sums down to 6e-33 (posteriors scaled to a total of 1e-20 are
// eleven decades inside).  A factor of exactly 0 makes the product 0 and the log -inf; frexp(0) = 0, so no NaN on the way.
constexpr int FMM_UNR = 8;

__global__ void __launch_bounds__(256)
    fmm_count_kernel(int64_t nnz, int64_t S, int k0, int kb, const int32_t* __restrict__ entry_snp,
                     const int32_t* __restrict__ entry_cell, const int32_t* __restrict__ clust,
                     const int32_t* __restrict__ ecnt, int32_t* __restrict__ nreads) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t k = clust[entry_cell[e]] - k0;
    if (k < 0 || k >= kb) continue;
    atomicAdd(nreads + (size_t)k * S + entry_snp[e], ecnt[(size_t)e * 3]);
  }
}

// grid: ceil(n_units / 4) workgroups of four waves; wave u <-> (part, donor block, tile) = (u / (nblk ntile),
// u / ntile % nblk, u % ntile).  cgls and nreads start at the first cluster of the batch (kb clusters); part is
// [kb][NP][V] (HWE: [kb][NP], with part_n beside it).
template <int VH, int T, bool HWE>
__global__ void __launch_bounds__(256)
    fmm_sweep_kernel(int64_t n_units, int ntile, int nblk, int64_t S, int kb, int NP, const double* __restrict__ cgls,
                     const int32_t* __restrict__ nreads, const uint8_t* __restrict__ has_gp, const double* __restrict__ gp,
                     const double* __restrict__ af, int V, double* __restrict__ part, int32_t* __restrict__ part_n) {
  constexpr int G = 64 / VH;  // SNPs side by side in a wave
  const int64_t u = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (u >= n_units) return;
  const int tile = (int)(u % ntile);
  const int64_t r = u / ntile;
  const int blk = (int)(r % nblk);
  const int64_t p = r / nblk;
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / VH;  // SNP slot of the lane
  const int j = G == 1 ? blk * 64 + lane : lane % VH;
  const bool jl = j < V;
  const size_t jo = (size_t)(jl ? j : V - 1) * 3;
  const size_t V3 = (size_t)V * 3;
  const int64_t s0 = p * FMM_PART, s1 = s0 + FMM_PART < S ? s0 + FMM_PART : S;

  const double* cg[T];
  const int32_t* cn[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int k = tile * T + t < kb ? tile * T + t : kb - 1;  // (a slot past the batch reads its last cluster again)
    cg[t] = cgls + (size_t)k * S * 9;
    cn[t] = nreads + (size_t)k * S;
  }
  double acc[T];
  int32_t ex[T], cnt[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 1.0, ex[t] = 0, cnt[t] = 0;

  for (int64_t sb = s0; sb < s1; sb += (int64_t)FMM_UNR * G) {
    double g0[FMM_UNR], g1[FMM_UNR], g2[FMM_UNR];
    int64_t sc[FMM_UNR];
    bool okh[FMM_UNR];
#pragma unroll
    for (int i = 0; i < FMM_UNR; ++i) {
      const int64_t s = sb + (int64_t)i * G + sub;
      const bool ok = s < s1;
      sc[i] = ok ? s : s1 - 1;  // (a slot past the end reads the last SNP again and counts as 1)
      okh[i] = ok & (has_gp[sc[i]] != 0);  // (& not &&: both loads are issued, nothing branches)
      if (HWE) {  // gp0s of :388-390
        const double a = af[sc[i]], b = 1.0 - a;
        g0[i] = b * b;
        g1[i] = 2.0 * a * b;
        g2[i] = a * a;
      } else {
        const double* g = gp + (size_t)sc[i] * V3 + jo;
        g0[i] = g[0];
        g1[i] = g[1];
        g2[i] = g[2];
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int i = 0; i < FMM_UNR; ++i) {
        const double* L = cg[t] + (size_t)sc[i] * 9;
        const double v = fma(g2[i], L[8], fma(g1[i], L[4], g0[i] * L[0]));
        const bool in = okh[i] & (cn[t][sc[i]] > 0);
        acc[t] *= in ? v : 1.0;
        if (HWE) cnt[t] += in ? 1 : 0;
      }
      prodacc_renorm(acc[t], ex[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (G > 1) {  // the G partial products of a donor, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
      for (int off = VH; off < 64; off <<= 1) {
        acc[t] *= __shfl_xor(acc[t], off, 64);
        ex[t] += __shfl_xor(ex[t], off, 64);
        if (HWE) cnt[t] += __shfl_xor(cnt[t], off, 64);
      }
    }
    const int k = tile * T + t;
    if (k < kb && jl && sub == 0) {
      const size_t row = (size_t)k * NP + (size_t)p;
      part[row * V + j] = prodacc_log(acc[t], ex[t]);
      if (HWE) part_n[row] = cnt[t];
    }
  }
}

// out[k][v] = part[k][0][v] + part[k][1][v] + ..., in this order; out_n[k] the same for the counts (V == 1)
__global__ void __launch_bounds__(256)
    fmm_join_kernel(int64_t n, int NP, int V, const double* __restrict__ part, const int32_t* __restrict__ part_n,
                    double* __restrict__ out, int32_t* __restrict__ out_n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t k = i / V;
  const int v = (int)(i - k * V);
  const double* q = part + (size_t)k * NP * V + v;
  double s = q[0];
  for (int p = 1; p < NP; ++p) s += q[(size_t)p * V];
  out[i] = s;
  if (part_n) {
    int32_t c = 0;
    for (int p = 0; p < NP; ++p) c += part_n[(size_t)k * NP + p];
    out_n[i] = c;
  }
}

struct fmm_args {
  int64_t S;
  int kb, NP, V;
  const double *cgls, *gp, *af;
  const int32_t* nreads;
  const uint8_t* has_gp;
  double* part;
  int32_t* part_n;
};

template <int VH, int T, bool HWE>
void launch_sweep(muxgl_handle* h, const fmm_args& a) {
  const int ntile = (a.kb + T - 1) / T, nblk = (a.V + 63) / 64;
  const int64_t n_units = (int64_t)a.NP * nblk * ntile;
  hipLaunchKernelGGL((fmm_sweep_kernel<VH, T, HWE>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units,
                     ntile, nblk, a.S, a.kb, a.NP, a.cgls, a.nreads, a.has_gp, a.gp, a.af, a.V, a.part, a.part_n);
}

template <int T>
void launch_donors(muxgl_handle* h, int VH, const fmm_args& a) {
#define CALL_S(W) launch_sweep<W, T, false>(h, a)
  DISPATCH_WIDTH(VH, CALL_S);
#undef CALL_S
}

// clusters per wave (DESIGN.md 4.2e has the measurement behind the default); MUXGL_FMX_MATCH_TILE=1|2|4|8 for the probe,
// read at each call.  The outputs do not depend on it.
int match_tile() {
  const char* s = getenv("MUXGL_FMX_MATCH_TILE");
  const int t = s ? atoi(s) : 0;
  return t == 1 || t == 2 || t == 4 || t == 8 ? t : 4;
}

int fmx_match_run(muxgl_handle* h, double* ll, double* ll0, int32_t* nsnps, float* kernel_ms) {
  const int K = h->K, V = h->V;
  const int64_t S = h->S;
  if (kernel_ms) *kernel_ms = 0.f;
  if (!ll && !ll0 && !nsnps) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  if (S == 0) {  // no SNPs: U is empty for every cluster
    if (ll) memset(ll, 0, sizeof(double) * (size_t)K * V);
    if (ll0) memset(ll0, 0, sizeof(double) * (size_t)K);
    if (nsnps) memset(nsnps, 0, sizeof(int32_t) * (size_t)K);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  const bool want_hwe = ll0 || nsnps;
  // the cut of the call (match_plan.hpp): parts, bytes of a cluster in a batch, clusters of a batch
  const int NP = match_plan::parts(S, FMM_PART);
  const double per_k = match_plan::bytes_per_cluster(S, V, NP, ll != nullptr);
  const int kb_cap = match_plan::clusters_per_batch(K, per_k, dev_slab_budget("MUXGL_FMX_SLAB_MB"));
  const int T = match_tile();
  const int nblk = (V + 63) / 64;
  if ((double)NP * nblk * ((kb_cap + T - 1) / T) / 4.0 >= 2147483647.0)
    MUXGL_FAIL(h, "muxgl_fmx_match_donors: a batch of %d clusters exceeds one launch (lower MUXGL_FMX_SLAB_MB)", kb_cap);
  const int VH = match_plan::lane_width(V);

  dev_tmp<double> d_part, d_part0, d_out, d_out0;
  dev_tmp<int32_t> d_nreads, d_partn, d_outn;
  if (ll && (dev_alloc(h, &d_part.p, (size_t)kb_cap * NP * V) || dev_alloc(h, &d_out.p, (size_t)kb_cap * V))) return 1;
  if (want_hwe && (dev_alloc(h, &d_part0.p, (size_t)kb_cap * NP) || dev_alloc(h, &d_partn.p, (size_t)kb_cap * NP) ||
                   dev_alloc(h, &d_out0.p, (size_t)kb_cap) || dev_alloc(h, &d_outn.p, (size_t)kb_cap)))
    return 1;
  if (dev_alloc(h, &d_nreads.p, (size_t)kb_cap * S)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, "muxgl_fmx_match_donors")) return 1;

  for (int k0 = 0; k0 < K; k0 += kb_cap) {
    const int kb = std::min(kb_cap, K - k0);
    if (ev.start(h)) return 1;
    HIPCHK(h, hipMemsetAsync(d_nreads.p, 0, sizeof(int32_t) * (size_t)kb * S, h->stream));
    if (h->nnz) {
      const int64_t blocks = std::min<int64_t>((h->nnz + 255) / 256, 16384);
      hipLaunchKernelGGL(fmm_count_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, h->nnz, S, k0, kb, h->d_entry_snp,
                         h->d_entry_cell, h->d_clust, h->d_ecnt, d_nreads.p);
      HIPCHK(h, hipGetLastError());
    }
    fmm_args a = {S, kb, NP, V, h->d_cgls + (size_t)k0 * S * 9, h->d_gp, h->d_af, d_nreads.p, h->d_has_gp, d_part.p, nullptr};
    if (ll) {
      switch (T) {
        case 1: launch_donors<1>(h, VH, a); break;
        case 2: launch_donors<2>(h, VH, a); break;
        case 8: launch_donors<8>(h, VH, a); break;
        default: launch_donors<4>(h, VH, a); break;
      }
      HIPCHK(h, hipGetLastError());
      const int64_t n = (int64_t)kb * V;
      hipLaunchKernelGGL(fmm_join_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, NP, V, d_part.p,
                         (const int32_t*)nullptr, d_out.p, (int32_t*)nullptr);
      HIPCHK(h, hipGetLastError());
    }
    if (want_hwe) {
      a.V = 1;
      a.part = d_part0.p;
      a.part_n = d_partn.p;
      launch_sweep<1, 1, true>(h, a);  // (its reads are per lane: a tile would share nothing)
      HIPCHK(h, hipGetLastError());
      hipLaunchKernelGGL(fmm_join_kernel, dim3((unsigned)((kb + 255) / 256)), dim3(256), 0, h->stream, (int64_t)kb, NP, 1,
                         d_part0.p, d_partn.p, d_out0.p, d_outn.p);
      HIPCHK(h, hipGetLastError());
    }
    if (ev.stop(h)) return 1;
    if (ll)
      HIPCHK(h, hipMemcpyAsync(ll + (size_t)k0 * V, d_out.p, sizeof(double) * (size_t)kb * V, hipMemcpyDeviceToHost, h->stream));
    if (ll0) HIPCHK(h, hipMemcpyAsync(ll0 + k0, d_out0.p, sizeof(double) * (size_t)kb, hipMemcpyDeviceToHost, h->stream));
    if (nsnps) HIPCHK(h, hipMemcpyAsync(nsnps + k0, d_outn.p, sizeof(int32_t) * (size_t)kb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ev.add();
  }
  return 0;
}

}  // namespace

extern "C" int muxgl_fmx_match_donors(muxgl_handle* h, double* ll, double* ll0, int32_t* nsnps, float* kernel_ms) {
  if (!h) return 1;
  MUXGL_NOT_FOR_GROUPS(h, "muxgl_fmx_match_donors");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->col || h->role != MUXGL_ROLE_FULL)
    MUXGL_FAIL(h, "muxgl_fmx_match_donors: not available on a slabbed handle (muxgl_fmx_set_column_slab): its cluster pileups "
                  "cover a SNP range only");
  if (!h->d_cell_ptr) MUXGL_FAIL(h, "muxgl_fmx_match_donors: no pileup set (muxgl_set_pileup)");
  if (!h->fmx_prepared) MUXGL_FAIL(h, "muxgl_fmx_match_donors: call muxgl_fmx_prepare first");
  if (h->K < 1 || !h->d_cgls) MUXGL_FAIL(h, "muxgl_fmx_match_donors: no clusters set (muxgl_fmx_set_clusters)");
  if (!h->d_gp || !h->d_has_gp || h->V < 1) MUXGL_FAIL(h, "muxgl_fmx_match_donors: no GP tensor set (muxgl_demux_set_gp)");
  if (h->fc0 != 0 || h->fc1 != h->C || h->fs0 != 0 || h->fs1 != h->S)
    MUXGL_FAIL(h, "muxgl_fmx_match_donors: not available on a sharded handle (muxgl_fmx_set_shard): its cluster pileups "
                  "cover a SNP range only");
  return fmx_match_run(h, ll, ll0, nsnps, kernel_ms);
}
