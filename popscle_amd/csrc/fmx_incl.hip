// fmx_incl.hip -- muxgl_fmx_inclusion: per droplet and cluster, the evidence that the cluster is in the droplet (as a
// singlet or as either half of a doublet) and the cluster it pairs best with.  Both are [C][K] tables: the row and column
// marginals of the triangle llks[j(j+1)/2 + k] that the LAST E-step of the handle formed (cmd_cram_freemux2.cpp:383-456),
// over the hypotheses of the scans :469-498 -- the reference keeps only the best and the next doublet of a droplet
// (:469-513).  Definitions: include/muxgl.h.
//
// Three steps per group of (cells x 64 x 64 blocks of clusters), a group's slab inside the streamed E-step's budget:
//   * the sweep of the streamed E-step (fmx_stream_sweep.hpp), unchanged in arithmetic and flags, over the cluster
//     posteriors the last E-step read (d_cgp; fmx_sng_state says whether they still are those): slab[cell][block][slot][lane].
//   * fmx_incl_fold_kernel, one workgroup per (cell, block of 64 clusters B): it OWNS the state of these 64 clusters and
//     walks the group's blocks in order (incl_fold_kernel's owner design, demux_incl.hip).  What is read how follows from
//     the slab's layout, which is not demuxlet's:
//       - an off-diagonal block (X, Y), X > Y, holds [slot k][lane j] = LL(64X + j, 64Y + k).  With X == B the clusters are
//         the lanes (row role): lane j reads its own column of slots as it lies, wave w the slots 16w .. 16w + 15.  With
//         Y == B the clusters are the slots (column role): the block goes through a padded tile in LDS, which is the
//         transpose, and lane k reads row k of it, wave w the lanes 16w .. 16w + 15 of the block.
//       - a diagonal block holds rotations: slot t - 1, lane j = LL of the pair (64B + j, 64B + ((j - t) & 63)), t = 1 .. 32
//         (rotation 32 valid from the higher lane only), slot 32 the singlets.  Every pair is there ONCE and feeds both of
//         its clusters: the lane that formed it reads in[(t - 1) 64 + j] (row role: block_hyps, wave w the rotations
//         8w + 1 .. 8w + 8, wave 0 also the singlet), the other cluster s reads in[(t - 1) 64 + ((s + t) & 63)] (column
//         role) -- the wave's lanes read one slot row rotated by t, still one contiguous 512 bytes, so no tile.
//       - lanes and partners >= K are skipped exactly as block_hyps skips them.
//   * fmx_incl_finish_kernel, lane = (cell, cluster): M + log S, the best value and its decoded partner.
//
// State per (cell, cluster), 32 bytes: stream_fold::evidence (M, S) and (best value, position p = hi(hi+1)/2 + lo of the
// scans).  `tot` has an evidence per (cell, row block X): every hypothesis is counted once, where it is read in the row
// role -- in an off-diagonal block that is the role of its higher cluster, in a diagonal block the lane that formed it.
//
// Determinism.  A thread pushes its hypotheses in a fixed order (slots / rotations ascending, the singlet last); a block's
// partial of a cluster is the four waves' as (0 + 1) + (2 + 3); a cluster's partials are merged into its state one block
// and role at a time, in stream_plan::block_list order, rows before columns in a diagonal block; tot's partial of a block
// is the xor butterfly (partner 1, 2, .., 32) over the 64 lanes of that merged row partial, merged per row block in the
// same order, and the row blocks ascending in the finish kernel.  A group only decides how many blocks one launch folds
// and a batch which cells share the device, so all four outputs are bit-identical from call to call, for any
// MUXGL_FMX_SLAB_MB, on a group and on slabbed ranks.  The best hypothesis is taken under a total order (value
// descending, then position ascending: fmx_better), so it does not depend on any grouping at all.
//
// Memory: within the budget (incl_plan.hpp) the slab of a group plus state and outputs of a batch of whole cells, finished
// and copied out before the next.  Nothing proportional to C x K^2.  The call reads state of the handle and writes none.
#include <algorithm>
#include <vector>

#include "fmx_call_body.hpp"
#include "fmx_stream_sweep.hpp"
#include "incl_plan.hpp"
#include "stream_fold.hpp"

namespace {

using stream_fold::evidence;

constexpr int32_t NO_POS = 0x7fffffff;
// doubles per row of the transposing tile.  Lane l reads tile[l TILE_LD + q] (ds_read_b64: bank = dword address mod 64 =
// 2 l + 2 q mod 64 at TILE_LD = 65, per half wave of 32 lanes): 32 lanes on 32 distinct bank pairs, no conflict.
constexpr int TILE_LD = CB + 1;

struct fincl_state {
  evidence ev;
  double bv;   // best LL over H_s (-1e300: none)
  int32_t bp;  // its position p = hi(hi+1)/2 + lo (NO_POS: none)
  int32_t pad;
  static __device__ __forceinline__ fincl_state empty() { return {{-__builtin_huge_val(), 0.0}, -1e300, NO_POS, 0}; }
  // (a value of -inf adds nothing to the sum and is never better than the empty -1e300)
  __device__ __forceinline__ void push(double v, double prior, int32_t pos) {
    ev.push(v + prior);
    if (fmx_better(v, pos, bv, bp)) bv = v, bp = pos;
  }
  static __device__ __forceinline__ fincl_state merge(const fincl_state& a, const fincl_state& b) {  // a first
    const bool ab = fmx_better(a.bv, a.bp, b.bv, b.bp);
    return {evidence::merge(a.ev, b.ev), ab ? a.bv : b.bv, ab ? a.bp : b.bp, 0};
  }
};
static_assert(sizeof(fincl_state) == 32, "incl_plan::fmx_state_bytes_per_cell counts 32 bytes");

__global__ void __launch_bounds__(256)
    fmx_incl_init_kernel(int64_t n_state, int64_t n_tot, fincl_state* __restrict__ st, evidence* __restrict__ totb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_state) st[i] = fincl_state::empty();
  if (i < n_tot) totb[i] = evidence{-__builtin_huge_val(), 0.0};
}

// grid = (cells of the batch, cluster blocks); slab of the group [cell of the batch][nb blocks][slot][lane]
__global__ void __launch_bounds__(256)
    fmx_incl_fold_kernel(int32_t b0, int32_t nb, const int32_t* __restrict__ blocks, int nblk, int K, double log_single_prior,
                         double log_double_prior, const double* __restrict__ slab, fincl_state* __restrict__ state,
                         evidence* __restrict__ totb) {
  __shared__ double tile[CB * TILE_LD];
  __shared__ fincl_state parts[4][CB];
  const int64_t ci = blockIdx.x;
  const int B = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = CB * B + lane;
  const bool sl = s < K;
  const bool owner = w == 0 && sl;

  fincl_state st = fincl_state::empty();        // of cluster s, in wave 0
  evidence tot = {-__builtin_huge_val(), 0.0};  // of row block B, in thread 0
  if (owner) st = state[ci * K + s];
  if (threadIdx.x == 0) tot = totb[ci * nblk + B];

  // the workgroup's partial of one block and role: the waves as (0 + 1) + (2 + 3), then into the state
  auto reduce = [&](const fincl_state& t, bool with_tot) {
    parts[w][lane] = t;
    __syncthreads();
    if (w == 0) {
      const fincl_state r = fincl_state::merge(fincl_state::merge(parts[0][lane], parts[1][lane]),
                                               fincl_state::merge(parts[2][lane], parts[3][lane]));
      st = fincl_state::merge(st, r);
      if (with_tot) {  // (lanes without a cluster hold the empty evidence)
        evidence e = r.ev;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) e = evidence::merge(e, evidence{__shfl_xor(e.M, m, 64), __shfl_xor(e.S, m, 64)});
        if (lane == 0) tot = evidence::merge(tot, e);
      }
    }
    __syncthreads();
  };

  for (int z = 0; z < nb; ++z) {
    const int bz = blocks[b0 + z];
    const int X = bz >> 16, Y = bz & 0xffff;
    if (X != B && Y != B) continue;  // (uniform over the workgroup)
    const double* in = slab + ((size_t)ci * nb + z) * SLAB;
    if (X == B) {  // row role: the lane's own values, as block_hyps walks them
      fincl_state t = fincl_state::empty();
      block_hyps(X, Y, w, lane, K, in, [&](int p, double v, bool singlet) {
        if (singlet)
          t.ev.push(v + log_single_prior);
        else
          t.push(v, log_double_prior, p);
      });
      reduce(t, true);
    }
    if (Y == B && X == B) {  // column role of a diagonal block: the pair the lane (s + t) & 63 formed with s
      fincl_state t = fincl_state::empty();
      if (sl) {
        for (int i = 0; i < 8; ++i) {
          const int r = 8 * w + i + 1, jj = (lane + r) & 63, sj = CB * B + jj;
          if (sj >= K || (r == 32 && jj < lane)) continue;  // (block_hyps' rule, seen from the partner)
          const int hi = sj > s ? sj : s, lo = sj > s ? s : sj;
          t.push(in[(r - 1) * CB + jj], log_double_prior, hi * (hi + 1) / 2 + lo);
        }
      }
      reduce(t, false);
    } else if (Y == B) {  // column role of an off-diagonal block: s is the slot, through the tile
      fincl_state t = fincl_state::empty();
      for (int kq = 16 * w; kq < 16 * w + 16; ++kq) tile[kq * TILE_LD + lane] = in[kq * CB + lane];
      __syncthreads();
      if (sl) {
        for (int jq = 16 * w; jq < 16 * w + 16; ++jq) {
          const int sj = CB * X + jq;
          if (sj >= K) break;
          t.push(tile[lane * TILE_LD + jq], log_double_prior, sj * (sj + 1) / 2 + s);
        }
      }
      reduce(t, false);  // (its barriers also keep the next block's tile stores behind these reads)
    }
  }
  if (owner) state[ci * K + s] = st;
  if (threadIdx.x == 0) totb[ci * nblk + B] = tot;
}

__device__ __forceinline__ int row_of(int p) {
  int r = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= p) ++r;
  while (r * (r + 1) / 2 > p) --r;
  return r;
}

// lane = (cell of the batch, cluster); the lane of cluster 0 also joins the cell's row blocks into tot.  A sum without a
// finite term is -inf
__global__ void __launch_bounds__(256)
    fmx_incl_finish_kernel(int64_t n, int K, int nblk, const fincl_state* __restrict__ state,
                           const evidence* __restrict__ totb, double* __restrict__ incl, double* __restrict__ tot,
                           double* __restrict__ dbl, int32_t* __restrict__ partner) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t ci = i / K;
  const int s = (int)(i - ci * K);
  const fincl_state st = state[i];
  incl[i] = st.ev.S > 0.0 ? st.ev.M + log(st.ev.S) : -__builtin_huge_val();
  dbl[i] = st.bv;
  int32_t pr = -1;
  if (st.bp != NO_POS) {
    const int hi = row_of(st.bp), lo = st.bp - hi * (hi + 1) / 2;
    pr = hi == s ? lo : hi;
  }
  partner[i] = pr;
  if (s == 0) {
    evidence e = totb[ci * nblk];
    for (int X = 1; X < nblk; ++X) e = evidence::merge(e, totb[ci * nblk + X]);
    tot[ci] = e.S > 0.0 ? e.M + log(e.S) : -__builtin_huge_val();
  }
}

template <class T>
int copy_out(muxgl_handle* h, T* dst, const T* d_src, size_t n) {
  if (dst && n) HIPCHK(h, hipMemcpyAsync(dst, d_src, sizeof(T) * n, hipMemcpyDeviceToHost, h->stream));
  return 0;
}

int fmx_inclusion_run(muxgl_handle* h, const muxgl_fmx_params* p, double* incl, double* tot, double* dbl, int32_t* partner) {
  const int K = h->K;
  const int64_t C = h->C;
  const int nblk = (K + CB - 1) / CB;
  const std::vector<int32_t> blocks = block_list(K);
  const int64_t nb_all = (int64_t)blocks.size();
  const size_t per = (size_t)SLAB * sizeof(double);
  const size_t spc = incl_plan::fmx_state_bytes_per_cell(K);
  const size_t budget = dev_slab_budget("MUXGL_FMX_SLAB_MB");
  const incl_plan::batches bt = incl_plan::cut_batches(C, nb_all, spc, per, budget);
  if (!bt.ok) MUXGL_FAIL(h, "%s", incl_plan::fmx_too_small_message(K, spc, per, budget).c_str());
  const int64_t batch = bt.batch, gb = bt.gb;
  const size_t nbk = (size_t)batch * K;

  dev_tmp<int32_t> d_blocks, d_partner;
  dev_tmp<double> d_slab, d_incl, d_tot, d_dbl;
  dev_tmp<fincl_state> d_state;
  dev_tmp<evidence> d_totb;
  if (dev_alloc(h, &d_blocks.p, blocks.size()) || dev_alloc(h, &d_slab.p, (size_t)batch * gb * SLAB) ||
      dev_alloc(h, &d_state.p, nbk) || dev_alloc(h, &d_totb.p, (size_t)batch * nblk) || dev_alloc(h, &d_incl.p, nbk) ||
      dev_alloc(h, &d_tot.p, (size_t)batch) || dev_alloc(h, &d_dbl.p, nbk) || dev_alloc(h, &d_partner.p, nbk))
    return 1;
  HIPCHK(h, hipMemcpyAsync(d_blocks.p, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, h->stream));
  const double lsp = log((1.0 - p->doublet_prior) / K);          // cmd_cram_freemux2.cpp:379
  const double ldp = log(p->doublet_prior / K / (K - 1) * 2.0);  // :380 (K = 1: no doublet reads it)
  tic(h, MUXGL_T_FMX_INCLUSION);
  for (int64_t c0 = 0; c0 < C; c0 += batch) {
    const int64_t nc = std::min(batch, C - c0);
    const int64_t n = nc * K;
    hipLaunchKernelGGL(fmx_incl_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, nc * nblk,
                       d_state.p, d_totb.p);
    HIPCHK(h, hipGetLastError());
    for (int64_t b0 = 0; b0 < nb_all; b0 += gb) {  // blocks in order (determinism, above)
      const int32_t nb = (int32_t)std::min(gb, nb_all - b0);
      if (sweep_launch(h, c0, nullptr, nc, (int32_t)b0, nb, d_blocks.p, d_slab.p)) return 1;
      hipLaunchKernelGGL(fmx_incl_fold_kernel, dim3((unsigned)nc, (unsigned)nblk), dim3(256), 0, h->stream, (int32_t)b0, nb,
                         d_blocks.p, nblk, K, lsp, ldp, d_slab.p, d_state.p, d_totb.p);
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(fmx_incl_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, K, nblk,
                       d_state.p, d_totb.p, d_incl.p, d_tot.p, d_dbl.p, d_partner.p);
    HIPCHK(h, hipGetLastError());
    if (c0 + nc == C) toc(h, MUXGL_T_FMX_INCLUSION);
    const size_t o = (size_t)c0 * K;
    if (copy_out(h, incl ? incl + o : nullptr, d_incl.p, (size_t)n) || copy_out(h, tot ? tot + c0 : nullptr, d_tot.p, (size_t)nc) ||
        copy_out(h, dbl ? dbl + o : nullptr, d_dbl.p, (size_t)n) ||
        copy_out(h, partner ? partner + o : nullptr, d_partner.p, (size_t)n))
      return 1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

}  // namespace

// why the handle cannot give the tables now (NULL: it can): muxgl_fmx_singlets' rules under this call's name; shared with
// the device group
const char* fmx_inclusion_refusal(const muxgl_handle* h) {
  if (!h->d_cell_ptr) return "muxgl_fmx_inclusion: no pileup set (muxgl_set_pileup)";
  if (!h->fmx_prepared) return "muxgl_fmx_inclusion: call muxgl_fmx_prepare first";
  if (h->K < 1) return "muxgl_fmx_inclusion: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)";
  if (h->fmx_sng_state == FMX_SNG_NONE)
    return "muxgl_fmx_inclusion: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep first)";
  if (h->fmx_sng_state != FMX_SNG_READY)
    return "muxgl_fmx_inclusion: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; the tables "
           "belong to an E-step's own posteriors: call it before the next iteration's posterior phase";
  return nullptr;
}

extern "C" int muxgl_fmx_inclusion(muxgl_handle* h, const muxgl_fmx_params* p, double* incl, double* tot, double* dbl,
                                   int32_t* partner) {
  if (!h) return 1;
  if (h->group) return group_fmx_inclusion(h, p, incl, tot, dbl, partner);
  HIPCHK(h, hipSetDevice(h->device));
  if (!p) MUXGL_FAIL(h, "muxgl_fmx_inclusion: fmx params NULL");
  if (const char* why = fmx_inclusion_refusal(h)) MUXGL_FAIL(h, "%s", why);
  if (h->C == 0 || (!incl && !tot && !dbl && !partner)) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing: the slots of the last iteration keep their values)
  if (fmx_inclusion_run(h, p, incl, tot, dbl, partner)) return 1;
  collect_timing(h);
  return 0;
}
