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
//     walks the group's blocks in order (incl_fold::owner).  What is read how follows from the slab's layout, which is
//     not demuxlet's:
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
// State and determinism: incl_fold.hpp.  The position is p = hi(hi+1)/2 + lo of the scans; every hypothesis is counted
// once in tot, where it is read in the row role -- in an off-diagonal block that is the role of its higher cluster, in a
// diagonal block the lane that formed it; a thread pushes slots / rotations ascending, the singlet last.  All four
// outputs are bit-identical for any MUXGL_FMX_SLAB_MB, on a group and on slabbed ranks.
//
// Memory: within the budget (incl_plan.hpp) the slab of a group plus state and outputs of a batch of whole cells, finished
// and copied out before the next.  Nothing proportional to C x K^2.  The call reads state of the handle and writes none.
#include <algorithm>
#include <vector>

#include "fmx_call_body.hpp"
#include "fmx_stream_sweep.hpp"
#include "incl_fold.hpp"

namespace {

using incl_fold::TILE_LD;
using stream_fold::evidence;

struct fincl_ops {
  static constexpr int32_t none = 0x7fffffff;
  static __device__ __forceinline__ bool before(double va, int32_t pa, double vb, int32_t pb) {
    return fmx_better(va, pa, vb, pb);
  }
};
using fincl_state = incl_fold::state<fincl_ops>;

// grid = (cells of the batch, cluster blocks); slab of the group [cell of the batch][nb blocks][slot][lane]
__global__ void __launch_bounds__(256)
    fmx_incl_fold_kernel(int32_t b0, int32_t nb, const int32_t* __restrict__ blocks, int nblk, int K, double log_single_prior,
                         double log_double_prior, const double* __restrict__ slab, fincl_state* __restrict__ state,
                         evidence* __restrict__ totb) {
  __shared__ double tile[CB * TILE_LD];
  incl_fold::owner<fincl_ops> o(K, nblk, state, totb);
  const int lane = o.lane, w = o.w, s = o.s, B = o.B;
  const bool sl = o.sl;
  for (int z = 0; z < nb; ++z) {
    const int bz = blocks[b0 + z];
    const int X = bz >> 16, Y = bz & 0xffff;
    if (X != B && Y != B) continue;  // (uniform over the workgroup)
    const double* in = slab + ((size_t)o.ci * nb + z) * SLAB;
    if (X == B) {  // row role: the lane's own values, as block_hyps walks them
      fincl_state t = fincl_state::empty();
      block_hyps(X, Y, w, lane, K, in, [&](int p, double v, bool singlet) {
        if (singlet)
          t.ev.push(v + log_single_prior);
        else
          t.push(v, log_double_prior, p);
      });
      o.reduce(t, true);
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
      o.reduce(t, false);
    } else if (Y == B) {  // column role of an off-diagonal block: s is the slot, through the tile
      fincl_state t = fincl_state::empty();
      incl_fold::tile_fill(tile, lane, w, in, false);
      if (sl) {
        for (int jq = 16 * w; jq < 16 * w + 16; ++jq) {
          const int sj = CB * X + jq;
          if (sj >= K) break;
          t.push(tile[lane * TILE_LD + jq], log_double_prior, sj * (sj + 1) / 2 + s);
        }
      }
      o.reduce(t, false);  // (its barriers also keep the next block's tile stores behind these reads)
    }
  }
  o.store(K, nblk, state, totb);
}

__device__ __forceinline__ int row_of(int p) {
  int r = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= p) ++r;
  while (r * (r + 1) / 2 > p) --r;
  return r;
}

// lane = (cell of the batch, cluster)
__global__ void __launch_bounds__(256)
    fmx_incl_finish_kernel(int64_t n, int K, int nblk, const fincl_state* __restrict__ state,
                           const evidence* __restrict__ totb, double* __restrict__ incl, double* __restrict__ tot,
                           double* __restrict__ dbl, int32_t* __restrict__ partner) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t ci = i / K;
  const int s = (int)(i - ci * K);
  const int32_t bp = incl_fold::finish_item(i, state, incl, dbl);
  int32_t pr = -1;
  if (bp != fincl_ops::none) {
    const int hi = row_of(bp), lo = bp - hi * (hi + 1) / 2;
    pr = hi == s ? lo : hi;
  }
  partner[i] = pr;
  incl_fold::finish_tot(ci, s, nblk, totb, tot);
}

int fmx_inclusion_run(muxgl_handle* h, const muxgl_fmx_params* p, double* incl, double* tot, double* dbl, int32_t* partner) {
  using incl_fold::copy_out;
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
    hipLaunchKernelGGL(incl_fold::init_kernel<fincl_ops>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, nc * nblk,
                       d_state.p, d_totb.p);
    HIPCHK(h, hipGetLastError());
    for (int64_t b0 = 0; b0 < nb_all; b0 += gb) {  // blocks in order (determinism: incl_fold.hpp)
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

extern "C" int muxgl_fmx_inclusion(muxgl_handle* h, const muxgl_fmx_params* p, double* incl, double* tot, double* dbl,
                                   int32_t* partner) {
  if (!h) return 1;
  if (h->group) return group_fmx_inclusion(h, p, incl, tot, dbl, partner);
  HIPCHK(h, hipSetDevice(h->device));
  if (!p) MUXGL_FAIL(h, "muxgl_fmx_inclusion: fmx params NULL");
  if (fmx_refuse(h, h, "muxgl_fmx_inclusion", "the tables belong")) return 1;
  if (h->C == 0 || (!incl && !tot && !dbl && !partner)) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing: the slots of the last iteration keep their values)
  if (fmx_inclusion_run(h, p, incl, tot, dbl, partner)) return 1;
  collect_timing(h);
  return 0;
}
