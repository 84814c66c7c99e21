// demux_incl.hip -- muxgl_demux_inclusion: per droplet and sample, the evidence that the sample is in the droplet (as a
// singlet or as either half of a doublet) and the doublet hypothesis it pairs best in.  Both are [C][V] tables: the row
// and column marginals of the pair matrix the reference's disabled .pair writer prints (cmd_cram_demuxlet.cpp:852-877),
// over the hypotheses that carry prior mass in :804-821 (definitions: include/muxgl.h).
//
// Three steps per group of (cells x 64 x 64 blocks), a group's slab inside the streamed call's budget:
//   * the sweep of the streamed call (demux_stream_sweep.hpp): slab[cell][block][n][k][j], the call's own per-entry
//     likelihoods in front of it (demux_entry_pg_launch works at any V).
//   * incl_fold_kernel, one workgroup per (cell, block of 64 samples B): it OWNS the state of these 64 samples and walks the
//     group's blocks in order (incl_fold::owner).  A block (X, Y) with X == B is reduced along k into the samples as j
//     (lane = j, wave w takes 16 partners k, values read as they lie); one with Y == B is reduced along j into the samples
//     as k (lane = k), read through a padded tile in LDS, which is the transpose.  A diagonal block feeds both roles, rows
//     first.  The singlet term (j, 0, 0) enters with the row role of block (B, 0).
//     The issue of a workgroup per (cell, block) with a merge of its own was weighed against this: the owner reads a block
//     of the slab twice (once per role), but needs no partials in memory and no third kernel, two workgroups never touch
//     one state, and the merge order holds by construction.  The sweep computes ~600 FP64 operations per slab value at
//     150 entries per cell, so the second read does not show.
//   * incl_finish_kernel, lane = (cell, sample): M + log S, the best value and its decoded hypothesis.
//
// State and determinism: incl_fold.hpp.  The position is the scan position (j V + k) A + n, which names partner, n and
// role; every hypothesis is in exactly one row role; a thread pushes the singlet first, then k ascending and n ascending
// (rows), n ascending and j ascending (columns).  All six outputs are bit-identical for any MUXGL_DEMUX_SLAB_MB.
//
// Memory: [nnz][A][9] entry likelihoods, and within the budget (incl_plan.hpp) the slab plus state and outputs of a batch
// of whole cells, finished and copied out before the next.  Nothing proportional to C x V^2.
#include <algorithm>
#include <vector>

#include "demux_stream_sweep.hpp"
#include "incl_fold.hpp"

namespace {

using namespace muxgl_call;
using incl_fold::TILE_LD;
using stream_fold::evidence;

struct incl_ops {
  static constexpr int32_t none = -1;
  static __device__ __forceinline__ bool before(double va, int32_t pa, double vb, int32_t pb) {
    return key_before(va, pa, vb, pb);
  }
};
using incl_state = incl_fold::state<incl_ops>;

// grid = (cells of the batch, sample blocks); slab of the group [cell of the batch][nb blocks][A][k][j]
__global__ void __launch_bounds__(256)
    incl_fold_kernel(int64_t c0, int32_t b0, int32_t nb, const int32_t* __restrict__ blocks, int nblk,
                     const int64_t* __restrict__ cell_ptr, int V, int nAlpha, call_alpha al, const double* __restrict__ slab,
                     incl_state* __restrict__ state, evidence* __restrict__ totb) {
  __shared__ double tile[SBLK * TILE_LD];
  const bool no_entries = cell_ptr[c0 + blockIdx.x] == cell_ptr[c0 + blockIdx.x + 1];  // every LL is 0 (no sweep wrote)
  incl_fold::owner<incl_ops> o(V, nblk, state, totb);
  const int lane = o.lane, w = o.w, s = o.s, B = o.B;
  const bool sl = o.sl;
  for (int z = 0; z < nb; ++z) {
    const int b = blocks[b0 + z];
    const int X = b / nblk, Y = b - X * nblk;
    if (X != B && Y != B) continue;  // (uniform over the workgroup)
    const double* in = slab + ((size_t)o.ci * nb + z) * nAlpha * SLAB_DOUBLES;
    if (X == B) {  // s is j: along k
      incl_state t = incl_state::empty();
      if (sl) {
        if (Y == 0 && w == 0) t.ev.push((no_entries ? 0.0 : in[lane]) + al.log_single_prior);  // (s, 0, 0), :806
        for (int kq = 16 * w; kq < 16 * w + 16; ++kq) {
          const int k = SBLK * Y + kq;
          if (k >= V || k == s) continue;
          for (int n = 1; n < nAlpha; ++n) {
            const bool sym = al.a[n] == 0.5;
            if (sym && k > s) continue;  // :812-813
            const double v = no_entries ? 0.0 : in[((size_t)n * SBLK + kq) * SBLK + lane];
            t.push(v, sym ? al.log_doublet_prior2 : al.log_doublet_prior1, (s * V + k) * nAlpha + n);
          }
        }
      }
      o.reduce(t, true);
    }
    if (Y == B) {  // s is k: along j, through the tile
      incl_state t = incl_state::empty();
      for (int n = 1; n < nAlpha; ++n) {
        const bool sym = al.a[n] == 0.5;
        incl_fold::tile_fill(tile, lane, w, in + (size_t)n * SLAB_DOUBLES, no_entries);
        if (sl) {
          for (int jq = 16 * w; jq < 16 * w + 16; ++jq) {
            const int j = SBLK * X + jq;
            if (j >= V || j == s || (sym && s > j)) continue;
            t.push(tile[lane * TILE_LD + jq], sym ? al.log_doublet_prior2 : al.log_doublet_prior1, (j * V + s) * nAlpha + n);
          }
        }
        __syncthreads();  // (the next n's tile stores stay behind these reads)
      }
      o.reduce(t, false);
    }
  }
  o.store(V, nblk, state, totb);
}

// lane = (cell of the batch, sample)
__global__ void __launch_bounds__(256)
    incl_finish_kernel(int64_t n, int V, int nAlpha, int nblk, const incl_state* __restrict__ state,
                       const evidence* __restrict__ totb, double* __restrict__ incl, double* __restrict__ tot,
                       double* __restrict__ dbl, int32_t* __restrict__ partner, int32_t* __restrict__ alpha_idx,
                       int32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t ci = i / V;
  const int s = (int)(i - ci * V);
  const int32_t bp = incl_fold::finish_item(i, state, incl, dbl);
  int32_t pr = -1, ai = -1, fi = -1;
  if (bp >= 0) {
    const int32_t q = bp / nAlpha;
    const int32_t j = q / V, k = q - j * V;
    ai = bp - q * nAlpha;
    fi = j == s ? 1 : 0;
    pr = j == s ? k : j;
  }
  partner[i] = pr;
  alpha_idx[i] = ai;
  first[i] = fi;
  incl_fold::finish_tot(ci, s, nblk, totb, tot);
}

}  // namespace

int demux_inclusion_run(muxgl_handle* h, const muxgl_demux_params* p, const demux_incl_out& out) {
  using incl_fold::copy_out;
  const int V = h->V, A = p->n_alpha;
  const int64_t C = h->C;
  if ((double)V * V * A >= 2147483648.0)
    MUXGL_FAIL(h, "muxgl_demux_inclusion: V=%d with %d alphas exceeds the int32 scan positions (V*V*n_alpha < 2^31)", V, A);
  bool all_sym = true;  // (also a grid without a doublet alpha: the singlets lie in the blocks Y = 0)
  for (int n = 1; n < A; ++n) all_sym = all_sym && p->alpha[n] == 0.5;
  const int nblk = (V + SBLK - 1) / SBLK;
  const std::vector<int32_t> blocks = stream_plan::block_list(nblk, all_sym, nblk);  // X * nblk + Y
  const int64_t nb_all = (int64_t)blocks.size();
  const size_t per = (size_t)A * SLAB_DOUBLES * sizeof(double);
  const size_t spc = incl_plan::state_bytes_per_cell(V);
  const size_t budget = dev_slab_budget("MUXGL_DEMUX_SLAB_MB");
  const incl_plan::batches bt = incl_plan::cut_batches(C, nb_all, spc, per, budget);
  if (!bt.ok) MUXGL_FAIL(h, "%s", incl_plan::too_small_message(V, spc, per, budget).c_str());
  const int64_t batch = bt.batch, gb = bt.gb;
  const size_t nbv = (size_t)batch * V;

  dev_tmp<int32_t> d_blocks, d_partner, d_alpha, d_first;
  dev_tmp<double> d_pg, d_slab, d_incl, d_tot, d_dbl;
  dev_tmp<incl_state> d_state;
  dev_tmp<evidence> d_totb;
  if (dev_alloc(h, &d_blocks.p, blocks.size()) || dev_alloc(h, &d_pg.p, (size_t)h->nnz * A * 9) ||
      dev_alloc(h, &d_slab.p, (size_t)batch * gb * A * SLAB_DOUBLES) || dev_alloc(h, &d_state.p, nbv) ||
      dev_alloc(h, &d_totb.p, (size_t)batch * nblk) || dev_alloc(h, &d_incl.p, nbv) || dev_alloc(h, &d_tot.p, (size_t)batch) ||
      dev_alloc(h, &d_dbl.p, nbv) || dev_alloc(h, &d_partner.p, nbv) || dev_alloc(h, &d_alpha.p, nbv) ||
      dev_alloc(h, &d_first.p, nbv))
    return 1;
  HIPCHK(h, hipMemcpyAsync(d_blocks.p, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, h->stream));
  const call_alpha al = make_call_alpha(p, V);
  tic(h, MUXGL_T_DEMUX_INCLUSION);
  if (h->nnz > 0 && demux_entry_pg_launch(h, p, d_pg.p)) return 1;
  for (int64_t c0 = 0; c0 < C; c0 += batch) {
    const int64_t nc = std::min(batch, C - c0);
    const int64_t n = nc * V;
    hipLaunchKernelGGL(incl_fold::init_kernel<incl_ops>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n,
                       nc * nblk, d_state.p, d_totb.p);
    HIPCHK(h, hipGetLastError());
    for (int64_t b0 = 0; b0 < nb_all; b0 += gb) {  // blocks in order (determinism: incl_fold.hpp)
      const int32_t nb = (int32_t)std::min(gb, nb_all - b0);
      if (sweep_dispatch(h, c0, nc, (int32_t)b0, nb, d_blocks.p, nblk, d_pg.p, A, d_slab.p)) return 1;
      hipLaunchKernelGGL(incl_fold_kernel, dim3((unsigned)nc, (unsigned)nblk), dim3(256), 0, h->stream, c0, (int32_t)b0, nb,
                         d_blocks.p, nblk, h->d_cell_ptr, V, A, al, d_slab.p, d_state.p, d_totb.p);
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(incl_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, V, A, nblk,
                       d_state.p, d_totb.p, d_incl.p, d_tot.p, d_dbl.p, d_partner.p, d_alpha.p, d_first.p);
    HIPCHK(h, hipGetLastError());
    if (c0 + nc == C) toc(h, MUXGL_T_DEMUX_INCLUSION);
    const size_t o = (size_t)c0 * V;
    if (copy_out(h, out.incl ? out.incl + o : nullptr, d_incl.p, (size_t)n) ||
        copy_out(h, out.tot ? out.tot + c0 : nullptr, d_tot.p, (size_t)nc) ||
        copy_out(h, out.dbl ? out.dbl + o : nullptr, d_dbl.p, (size_t)n) ||
        copy_out(h, out.partner ? out.partner + o : nullptr, d_partner.p, (size_t)n) ||
        copy_out(h, out.alpha_idx ? out.alpha_idx + o : nullptr, d_alpha.p, (size_t)n) ||
        copy_out(h, out.first ? out.first + o : nullptr, d_first.p, (size_t)n))
      return 1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int muxgl_demux_inclusion(muxgl_handle* h, const muxgl_demux_params* p, double* incl, double* tot, double* dbl,
                                     int32_t* partner, int32_t* alpha_idx, int32_t* first) {
  if (!h) return 1;
  const demux_incl_out out = {incl, tot, dbl, partner, alpha_idx, first};
  if (h->group) return group_demux_inclusion(h, p, out);
  HIPCHK(h, hipSetDevice(h->device));
  if (!p) MUXGL_FAIL(h, "demux params NULL");
  if (p->n_alpha < 1 || p->n_alpha > MUXGL_MAX_ALPHA) MUXGL_FAIL(h, "n_alpha=%d outside [1,%d]", p->n_alpha, MUXGL_MAX_ALPHA);
  if (!h->d_cell_ptr) MUXGL_FAIL(h, "no pileup set (muxgl_set_pileup)");
  if (!h->d_gp) MUXGL_FAIL(h, "no GP tensor set (muxgl_demux_set_gp)");
  if (h->C == 0) return 0;
  // (no clear_timing: the slots of the last muxgl_demux_run keep their values)
  if (demux_inclusion_run(h, p, out)) return 1;
  collect_timing(h);
  return 0;
}
