// demux_incl.hip -- muxgl_demux_inclusion: per droplet and sample, the evidence that the sample is in the droplet (as a
// singlet or as either half of a doublet) and the doublet hypothesis it pairs best in.  Both are [C][V] tables: the row
// and column marginals of the pair matrix the reference's disabled .pair writer prints (cmd_cram_demuxlet.cpp:852-877),
// over the hypotheses that carry prior mass in :804-821 (definitions: include/muxgl.h).
//
// Three steps per group of (cells x 64 x 64 blocks), a group's slab inside the streamed call's budget:
//   * the sweep of the streamed call (demux_stream_sweep.hpp): slab[cell][block][n][k][j], the call's own per-entry
//     likelihoods in front of it (demux_entry_pg_launch works at any V).
//   * incl_fold_kernel, one workgroup per (cell, block of 64 samples B): it OWNS the state of these 64 samples and walks
//     the group's blocks in order.  A block (X, Y) with X == B is reduced along k into the samples as j (lane = j, wave w
//     takes 16 partners k, values read as they lie); one with Y == B is reduced along j into the samples as k (lane = k),
//     read through a padded tile in LDS, which is the transpose.  A diagonal block feeds both roles, rows first.  The
//     singlet term (j, 0, 0) enters with the row role of block (B, 0).
//     The issue of a workgroup per (cell, block) with a merge of its own was weighed against this: the owner reads a block
//     of the slab twice (once per role), but needs no partials in memory and no third kernel, two workgroups never touch
//     one state, and the merge order below holds by construction.  The sweep computes ~600 FP64 operations per slab
//     value at 150 entries per cell, so the second read does not show.
//   * incl_finish_kernel, lane = (cell, sample): M + log S, the best value and its decoded hypothesis.
//
// State per (cell, sample), 32 bytes: stream_fold::evidence (M, S) and (best value, scan position).  Scan position
// (j V + k) A + n names partner, n and role.  `tot` has an evidence per (cell, row block X): every hypothesis is in
// exactly one row role.
//
// Determinism: a thread pushes its hypotheses in a fixed order; a block's partial of a sample is the four waves' as
// (0 + 1) + (2 + 3); a sample's partials are merged into its state one block at a time in stream_plan::block_list order
// (rows before columns in a diagonal block); tot's partial of a block is a butterfly over the 64 lanes of that merged row
// partial, merged per row block in the same order, and the row blocks ascending at the end.  A group only decides how
// many blocks one launch folds and a batch which cells share the device, so all six outputs are bit-identical from call
// to call and for any MUXGL_DEMUX_SLAB_MB.  The best hypothesis is taken under a total order (value descending, then scan
// position ascending).
//
// Memory: [nnz][A][9] entry likelihoods, and within the budget (incl_plan.hpp) the slab plus state and outputs of a batch
// of whole cells, finished and copied out before the next.  Nothing proportional to C x V^2.
#include <algorithm>
#include <vector>

#include "demux_stream_sweep.hpp"
#include "incl_plan.hpp"
#include "stream_fold.hpp"

namespace {

using namespace muxgl_call;
using stream_fold::evidence;

constexpr int TILE_LD = SBLK + 1;  // doubles per row of the transposing tile: lanes reading a column hit different banks

struct incl_state {
  evidence ev;
  double bv;   // best LL over H_s (-1e300: none)
  int32_t bp;  // its scan position (j V + k) A + n (-1: none)
  int32_t pad;
  static __device__ __forceinline__ incl_state empty() { return {{-__builtin_huge_val(), 0.0}, -1e300, -1, 0}; }
  __device__ __forceinline__ void push(double v, double prior, int32_t pos) {
    ev.push(v + prior);
    if (key_before(v, pos, bv, bp)) bv = v, bp = pos;
  }
  static __device__ __forceinline__ incl_state merge(const incl_state& a, const incl_state& b) {  // a first
    const bool ab = key_before(a.bv, a.bp, b.bv, b.bp);
    return {evidence::merge(a.ev, b.ev), ab ? a.bv : b.bv, ab ? a.bp : b.bp, 0};
  }
};
static_assert(sizeof(incl_state) == 32, "incl_plan::state_bytes_per_cell counts 32 bytes");

__global__ void __launch_bounds__(256)
    incl_init_kernel(int64_t n_state, int64_t n_tot, incl_state* __restrict__ st, evidence* __restrict__ totb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_state) st[i] = incl_state::empty();
  if (i < n_tot) totb[i] = evidence{-__builtin_huge_val(), 0.0};
}

// grid = (cells of the batch, sample blocks); slab of the group [cell of the batch][nb blocks][A][k][j]
__global__ void __launch_bounds__(256)
    incl_fold_kernel(int64_t c0, int32_t b0, int32_t nb, const int32_t* __restrict__ blocks, int nblk,
                     const int64_t* __restrict__ cell_ptr, int V, int nAlpha, call_alpha al, const double* __restrict__ slab,
                     incl_state* __restrict__ state, evidence* __restrict__ totb) {
  __shared__ double tile[SBLK * TILE_LD];
  __shared__ incl_state parts[4][SBLK];
  const int64_t ci = blockIdx.x;
  const int B = blockIdx.y;
  const bool no_entries = cell_ptr[c0 + ci] == cell_ptr[c0 + ci + 1];  // every LL is 0 (the sweep wrote nothing)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = SBLK * B + lane;
  const bool sl = s < V;
  const bool owner = w == 0 && sl;

  incl_state st = incl_state::empty();           // of sample s, in wave 0
  evidence tot = {-__builtin_huge_val(), 0.0};   // of row block B, in thread 0
  if (owner) st = state[ci * V + s];
  if (threadIdx.x == 0) tot = totb[ci * nblk + B];

  // the workgroup's partial of one block and role: the waves as (0 + 1) + (2 + 3), then into the state
  auto reduce = [&](const incl_state& t, bool with_tot) {
    parts[w][lane] = t;
    __syncthreads();
    if (w == 0) {
      const incl_state r = incl_state::merge(incl_state::merge(parts[0][lane], parts[1][lane]),
                                             incl_state::merge(parts[2][lane], parts[3][lane]));
      st = incl_state::merge(st, r);
      if (with_tot) {  // (lanes without a sample hold the empty evidence)
        evidence e = r.ev;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) e = evidence::merge(e, evidence{__shfl_xor(e.M, m, 64), __shfl_xor(e.S, m, 64)});
        if (lane == 0) tot = evidence::merge(tot, e);
      }
    }
    __syncthreads();
  };

  for (int z = 0; z < nb; ++z) {
    const int b = blocks[b0 + z];
    const int X = b / nblk, Y = b - X * nblk;
    if (X != B && Y != B) continue;  // (uniform over the workgroup)
    const double* in = slab + ((size_t)ci * nb + z) * nAlpha * SLAB_DOUBLES;
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
      reduce(t, true);
    }
    if (Y == B) {  // s is k: along j, through the tile
      incl_state t = incl_state::empty();
      for (int n = 1; n < nAlpha; ++n) {
        const bool sym = al.a[n] == 0.5;
        for (int kq = 16 * w; kq < 16 * w + 16; ++kq)
          tile[kq * TILE_LD + lane] = no_entries ? 0.0 : in[((size_t)n * SBLK + kq) * SBLK + lane];
        __syncthreads();
        if (sl) {
          for (int jq = 16 * w; jq < 16 * w + 16; ++jq) {
            const int j = SBLK * X + jq;
            if (j >= V || j == s || (sym && s > j)) continue;
            t.push(tile[lane * TILE_LD + jq], sym ? al.log_doublet_prior2 : al.log_doublet_prior1, (j * V + s) * nAlpha + n);
          }
        }
        __syncthreads();
      }
      reduce(t, false);
    }
  }
  if (owner) state[ci * V + s] = st;
  if (threadIdx.x == 0) totb[ci * nblk + B] = tot;
}

// lane = (cell of the batch, sample); the lane of sample 0 also joins the cell's row blocks into tot
__global__ void __launch_bounds__(256)
    incl_finish_kernel(int64_t n, int V, int nAlpha, int nblk, const incl_state* __restrict__ state,
                       const evidence* __restrict__ totb, double* __restrict__ incl, double* __restrict__ tot,
                       double* __restrict__ dbl, int32_t* __restrict__ partner, int32_t* __restrict__ alpha_idx,
                       int32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t ci = i / V;
  const int s = (int)(i - ci * V);
  const incl_state st = state[i];
  incl[i] = st.ev.M + log(st.ev.S);
  dbl[i] = st.bv;
  int32_t pr = -1, ai = -1, fi = -1;
  if (st.bp >= 0) {
    const int32_t q = st.bp / nAlpha;
    const int32_t j = q / V, k = q - j * V;
    ai = st.bp - q * nAlpha;
    fi = j == s ? 1 : 0;
    pr = j == s ? k : j;
  }
  partner[i] = pr;
  alpha_idx[i] = ai;
  first[i] = fi;
  if (s == 0) {
    evidence e = totb[ci * nblk];
    for (int X = 1; X < nblk; ++X) e = evidence::merge(e, totb[ci * nblk + X]);
    tot[ci] = e.M + log(e.S);
  }
}

template <class T>
int copy_out(muxgl_handle* h, T* dst, const T* d_src, size_t n) {
  if (dst && n) HIPCHK(h, hipMemcpyAsync(dst, d_src, sizeof(T) * n, hipMemcpyDeviceToHost, h->stream));
  return 0;
}

}  // namespace

int demux_inclusion_run(muxgl_handle* h, const muxgl_demux_params* p, const demux_incl_out& out) {
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
    hipLaunchKernelGGL(incl_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, nc * nblk, d_state.p,
                       d_totb.p);
    HIPCHK(h, hipGetLastError());
    for (int64_t b0 = 0; b0 < nb_all; b0 += gb) {  // blocks in order (determinism, above)
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
