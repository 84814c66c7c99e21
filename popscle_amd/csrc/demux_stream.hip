// demux_stream.hip -- the streamed demuxlet call: any number of samples, device memory independent of C x V^2.
//
// The other paths materialise every hypothesis of a cell before the call reads them: the wave path's result slabs
// ([C][64 x 64 blocks][A][4096]) and, beyond 64 samples, the [C][V][V][A] tensor gathered from them.  The call only needs
// a few numbers per cell -- the top of each scan and two evidence sums -- so here the pair matrix is walked in 64 x 64
// blocks, a GROUP of (cells x blocks) at a time whose slab fits a fixed budget, and after each group a fold kernel merges
// the slab into a running state per cell; the slab is then reused.  A last kernel makes the call from that state with
// demux_call_decide (demux_call_body.hpp), the code every other call kernel ends in.
//
// Reference being replaced: cmd_cram_demuxlet.cpp:733-747 (pair sweep), :788-991 (evidence, scans, call).
//
// Why not the wave kernels of demux_wave.hip on these blocks: they would need to be edited (their entry points, plan and
// work units live in that file's anonymous namespace), and the machine code of the headline paths must not change.  The
// sweep (demux_stream_sweep.hpp, shared with demux_incl.hip) is the same arithmetic -- u = g_j . pG per (entry, alpha),
// then g_k . u per hypothesis, as a product in mantissa / exponent form with one log per hypothesis -- in a plainer
// mapping: lane = sample j of the block, the wave's KT partner samples k are wave-uniform (scalar loads), all alphas of
// the grid in one launch.
//
// State per cell, the fold and why records are bit-identical across budgets: stream_fold.hpp; groups and block list:
// stream_plan.hpp.  Here the lists are muxgl_call::top2 and the evidence sums those of sumLLK and sngLLK.  Ordering rule:
// value descending, then scan position ascending (muxgl_call::key_before), which is what the reference's update rule
// (bv < v, then nv < v) leaves.  Scan positions: j for singlets, (j V + k) A + n for doublets.  An alpha = 0.5 pair is
// listed once, as (lo, hi), with the value computed in the (hi, lo) orientation; demux_call_decide names its mirror the
// runner-up.
#include <algorithm>
#include <vector>

#include "demux_stream_sweep.hpp"
#include "stream_fold.hpp"

namespace {

using namespace muxgl_call;

// the lists of the state and their butterfly: DPP pairings (lane_partner)
struct demux_top2_ops {
  using list = top2;
  static __device__ __forceinline__ top2 empty() { return top2{-1e300, -1e300, -1, -1, -1e300}; }
  static __device__ __forceinline__ top2 merge(const top2& a, const top2& b) { return top2_merge<true>(a, b); }
  template <int M>
  static __device__ __forceinline__ top2 partner(const top2& t) { return top2_partner<M, true>(t); }
  template <int M>
  static __device__ __forceinline__ double partner(double x) { return lane_partner<M>(x); }
};
using stream_state = stream_fold::stream_state<demux_top2_ops>;

// Fold of one group: one workgroup per cell of the group (stream_fold::fold_blocks); a thread's hypotheses of a block
__global__ void __launch_bounds__(256)
    stream_fold_kernel(int64_t c0, int32_t b0, int32_t nb, const int32_t* __restrict__ blocks, int nblk,
                       const int64_t* __restrict__ cell_ptr, int V, int nAlpha, call_alpha al,
                       const double* __restrict__ slab, stream_state* __restrict__ state) {
  const int64_t c = c0 + blockIdx.x;
  if (cell_ptr[c] == cell_ptr[c + 1]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  stream_fold::fold_blocks(nb, state + c, [&](int z, stream_state& t) {
    const int b = blocks[b0 + z];
    const int X = b / nblk, Y = b - X * nblk;
    const int j = SBLK * X + lane;
    const double* in = slab + ((size_t)blockIdx.x * nb + z) * nAlpha * SLAB_DOUBLES;
    if (j >= V) return;
    if (Y == 0 && w == 0) {  // singlet of sample j (:806,828)
      const double v = in[lane];
      top2_insert(t.sng, v, j);
      const double term = v + al.log_single_prior;
      t.all.push(term);
      t.sgl.push(term);
    }
    for (int kq = 16 * w; kq < 16 * w + 16; ++kq) {
      const int k = SBLK * Y + kq;
      if (k >= V || k == j) continue;
      for (int n = 1; n < nAlpha; ++n) {
        const double v = in[((size_t)n * SBLK + kq) * SBLK + lane];
        if (al.a[n] == 0.5) {  // (hi, lo) orientation only, listed as (lo, hi): see the header
          if (k > j) continue;
          t.all.push(v + al.log_doublet_prior2);  // :812-815
          top2_insert(t.dbl, v, (k * V + j) * nAlpha + n);
        } else {
          t.all.push(v + al.log_doublet_prior1);
          top2_insert(t.dbl, v, (j * V + k) * nAlpha + n);
        }
      }
    }
  });
}

// the call from the state: one lane per cell (demux_call_decide's note)
__global__ void __launch_bounds__(64)
    stream_call_kernel(int64_t C, const int64_t* __restrict__ cell_ptr, int V, int nAlpha, call_alpha al,
                       const stream_state* __restrict__ state, muxgl_demux_cell* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const stream_state& s = state[c];
  const call_partial cp{s.sng, s.dbl, s.all.M, s.all.S, s.sgl.M, s.sgl.S};
  demux_call_decide(cp, (int32_t)(cell_ptr[c + 1] - cell_ptr[c]), V, nAlpha, al, out + c);
}

}  // namespace

int demux_stream_launch(muxgl_handle* h, const muxgl_demux_params* p) {
  const int V = h->V, A = p->n_alpha;
  if ((double)V * V * A >= 2147483648.0)
    MUXGL_FAIL(h, "streamed demuxlet call: V=%d with %d alphas exceeds the int32 scan positions (V*V*n_alpha < 2^31)", V, A);
  if (h->want_full_ll)
    MUXGL_FAIL(h, "muxgl_demux_run: full_ll is not available on the streamed path (V=%d; more than 255 samples, a job whose "
                  "[C][V][V][A] tensor does not fit the device, or MUXGL_FLAG_FORCE_STREAMED_CALL): pass full_ll = NULL", V);
  bool all_sym = true;
  for (int n = 1; n < A; ++n) all_sym = all_sym && p->alpha[n] == 0.5;
  // blocks that hold a hypothesis the call reads: with alpha = 0.5 only the (hi, lo) orientation, and the singlets in Y = 0
  // -- the only blocks of a grid without a doublet alpha (the reference then calls among the singlets alone)
  const int nblk = (V + SBLK - 1) / SBLK;
  std::vector<int32_t> blocks = stream_plan::block_list(nblk, all_sym, nblk);  // X * nblk + Y
  if (A == 1) {
    blocks.clear();
    for (int X = 0; X < nblk; ++X) blocks.push_back(X * nblk);
  }
  const int64_t nb_all = (int64_t)blocks.size();
  const size_t per = (size_t)A * SLAB_DOUBLES * sizeof(double);  // one (cell, block) of the slab
  const auto [gc, gb] = stream_plan::cut_groups(h->C, nb_all, per, dev_slab_budget("MUXGL_DEMUX_SLAB_MB"));

  dev_tmp<int32_t> d_blocks;
  dev_tmp<double> d_pg, d_slab;
  dev_tmp<stream_state> d_state;
  if (dev_alloc(h, &d_blocks.p, blocks.size())) return 1;
  if (dev_alloc(h, &d_pg.p, (size_t)h->nnz * A * 9)) return 1;
  if (dev_alloc(h, &d_slab.p, (size_t)gc * gb * A * SLAB_DOUBLES)) return 1;
  if (dev_alloc(h, &d_state.p, (size_t)h->C)) return 1;
  HIPCHK(h, hipMemcpyAsync(d_blocks.p, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, h->stream));
  tic(h, MUXGL_T_DEMUX_SWEEP);
  if (demux_entry_pg_launch(h, p, d_pg.p)) return 1;
  hipLaunchKernelGGL(stream_fold::stream_init_kernel<demux_top2_ops>, dim3((unsigned)((h->C + 255) / 256)), dim3(256), 0,
                     h->stream, h->C, d_state.p);
  HIPCHK(h, hipGetLastError());
  const call_alpha al = make_call_alpha(p, V);
  for (int64_t c0 = 0; c0 < h->C; c0 += gc) {
    const int64_t nc = std::min(gc, h->C - c0);
    for (int64_t b0 = 0; b0 < nb_all; b0 += gb) {  // blocks in order: stream_fold.hpp (determinism)
      const int32_t nb = (int32_t)std::min(gb, nb_all - b0);
      if (sweep_dispatch(h, c0, nc, (int32_t)b0, nb, d_blocks.p, nblk, d_pg.p, A, d_slab.p)) return 1;
      hipLaunchKernelGGL(stream_fold_kernel, dim3((unsigned)nc), dim3(256), 0, h->stream, c0, (int32_t)b0, nb, d_blocks.p,
                         nblk, h->d_cell_ptr, V, A, al, d_slab.p, d_state.p);
      HIPCHK(h, hipGetLastError());
    }
  }
  toc(h, MUXGL_T_DEMUX_SWEEP);
  tic(h, MUXGL_T_DEMUX_CALL);
  hipLaunchKernelGGL(stream_call_kernel, dim3((unsigned)((h->C + 63) / 64)), dim3(64), 0, h->stream, h->C, h->d_cell_ptr,
                     V, A, al, d_state.p, h->d_dcells);
  HIPCHK(h, hipGetLastError());
  toc(h, MUXGL_T_DEMUX_CALL);
  return 0;
}
