// stream_fold.hpp -- the device side the streamed calls share (demux_stream.hip, fmx_stream.hip): the running state of a
// cell and the fold of a group's slab into it.
//
// State per cell (stream_state): the top two (value, scan position) and the third value of the singlet and of the doublet
// scan, and two evidence sums, each as (largest term M, sum S of exp(term - M)).  What the list type is, how two lists
// merge and how a lane reaches its butterfly partner differ between the two algorithms and come from a traits struct:
//   struct Ops { using list; list empty(); list merge(a, b);  template <int M> list partner(list), double partner(double); }
//
// Determinism: records are bit-identical whatever the budget cuts (tests/test_demux_many_samples_gpu.py,
// tests/test_fmx_many_clusters_gpu.py).
//   * The top two of a scan are taken under a total order (value descending, then scan position ascending), so they and
//     the third value do not depend on how the hypotheses are grouped.
//   * The evidence sums are rounded along the way, so their tree is fixed: a block's partial is reduced thread -> wave
//     butterfly (partner 1, 2, .., 32 as Ops pairs the lanes) -> the four waves as (0 + 1) + (2 + 3), and a cell's
//     partials are merged into its state in block order (stream_plan::block_list), one block at a time.  A group only
//     decides how many blocks one launch folds.  evidence::merge is one fixed expression with a first, and each
//     algorithm keeps its own pairing of the lanes: another pairing gives other bits.
#pragma once
#include "demux_call_body.hpp"

namespace stream_fold {

struct evidence {
  double M, S;  // largest term, sum of exp(term - M)
  __device__ __forceinline__ void push(double t) {
    using muxgl_call::exp_nonpos;
    if (!(t > -__builtin_huge_val())) return;  // exp(-inf) adds nothing
    if (t > M) {
      S = (S > 0.0 ? S * exp_nonpos(M - t) : 0.0) + 1.0;
      M = t;
    } else {
      S += exp_nonpos(t - M);
    }
  }
  static __device__ __forceinline__ evidence merge(const evidence& a, const evidence& b) {
    using muxgl_call::exp_nonpos;
    evidence r;
    r.M = fmax(a.M, b.M);
    r.S = (a.S > 0.0 ? a.S * exp_nonpos(a.M - r.M) : 0.0) + (b.S > 0.0 ? b.S * exp_nonpos(b.M - r.M) : 0.0);
    return r;
  }
};

template <class Ops>
struct stream_state {
  typename Ops::list sng, dbl;
  evidence all, sgl;  // every hypothesis; the singlets alone
  static __device__ __forceinline__ stream_state empty() {
    return {Ops::empty(), Ops::empty(), {-__builtin_huge_val(), 0.0}, {-__builtin_huge_val(), 0.0}};
  }
  static __device__ __forceinline__ stream_state merge(const stream_state& a, const stream_state& b) {  // a first
    return {Ops::merge(a.sng, b.sng), Ops::merge(a.dbl, b.dbl), evidence::merge(a.all, b.all), evidence::merge(a.sgl, b.sgl)};
  }
};

// the state of the lane's partner in step M of the butterfly
template <int M, class Ops>
__device__ __forceinline__ stream_state<Ops> partner(const stream_state<Ops>& s) {
  return {Ops::template partner<M>(s.sng), Ops::template partner<M>(s.dbl),
          {Ops::template partner<M>(s.all.M), Ops::template partner<M>(s.all.S)},
          {Ops::template partner<M>(s.sgl.M), Ops::template partner<M>(s.sgl.S)}};
}

template <class Ops>
__global__ void __launch_bounds__(256) stream_init_kernel(int64_t n, stream_state<Ops>* __restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st[i] = stream_state<Ops>::empty();
}

// Fold of one group by the workgroup (256 threads) of one cell: for z = 0 .. nb - 1, the group's blocks in order,
// partial(z, t) adds the thread's hypotheses of block z to the empty state t; the workgroup's states are reduced in the
// fixed tree of the header and merged into *cell by thread 0.
template <class Ops, class F>
__device__ __forceinline__ void fold_blocks(int32_t nb, stream_state<Ops>* __restrict__ cell, F&& partial) {
  using state = stream_state<Ops>;
  __shared__ state parts[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  state st = *cell;  // (read by every thread, written by thread 0 at the end)
  for (int z = 0; z < nb; ++z) {
    state t = state::empty();
    partial(z, t);
    wave_for<0, 6>([&](auto sc) {
      constexpr int m = 1 << decltype(sc)::value;
      t = state::merge(t, partner<m>(t));
    });
    if (lane == 0) parts[w] = t;
    __syncthreads();
    if (threadIdx.x == 0)
      st = state::merge(st, state::merge(state::merge(parts[0], parts[1]), state::merge(parts[2], parts[3])));
    __syncthreads();
  }
  if (threadIdx.x == 0) *cell = st;
}

}  // namespace stream_fold
