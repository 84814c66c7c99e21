// incl_fold.hpp -- what the two inclusion calls share (demux_incl.hip, fmx_incl.hip): the state of a (cell, item) -- an
// item is a sample or a cluster --, the owner's side of the fold of a group's slab into it by the workgroup that owns 64
// items, the transposing tile and the half of the finish kernels that does not decode.  What a position means, which is
// the "none" position and which total order picks the best hypothesis come from a traits struct:
//   struct Ops { static constexpr int32_t none;  static bool before(va, pa, vb, pb); }   // value, position of a and b
//
// State per (cell, item), 32 bytes: stream_fold::evidence (M, S) and (best value, its position).  `tot` has an evidence
// per (cell, row block X): each unit sees to it that every hypothesis is read in exactly one row role.
//
// Determinism: all outputs are bit-identical from call to call, for any slab budget, on a device group and on slabbed
// ranks, because the tree of the rounded sums is fixed.  A thread pushes its hypotheses in a fixed order (the units say
// which); a block's partial of an item is the four waves' as (0 + 1) + (2 + 3); an item's partials are merged into its
// state one block and role at a time, in stream_plan::block_list order, rows before columns in a diagonal block; tot's
// partial of a block is the xor butterfly (partner 1, 2, .., 32) over the 64 lanes of that merged row partial, merged per
// row block in the same order, and the row blocks ascending in finish_item.  A group only decides how many blocks one
// launch folds and a batch which cells share the device.  The best hypothesis is taken under Ops::before, a total order
// (value descending, then position ascending), so it does not depend on any grouping at all.
#pragma once
#include "incl_plan.hpp"
#include "stream_fold.hpp"

namespace incl_fold {

using stream_fold::evidence;

template <class Ops>
struct state {
  evidence ev;
  double bv;   // best LL over H_s (-1e300: none)
  int32_t bp;  // its position (Ops::none: none)
  int32_t pad;
  static __device__ __forceinline__ state empty() { return {{-__builtin_huge_val(), 0.0}, -1e300, Ops::none, 0}; }
  // (a value of -inf adds nothing to the sum and is never better than the empty -1e300)
  __device__ __forceinline__ void push(double v, double prior, int32_t pos) {
    ev.push(v + prior);
    if (Ops::before(v, pos, bv, bp)) bv = v, bp = pos;
  }
  static __device__ __forceinline__ state merge(const state& a, const state& b) {  // a first
    const bool ab = Ops::before(a.bv, a.bp, b.bv, b.bp);
    return {evidence::merge(a.ev, b.ev), ab ? a.bv : b.bv, ab ? a.bp : b.bp, 0};
  }
};

template <class Ops>
__global__ void __launch_bounds__(256)
    init_kernel(int64_t n_state, int64_t n_tot, state<Ops>* __restrict__ st, evidence* __restrict__ totb) {
  static_assert(sizeof(state<Ops>) == 32, "incl_plan::state_bytes_per_cell counts 32 bytes");
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_state) st[i] = state<Ops>::empty();
  if (i < n_tot) totb[i] = evidence{-__builtin_huge_val(), 0.0};
}

// The owner's side of the fold of one group by the workgroup (256 threads) of (cell blockIdx.x, item block B = blockIdx.y),
// which OWNS the state of the items s = 64 B + lane (n items a cell; sl: s is one).  The unit's kernel constructs it (the
// loads), walks the group's blocks in order in a plain loop of its own -- the compiler shapes that loop as it did before
// the owner was shared -- and per role of a block has every thread push its hypotheses into an empty state t and all 256
// threads call reduce(t, with_tot): the workgroup's partial of that block and role, into the state and, in the row role
// (with_tot), into tot.  reduce ends with a barrier, so LDS that a role read is free for the next one to write.  store()
// at the end.
template <class Ops>
struct owner {
  using state = incl_fold::state<Ops>;
  const int64_t ci;  // cell of the batch
  const int B, lane, w, s;
  const bool sl;
  state st;      // of item s, in wave 0
  evidence tot;  // of row block B, in thread 0
  __device__ __forceinline__ owner(int n, int nblk, const state* __restrict__ st_all, const evidence* __restrict__ totb)
      : ci(blockIdx.x), B(blockIdx.y), lane(threadIdx.x & 63), w(threadIdx.x >> 6), s(64 * B + lane), sl(s < n),
        st(state::empty()), tot{-__builtin_huge_val(), 0.0} {
    if (w == 0 && sl) st = st_all[ci * n + s];
    if (threadIdx.x == 0) tot = totb[ci * nblk + B];
  }
  __device__ __forceinline__ void reduce(const state& t, bool with_tot) {
    __shared__ state parts[4][64];
    parts[w][lane] = t;
    __syncthreads();
    if (w == 0) {
      const state r =
          state::merge(state::merge(parts[0][lane], parts[1][lane]), state::merge(parts[2][lane], parts[3][lane]));
      st = state::merge(st, r);
      if (with_tot) {  // (lanes without an item hold the empty evidence)
        evidence e = r.ev;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) e = evidence::merge(e, evidence{__shfl_xor(e.M, m, 64), __shfl_xor(e.S, m, 64)});
        if (lane == 0) tot = evidence::merge(tot, e);
      }
    }
    __syncthreads();
  }
  __device__ __forceinline__ void store(int n, int nblk, state* __restrict__ st_all, evidence* __restrict__ totb) const {
    if (w == 0 && sl) st_all[ci * n + s] = st;
    if (threadIdx.x == 0) totb[ci * nblk + B] = tot;
  }
};

// doubles per row of the transposing tile.  Lane l reads tile[l TILE_LD + q] (ds_read_b64: bank = dword address mod 64 =
// 2 l + 2 q mod 64 at TILE_LD = 65, per half wave of 32 lanes): 32 lanes on 32 distinct bank pairs, no conflict.
constexpr int TILE_LD = 64 + 1;
// wave w stores its 16 slot rows of a block's [slot][lane] values (zeros: every value is 0 and `rows` is not read); after
// the barrier tile[lane TILE_LD + q] is the transpose
__device__ __forceinline__ void tile_fill(double* tile, int lane, int w, const double* rows, bool zeros) {
  for (int kq = 16 * w; kq < 16 * w + 16; ++kq) tile[kq * TILE_LD + lane] = zeros ? 0.0 : rows[kq * 64 + lane];
  __syncthreads();
}

// The shared half of the finish kernels, around the unit's decoding of the position finish_item returns: incl and dbl of
// item i, then finish_tot on the lane of item s == 0, the cell's row blocks joined ascending into tot.  A sum without a
// finite term is -inf: the guard gives the bits of the unguarded M + log S, since S == 0 only with M == -inf, and
// -inf + log 0 = -inf (S is never NaN: evidence::push drops a term that is not > -inf, a NaN among them).
__device__ __forceinline__ double log_sum(const evidence& e) { return e.S > 0.0 ? e.M + log(e.S) : -__builtin_huge_val(); }
template <class Ops>
__device__ __forceinline__ int32_t finish_item(int64_t i, const state<Ops>* __restrict__ st_all, double* __restrict__ incl,
                                               double* __restrict__ dbl) {
  const state<Ops> st = st_all[i];
  incl[i] = log_sum(st.ev);
  dbl[i] = st.bv;
  return st.bp;
}
__device__ __forceinline__ void finish_tot(int64_t ci, int s, int nblk, const evidence* __restrict__ totb,
                                           double* __restrict__ tot) {
  if (s != 0) return;
  evidence e = totb[ci * nblk];
  for (int X = 1; X < nblk; ++X) e = evidence::merge(e, totb[ci * nblk + X]);
  tot[ci] = log_sum(e);
}

template <class T>
int copy_out(muxgl_handle* h, T* dst, const T* d_src, size_t n) {
  if (dst && n) HIPCHK(h, hipMemcpyAsync(dst, d_src, sizeof(T) * n, hipMemcpyDeviceToHost, h->stream));
  return 0;
}

}  // namespace incl_fold
