// incl_plan.hpp -- the host side of muxgl_demux_inclusion (demux_incl.hip) and muxgl_fmx_inclusion (fmx_incl.hip): how the
// cells are cut into batches whose state shares the slab budget with the sweep's slab.  Plain C++ (no HIP), like stream_plan.hpp, so
// tests/test_demux_inclusion.py compiles it on its own and pins the arithmetic.
#pragma once
#include <cstdio>
#include <string>

#include "stream_plan.hpp"

namespace incl_plan {

// bytes the call holds per cell of a batch of n items (samples, clusters) besides the slab: the state (32 B per item:
// evidence, best value, position), the outputs the finish kernel writes (out_bytes_per_item: demuxlet 8 + 8 + 4 + 4 + 4 =
// 28, freemuxlet 8 + 8 + 4 = 20; and 8 B per cell) and the evidence of `tot` per 64-item row block (16 B)
inline size_t state_bytes_per_cell(int n, size_t out_bytes_per_item) {
  const size_t nblk = ((size_t)n + 63) / 64;
  return (size_t)n * (32 + out_bytes_per_item) + nblk * 16 + 8;
}

// A batch of whole cells keeps its state on the device while its (cells x blocks) are swept in groups
// (stream_plan::cut_groups over the batch); the batch is finished and copied out before the next.  batch = as many
// cells as fit the budget with one block of slab each, so a group is always (the whole batch) x (gb blocks).
// ok = false: not even one cell's state and one (cell, block) of slab fit -- the caller reports it, naming the variable.
struct batches {
  bool ok;
  int64_t batch;  // cells of a batch (the last may be shorter)
  int64_t gb;     // blocks of a group
};
inline batches cut_batches(int64_t cells, int64_t blocks, size_t state_per_cell, size_t slab_per_cell_block, size_t budget) {
  const size_t one = state_per_cell + slab_per_cell_block;
  if (cells < 1 || blocks < 1 || budget < one) return {false, 0, 0};
  const int64_t batch = std::min<int64_t>(cells, (int64_t)(budget / one));
  const stream_plan::stream_groups g =
      stream_plan::cut_groups(batch, blocks, slab_per_cell_block, budget - (size_t)batch * state_per_cell);
  return {true, g.gc, g.gb};  // (g.gc == batch: one block of every cell of the batch fits what the state leaves)
}

// what `call` reports when cut_batches says no: n items, named `letter` (V samples, K clusters), budget variable `env`
inline std::string too_small_message(const char* call, char letter, int n, size_t state_per_cell, size_t slab_per_cell_block,
                                     size_t budget, const char* env) {
  char buf[320];
  snprintf(buf, sizeof(buf),
           "%s: the state of one cell (%zu bytes at %c=%d) and one block of the sweep (%zu bytes) exceed the slab budget of "
           "%zu bytes: raise %s",
           call, state_per_cell, letter, n, slab_per_cell_block, budget, env);
  return buf;
}

// the two calls' bindings of these, which the units and the probes under tests/csrc both use
inline size_t state_bytes_per_cell(int V) { return state_bytes_per_cell(V, 28); }
inline size_t fmx_state_bytes_per_cell(int K) { return state_bytes_per_cell(K, 20); }
inline std::string too_small_message(int V, size_t state_per_cell, size_t slab_per_cell_block, size_t budget) {
  return too_small_message("muxgl_demux_inclusion", 'V', V, state_per_cell, slab_per_cell_block, budget,
                           "MUXGL_DEMUX_SLAB_MB");
}
inline std::string fmx_too_small_message(int K, size_t state_per_cell, size_t slab_per_cell_block, size_t budget) {
  return too_small_message("muxgl_fmx_inclusion", 'K', K, state_per_cell, slab_per_cell_block, budget, "MUXGL_FMX_SLAB_MB");
}

}  // namespace incl_plan
