// stream_plan.hpp -- the host side of the streamed paths (demux_stream.hip, fmx_stream.hip, demux_singlets.hip): the slab
// budget, the cut of (cells x blocks) into groups whose slab fits it, and the list of 64 x 64 blocks of a pair matrix.
// Plain C++ (no HIP), so tests/test_stream_plan.py compiles it on its own and pins the arithmetic.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace stream_plan {

// slab budget in bytes: the variable env_mb (MUXGL_DEMUX_SLAB_MB, MUXGL_FMX_SLAB_MB) in MB when it holds a positive
// number, else 4 GiB bounded by a third of the device's memory (the handle cache's cap; device_total = 0: unknown).
// The environment is read at each call, so that a test can change it between handles.
inline size_t slab_budget_bytes(const char* env_mb, size_t device_total) {
  if (const char* s = getenv(env_mb)) {
    const long long mb = atoll(s);
    if (mb > 0) return (size_t)mb << 20;
  }
  const size_t b = (size_t)4 << 30;
  return device_total > 0 ? std::min(b, device_total / 3) : b;
}

// groups of a sweep over cells x blocks (both >= 1) whose slab takes bytes_per_cell_block per (cell, block): all cells x
// as many blocks as fit the budget; if one block of every cell does not fit, one block x as many cells as fit.  gb is
// a grid dimension (<= 65535); a budget below one (cell, block) counts as one.
struct stream_groups {
  int64_t gc, gb;  // cells, blocks of a group
};
inline stream_groups cut_groups(int64_t cells, int64_t blocks, size_t bytes_per_cell_block, size_t budget) {
  const size_t per = bytes_per_cell_block;
  budget = std::max(budget, per);
  stream_groups g;
  if ((size_t)cells * per <= budget) {
    g.gc = cells;
    g.gb = std::min<int64_t>(blocks, (int64_t)(budget / ((size_t)cells * per)));
  } else {
    g.gb = 1;
    g.gc = (int64_t)(budget / per);
  }
  g.gb = std::min<int64_t>(g.gb, 65535);
  g.gc = std::min<int64_t>(g.gc, (int64_t)1 << 30);
  return g;
}

// the blocks (X, Y) of an nblk x nblk pair matrix as X * stride + Y (stride >= nblk; each user decodes its own), X
// ascending, then Y: the sweep order, and with it the order in which a cell's partials are merged (stream_fold.hpp).
// lower_only: X >= Y.
inline std::vector<int32_t> block_list(int nblk, bool lower_only, int32_t stride) {
  std::vector<int32_t> b;
  for (int X = 0; X < nblk; ++X)
    for (int Y = 0; Y < (lower_only ? X + 1 : nblk); ++Y) b.push_back(X * stride + Y);
  return b;
}

}  // namespace stream_plan
