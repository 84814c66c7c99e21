// Test shim around popscle_amd/csrc/stream_plan.hpp: the slab budget, the cut of a streamed sweep into groups and the
// block list.  Plain C++; nothing here touches a device (see tests/test_stream_plan.py).
#include "stream_plan.hpp"

using namespace stream_plan;

extern "C" {

uint64_t probe_budget(const char* env_mb, uint64_t device_total) { return slab_budget_bytes(env_mb, (size_t)device_total); }

void probe_cut(int64_t cells, int64_t blocks, uint64_t per, uint64_t budget, int64_t* gc, int64_t* gb) {
  const stream_groups g = cut_groups(cells, blocks, (size_t)per, (size_t)budget);
  *gc = g.gc;
  *gb = g.gb;
}

// writes at most cap block codes to out and returns the length of the list
int probe_blocks(int nblk, int lower_only, int32_t stride, int cap, int32_t* out) {
  const std::vector<int32_t> b = block_list(nblk, lower_only != 0, stride);
  for (int i = 0; i < (int)b.size() && i < cap; ++i) out[i] = b[i];
  return (int)b.size();
}
}
