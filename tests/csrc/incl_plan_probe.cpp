// Test shim around popscle_amd/csrc/incl_plan.hpp: the cut of muxgl_demux_inclusion's cells into batches whose state
// shares the slab budget with the sweep's slab.  Plain C++; nothing here touches a device (see tests/test_demux_inclusion.py).
#include <cstring>

#include "incl_plan.hpp"

extern "C" {

uint64_t probe_state_bytes(int V) { return incl_plan::state_bytes_per_cell(V); }

// 1 and (batch, gb) when the cut exists; else 0 and the message the library reports in msg[cap]
int probe_batches(int64_t cells, int64_t blocks, int V, uint64_t per, uint64_t budget, int64_t* batch, int64_t* gb, char* msg,
                  int cap) {
  const size_t spc = incl_plan::state_bytes_per_cell(V);
  const incl_plan::batches b = incl_plan::cut_batches(cells, blocks, spc, (size_t)per, (size_t)budget);
  *batch = b.batch;
  *gb = b.gb;
  if (!b.ok) {
    strncpy(msg, incl_plan::too_small_message(V, spc, (size_t)per, (size_t)budget).c_str(), (size_t)cap - 1);
    msg[cap - 1] = 0;
  }
  return b.ok ? 1 : 0;
}
}
