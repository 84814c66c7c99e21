// Test shim around the freemuxlet E-step chooser of popscle_amd/csrc/path_choice.hpp with the facts of the streamed
// E-step (fll_bytes, device_bytes) passed as well.  Plain C++; nothing here touches a device.  States are bit sets (see
// tests/test_path_choice_fmx_stream.py).
#include "path_choice.hpp"

using namespace path_choice;

extern "C" {

// states: 1 fqrow, 2 qrow, 4 row
int probe_fmx_estep2(int K, int32_t flags, int64_t S, int states, double row2_part_bytes, int64_t wave_items,
                     double fll_bytes, double device_bytes) {
  return (int)choose_fmx_estep({K, flags, S, (states & 1) != 0, (states & 2) != 0, (states & 4) != 0, row2_part_bytes,
                                wave_items, fll_bytes, device_bytes});
}

double probe_fll_bytes(int64_t rows, int K) { return fmx_fll_bytes(rows, K); }
}
