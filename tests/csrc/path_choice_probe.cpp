// Test shim around popscle_amd/csrc/path_choice.hpp: every chooser with its facts passed flat.  Plain C++; nothing here
// touches a device.  States are bit sets (see tests/test_path_choice.py).
#include "path_choice.hpp"

using namespace path_choice;

extern "C" {

// states: 1 row, 2 qrow, 4 d_gpq, 8 d_qent, 16 wave.  Returns the demux_path; *ll_first: demux_ll_first
int probe_demux(int V, int A, const double* alpha, int32_t flags, int64_t C, int64_t S, int states, int want_full_ll,
                double row2_part_bytes, double wave_bytes, double device_bytes, int* ll_first) {
  const demux_facts f = {V, A, alpha, flags, C, S, (states & 1) != 0, (states & 2) != 0, (states & 4) != 0,
                         (states & 8) != 0, (states & 16) != 0, want_full_ll != 0, row2_part_bytes, wave_bytes,
                         device_bytes};
  const demux_path p = choose_demux_path(f);
  *ll_first = demux_ll_first(f, p);
  return (int)p;
}

double probe_wave_bytes(int64_t nnz, int64_t C, int64_t n_over, int V, int A) {
  return demux_wave_sizes(nnz, C, n_over, V, A).bytes();
}

// states: 1 fqrow, 2 qrow, 4 row
int probe_fmx_estep(int K, int32_t flags, int64_t S, int states, double row2_part_bytes, int64_t wave_items) {
  return (int)choose_fmx_estep({K, flags, S, (states & 1) != 0, (states & 2) != 0, (states & 4) != 0, row2_part_bytes,
                                wave_items});
}

int probe_fmx_call(int K, int32_t flags) { return (int)choose_fmx_call(K, flags); }

int probe_fmx_mstep(int K, int32_t flags, int64_t ns, int64_t nnz, int64_t C) {
  return (int)choose_fmx_mstep({K, flags, ns, nnz, C});
}

int probe_greedy(int K, int32_t flags, int64_t P, int cus, int gb) { return (int)choose_greedy({K, flags, P, cus, gb}); }
}
