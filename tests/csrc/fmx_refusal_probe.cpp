// C shim over popscle_amd/csrc/fmx_refusal.hpp for tests/test_fmx_refusal.py (host only: no device code)
#include <cstdint>

#include "fmx_refusal.hpp"

extern "C" {

int probe_fmx_refusal(const char* who, const char* what, int have_pileup, int prepared, int K, int sng_state, char* why,
                      uint64_t n) {
  return fmx_table_refusal(who, what, have_pileup != 0, prepared != 0, K, sng_state, why, (size_t)n);
}

int probe_fmx_sng_state(int i) { return i == 0 ? FMX_SNG_NONE : i == 1 ? FMX_SNG_READY : FMX_SNG_STALE; }
}
