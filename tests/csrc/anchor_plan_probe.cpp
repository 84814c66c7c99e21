// Test shim around popscle_amd/csrc/anchor_plan.hpp, the relabelling of the greedy clusters an anchored freemuxlet run
// starts from.  Plain C++; nothing here touches a device (see tests/test_anchor_plan.py).
#include "anchor_plan.hpp"

extern "C" {

// new_id[K], match[n], match_llr[n]: anchor_plan::start's three vectors
void probe_anchor_plan(int K, int V, const double* llr, const int32_t* nsnps, const int64_t* ncells, int n, const int32_t* donor,
                       int32_t* new_id, int32_t* match, double* match_llr) {
  const anchor_plan::start st = anchor_plan::plan(K, V, llr, nsnps, ncells, n, donor);
  for (int k = 0; k < K; ++k) new_id[k] = st.new_id[(size_t)k];
  for (int i = 0; i < n; ++i) match[i] = st.match[(size_t)i], match_llr[i] = st.match_llr[(size_t)i];
}
}
