// Test shim around popscle_amd/csrc/match_plan.hpp, the cut of a muxgl_fmx_match_donors call: the parts of a cluster's
// SNPs, the donor lanes of a SNP slot, the bytes a cluster of a batch takes and the clusters of a batch for a budget.
// Plain C++; nothing here touches a device (see tests/test_fmx_match.py).
#include "match_plan.hpp"

extern "C" {

// part: FMM_PART of fmx_match.hip; want_ll: the call is asked for ll (0: ll0 and / or nsnps alone); budget in bytes
void probe_match_plan(int64_t S, int V, int K, int64_t part, int want_ll, uint64_t budget, int* np, int* vh, double* per_k,
                      int* kb) {
  *np = match_plan::parts(S, part);
  *vh = match_plan::lane_width(V);
  *per_k = match_plan::bytes_per_cluster(S, V, *np, want_ll != 0);
  *kb = match_plan::clusters_per_batch(K, *per_k, (size_t)budget);
}
}
