// match_plan.hpp -- the host side of muxgl_fmx_match_donors (fmx_match.hip): how a call is cut.  Plain C++ (no HIP), like
// stream_plan.hpp and incl_plan.hpp, so tests/test_fmx_match.py compiles it on its own (tests/csrc/match_plan_probe.cpp)
// and pins the arithmetic, and the GPU tests state their preconditions (how many batches, which kernel width) from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "lane_width.hpp"

namespace match_plan {

// parts of `part` consecutive SNPs a cluster's S SNPs are cut into (S >= 1): one log per (cluster, part, donor)
inline int parts(int64_t S, int64_t part) { return (int)((S + part - 1) / part); }

// donor lanes of a SNP slot: V rounded up to a power of two, 64 from 33 donors on (64 / VH SNPs side by side in a wave)
using ::lane_width;

// bytes of a cluster in a batch: logs of the parts (donors, where ll is asked for; HWE), counts of the parts, read
// counts, results
inline double bytes_per_cluster(int64_t S, int V, int NP, bool want_ll) {
  return (want_ll ? 8.0 * NP * V + 8.0 * V : 0.0) + 12.0 * NP + 4.0 * (double)S + 12.0;
}

// clusters of a batch (the last may be shorter): as many as the budget holds, at least one, at most K
inline int clusters_per_batch(int K, double per_k, size_t budget) {
  return (int)std::min<double>((double)K, std::max(1.0, (double)budget / per_k));
}

}  // namespace match_plan
