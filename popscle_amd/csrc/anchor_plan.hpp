// anchor_plan.hpp -- where an anchored freemuxlet run starts (muxgl_fmx_set_anchors; plain C++, no device).
//
// An anchored cluster needs no cells to have a genotype; the free clusters do, and the droplets of the genotyped donors
// should not start inside them.  The default start is made of calls the library already has: the greedy start with all K
// clusters, muxgl_fmx_set_clusters, muxgl_demux_set_gp(panel), muxgl_fmx_match_donors -- and then this relabelling of the
// greedy clusters, from llr[K][V] = ll - ll0 of the match, the markers nsnps[K] it saw, the cells of every greedy cluster
// and the anchored donors donor[n] (cluster i of the run is donor[i]):
//
//   candidates  (greedy cluster k, anchor i) ordered by llr[k][donor[i]] descending, then k ascending, then i ascending;
//               a NaN counts as -inf and a cluster with nsnps == 0 is no candidate
//   accepted    one to one, in that order, while llr > 0 -- the Bayes factor's own zero: "this donor" against "somebody
//               from the population".  An accepted cluster k becomes cluster i
//   anchors     without a match start empty
//   leftovers   the unmatched greedy clusters fill the free ids n .. K-1 in order of cell count descending, then id
//               ascending; those that do not fit leave their cells unassigned (-1) and the first E-step calls them
//
// popscle_amd/freemuxlet.py anchor_start is the same function in numpy; tests/test_anchor_plan.py holds the two equal.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace anchor_plan {

struct start {
  std::vector<int32_t> new_id;    // [K] the run's cluster of every greedy cluster, or -1
  std::vector<int32_t> match;     // [n] the greedy cluster an anchor starts from, or -1
  std::vector<double> match_llr;  // [n] its llr, or NaN
};

inline start plan(int K, int V, const double* llr /*[K][V]*/, const int32_t* nsnps /*[K]*/, const int64_t* ncells /*[K]*/,
                  int n, const int32_t* donor /*[n], each in [0, V)*/) {
  start st;
  st.new_id.assign((size_t)K, -1);
  st.match.assign((size_t)n, -1);
  st.match_llr.assign((size_t)n, std::numeric_limits<double>::quiet_NaN());
  struct cand {
    double v;
    int32_t k, i;
  };
  std::vector<cand> cs;
  for (int32_t k = 0; k < K; ++k) {
    if (nsnps[k] == 0) continue;
    for (int32_t i = 0; i < n; ++i) {
      const double v = llr[(size_t)k * V + donor[i]];
      if (v > 0.0) cs.push_back(cand{v, k, i});  // (false for a NaN; what is not above zero is never accepted)
    }
  }
  std::sort(cs.begin(), cs.end(), [](const cand& a, const cand& b) {
    if (a.v != b.v) return a.v > b.v;
    if (a.k != b.k) return a.k < b.k;
    return a.i < b.i;
  });
  std::vector<uint8_t> taken((size_t)K, 0);
  for (const cand& c : cs) {
    if (taken[(size_t)c.k] || st.match[(size_t)c.i] >= 0) continue;
    taken[(size_t)c.k] = 1;
    st.new_id[(size_t)c.k] = c.i;
    st.match[(size_t)c.i] = c.k;
    st.match_llr[(size_t)c.i] = c.v;
  }
  std::vector<int32_t> left;
  for (int32_t k = 0; k < K; ++k)
    if (!taken[(size_t)k]) left.push_back(k);
  std::stable_sort(left.begin(), left.end(), [&](int32_t a, int32_t b) { return ncells[a] > ncells[b]; });  // (ids ascending within a count)
  for (size_t j = 0; j < left.size() && n + (int64_t)j < K; ++j) st.new_id[(size_t)left[j]] = n + (int32_t)j;
  return st;
}

}  // namespace anchor_plan

// ---- `freemuxlet --anchor-refine-list FILE`: which anchored donors are MUXGL_ANCHOR_PRIOR (freemuxlet.refine_modes is the
// same function in Python).  ids: the anchored donors in cluster order; listed: the text of FILE, one sample ID per line --
// the first white-space separated word; empty lines and lines starting with '#' do not count.  A listed donor is PRIOR (1),
// the others HELD (0); naming one twice is allowed.  An ID that is no anchored donor: false, with the ID in *unknown.
#include <sstream>
#include <string>

namespace anchor_plan {

inline bool refine_modes(const std::vector<std::string>& ids, const std::string& listed, std::vector<uint8_t>* mode,
                         std::string* unknown) {
  mode->assign(ids.size(), 0);
  std::istringstream in(listed);
  std::string line, word;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    if (!(ls >> word) || word[0] == '#') continue;
    bool found = false;
    for (size_t i = 0; i < ids.size(); ++i)
      if (ids[i] == word) (*mode)[i] = 1, found = true;
    if (!found) {
      *unknown = word;
      return false;
    }
  }
  return true;
}

}  // namespace anchor_plan
