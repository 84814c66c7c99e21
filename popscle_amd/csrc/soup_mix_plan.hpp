// soup_mix_plan.hpp -- the host side of muxgl_demux_soup_mix (soup_mix.hip): which markers of a read histogram take part,
// how they are cut into the blocks of the update sweep, and how a wave is packed below 64 components.  Plain C++ (no HIP),
// like match_plan.hpp and table_plan.hpp, so tests/test_soup_mix.py compiles it on its own
// (tests/csrc/soup_mix_plan_probe.cpp) and holds it against a direct loop, and the GPU tests state their preconditions
// (how many blocks, which lane width) from it.
//
// A histogram is a list of records (key, count) with key = marker * 256 + read byte, strictly ascending, count > 0 and no
// byte MUXGL_READ_OTHER.  Every cut below depends on the histogram, the panel's has_gp and the number of components alone:
// that is what makes the fit the same number on one device, on a group and through the sharded driver.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "lane_width.hpp"

namespace soup_mix_plan {

// active markers per block of the update sweep: one partial row of the transposed product per block, added in block
// order.  A constant: it is part of every rounded sum's tree, so it may depend on no device and no budget.
constexpr int UPDATE_BLOCK = 256;

// component lanes of a marker slot: M rounded up to a power of two, 64 from 33 components on (64 / width markers side by
// side in a wave; beyond 64 components a lane takes the components lane, lane + 64, ...)
using ::lane_width;
inline int markers_per_wave(int M) { return 64 / lane_width(M); }
inline int64_t waves(int64_t n_markers, int M) {
  const int g = markers_per_wave(M);
  return (n_markers + g - 1) / g;
}
inline int64_t update_blocks(int64_t n_active) { return (n_active + UPDATE_BLOCK - 1) / UPDATE_BLOCK; }

// why a histogram is refused: 0 fine, else the index of the offending record in *at
enum { HIST_OK = 0, HIST_UNSORTED = 1, HIST_MARKER = 2, HIST_BYTE = 3, HIST_COUNT = 4 };
inline int check_hist(int64_t n_rec, const int64_t* keys, const int64_t* counts, int64_t S, int64_t* at) {
  for (int64_t i = 0; i < n_rec; ++i) {
    *at = i;
    if (keys[i] < 0 || (keys[i] >> 8) >= S) return HIST_MARKER;
    if ((keys[i] & 0xFF) == 0xFF) return HIST_BYTE;
    if (i > 0 && keys[i] <= keys[i - 1]) return HIST_UNSORTED;
    if (counts[i] <= 0) return HIST_COUNT;
  }
  return HIST_OK;
}

// the markers of a list and their records: marker[i] has the records rec[rec_ptr[i] .. rec_ptr[i + 1]), each a position in
// the histogram, in key order
struct marker_list {
  std::vector<int32_t> marker;
  std::vector<int64_t> rec_ptr;  // [marker.size() + 1]
  std::vector<int64_t> rec;      // [rec_ptr.back()]
  int64_t n_reads = 0;           // the counts of the list's records added up
};

// the candidates: the markers with genotypes and at least one record, ascending (the histogram is sorted by marker)
inline marker_list candidates(int64_t n_rec, const int64_t* keys, const int64_t* counts, const uint8_t* has_gp) {
  marker_list c;
  for (int64_t i = 0; i < n_rec;) {
    const int64_t s = keys[i] >> 8;
    int64_t j = i;
    while (j < n_rec && (keys[j] >> 8) == s) ++j;
    if (has_gp[s]) {
      c.marker.push_back((int32_t)s);
      c.rec_ptr.push_back((int64_t)c.rec.size());
      for (int64_t k = i; k < j; ++k) {
        c.rec.push_back(k);
        c.n_reads += counts[k];
      }
    }
    i = j;
  }
  c.rec_ptr.push_back((int64_t)c.rec.size());
  return c;
}

// the active markers: the candidates whose R + A at the start (ra[i], from the device) is above 0
inline marker_list active(const marker_list& c, const double* ra, const int64_t* counts) {
  marker_list a;
  for (size_t i = 0; i < c.marker.size(); ++i) {
    if (!(ra[i] > 0.0)) continue;
    a.marker.push_back(c.marker[i]);
    a.rec_ptr.push_back((int64_t)a.rec.size());
    for (int64_t k = c.rec_ptr[i]; k < c.rec_ptr[i + 1]; ++k) {
      a.rec.push_back(c.rec[(size_t)k]);
      a.n_reads += counts[c.rec[(size_t)k]];
    }
  }
  a.rec_ptr.push_back((int64_t)a.rec.size());
  return a;
}

}  // namespace soup_mix_plan
