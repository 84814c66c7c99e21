// soup_mix_plan_probe.cpp -- popscle_amd/csrc/soup_mix_plan.hpp behind a C interface for tests/test_soup_mix.py (plain C++:
// no device code, no device is touched).
#include "soup_mix_plan.hpp"

namespace sp = soup_mix_plan;

extern "C" {

// out[0..3] = UPDATE_BLOCK, lane_width(M), markers_per_wave(M), waves(n_markers, M); out[4] = update_blocks(n_markers)
void probe_soup_mix_cut(int M, int64_t n_markers, int64_t* out) {
  out[0] = sp::UPDATE_BLOCK;
  out[1] = sp::lane_width(M);
  out[2] = sp::markers_per_wave(M);
  out[3] = sp::waves(n_markers, M);
  out[4] = sp::update_blocks(n_markers);
}

int probe_soup_mix_check(int64_t n_rec, const int64_t* keys, const int64_t* counts, int64_t S, int64_t* at) {
  return sp::check_hist(n_rec, keys, counts, S, at);
}

// the candidates, then the active ones among them by ra [candidates]: ra == NULL stops after the candidates.  marker
// [n_rec], rec_ptr [n_rec + 1], rec [n_rec]; returns the number of markers, *n_reads their reads
int64_t probe_soup_mix_lists(int64_t n_rec, const int64_t* keys, const int64_t* counts, const uint8_t* has_gp, const double* ra,
                             int32_t* marker, int64_t* rec_ptr, int64_t* rec, int64_t* n_reads) {
  sp::marker_list l = sp::candidates(n_rec, keys, counts, has_gp);
  if (ra) l = sp::active(l, ra, counts);
  for (size_t i = 0; i < l.marker.size(); ++i) marker[i] = l.marker[i];
  for (size_t i = 0; i < l.rec_ptr.size(); ++i) rec_ptr[i] = l.rec_ptr[i];
  for (size_t i = 0; i < l.rec.size(); ++i) rec[i] = l.rec[i];
  *n_reads = l.n_reads;
  return (int64_t)l.marker.size();
}
}
