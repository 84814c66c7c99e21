// Test shim around popscle_amd/csrc/pairs_plan.hpp, the cut of a muxgl_fmx_cluster_pairs call: the parts of the SNPs, the
// partner lanes of a SNP slot, the partner blocks, the bytes a row cluster of a batch takes, the row clusters of a batch
// for a budget, the batches of a block, and which (partner block, tile) units are launched.
// Plain C++; nothing here touches a device (see tests/test_fmx_pairs.py).
#include "pairs_plan.hpp"

extern "C" {

int64_t probe_pairs_part() { return pairs_plan::PART; }
int probe_pairs_tmax() { return pairs_plan::TMAX; }

// budget in bytes
void probe_pairs_plan(int64_t S, int K, uint64_t budget, int* np, int* kh, int* nblocks, double* per_row, int* rows) {
  *np = pairs_plan::parts(S);
  *kh = pairs_plan::lane_width(K);
  *nblocks = pairs_plan::blocks(K);
  *per_row = pairs_plan::bytes_per_row(*np);
  *rows = pairs_plan::rows_per_batch(K, *per_row, (size_t)budget);
}

// the batches of block Y at `rows` row clusters per batch: r0[i], r1[i] (first row, one past the last); returns their number
int probe_pairs_batches(int K, int Y, int rows, int cap, int* r0, int* r1) {
  const int n = pairs_plan::batches(K, Y, rows);
  for (int i = 0; i < n && i < cap; ++i) {
    r0[i] = pairs_plan::first_row(Y) + i * rows;
    r1[i] = std::min(K, r0[i] + rows);
  }
  return n;
}

// the launched units of a call as the host loop of fmx_pairs.hip walks them (block, batch, tile): ys[i], tiles[i];
// returns their number (only the first `cap` are written).  Every walked unit is checked against unit_exists: -1 if
// the walk and the predicate disagree.
int probe_pairs_units(int K, int T, int rows, int cap, int* ys, int* tiles) {
  int n = 0;
  for (int Y = 0; Y < pairs_plan::blocks(K); ++Y)
    for (int r0 = pairs_plan::first_row(Y); r0 < K; r0 += rows) {
      const int r1 = std::min(K, r0 + rows);
      const int lo = std::max(pairs_plan::first_tile(Y, T), r0 / T), hi = (r1 + T - 1) / T;
      for (int t = lo; t < hi; ++t, ++n) {
        if (!pairs_plan::unit_exists(K, Y, t, T)) return -1;
        if (n < cap) ys[n] = Y, tiles[n] = t;
      }
    }
  return n;
}

int probe_pairs_unit_exists(int K, int Y, int tile, int T) { return pairs_plan::unit_exists(K, Y, tile, T) ? 1 : 0; }
}
