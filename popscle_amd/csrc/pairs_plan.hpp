// pairs_plan.hpp -- the host side of muxgl_fmx_cluster_pairs (fmx_pairs.hip): how a call is cut.  Plain C++ (no HIP), in the
// manner of match_plan.hpp, so tests/test_fmx_pairs.py compiles it on its own (tests/csrc/pairs_plan_probe.cpp) and pins the
// arithmetic, and the GPU tests state their preconditions (how many batches, which kernel width) from it.
//
// The triangle of pairs a > b is cut into partner blocks Y of 64 clusters b (lane = b - 64 Y) and tiles of T row clusters
// a (tile i holds a = i T .. i T + T - 1, aligned to multiples of T over the whole call, whatever the block or the batch).
// Block Y exists when it holds a b that some a is above: 64 Y < K - 1.  Its first tile is the one that holds a = 64 Y + 1,
// and every later tile up to the one holding K - 1 belongs to it; lanes with b >= a or b >= K compute and do not store.
// The row clusters of a block are swept in batches of a multiple of PAIRS_TMAX rows, so a batch starts at a tile boundary
// for every tile size.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace pairs_plan {

constexpr int64_t PART = 2048;  // SNPs per part: one log per (pair, part) and product
constexpr int TMAX = 8;         // the largest tile of row clusters a wave carries

// parts of PART consecutive SNPs the S SNPs are cut into (S >= 1)
inline int parts(int64_t S) { return (int)((S + PART - 1) / PART); }

// partner lanes of a SNP slot: K rounded up to a power of two, at least 2, 64 from 33 clusters on (64 / KH SNPs side by
// side in a wave)
inline int lane_width(int K) {
  int KH = 64;
  while (KH > 2 && KH / 2 >= K) KH /= 2;
  return KH;
}

// partner blocks of a call: those with 64 Y < K - 1
inline int blocks(int K) { return K < 2 ? 0 : (K - 2) / 64 + 1; }

// first tile of block Y (the one holding a = 64 Y + 1) and one past the last tile of the call
inline int first_tile(int Y, int T) { return (64 * Y + 1) / T; }
inline int end_tile(int K, int T) { return (K + T - 1) / T; }

// whether the unit (block Y, tile) is launched: it holds a pair a > b with a < K
inline bool unit_exists(int K, int Y, int tile, int T) {
  return Y >= 0 && Y < blocks(K) && tile >= first_tile(Y, T) && tile < end_tile(K, T);
}

// bytes of a row cluster in a batch: per part and partner lane two logs and a count
inline double bytes_per_row(int NP) { return 20.0 * 64.0 * NP; }

// row clusters of a batch (the last of a block may be shorter): as many as the budget holds, a multiple of TMAX, at
// least TMAX, at most K rounded up to it
inline int rows_per_batch(int K, double per_row, size_t budget) {
  const double cap = (double)((K + TMAX - 1) / TMAX) * TMAX;
  const double fit = std::min(cap, (double)budget / per_row);
  return std::max(TMAX, (int)(fit / TMAX) * TMAX);
}

// first row of block Y's first batch: the start of the TMAX-aligned group holding a = 64 Y + 1 (so that batches start at
// tile boundaries of every tile size); tiles of it below first_tile are not launched
inline int first_row(int Y) { return (64 * Y + 1) / TMAX * TMAX; }

// batches block Y is swept in
inline int batches(int K, int Y, int rows) { return (K - first_row(Y) + rows - 1) / rows; }

}  // namespace pairs_plan
