// table_plan.hpp -- the host side of the five per-droplet table calls (demux_singlets.hip, fmx_singlets.hip,
// demux_unknown.hip, fmx_unknown.hip and, through ambient_table.hpp, the two ambient tables): how the cells of a call are
// cut into work items and swept in batches, what a cell costs, and the words of the two refusals.  Plain C++ (no HIP), in
// the manner of pairs_plan.hpp, so tests/test_table_plan.py compiles it on its own (tests/csrc/table_plan_probe.cpp) and
// holds it to the loops it replaced.  The host body that drives a plan on a device is table_call.hpp's.
//
// A cell of more than PART entries is cut into ceil(len / PART) parts, every other cell (an empty one too) is one part.
// A part is one work item with a slab row of its own: the first part of a cell writes the cell's row (rows [0, cells of
// the batch)), the further parts the rows behind those, in cell order; their logs are added to the cell's in part order.
// The cut of a cell depends on the cell alone -- not on the budget, the batch or the other cells of the handle -- which
// is what makes a table bit-identical for any budget, on one device, on a group and through the sharded driver.
// Cells are swept in batches of whole cells, in order: a batch takes cells while their summed cost fits the budget, and
// always at least one.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace table_plan {

constexpr int64_t PART = 2048;  // entries per part of a long cell (the wave kernels' cut, common.hpp wave_item)

// one work item: the entries [e0, e1) of one cell, result row `row` of the slab
struct item {
  int64_t e0, e1, row;
};
// a cell of several parts: slab[row] += slab[first] + ... + slab[first + count - 1], in this order
struct cut {
  int64_t row, first, count;
};
// the further parts of every cell of a batch (count = 0: none), for a kernel that walks all cells
struct cell {
  int64_t first, count;
};

inline int64_t parts(int64_t len) { return len > PART ? (len + PART - 1) / PART : 1; }

// The two cut policies: where part k of a cell of n entries in np parts begins (part k = [begin(k), begin(k + 1))).
// fixed: parts of PART entries, the last one shorter (demuxlet's two tables)
inline int64_t fixed_begin(int64_t n, int64_t /*np*/, int64_t k) { return std::min(n, k * PART); }
// equal: the wave plan's equal parts, as fmx_stream.hip's sweep_block cuts a cell (freemuxlet)
inline int64_t equal_begin(int64_t n, int64_t np, int64_t k) { return n * k / np; }
using begin_fn = int64_t (*)(int64_t n, int64_t np, int64_t k);

struct batches {
  std::vector<int64_t> end;  // one past the last cell of each batch
  int64_t max_rows = 0, max_cells = 0, max_cuts = 0, max_entries = 0;  // the largest batch in each measure
  int64_t over = -1;         // the first cell whose cost alone exceeds the budget (it is a batch of its own), or none
};

// cost(len, parts) of a cell, in the unit of the budget
template <class Cost>
batches plan(const int64_t* cell_ptr, int64_t C, size_t budget, Cost cost) {
  batches b;
  for (int64_t c0 = 0; c0 < C;) {
    size_t used = 0;
    int64_t rows = 0, cuts = 0, c1 = c0;
    for (; c1 < C; ++c1) {
      const int64_t len = cell_ptr[c1 + 1] - cell_ptr[c1], np = parts(len);
      const size_t w = cost(len, np);
      if (w > budget && b.over < 0) b.over = c1;
      if (c1 > c0 && used + w > budget) break;
      used += w;
      rows += np;
      cuts += np > 1;
    }
    b.end.push_back(c1);
    b.max_rows = std::max(b.max_rows, rows);
    b.max_cells = std::max(b.max_cells, c1 - c0);
    b.max_cuts = std::max(b.max_cuts, cuts);
    b.max_entries = std::max(b.max_entries, cell_ptr[c1] - cell_ptr[c0]);
    c0 = c1;
  }
  return b;
}

// device bytes of a cell in a batch of a singlet table of W columns: its slab rows, one per part (the slab alone counts,
// as ever: parts x 8 W <= budget is parts <= budget / (8 W), the row count the two calls once divided out themselves)
inline size_t singlet_bytes(int64_t np, int W) { return (size_t)np * sizeof(double) * (size_t)W; }

// device bytes of a cell in a batch of the unknown-donor call at A alphas and VC = V + 1 columns: its entries' weights,
// its slab rows (one per part) with their items, and its rows of the three tables with its record
inline size_t unknown_bytes(int64_t len, int64_t np, int A, int VC) {
  const size_t row_bytes = sizeof(double) * (size_t)A * 2 * VC;
  return (size_t)len * A * 6 * sizeof(double) + (size_t)np * (row_bytes + sizeof(item)) + row_bytes + sizeof(cell);
}

// device bytes of a cell in a batch of an ambient call (ambient_table.hpp) at NR rhos and V columns: its entries' weights
// (three per rho, 24 bytes per entry and rho), its slab rows (one per part) with their items, and its row of the table with
// its record
inline size_t ambient_bytes(int64_t len, int64_t np, int NR, int V) {
  const size_t row_bytes = sizeof(double) * (size_t)NR * V;
  return (size_t)len * NR * 3 * sizeof(double) + (size_t)np * (row_bytes + sizeof(item)) + row_bytes + sizeof(cell);
}

// device bytes of a cell in a batch of freemuxlet's unknown-donor call at K clusters: its entries' weights (three and two
// scalars, 40 bytes an entry), its slab rows of K + 2 doubles (one per part) with their items, and its rows of the three
// tables (K + 2 doubles)
inline size_t fmx_unknown_bytes(int64_t len, int64_t np, int K) {
  const size_t row_bytes = sizeof(double) * ((size_t)K + 2);
  return (size_t)len * 5 * sizeof(double) + (size_t)np * (row_bytes + sizeof(item)) + row_bytes;
}

// freemuxlet's ambient call at NR rhos and K clusters: the same table (ambient_table.hpp), the same bytes
inline size_t fmx_ambient_bytes(int64_t len, int64_t np, int NR, int K) { return ambient_bytes(len, np, NR, K); }

// the items of the batch [c0, c1), and per cell of several parts its cut and/or per cell its record (NULL: not wanted)
inline void fill(const int64_t* cell_ptr, int64_t c0, int64_t c1, begin_fn begin, std::vector<item>& items,
                 std::vector<cut>* cuts, std::vector<cell>* cells) {
  items.clear();
  if (cuts) cuts->clear();
  if (cells) cells->clear();
  int64_t over = c1 - c0;  // first free row behind the cells' own
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t b = cell_ptr[c], n = cell_ptr[c + 1] - b, np = parts(n);
    items.push_back(item{b, b + begin(n, np, 1), c - c0});
    if (cuts && np > 1) cuts->push_back(cut{c - c0, over, np - 1});
    if (cells) cells->push_back(cell{over, np - 1});
    for (int64_t k = 1; k < np; ++k) items.push_back(item{b + begin(n, np, k), b + begin(n, np, k + 1), over++});
  }
}

// whether `units` work units at `per_block` a workgroup need more workgroups than one launch takes
inline bool exceeds_one_launch(double units, double per_block) { return units / per_block >= 2147483647.0; }

// ---- the two refusals of a table call, in one wording.  who: the call's name; env: the variable that sets the budget;
// shape: the call's words for the size of a row, "65 samples" or "4 alphas x 65 samples":
inline std::string shape(int n, const char* noun) { return std::to_string(n) + " " + noun; }
inline std::string shape(int n, const char* noun, int m, const char* of) { return shape(n, noun) + " x " + shape(m, of); }

// droplet `droplet` (an index of the whole pileup) of `entries` entries costs `bytes` alone, more than the budget
inline std::string alone_message(const char* who, int64_t droplet, int64_t entries, const std::string& shape, size_t bytes,
                                 size_t budget, const char* env) {
  char buf[512];
  snprintf(buf, sizeof(buf), "%s: droplet %lld alone (%lld entries x %s: %.1f MB) exceeds the budget of %.1f MB (raise %s)", who,
           (long long)droplet, (long long)entries, shape.c_str(), (double)bytes / 1048576.0, (double)budget / 1048576.0, env);
  return buf;
}

// the largest batch, of `rows` slab rows, needs more workgroups than one launch takes
inline std::string launch_message(const char* who, int64_t rows, const std::string& shape, const char* env) {
  char buf[512];
  snprintf(buf, sizeof(buf), "%s: a batch of %lld rows x %s exceeds one launch (lower %s)", who, (long long)rows, shape.c_str(),
           env);
  return buf;
}

}  // namespace table_plan
