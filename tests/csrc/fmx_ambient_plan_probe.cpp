// Test shim around popscle_amd/csrc/table_plan.hpp as muxgl_fmx_ambient (fmx_ambient.hip) uses it: the cost of a cell in
// device bytes at NR rhos and K clusters, the batches of whole cells that cost yields for a budget, and the work items and
// cell records of a batch under the equal cut.  Plain C++; nothing here touches a device (see tests/test_fmx_ambient.py).
#include "table_plan.hpp"

extern "C" {

int64_t probe_fam_part() { return table_plan::PART; }
uint64_t probe_fam_bytes(int64_t len, int NR, int K) { return table_plan::fmx_ambient_bytes(len, table_plan::parts(len), NR, K); }

// ends[i]: one past the last cell of batch i (at most C are written); maxima: rows, cells, cuts, entries; *over: the first
// cell that exceeds the budget alone, or -1.  Returns the batches.
int64_t probe_fam_plan(const int64_t* cell_ptr, int64_t C, uint64_t budget, int NR, int K, int64_t* ends, int64_t* maxima,
                       int64_t* over) {
  const table_plan::batches b = table_plan::plan(
      cell_ptr, C, (size_t)budget, [=](int64_t len, int64_t np) { return table_plan::fmx_ambient_bytes(len, np, NR, K); });
  for (size_t i = 0; i < b.end.size(); ++i) ends[i] = b.end[i];
  maxima[0] = b.max_rows, maxima[1] = b.max_cells, maxima[2] = b.max_cuts, maxima[3] = b.max_entries;
  *over = b.over;
  return (int64_t)b.end.size();
}

// the batch [c0, c1) as the call fills it: items[i] = (e0, e1, row), recs[c] = (first, count).  Returns the items.
int64_t probe_fam_fill(const int64_t* cell_ptr, int64_t c0, int64_t c1, int64_t* items, int64_t* recs) {
  std::vector<table_plan::item> it;
  std::vector<table_plan::cell> cells;
  table_plan::fill(cell_ptr, c0, c1, table_plan::equal_begin, it, nullptr, &cells);
  for (size_t i = 0; i < it.size(); ++i) items[3 * i] = it[i].e0, items[3 * i + 1] = it[i].e1, items[3 * i + 2] = it[i].row;
  for (size_t i = 0; i < cells.size(); ++i) recs[2 * i] = cells[i].first, recs[2 * i + 1] = cells[i].count;
  return (int64_t)it.size();
}
}
