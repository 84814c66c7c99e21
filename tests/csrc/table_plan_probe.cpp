// Test shim around popscle_amd/csrc/table_plan.hpp, the host side of the per-droplet tables: the batches of cells
// for a budget, and per batch the work items with the cuts (singlet tables) or the cell records (unknown-donor call), as
// each of the three callers asks for them; the words of the two refusals of all five calls; the lane width
// (lane_width.hpp).
// Plain C++; nothing here touches a device (see tests/test_table_plan.py).
#include <cstring>

#include "lane_width.hpp"
#include "table_plan.hpp"

namespace {

// the callers: 0 muxgl_demux_singlets (cost = rows, fixed parts, cuts), 1 muxgl_fmx_singlets (rows, equal parts, cuts),
// 2 muxgl_demux_unknown (cost = bytes at A alphas and V samples, fixed parts, cell records)
table_plan::batches plan_of(int caller, const int64_t* cell_ptr, int64_t C, uint64_t budget, int A, int V) {
  if (caller == 2)
    return table_plan::plan(cell_ptr, C, (size_t)budget,
                            [=](int64_t len, int64_t np) { return table_plan::unknown_bytes(len, np, A, V + 1); });
  return table_plan::plan(cell_ptr, C, (size_t)budget, [](int64_t, int64_t np) { return (size_t)np; });
}

// the words of the five calls for the size of a row, as each hands them to table_call (tests/test_table_plan.py finds
// these expressions in the units): 0 muxgl_demux_singlets, 1 muxgl_fmx_singlets, 2 muxgl_demux_unknown, 3
// muxgl_fmx_unknown, 4 an ambient table (NR rhos, W of call.noun)
struct shapes {
  std::string launch, alone;
};
struct ambient_call {
  const char* noun;
};
shapes shapes_of(int which, int A, int W, const char* noun) {
  const int V = W, K = W, NR = A;
  const ambient_call call = {noun};
  switch (which) {
    case 0: return {table_plan::shape(V, "samples"), ""};
    case 1: return {table_plan::shape(K, "clusters"), ""};
    case 2: return {table_plan::shape(V, "samples", A, "alphas"), table_plan::shape(A, "alphas", V, "samples")};
    case 3: return {table_plan::shape(K, "clusters"), table_plan::shape(K, "clusters")};
    default: return {table_plan::shape(W, call.noun, NR, "rhos"), table_plan::shape(NR, "rhos", W, call.noun)};
  }
}

}  // namespace

extern "C" {

int probe_lane_width(int n) { return lane_width(n); }

// the two refusals as call `call` (shapes_of) words them; an empty string where the call has no such refusal
void probe_table_alone_message(int call, const char* who, int64_t droplet, int64_t entries, int A, int W, const char* noun,
                               uint64_t bytes, uint64_t budget, const char* env, char* out, size_t out_len) {
  const shapes sh = shapes_of(call, A, W, noun);
  const std::string m = sh.alone.empty() ? "" : table_plan::alone_message(who, droplet, entries, sh.alone, bytes, budget, env);
  snprintf(out, out_len, "%s", m.c_str());
}
void probe_table_launch_message(int call, const char* who, int64_t rows, int A, int W, const char* noun, const char* env,
                                char* out, size_t out_len) {
  snprintf(out, out_len, "%s", table_plan::launch_message(who, rows, shapes_of(call, A, W, noun).launch, env).c_str());
}

int64_t probe_table_part() { return table_plan::PART; }
int probe_table_sizes(int which) {
  return which == 0 ? (int)sizeof(table_plan::item) : which == 1 ? (int)sizeof(table_plan::cut) : (int)sizeof(table_plan::cell);
}
uint64_t probe_table_unknown_bytes(int64_t len, int A, int V) {
  return table_plan::unknown_bytes(len, table_plan::parts(len), A, V + 1);
}
int probe_table_exceeds(double units, double per_block) { return table_plan::exceeds_one_launch(units, per_block) ? 1 : 0; }

// budget in the caller's unit (rows or bytes).  ends[i]: one past the last cell of batch i (at most C are written);
// maxima: rows, cells, cuts, entries; *over: the first cell that exceeds the budget alone, or -1.  Returns the batches.
int64_t probe_table_plan(int caller, const int64_t* cell_ptr, int64_t C, uint64_t budget, int A, int V, int64_t* ends,
                         int64_t* maxima, int64_t* over) {
  const table_plan::batches b = plan_of(caller, cell_ptr, C, budget, A, V);
  for (size_t i = 0; i < b.end.size(); ++i) ends[i] = b.end[i];
  maxima[0] = b.max_rows, maxima[1] = b.max_cells, maxima[2] = b.max_cuts, maxima[3] = b.max_entries;
  *over = b.over;
  return (int64_t)b.end.size();
}

// the batch [c0, c1) as the caller fills it: items[i] = (e0, e1, row); recs = the cuts (row, first, count) of callers 0
// and 1, the cell records (first, count) of caller 2.  Returns the items; *n_recs the records.  The arrays hold at least
// rows-of-the-batch items and c1 - c0 records.
int64_t probe_table_fill(int caller, const int64_t* cell_ptr, int64_t c0, int64_t c1, int64_t* items, int64_t* recs,
                         int64_t* n_recs) {
  std::vector<table_plan::item> it;
  std::vector<table_plan::cut> cuts;
  std::vector<table_plan::cell> cells;
  table_plan::fill(cell_ptr, c0, c1, caller == 1 ? table_plan::equal_begin : table_plan::fixed_begin, it,
                   caller == 2 ? nullptr : &cuts, caller == 2 ? &cells : nullptr);
  for (size_t i = 0; i < it.size(); ++i) items[3 * i] = it[i].e0, items[3 * i + 1] = it[i].e1, items[3 * i + 2] = it[i].row;
  for (size_t i = 0; i < cuts.size(); ++i) recs[3 * i] = cuts[i].row, recs[3 * i + 1] = cuts[i].first, recs[3 * i + 2] = cuts[i].count;
  for (size_t i = 0; i < cells.size(); ++i) recs[2 * i] = cells[i].first, recs[2 * i + 1] = cells[i].count;
  *n_recs = (int64_t)(caller == 2 ? cells.size() : cuts.size());
  return (int64_t)it.size();
}
}
