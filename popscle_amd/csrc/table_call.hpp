// table_call.hpp -- the device side of table_plan.hpp: the host body (table_batches) that drives a plan for the five
// per-droplet table calls (demux_singlets.hip, fmx_singlets.hip, demux_unknown.hip, fmx_unknown.hip and, through
// ambient_table.hpp, the two ambient tables), and the join of the parts of a long cell.  The other kernels are the units'.
//
// The protocol of a call, stated here once:
//   1. plan(): cell_ptr comes to the host; the cells are cut into batches of whole cells whose cost (the unit's, in
//      bytes) fits the budget of the unit's variable.  A droplet that exceeds the budget alone is refused where the unit
//      has words for it (the singlet tables take it as a batch of its own), a largest batch that one launch cannot hold
//      for all.  The device lists of items and records are made for the largest batch.
//   2. The unit makes its buffers from the plan's maxima (bt), opens its timer and does the once-per-call work that
//      precedes the first upload (a prior or profile to the device, demuxlet's whole-pileup weights).
//   3. run(), per batch in cell order: fill the host lists; upload them and DRAIN THE STREAM, so that the next batch may
//      refill the host vectors; timer start; the unit's launches (a once-per-call kernel inside the first bracket tests
//      b.c0 == 0); timer stop: the kernel bracket CLOSES BEFORE THE COPY-OUT; the unit's copy-out; stream synchronise: a
//      batch HAS LEFT THE DEVICE BEFORE THE NEXT OVERWRITES the slab and the lists; timer add.
#pragma once
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "table_plan.hpp"

// slab[row][j] += slab[first][j] + ... + slab[first + count - 1][j] for the cells of several parts: the logs of the parts
// of a cell, added in entry order (lane = (cut, column)); slab is [rows][V].  A template so that only the units that
// launch it (the two singlet tables and freemuxlet's unknown-donor call, T = double) hold a copy.
template <typename T>
__global__ void __launch_bounds__(256)
    table_join_kernel(int64_t n_cuts, const table_plan::cut* __restrict__ cuts, int V, T* __restrict__ slab) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cuts * V) return;
  const int64_t c = i / V;
  const int j = (int)(i - c * V);
  const table_plan::cut ct = cuts[c];
  T s = slab[(size_t)ct.row * V + j];
  for (int64_t k = 0; k < ct.count; ++k) s += slab[(size_t)(ct.first + k) * V + j];
  slab[(size_t)ct.row * V + j] = s;
}

// what a unit says about its call
struct table_call {
  const char* who;             // the call's name, for the messages and the event pair
  const char* budget_env;      // the variable that sets the budget, named in the messages
  table_plan::begin_fn begin;  // the cut policy of a long cell
  // the launch-size checks over the largest batch: wave units of the sweep per slab row (four to a workgroup), lanes of
  // the widest lane-per-element kernel per slab row and per cell (256 to a workgroup; 0: none)
  double waves_per_row, lanes_per_row, lanes_per_cell;
  // the size of a row in words, in the launch refusal and in that of a droplet over the budget alone (empty: none)
  std::string launch_shape, alone_shape;
};

// one batch, as the unit's launch and copy-out callables see it
template <class Rec>
struct table_batch {
  int64_t c0, c1, eb0, eb1;         // the cells [c0, c1) of the handle and their entries [eb0, eb1)
  int64_t n_items;                  // work items = slab rows of the batch
  const table_plan::item* d_items;  // [n_items]
  const Rec* d_recs;                // the cuts of the cells of several parts, or a record per cell
  const std::vector<Rec>& recs;     // their host copy
  int64_t nc() const { return c1 - c0; }
};

// the join of the long cells of a batch over the W columns of a slab row; a batch without one launches nothing
template <typename T>
int table_join(muxgl_handle* h, const table_batch<table_plan::cut>& b, int W, T* d_slab) {
  if (b.recs.empty()) return 0;
  const int64_t n = (int64_t)b.recs.size() * W;
  hipLaunchKernelGGL(table_join_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (int64_t)b.recs.size(),
                     b.d_recs, W, d_slab);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// How a call is timed: start(h) / stop(h, last batch?) around every batch's launches, add() behind its synchronise.  Two
// policies: call_events (common.hpp), a bracket per batch added to the caller's *kernel_ms, and this one, one bracket
// over the call in a timing slot of the handle (the singlet tables): the unit's tic opens it, the last stop closes it.
struct table_slot_timer {
  int slot;
  int start(muxgl_handle*) { return 0; }
  int stop(muxgl_handle* h, bool last) { return last ? (toc(h, slot), 0) : 0; }
  void add() {}
};

// The host body of a table call (the protocol above).  Rec: table_plan::cut for a unit that joins long cells in the slab,
// table_plan::cell for one whose emit kernel walks every cell.
template <class Rec>
struct table_batches {
  std::vector<int64_t> cell_ptr;  // the handle's, on the host
  table_plan::batches bt;         // the plan: the unit sizes its buffers from its maxima

  // cost(len, parts): device bytes of a cell.  0, or 1 with the handle's message set.
  template <class Cost>
  int plan(muxgl_handle* h, const table_call& call, Cost cost) {
    const int64_t C = h->C;
    cell_ptr.resize((size_t)C + 1);
    HIPCHK(h, hipMemcpyAsync(cell_ptr.data(), h->d_cell_ptr, sizeof(int64_t) * (size_t)(C + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t budget = dev_slab_budget(call.budget_env);
    bt = table_plan::plan(cell_ptr.data(), C, budget, cost);
    if (bt.over >= 0 && !call.alone_shape.empty()) {
      const int64_t len = cell_ptr[(size_t)bt.over + 1] - cell_ptr[(size_t)bt.over];
      MUXGL_FAIL(h, "%s", table_plan::alone_message(call.who, h->cell_base + bt.over, len, call.alone_shape,
                                                    cost(len, table_plan::parts(len)), budget, call.budget_env).c_str());
    }
    if (table_plan::exceeds_one_launch((double)bt.max_rows * call.waves_per_row, 4.0) ||
        table_plan::exceeds_one_launch(std::max(bt.max_rows * call.lanes_per_row, bt.max_cells * call.lanes_per_cell), 256.0))
      MUXGL_FAIL(h, "%s", table_plan::launch_message(call.who, bt.max_rows, call.launch_shape, call.budget_env).c_str());
    begin = call.begin;
    if (dev_alloc(h, &d_items.p, (size_t)bt.max_rows)) return 1;
    return dev_alloc(h, &d_recs.p, (size_t)(wants_cuts ? bt.max_cuts : bt.max_cells));
  }

  // launch(b) and copy_out(b) for every batch b, in cell order; each returns 0, or 1 with the handle's message set
  template <class Timer, class Launch, class CopyOut>
  int run(muxgl_handle* h, Timer&& timer, Launch&& launch, CopyOut&& copy_out) {
    const int64_t C = (int64_t)cell_ptr.size() - 1;
    int64_t c0 = 0;
    for (const int64_t c1 : bt.end) {
      if constexpr (wants_cuts)
        table_plan::fill(cell_ptr.data(), c0, c1, begin, items, &recs, nullptr);
      else
        table_plan::fill(cell_ptr.data(), c0, c1, begin, items, nullptr, &recs);
      const table_batch<Rec> b = {c0, c1, cell_ptr[(size_t)c0], cell_ptr[(size_t)c1], (int64_t)items.size(), d_items.p, d_recs.p, recs};
      // (the copies come from pageable memory: they have left the vectors when they return)
      HIPCHK(h, hipMemcpyAsync(d_items.p, items.data(), sizeof(table_plan::item) * items.size(), hipMemcpyHostToDevice, h->stream));
      if (!recs.empty()) HIPCHK(h, hipMemcpyAsync(d_recs.p, recs.data(), sizeof(Rec) * recs.size(), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (timer.start(h)) return 1;
      if (launch(b)) return 1;
      if (timer.stop(h, c1 == C)) return 1;
      if (copy_out(b)) return 1;
      HIPCHK(h, hipStreamSynchronize(h->stream));
      timer.add();
      c0 = c1;
    }
    return 0;
  }

 private:
  static constexpr bool wants_cuts = std::is_same<Rec, table_plan::cut>::value;
  table_plan::begin_fn begin = nullptr;
  dev_tmp<table_plan::item> d_items;
  dev_tmp<Rec> d_recs;
  std::vector<table_plan::item> items;
  std::vector<Rec> recs;
};
