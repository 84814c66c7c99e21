// table_call.hpp -- what the per-droplet table calls share on the device side of table_plan.hpp: the upload of a batch's
// work lists and the join of the parts of a long cell.  The sweep and weight kernels stay in their units.
#pragma once
#include <vector>

#include "common.hpp"
#include "table_plan.hpp"

// slab[row][j] += slab[first][j] + ... + slab[first + count - 1][j] for the cells of several parts: the logs of the parts
// of a cell, added in entry order (lane = (cut, column)); slab is [rows][V].  A template so that only the units that
// launch it (the two singlet tables, T = double) hold a copy.
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

// the items of a batch and its cuts or cell records to the device; the stream is drained, so the vectors may be refilled
// (the copies come from pageable memory: they have left the vectors when they return)
template <typename R>
int table_upload(muxgl_handle* h, const std::vector<table_plan::item>& items, table_plan::item* d_items,
                 const std::vector<R>& recs, R* d_recs) {
  HIPCHK(h, hipMemcpyAsync(d_items, items.data(), sizeof(table_plan::item) * items.size(), hipMemcpyHostToDevice, h->stream));
  if (!recs.empty()) HIPCHK(h, hipMemcpyAsync(d_recs, recs.data(), sizeof(R) * recs.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
