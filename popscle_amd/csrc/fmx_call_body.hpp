// fmx_call_body.hpp -- what both freemuxlet call kernels share besides their common tail (fmx_call_finish.inc): the
// top two of a scan (fmx_top2, fmx_better, fmx_top2_push) and the packing of the previous state for the exact path.
// Users: fmx_call_kernel (fmx_kernels.hip), which scans the [C][K(K+1)/2] table, and the streamed E-step (fmx_stream.hip),
// which keeps only the scan results per cell.
#pragma once
#include "common.hpp"
#include "demux_call_body.hpp"

// top two of a scan under the reference's update rule (strict >, first come first kept): the two largest under the
// total order (value descending, scan position ascending), which is associative -- lanes scan strided positions and
// merge their lists
struct fmx_top2 {
  double v1, v2;
  int32_t p1, p2;
  double v3;  // third-largest value (no position), for the exact-call pass: see muxgl_fmx_cell
};
__device__ __forceinline__ bool fmx_better(double va, int32_t pa, double vb, int32_t pb) {
  return va > vb || (va == vb && pa < pb);
}
__device__ __forceinline__ void fmx_top2_push(fmx_top2& t, double v, int32_t p) {
  if (fmx_better(v, p, t.v1, t.p1)) {
    t.v3 = t.v2;
    t.v2 = t.v1, t.p2 = t.p1;
    t.v1 = v, t.p1 = p;
  } else if (fmx_better(v, p, t.v2, t.p2)) {
    t.v3 = t.v2;
    t.v2 = v, t.p2 = p;
  } else {
    t.v3 = fmax(t.v3, v);
  }
}

// (type, jBest, kBest) before the running iteration, for the exact path's nchanged rules (fmx_exact.hip: fmx_unpack_prev).
// A byte each up to 255 clusters; beyond that (WIDE) the type in a byte and the cluster indices in 12 bits each, 0xfff
// meaning none (MUXGL_MAX_CLUSTERS = 1024 < 0xfff)
template <bool WIDE>
__host__ __device__ __forceinline__ int32_t fmx_pack_prev(int32_t type, int32_t j, int32_t k) {
  if (WIDE) return (int32_t)((uint32_t)(type & 0xff) | ((uint32_t)(j & 0xfff) << 8) | ((uint32_t)(k & 0xfff) << 20));
  return (type & 0xff) | ((j & 0xff) << 8) | ((k & 0xff) << 16);
}
inline void fmx_unpack_prev(int32_t ps, bool wide, int32_t* type, int32_t* j, int32_t* k) {
  *type = (int8_t)(ps & 0xff);
  if (wide) {
    const uint32_t u = (uint32_t)ps, pj = (u >> 8) & 0xfff, pk = (u >> 20) & 0xfff;
    *j = pj == 0xfff ? -1 : (int32_t)pj;
    *k = pk == 0xfff ? -1 : (int32_t)pk;
  } else {
    const int32_t pj = (ps >> 8) & 0xff, pk = (ps >> 16) & 0xff;
    *j = pj == 0xff ? -1 : pj;
    *k = pk == 0xff ? -1 : pk;
  }
}
