// path_choice.hpp -- which kernel path a demuxlet or freemuxlet job takes.  The source of truth for the routing: each
// launcher gathers the facts a decision reads, calls its chooser here and switches on the result; the path flags
// (MUXGL_FLAG_FORCE_*) and the fit rules are read nowhere else.  Plain C++ (no HIP), so tests/test_path_choice.py
// compiles it on its own and pins the table.
#pragma once
#include <cstddef>
#include <cstdint>

#include "muxgl.h"

namespace path_choice {

// per-chunk partials of the two-per-lane row kernels (17..32 samples / clusters) beyond this many bytes: another path
constexpr double ROW2_PART_LIMIT = 64e9;
// the wave path's pG table, result slabs and (V > 64) call tensor beyond this many bytes: another path
constexpr double WAVE_BYTE_LIMIT = 230e9;

constexpr int32_t FORCE_T = MUXGL_FLAG_FORCE_TILE_SWEEP, FORCE_R = MUXGL_FLAG_FORCE_ROW_KERNEL,
                  FORCE_W = MUXGL_FLAG_FORCE_WAVE_KERNEL, FORCE_X = MUXGL_FLAG_FORCE_STREAMED_CALL,
                  FORCE_XE = MUXGL_FLAG_FORCE_STREAMED_ESTEP;

// what the demuxlet wave path holds on the device, in doubles: the pG table (entry-indexed), the result slabs of the
// cells and their parts (64 x 64 blocks of the pair matrix), and beyond 64 samples the [C][V][V][A] tensor the call reads
struct wave_sizes {
  size_t pg, llw, call;
  double bytes() const { return ((double)pg + (double)llw + (double)call) * 8.0; }
};
inline wave_sizes demux_wave_sizes(int64_t nnz, int64_t C, int64_t n_over, int V, int A) {
  const int nblk = (V + 63) / 64;
  return {(size_t)nnz * A * 9, (size_t)(C + n_over) * nblk * nblk * A * 4096, nblk > 1 ? (size_t)C * V * V * A : 0};
}

// ---- demuxlet (demux_launch; runs only when C > 0)
enum class demux_path { stream, oct8, oct16, row, row2, wave, tile };

struct demux_facts {
  int V, n_alpha;
  const double* alpha;
  int32_t flags;
  int64_t C, S;
  bool row, qrow, d_gpq, d_qent, wave;  // which per-handle states exist
  bool want_full_ll;                    // the caller asked for the [C][V][V][A] tensor
  double row2_part_bytes;               // the row2 kernel's chunk partials (row's chunk tables)
  double wave_bytes;                    // demux_wave_sizes(...).bytes()
  double device_bytes;                  // total device memory; 0 when unknown
};

inline bool default_grid(int A, const double* alpha) { return A == 2 && alpha[0] == 0.0 && alpha[1] == 0.5; }

// the row kernel's instantiations: at most one 0.5 and at most five other values among alpha[1..]
inline bool row_grid(int A, const double* alpha) {
  int nns = 0, nsy = 0;
  for (int n = 1; n < A; ++n) (alpha[n] == 0.5 ? nsy : nns) += 1;
  return nsy <= 1 && nns <= 5;
}

inline demux_path choose_demux_path(const demux_facts& f) {
  const int V = f.V, A = f.n_alpha;
  const bool T = f.flags & FORCE_T, R = f.flags & FORCE_R, W = f.flags & FORCE_W, X = f.flags & FORCE_X;
  // more than 255 samples, the flag, or a job neither the wave path nor the tile sweep's tensor fits
  if (V > 255 || (V > 32 && X)) return demux_path::stream;
  if (V > 32 && A >= 2 && f.wave_bytes > WAVE_BYTE_LIMIT && f.device_bytes > 0 &&
      (double)f.C * V * V * A * 8.0 > 0.9 * f.device_bytes)
    return demux_path::stream;
  // the default grid {0, 0.5}: the oct tiling (row offsets of the linear entries' records are 32-bit byte offsets)
  const unsigned P = V <= 16 ? 8 : 16;
  if (V <= 32 && f.qrow && f.d_gpq && f.d_qent && (uint64_t)(f.S + 1) * (32u * P) < ((uint64_t)1 << 32) && !T && !R &&
      !W && default_grid(A, f.alpha))
    return P == 8 ? demux_path::oct8 : demux_path::oct16;
  if (V <= 16 && f.row && !T && !W && row_grid(A, f.alpha)) return demux_path::row;
  if (V > 16 && V <= 32 && f.row && !T && !W && A == 2 && f.alpha[1] == 0.5 && f.alpha[0] != 0.5 &&
      f.row2_part_bytes <= ROW2_PART_LIMIT)
    return demux_path::row2;
  // one wave per cell and 64 x 64 block.  Not for singlets only; not where a handful of samples beyond a block boundary
  // fill the extra blocks so thinly that the tile sweep is faster (measured: V = 65 tile 195 ms vs 249 ms, V = 96 tile
  // 497 ms vs 253 ms, per 2000 cells); at V <= 16 the row / oct kernels are better
  const bool thin = V > 64 && V % 64 != 0 && V % 64 <= 8 && V < 128;
  if (f.wave && !T && A >= 2 && !thin && (V > 16 || W) && f.wave_bytes <= WAVE_BYTE_LIMIT) return demux_path::wave;
  return demux_path::tile;
}

// whether demux_launch makes the LL tensor ready (demux_ensure_ll) before the sweep of path p; the wave path makes it
// itself when it writes it
inline bool demux_ll_first(const demux_facts& f, demux_path p) {
  if (p == demux_path::stream) return false;
  if (p == demux_path::tile || f.V <= 16) return true;
  return f.V <= 32 && f.want_full_ll && !(f.flags & (FORCE_T | FORCE_W));
}

// ---- freemuxlet E-step (fmx_phase_estep; runs only when the cell shard is not empty)
enum class fmx_estep_path { oct, row2, wave, pair, stream };

struct fmx_estep_facts {
  int K;
  int32_t flags;
  int64_t S;
  bool fqrow, qrow;        // the oct E-step's chunk tables, or the whole pileup's to cut them from
  bool row;                // row chunk tables of the shard (frow) or the pileup (row)
  double row2_part_bytes;  // the row2 kernel's chunk partials (those tables)
  int64_t wave_items;      // work units of the wave plan (0: none)
  double fll_bytes;        // the [C][K(K+1)/2] table the other paths write (fmx_fll_bytes); 0 when unknown
  double device_bytes;     // total device memory; 0 when unknown
};

// what the E-step of every path but the streamed one writes and the call reads: a row of K(K+1)/2 doubles per cell and
// per extra part of a long cell (fmx_wave_fll_rows)
inline double fmx_fll_bytes(int64_t rows, int K) { return (double)rows * ((double)K * (K + 1) / 2) * 8.0; }

inline fmx_estep_path choose_fmx_estep(const fmx_estep_facts& f) {
  const bool T = f.flags & FORCE_T, R = f.flags & FORCE_R, W = f.flags & FORCE_W, XE = f.flags & FORCE_XE;
  // more than 255 clusters, the flag, or a job whose table does not fit the device (fmx_stream.hip)
  if (f.K > 255 || (f.K > 32 && XE)) return fmx_estep_path::stream;
  if (f.fll_bytes > 0 && f.device_bytes > 0 && f.fll_bytes > 0.9 * f.device_bytes) return fmx_estep_path::stream;
  // (row offsets of the posterior rows are 32-bit byte offsets)
  if (f.K <= 16 && (f.fqrow || f.qrow) && !T && !R && f.S + 1 < ((int64_t)1 << 23)) return fmx_estep_path::oct;
  if (f.K > 16 && f.K <= 32 && f.row && !T && !W && f.row2_part_bytes <= ROW2_PART_LIMIT) return fmx_estep_path::row2;
  if (f.K > 32 && !T && f.wave_items > 0) return fmx_estep_path::wave;
  return fmx_estep_path::pair;  // workgroup = (cell, tile of pairs)
}

// ---- freemuxlet call (not consulted on the streamed E-step, which makes its own call): few hypotheses per cell make a wave per cell mostly overhead (0.54 against 0.13 ms at configs[3])
enum class fmx_call_path { lane_per_cell, wave_per_cell };

inline fmx_call_path choose_fmx_call(int K, int32_t flags) {
  return (flags & FORCE_T) || K <= 24 ? fmx_call_path::lane_per_cell : fmx_call_path::wave_per_cell;
}

// ---- freemuxlet M-step (fmx_mstep_launch; runs only when the SNP shard and K are not empty)
enum class fmx_mstep_path { stream, chain };

struct fmx_mstep_facts {
  int K;
  int32_t flags;
  int64_t ns, nnz, C;  // SNPs of the shard, entries, cells d_clust spans
};

// stream: lane = chain, the SNP's list as a stream; chain: lane = (SNP, cluster), every chain walks its list
inline fmx_mstep_path choose_fmx_mstep(const fmx_mstep_facts& f) {
  return !(f.flags & FORCE_T) && f.K <= 64 && f.ns > 0 && f.nnz > 0 && f.C > 0 ? fmx_mstep_path::stream
                                                                                  : fmx_mstep_path::chain;
}

// ---- freemuxlet greedy start (muxgl_fmx_greedy_init): the up-front choice; residency and launch failures of the
// batched kernel still fall back to the serial one at run time
enum class greedy_path { batched, serial };

struct greedy_facts {
  int K;
  int32_t flags;
  int64_t P;  // entries to cluster
  int cus;    // compute units of the device (the batched kernel keeps 2 gb workgroups resident, one per unit)
  int gb;     // cells per batch
};

inline greedy_path choose_greedy(const greedy_facts& f) {
  return f.K <= 64 && f.P > 0 && f.P < ((int64_t)1 << 31) && !(f.flags & FORCE_T) && f.cus >= 2 * f.gb
             ? greedy_path::batched
             : greedy_path::serial;
}

}  // namespace path_choice
