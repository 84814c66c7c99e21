// common.hpp -- handle layout, error plumbing and small device helpers shared by the libmuxgl translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <unordered_map>
#include <unordered_set>

#include "../../include/muxgl.h"
#include "fit_args.hpp"
#include "fmx_refusal.hpp"
#include "lane_width.hpp"
#include "path_choice.hpp"
#include "stream_plan.hpp"

constexpr int MUXGL_ROW_CH = 128;   // entries per chunk of the row kernels (16-lane slots)
constexpr int MUXGL_QUAD_CH = 192;  // entries per chunk of the freemuxlet oct E-step (configs[3], E-step in ms: 128: 1.63,
                                    // 160: 1.58, 192: 1.50, 256: 1.49)
constexpr int MUXGL_OCT_CH = 192;   // entries per chunk of the demuxlet oct kernel (8-lane slots).  Measured at configs[1]
                                    // (sweep + finish, ms): 96: 0.270 + 0.107, 128: 0.258 + 0.083, 160: 0.243 + 0.074,
                                    // 192: 0.252 + 0.068, 224: 0.250 + 0.066, 256: 0.253 + 0.067, 320: 0.281 + 0.066 --
                                    // longer chunks are fewer partial products for the finish kernel, shorter ones more
                                    // work units to balance.  A constant: a cell's cut must not depend on its neighbours.

// per-entry record of the quad kernel: everything phase 1 needs for an entry with <= 4 reads in ONE 16-byte load
struct quad_entry {
  int32_t snp;      // SNP id
  uint32_t nreads;  // reads of the entry
  uint32_t first4;  // its first four packed read bytes (byte k = read k)
  uint32_t r0;      // offset of read 0 in the reads array (used only beyond four reads)
};

// Record of a linear entry (at most one usable read) of the quad kernel's sweep: its marker and the read byte that
// counts.  code 0xFF (MUXGL_READ_OTHER never counts) = no usable read, or a marker without genotypes.
struct quad_lrec {
  int32_t snp;
  uint32_t code;
};

// one work unit of the row kernels (demux_row.hip, fmx_kernels.hip): <= 128 consecutive entries of one cell
struct row_chunk {
  int64_t e0;
  int32_t len;
  int32_t cell;
};

// chunk tables of the row kernels, built by demux_row_plan() at muxgl_set_pileup time
struct muxgl_row_state {
  row_chunk* d_chunks = nullptr;        // launch order: non-increasing length, then ascending first SNP
  int64_t* d_cell_chunk_ptr = nullptr;  // [C+1]
  int32_t* d_cell_chunks = nullptr;     // chunk positions of each cell in entry order
  int32_t* d_kmap = nullptr;            // [16][16]: sample held by lane j after t DPP row rotations
  int32_t* d_tmap = nullptr;            // [P/2][P]: position seen by a lane of the oct tiling after each rotation (P = tmap_p)
  int tmap_p = 0;
  double* d_part = nullptr;             // per-chunk partial log-likelihoods (row kernels) / mantissas (quad kernel)
  quad_entry* d_qent_lin = nullptr;     // quad kernel: the entry records with every chunk's linear entries first ...
  int32_t* d_chunk_nlin = nullptr;      // ... and how many they are, per chunk (demux_oct.hip, built on first use)
  uint2* d_orec = nullptr;              // ... and the linear ones as {row offset, table offset} records, step-major per
  int64_t* d_unit_ptr = nullptr;        //     unit of eight chunks: unit u starts at d_orec[d_unit_ptr[u]] (demux_oct.hip)
  int32_t* d_quad_order = nullptr;      // ... and the launch order of the chunks (sorted by trip count within buckets)
  // freemuxlet oct E-step (fmx_oct.hip, built on first use after muxgl_fmx_prepare): per chunk, its linear entries
  // as {c0, c1, snp} records in front, then the SNP ids and six likelihoods of the others
  int32_t* d_fq_nlin = nullptr;
  int32_t *d_fo_lsteps = nullptr, *d_fo_gsteps = nullptr;  // steps of every unit's two loops (fmx_oct.hip)
  int64_t *d_fo_lptr = nullptr, *d_fo_gptr = nullptr;      // first record of every unit in the step-major tables below
  uint32_t *d_fo_loff = nullptr, *d_fo_goff = nullptr;     // row offsets of the linear / other entries
  double2* d_fo_lc = nullptr;                              // (c0, c1) of the linear entries
  double* d_fo_ggl = nullptr;                              // six likelihoods of the other entries
  int32_t* d_fq_order = nullptr;        // launch order of the chunks, as d_quad_order
  int32_t* d_part_e = nullptr;          // per-chunk partial exponents (quad kernel)
  int32_t* d_chunk_pos = nullptr;       // position of every chunk in its cell's list: where the oct kernel leaves its partials
  size_t part_cap = 0, part_e_cap = 0;
  int64_t n_chunks = 0;
  // oct sweep as a pipeline of two cell groups (demux_oct.hip, built with d_quad_order): cells [0, oct_cut) and the rest;
  // 0: one group.  Group g's units are [oct_unit0[g], oct_unit0[g + 1]), each range a multiple of eight.
  int64_t oct_cut = 0;
  int64_t oct_unit0[3] = {0, 0, 0};
  int64_t oct_round = 0;                // units of one residency round of the sweep kernel on this device
  int oct_groups_run = 0;               // cell groups of the last run (1 or 2)
};

// what a handle's pileup is (muxgl_fmx_set_column_slab / device groups): the whole pileup, the cell-major row slab of a
// rank (its cells, every SNP: E-step, scans, re-assignment), or the column slab (every cell, its SNPs: ordered M-step)
enum { MUXGL_ROLE_FULL = 0, MUXGL_ROLE_ROWS = 1, MUXGL_ROLE_COLS = 2 };

struct muxgl_group;

constexpr double kMinNormGL = 1e-6;  // freemuxlet's floor of a normalised likelihood, MIN_NORM_GL (sc_drop_seq.h:14)

// records of the wave E-step's entry streams (fmx_wave.hip)
struct fmx_lrec {  // a linear entry: glis[g1][g2] = c0 + c1 (g1 + g2)
  double c0, c1;
  int32_t snp, pad;
};
struct fmx_grec {  // any other entry: its index and SNP
  int64_t e;
  int32_t snp, pad;
};
// exact scan results of a settled near-tie cell (fmx_exact.hip), read back by fmx_call_kernel while the cell's inputs last
struct fmx_xc {
  int32_t sBest, sNext, dBest1, dBest2, dNext1, dNext2;
  double sngBestLLK, sngNextLLK, dblBestLLK, dblNextLLK;
};

struct muxgl_handle {
  std::multimap<size_t, void*> pool;   // cached device blocks by size (dev_alloc / dev_free below)
  size_t pool_bytes = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = true;
  // the oct path's second cell group (demux_oct.hip) runs on a stream of the handle's own, forked from `stream` and
  // joined by the HOST: muxgl_demux_run waits for both streams before it returns (join_stream2 below), so every other
  // call sees one stream.  Stream and events are made by the first two-group run (a handle that never takes that path
  // has none) and go with the handle
  hipStream_t stream2 = nullptr;
  bool stream2_busy = false;        // work of the current run is outstanding on stream2
  hipEvent_t ev_fork = nullptr;     // the fork where no timing event is recorded (MUXGL_NO_EVENTS)
  hipEvent_t ev_sweep2 = nullptr;   // end of the second group's sweep: a time stamp
  hipEvent_t ev_finish2 = nullptr;  // end of the second group's finish: a time stamp
  bool split_timed = false;  // the brackets SWEEP / REDUCE of this run are those of a two-group run (collect_timing)
  std::string err;
  int role = MUXGL_ROLE_FULL;
  muxgl_handle* col = nullptr;         // column slab of a slabbed handle (owned; same device, same stream)
  int64_t C_total = 0, cell_base = 0;  // slabbed handle: cells of the whole job, global id of local cell 0
  int64_t slab_s0 = 0, slab_s1 = 0;    // column slab: its SNP range
  muxgl_group* group = nullptr;        // device group behind this handle (muxgl_group.hip); the fields below are unused then
  int32_t* h_fstat = nullptr;          // pinned: counters of the last E-step (asynchronous phases)
  hipEvent_t ev_stat = nullptr;

  // packed pileup (device)
  int64_t C = 0, S = 0, nnz = 0, R = 0;
  int64_t* d_cell_ptr = nullptr;
  int32_t* d_entry_snp = nullptr;
  int64_t* d_entry_rptr = nullptr;
  uint8_t* d_reads = nullptr;
  int32_t* d_entry_cell = nullptr;  // cell id of each entry (for SNP-major views)
  quad_entry* d_qent = nullptr;     // [nnz] packed records of the quad kernel (built when R < 2^32)
  // One bit per entry: the entry has at most one usable read, so its likelihoods are LINEAR in the two genotypes
  // (demuxlet: pG[l][m] = A + Bl*l + Bm*m, cmd_cram_demuxlet.cpp:673-685 for a single factor) and a pair hypothesis is a
  // two-term form in the samples' moments (sum g, sum l*g) instead of a three-term one -- see demux_wave.hip.
  uint32_t* d_lin = nullptr;        // [ceil(nnz/32)] demuxlet
  int64_t* d_lin_rank = nullptr;    // demuxlet wave kernels, built on first use: plan_build_bit_streams of d_lin
  fmx_grec* d_lin_rec = nullptr;    // [n_lin_rec] {entry, snp} of the linear entries, in entry order
  fmx_grec* d_gen_rec = nullptr;    // [nnz - n_lin_rec] the others
  int64_t n_lin_rec = -1;
  uint2* d_ring_rec = nullptr;      // demux_ring.hip: {snp, table row} of the linear entries, in stream order
  double* d_ring_lut = nullptr;     // ... and the table of (A, Bl, Bm) rows of the current launch
  int64_t ring_rec_n = -1;
  uint32_t* d_flin = nullptr;       // [ceil(nnz/32)] freemuxlet: additionally, no clamp fired (checked on the values)
  // The wave E-step's two streams (fmx_wave.hip, built on first use): a cell's linear entries as 24-byte records
  // {c0, c1, snp} and its other entries as {entry, snp}, both in entry order; d_flin_rank[w] = linear entries before
  // entry 32 w (so a cut of a long cell finds its place in both streams); d_cE[S][K] = g1 + 2 g2 of the posteriors.
  int64_t* d_flin_rank = nullptr;   // [ceil(nnz/32) + 1]
  fmx_lrec* d_lrec = nullptr;
  fmx_grec* d_grec = nullptr;
  double* d_cE = nullptr;
  int64_t n_lrec = -1, cE_n = 0;
  int64_t max_cell_entries = 0;

  // Phred LUT: [0..127] = phred2Err, [128..255] = phred2Mat (bq is 7 bits in the packed read byte)
  double* d_lut = nullptr;

  // demuxlet
  int32_t V = 0;
  double* d_gp = nullptr;
  uint8_t* d_has_gp = nullptr;
  double* d_gpq = nullptr;   // V <= 16: GP tensor re-laid for the quad kernel, [S][6][4][2] (demux_oct.hip)
  double gp_min_sum = 1.0;    // V > 32: smallest sum of a genotype triple (muxgl_demux_set_gp): below 0.35 the split sweep
  bool gp_unit_sums = false;  // V <= 16: every triple sums to 1 within 4 ulp; d_gpq / d_gmq then carry no sums (demux_oct.hip)
  double* d_gp0s = nullptr;  // V <= 16: per-SNP sum of sample 0's triple (the factor every singlet carries, :806)
  double* d_gmq = nullptr;   // V <= 16: moments (s, rho) of every triple in the quad layout, [S + 1][4][4][2] (demux_oct.hip)
  double* d_ll = nullptr;  // [C][V][V][A]
  double* d_llw = nullptr; // wave path: [C][A][64 rotation steps][64 lanes], see demux_wave.hip
  size_t llw_cap = 0;
  bool ll_wave = false;    // the last sweep left its result in d_llw
  size_t ll_cap = 0;
  bool ll_zeroed = false;
  muxgl_demux_cell* d_dcells = nullptr;
  muxgl_demux_cell* h_dcells = nullptr;  // pinned, device-visible
  bool want_full_ll = false;     // this run must leave the LL tensor in d_ll
  bool records_on_host = false;  // the launch wrote the records into h_dcells itself (no D2H copy needed)
  int64_t dcells_cap = 0;
  uint32_t* d_pairs = nullptr;  // packed (j | k<<8 | nmask<<16) work list of the sweep
  int32_t n_pairs = 0;
  int32_t pairs_cap = 0;
  muxgl_demux_params last_dp{};
  bool have_dp = false;
  bool pairs_valid = false;
  struct muxgl_row_state* row = nullptr;  // chunk tables of the V<=16 row kernel (demux_row.hip)
  struct muxgl_row_state* qrow = nullptr; // chunk tables of the default-grid quad kernel (demux_oct.hip)
  struct muxgl_wave_state* wave = nullptr; // cell order + pG table of the 16 < V <= 64 wave kernel (demux_wave.hip)
  int32_t flags = 0;

  // freemuxlet
  double* d_af = nullptr;
  int64_t greedy_near_ties = 0, greedy_overruled = 0;  // of the last muxgl_fmx_greedy_init (fmx_greedy.hip)
  int64_t fmx_exact_scores = 0;  // of the last muxgl_fmx_prepare (score_exact.hpp)
  double* d_egls = nullptr;       // [nnz][9] entry pileup likelihoods (b1)
  int32_t* d_ecnt = nullptr;      // [nnz][3] nreads,nref,nalt
  int32_t K = 0;
  double* d_cgls = nullptr;       // [K][S][9] cluster pileup likelihoods
  int32_t* d_ccnt = nullptr;      // [K][S][3]
  double* d_cgp = nullptr;        // [S][K][3] cluster genotype posteriors for the E-step
  int32_t* d_clust = nullptr;     // [C] current singlet cluster or -1
  uint8_t* d_clust8 = nullptr;    // the same as bytes (255: none), rewritten by every M-step (fmx_mstep.hip)
  int64_t clust8_n = -1;
  muxgl_fmx_cell* d_fcells = nullptr;
  muxgl_fmx_cell* h_fcells = nullptr;  // pinned
  double* d_fll = nullptr;        // [C][K(K+1)/2]; not allocated when the E-step is streamed (fmx_stream.hip)
  bool fmx_streamed = false;      // muxgl_fmx_set_clusters chose the streamed E-step (path_choice.hpp)
  int fmx_sng_state = 0;          // FMX_SNG_*: is d_cgp what the last E-step read? (muxgl_fmx_singlets, fmx_singlets.hip)
  // anchored clusters (fmx_anchor.hip): clusters 0 .. n_anchor-1 read column d_anchor[i] of the panel d_gp instead of
  // their pileups.  Part of the cluster state; they go with the clusters and with the panel (fmx_anchors_drop)
  int32_t n_anchor = 0;
  int32_t* d_anchor = nullptr;    // [n_anchor] donor of every anchored cluster, each in [0, V)
  // their modes (muxgl_fmx_set_anchors_mode): a MUXGL_ANCHOR_PRIOR cluster is a free cluster whose Hardy-Weinberg triple in
  // the posterior's product is the panel row (fmx_prior_kernel, behind fmx_anchor_kernel, and its twin in rows_kernel)
  int32_t n_prior = 0;
  uint8_t* d_anchor_mode = nullptr;  // [n_anchor] MUXGL_ANCHOR_*
  int32_t* d_prior = nullptr;        // [n_prior] the PRIOR clusters, ascending
  bool cgp_valid = false;            // a posterior phase has written d_cgp for these clusters (muxgl_fmx_get_cluster_gp)
  // the streamed E-step's buffers (fmx_stream.hip), kept between iterations: block list, slab, per-cell states
  int32_t* d_fblocks = nullptr;
  int fblocks_k = -1;
  double* d_fslab = nullptr;
  size_t fslab_cap = 0;
  double* d_fss = nullptr;
  size_t fss_cap = 0;
  int32_t* d_fstat = nullptr;     // nsingle, namb, nchanged, cells listed for the exact-call path
  // near-tie calls (fmx_exact.hip): what fmx_call_kernel keeps aside for the exact path
  int32_t* d_prev_clust = nullptr;  // the assignments the cluster pileups of the running iteration were built from: a copy
                                    // of d_clust taken before the call kernel runs, on the handle that runs the M-step
  int32_t* d_prev_state = nullptr;  // [C] (type, jBest, kBest) before the running iteration (fmx_pack_prev)
  int32_t* d_flagged = nullptr;     // [C] cells whose call is within rounding reach, d_fstat[3] of them
  int32_t* d_xc_epoch = nullptr;    // [C] epoch a cell's entry of d_xc was written in (0: none)
  fmx_xc* d_xc = nullptr;           // [C] exact scan results of settled cells
  int32_t xs_epoch = 1;             // advances whenever the E-step's inputs may have changed
  bool xs_keep = false, xs_have_p = false;
  muxgl_fmx_params xs_p{};
  int64_t fmx_exact_cells = 0, fmx_exact_changed = 0, fmx_exact_unresolved = 0;  // since muxgl_fmx_set_clusters
  struct fmx_exact_state* xs = nullptr;  // between steps A and C of the exact path (fmx_exact.hip)
  int32_t fmx_listed = 0;                // cells the last fetch of a sharded phase found listed and left open
  std::vector<int32_t> xs_snps;          // muxgl_fmx_exact_snps: the list between the size query and the copy
  bool xs_snps_valid = false;
  // SNP-major (CSC) view of the entries, cells ascending inside each SNP: M-step walks it
  int64_t* d_snp_ptr = nullptr;   // [S+1]
  int64_t* d_snp_entry = nullptr; // [nnz] entry index
  int32_t* d_snp_cell = nullptr;  // [nnz] cell id of the same SNP-major element
  double* d_segls = nullptr;      // [nnz][9] entry likelihoods in SNP-major order (freemuxlet-old's kernels)
  double* d_segls6 = nullptr;     // [nnz][6] their six distinct values {00,11,22,01,02,12}: the ordered M-step streams them
  uint16_t* d_scode = nullptr;    // [nnz] SNP-major: read byte of an entry with at most one usable read, 0x100 otherwise (fmx_scode_kernel)
  double* d_mtab = nullptr;       // [256][6] the six values of a one-read entry by its read byte (fmx_mstep.hip)
  int32_t* d_secnt = nullptr;     // [nnz][3] entry counts in SNP-major order
  bool fmx_prepared = false;
  int64_t fc0 = 0, fc1 = 0, fs0 = 0, fs1 = 0;  // active cell / SNP shard of the EM phases (default: everything)
  muxgl_row_state* frow = nullptr;             // chunk tables restricted to the cell shard
  muxgl_row_state* fqrow = nullptr;            // same for the quad E-step
  double* d_cgpq = nullptr;                    // [S][6][4][2] cluster-GP rows re-laid per quad (fmx_oct.hip)
  double* d_ceq = nullptr;                     // [S + 1][2][4][2] their moments E = g1 + 2 g2 (fmx_oct.hip)
  size_t ceq_cap = 0;
  size_t cgpq_cap = 0;

  // freemuxlet-old (fmx_old.hip)
  int8_t* d_sgn = nullptr;  // [C][sgn_ld] vote sign of every ordered cell pair: +1 / -1 / 0 against --bf-thres
  int64_t sgn_ld = 0;       // row stride, a multiple of 16 with at least 16 zero bytes of padding

  hipEvent_t ev[2 * MUXGL_T_COUNT] = {};
  bool ev_used[MUXGL_T_COUNT] = {};
  int ev_start[MUXGL_T_COUNT] = {};  // index into ev[] of a slot's start event (toc_tic: the previous slot's stop event)
  float ms[MUXGL_T_COUNT] = {};
  double ms_sum[MUXGL_T_COUNT] = {};  // the same summed over the calls since muxgl_get_timing_sum(.., reset = 1)
  int64_t ms_calls = 0;
};

// a device group behind one handle (muxgl_group.hip; soup_mix.hip walks the members for its two calls)
struct muxgl_group {
  int n = 0;
  std::vector<muxgl_handle*> m;
  std::vector<int64_t> cb, eb, sb;  // [n+1] cell, entry and SNP cuts
  int64_t C = 0, S = 0, nnz = 0, R = 0;
  int32_t V = 0, K = 0, n_alpha = 0;
  bool have_pileup = false, have_cols = false, prepared = false;
  muxgl_demux_cell* h_dcells = nullptr;  // [C] records of the last demuxlet run, in cell order
  std::vector<hipEvent_t> ev_gp, ev_es;  // per member: posterior rows ready / assignments ready
  float ms[MUXGL_T_COUNT] = {};
  int32_t peer_pairs = 0, peer_enabled = 0, peer_refused = 0;  // of group_create's walk over the member pairs
};

extern thread_local std::string g_muxgl_create_error;

// The anchors of muxgl_fmx_set_anchors go: with the clusters (muxgl_fmx_set_clusters, muxgl_fmx_prepare, a new pileup or
// slab) and with the panel they index (demux_panel_release).  Where there were some, d_cgp is no longer what the next
// E-step reads: as muxgl_fmx_set_anchors itself, no table of the last E-step and no settled near-tie cell survives.
static inline void fmx_anchors_drop(muxgl_handle* h) {
  if (h->n_anchor == 0) return;
  h->n_anchor = 0;
  h->n_prior = 0;
  h->fmx_sng_state = FMX_SNG_NONE;
  h->xs_keep = false;
  ++h->xs_epoch;
}

// MUXGL_TIMING=1: host-side stage times of the hand-over calls on stderr
struct host_timer {
  bool on;
  double t0;
  static double now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
  }
  host_timer() : on(getenv("MUXGL_TIMING") != nullptr), t0(now()) {}
  void lap(const char* what) {
    if (!on) return;
    const double t = now();
    fprintf(stderr, "[muxgl] %-44s %8.1f ms\n", what, (t - t0) * 1e3);
    t0 = t;
  }
};

#define MUXGL_FAIL(h, ...)                                  \
  do {                                                      \
    char _buf[512];                                         \
    snprintf(_buf, sizeof(_buf), __VA_ARGS__);              \
    (h)->err = _buf;                                        \
    return 1;                                               \
  } while (0)

#define HIPCHK(h, call)                                                                         \
  do {                                                                                          \
    hipError_t _e = (call);                                                                     \
    if (_e != hipSuccess) MUXGL_FAIL(h, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),  \
                                     __FILE__, __LINE__);                                       \
  } while (0)

// CALL(W) for the lane width W of a sweep whose lanes are (entry slot, column): the columns rounded up to a power of two,
// 64 from 33 columns on (lane_width.hpp), in the manner of demux_entry.hpp's DISPATCH_NA.  It names the seven
// widths a unit instantiates (fmx_pairs.hip has no width 1 and keeps a switch of its own).
#define DISPATCH_WIDTH(W, CALL) \
  switch (W) {                  \
    case 1: CALL(1); break;     \
    case 2: CALL(2); break;     \
    case 4: CALL(4); break;     \
    case 8: CALL(8); break;     \
    case 16: CALL(16); break;   \
    case 32: CALL(32); break;   \
    default: CALL(64); break;   \
  }

// ---- device memory: dev_alloc / dev_free with a per-handle cache of large blocks -----------------------------------------
// The phases of a run allocate and free tens of GB each (entry likelihoods, the greedy start's tables, cluster pileups);
// hipMalloc of memory that was in use before costs ~30 ms per GB on these boxes (the driver clears it) and hipFree drains
// the device.  Blocks of DEV_POOL_MIN bytes or more therefore go back to a cache of the handle that allocated them and
// are handed out again to a request they fit (best fit, at most a quarter + 16 MB larger than asked for); the stream of
// the handle is drained before a cached block is reused, which is what hipFree would have done when it was released.
// A failed hipMalloc empties every cache of the process and tries again; muxgl_destroy empties the handle's.
// MUXGL_NO_POOL=1 turns the cache off.
constexpr size_t DEV_POOL_MIN = (size_t)8 << 20;
struct dev_block_info {
  size_t bytes;
  muxgl_handle* owner;  // NULL once its handle is gone: the block is then freed for good
};
struct dev_registry {
  std::mutex mu;
  std::unordered_map<void*, dev_block_info> blocks;   // live and cached blocks of at least DEV_POOL_MIN bytes
  std::unordered_set<muxgl_handle*> handles;          // handles with a cache
};
inline dev_registry& dev_reg() {
  static dev_registry r;
  return r;
}
inline bool dev_pool_on() {
  static const bool on = getenv("MUXGL_NO_POOL") == nullptr;
  return on;
}
void dev_pool_release(muxgl_handle* h, bool forget_owner);  // muxgl_api.hip
void dev_pool_release_all();
// hipMalloc for buffers that do not go through the cache (rocprim temporaries): on failure the cached blocks of every handle
// go back to the driver and the allocation is tried once more, as dev_alloc does
hipError_t dev_malloc_retry(void** p, size_t bytes);

int dev_alloc_bytes(muxgl_handle* h, void** p, size_t bytes);  // muxgl_api.hip
void dev_free_bytes(void* p);

template <typename T>
static inline void dev_free(T** p) {
  if (*p) dev_free_bytes((void*)*p);
  *p = nullptr;
}

template <typename T>
static inline int dev_alloc(muxgl_handle* h, T** p, size_t n) {
  dev_free(p);
  if (n == 0) n = 1;
  return dev_alloc_bytes(h, (void**)p, n * sizeof(T));
}

// a temporary of one call: dev_alloc(h, &t.p, n), freed (back to the handle's cache) when t goes out of scope
template <typename T>
struct dev_tmp {
  T* p = nullptr;
  dev_tmp() = default;
  dev_tmp(const dev_tmp&) = delete;
  dev_tmp& operator=(const dev_tmp&) = delete;
  ~dev_tmp() { dev_free(&p); }
};

// slab budget of the streamed paths on the current device (stream_plan.hpp)
static inline size_t dev_slab_budget(const char* env_mb) {
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) tot = 0;
  return stream_plan::slab_budget_bytes(env_mb, tot);
}

static inline bool timing_off() {  // MUXGL_NO_EVENTS=1: no hipEvent records around the kernels (launch-gap experiments)
  static const bool off = getenv("MUXGL_NO_EVENTS") != nullptr;
  return off;
}
// A call's own event pair, for the calls that report their kernel time through a `kernel_ms` argument and leave the
// handle's timing slots alone.  The events exist only when kernel_ms is wanted and timing is on; start / stop record
// them around the kernels, add() (behind a stream synchronise) adds the bracket to *kernel_ms; they are destroyed on
// every way out of the call.
struct call_events {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float* ms = nullptr;
  call_events() = default;
  call_events(const call_events&) = delete;
  call_events& operator=(const call_events&) = delete;
  ~call_events() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  int create(muxgl_handle* h, float* kernel_ms, const char* who) {
    if (!kernel_ms || timing_off()) return 0;
    HIPCHK(h, hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) MUXGL_FAIL(h, "%s: hipEventCreate failed", who);
    ms = kernel_ms;
    return 0;
  }
  int start(muxgl_handle* h) {
    if (ms) HIPCHK(h, hipEventRecord(ev0, h->stream));
    return 0;
  }
  int stop(muxgl_handle* h, bool /*last batch (table_call.hpp)*/ = false) {
    if (ms) HIPCHK(h, hipEventRecord(ev1, h->stream));
    return 0;
  }
  void add() {
    float t = 0.f;
    if (ms && hipEventElapsedTime(&t, ev0, ev1) == hipSuccess) *ms += t;
  }
};

static inline void tic(muxgl_handle* h, int id) {
  if (timing_off()) return;
  (void)hipEventRecord(h->ev[2 * id], h->stream);
  h->ev_start[id] = 2 * id;
  h->ev_used[id] = true;
}
// stop of slot `id` and start of slot `next` as ONE event record (a record costs ~2.6 us of host time per call)
static inline void toc_tic(muxgl_handle* h, int id, int next) {
  if (timing_off()) return;
  (void)hipEventRecord(h->ev[2 * id + 1], h->stream);
  h->ev_start[next] = 2 * id + 1;
  h->ev_used[next] = true;
}
static inline void toc(muxgl_handle* h, int id) {
  if (timing_off()) return;
  (void)hipEventRecord(h->ev[2 * id + 1], h->stream);
}
static inline void clear_timing(muxgl_handle* h) {
  h->split_timed = false;
  for (int i = 0; i < MUXGL_T_COUNT; ++i) {
    h->ev_used[i] = false;
    h->ms[i] = 0.f;
  }
}
// The host's join of a two-group run of the oct path (demux_oct.hip): waits for what the run left on stream2.  Called
// behind the wait for the handle's stream by whoever reads the run's records or timing slots, and in front of whatever
// frees what the second group writes (muxgl_set_pileup, muxgl_destroy): nothing is outstanding on stream2 outside a run.
static inline hipError_t join_stream2(muxgl_handle* h) {
  if (!h->stream2_busy) return hipSuccess;
  h->stream2_busy = false;
  return hipStreamSynchronize(h->stream2);
}
// Reads the brackets recorded since the last call: a slot is summed ONCE per bracket (its `used` mark is cleared here,
// so the phased API, which collects after every phase, does not add the earlier phases' times again) and only when
// the elapsed-time query succeeds; ms[] keeps the last value of every slot until clear_timing.  ms_calls counts the
// collecting calls (include/muxgl.h says which entry points those are).
static inline void collect_timing(muxgl_handle* h) {
  if (h->split_timed) {
    // The oct path ran as two cell groups on two streams (demux_oct.hip).  With A = the start (start event of SWEEP),
    // E1 / E2 = the ends of the two sweeps (stop event of SWEEP, ev_sweep2) and F1 / F2 = the ends of the two finishes
    // (stop event of REDUCE, ev_finish2): SWEEP = max(E1, E2) - A and REDUCE = max(F1, F2) - A - SWEEP, the later of two
    // elapsed times each, taken here on the host -- nothing on the device orders one group behind the other.
    h->split_timed = false;
    h->ev_used[MUXGL_T_DEMUX_SWEEP] = h->ev_used[MUXGL_T_DEMUX_REDUCE] = false;
    float t1 = 0.f, t2 = 0.f, tf = 0.f, tf2 = 0.f;
    hipEvent_t a = h->ev[2 * MUXGL_T_DEMUX_SWEEP];
    if (hipEventElapsedTime(&t1, a, h->ev[2 * MUXGL_T_DEMUX_SWEEP + 1]) == hipSuccess &&
        hipEventElapsedTime(&t2, a, h->ev_sweep2) == hipSuccess &&
        hipEventElapsedTime(&tf, a, h->ev[2 * MUXGL_T_DEMUX_REDUCE + 1]) == hipSuccess &&
        hipEventElapsedTime(&tf2, a, h->ev_finish2) == hipSuccess) {
      tf = tf > tf2 ? tf : tf2;
      const float ts = t1 > t2 ? t1 : t2, tr = tf > ts ? tf - ts : 0.f;
      h->ms[MUXGL_T_DEMUX_SWEEP] = ts;
      h->ms_sum[MUXGL_T_DEMUX_SWEEP] += (double)ts;
      h->ms[MUXGL_T_DEMUX_REDUCE] = tr;
      h->ms_sum[MUXGL_T_DEMUX_REDUCE] += (double)tr;
    }
  }
  for (int i = 0; i < MUXGL_T_COUNT; ++i) {
    if (h->ev_used[i]) {
      h->ev_used[i] = false;
      float t = 0.f;
      if (hipEventElapsedTime(&t, h->ev[h->ev_start[i]], h->ev[2 * i + 1]) == hipSuccess) {
        h->ms[i] = t;
        h->ms_sum[i] += (double)t;
      }
    }
  }
  ++h->ms_calls;
}

// ---- device helpers ---------------------------------------------------------------------------------------------

// product accumulator: value = m * 2^e, renormalised to m in [0.5,1) every few factors so that a cell's
// sum of log(sumP) becomes one log() at the end:  sum log x_i = log(prod mantissas) + ln2 * sum exponents
struct prodacc {
  double m;
  int32_t e;
};
__device__ __forceinline__ void prodacc_renorm(double& m, int32_t& e) {
  int ex;
  m = frexp(m, &ex);
  e += ex;
}
// log of a positive finite double for the end of a product accumulator (round 5).  The library log costs 98 vector
// instructions for special cases a product of positive likelihoods does not have; at 64 samples and six alphas a cell has
// 18 208 hypotheses, one log each: 3 % of the sweep's instructions.  Here: x = f 2^k with f in [sqrt(1/2), sqrt(2)),
// log f = 2 atanh(z), z = (f - 1) / (f + 1), |z| <= 0.1716, as the odd series up to z^21 (truncation 2e-17 relative to z);
// ~30 instructions, absolute error <= 2e-16 + 1 ulp of the result.  x = 0 gives -inf (the series' own result would be
// meaningless there), as log does.
__device__ __forceinline__ double pos_log(double x, double k0) {
  int ee;
  double f = frexp(x, &ee);  // [0.5, 1)
  const bool lo = f < 0.70710678118654752440;
  f = lo ? f + f : f;
  const double k = (double)(ee - (lo ? 1 : 0)) + k0;
  const double z = (f - 1.0) / (f + 1.0);
  const double w = z * z;
  double p = 1.0 / 21.0;
  p = fma(p, w, 1.0 / 19.0);
  p = fma(p, w, 1.0 / 17.0);
  p = fma(p, w, 1.0 / 15.0);
  p = fma(p, w, 1.0 / 13.0);
  p = fma(p, w, 1.0 / 11.0);
  p = fma(p, w, 1.0 / 9.0);
  p = fma(p, w, 1.0 / 7.0);
  p = fma(p, w, 1.0 / 5.0);
  p = fma(p, w, 1.0 / 3.0);
  const double zz = z + z;
  const double r = fma(zz * w, p, zz);  // 2 atanh(z)
  // k ln 2 in two pieces (the high one exact for |k| < 2^21), smallest terms first
  const double v = fma(k, 6.93147180369123816490e-01, fma(k, 1.90821492927058770002e-10, r));
  // log's own conventions outside the domain: 0 -> -inf; a negative or NaN product (a corrupt genotype tensor) stays NaN
  // instead of turning into a -inf score that later sums would absorb
  return x > 0.0 ? v : (x == 0.0 ? -__builtin_huge_val() : __builtin_nan(""));
}
__device__ __forceinline__ double prodacc_log(double m, int32_t e) { return pos_log(m, (double)e); }

// ---- the ring of partner values of the wave kernels (demux_wave.hip, fmx_wave.hip) ----
// One 8-byte read per lane from the ring in LDS, at an immediate offset from the lane's slot.  As an opaque instruction
// because two such reads with one base are otherwise merged into a ds_read2_b64, which takes 8 LDS cycles instead of
// 2 + 2 (MI355X_MICROARCH.md, LDS table).  The caller waits (s_waitcnt lgkmcnt) before using the value; "memory" keeps
// the next entry's ring stores behind it.
template <int OFF>
__device__ __forceinline__ double wave_ring_rd(uint32_t a) {
  double v;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF) : "memory");
  return v;
}
typedef double dbl2 __attribute__((ext_vector_type(2)));
// ... and 16 bytes (two doubles at a 16-byte aligned address): 4 LDS cycles, and one DS instruction where two 8-byte reads
// are two
template <int OFF>
__device__ __forceinline__ dbl2 wave_ring_rd128(uint32_t a) {
  dbl2 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF) : "memory");
  return v;
}
template <int I, int N, class F>
__device__ __forceinline__ void wave_for(F&& f) {  // f(integral_constant<int, I>) ... f(integral_constant<int, N - 1>)
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    wave_for<I + 1, N>(f);
  }
}

// which entries of a cell a wave-per-cell sweep walks: all of them, or those whose bit in the linear-entry set is
// set / clear (plan_build_lin, fmx_entry_kernel)
enum { EM_ALL = 0, EM_LINEAR = 1, EM_GENERAL = 2 };
// first entry >= e in [e, e1) of the kind the launch sweeps (wave-uniform: scalar loads and bit scans)
template <int EM>
__device__ __forceinline__ int64_t wave_next_entry(const uint32_t* __restrict__ lin, int64_t e, int64_t e1) {
  if (EM == EM_ALL) return e;
  while (e < e1) {
    uint32_t w = lin[e >> 5];
    if (EM == EM_GENERAL) w = ~w;
    w >>= (uint32_t)(e & 31);
    if (w) {
      e += __builtin_ctz(w);
      return e < e1 ? e : e1;
    }
    e = (e | 31) + 1;
  }
  return e1;
}

// where the entries [e0, e1) of a work unit lie in the stream of the set (EM_LINEAR) or clear (EM_GENERAL) bits of `bits`
// (plan_build_bit_streams): set bits before e = rank[e / 32] + set bits below e in its word
template <int EM>
__device__ __forceinline__ void wave_stream_range(const uint32_t* __restrict__ bits, const int64_t* __restrict__ rank, int64_t e0,
                                                  int64_t e1, int64_t& i0, int64_t& i1) {
  auto before = [&](int64_t e) {
    int64_t r = rank[e >> 5];
    if (e & 31) r += __popc(bits[e >> 5] & ((1u << (e & 31)) - 1u));
    return r;
  };
  const int64_t l0 = before(e0), l1 = before(e1);
  i0 = EM == EM_LINEAR ? l0 : e0 - l0;
  i1 = EM == EM_LINEAR ? l1 : e1 - l1;
}

// Workgroup -> work-unit index with XCD affinity.  The dispatcher is observed to place workgroup b on XCD b % 8
// (MI355X_MICROARCH.md; used for speed only, nothing depends on it): the work list is cut into 8 contiguous blocks,
// one per XCD, so that workgroups resident on one XCD walk neighbouring work units -- here neighbouring SNP windows of
// the GP tensor, which then fit that XCD's 4 MiB L2.  n8 = ceil(n/8); the result may be >= n (caller checks).
__device__ __forceinline__ int xcd_swizzle(int b, int n8) { return (b & 7) * n8 + (b >> 3); }

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// sc_drop_seq.cpp:5-8
__device__ __forceinline__ double dev_logadd(double la, double lb) {
  if (la > lb) return la + log(1.0 + exp(lb - la));
  return lb + log(1.0 + exp(la - lb));
}

// Work unit of the wave kernels (demux_wave.hip, fmx_wave.hip): a run of entries of one cell.  A cell is walked by one
// wave, so a launch cannot end before its longest cell has been walked; with few cells that walk IS the launch (10 k
// cells: 10 ms for any shape), with many it hides behind throughput-bound work.  Cells longer than 2048 entries are
// therefore cut into equal parts, each with a result slab of its own (part 0: the cell's slab, the others: overflow
// slabs behind the C cell slabs), and the parts' log-likelihoods are added up afterwards.  The cut depends on the cell
// alone, so a cell's result does not depend on which other cells share the handle (shards reproduce the whole run bit
// for bit).
struct wave_item {
  int64_t e0, e1;  // entries
  int64_t slab;    // result slab (in units of one cell's slabs)
  int64_t cell;
};
struct wave_cut {
  int64_t cell, first, count;  // overflow slabs [first, first + count)
};
// the wave plan of a handle (demux_wave_plan, at muxgl_set_pileup time) and the wave path's tables (demux_wave.hip)
struct muxgl_wave_state {
  int32_t* d_order = nullptr;  // cells, longest first
  wave_item* d_items = nullptr;  // work units of the demuxlet wave kernels, longest first
  wave_cut* d_cuts = nullptr;    // cells cut into several units
  int64_t n_items = 0, n_cuts = 0, n_over = 0;
  double* d_pg = nullptr;      // [nnz][A][9]
  double* d_gm = nullptr;      // [S][V][2], see wave_gm_kernel
  size_t gm_cap = 0;
  size_t pg_cap = 0;
};
struct ring_sel {          // one launch of demux_ring.hip
  int32_t n[4];            // alpha indices of the non-symmetric slots
  int32_t nsym;            // ... of the symmetric slot (0: none)
  int32_t with_singlet;    // the launch also fills llw[c][block][0][0][lane]
  int32_t jbase, blk, nblk2;  // first sample of the diagonal block, its slab, slabs per cell
};

// kernel launchers implemented in the kernel TUs.  Which one runs is decided by demux_launch, fmx_phase_estep, ... from
// the choosers of path_choice.hpp; a launcher is only called for a job its path takes (0 ok, 1 error)
int demux_launch(muxgl_handle* h, const muxgl_demux_params* p);
int demux_stream_launch(muxgl_handle* h, const muxgl_demux_params* p);   // streamed sweep + fold + call
int demux_singlets_run(muxgl_handle* h, const muxgl_demux_params* p, double* sng);  // demux_singlets.hip: [C][V] to the host
// demux_unknown.hip: the three tables of muxgl_demux_unknown to the host (any may be NULL), rows of the handle's own cells
int demux_unknown_run(muxgl_handle* h, const muxgl_demux_params* p, const double* gp0, double* ll_ju, double* ll_uj,
                      double* ll_uu, float* kernel_ms);
// demux_ambient.hip: the table of muxgl_demux_ambient to the host, rows of the handle's own cells.  n_rho and rho are
// checked by the caller (demux_ambient_bad_rho), amb_af here, against the handle's has_gp
int demux_ambient_run(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int n_rho, const double* rho,
                      double* ll_amb, float* kernel_ms);
int demux_ambient_bad_rho(int n_rho, const double* rho);  // the first rho that is not a finite number in [0, 1], or -1
// demux_ambient.hip: amb_af against the handle's has_gp (a finite number in [0, 1] wherever a marker has genotypes), for
// the call named `who`
int demux_ambient_check_af(muxgl_handle* h, const double* amb_af, const char* who);
// demux_ambient_fit.hip: the fit of muxgl_demux_ambient_fit to the host, rows of the handle's own cells; the arguments but
// amb_af are checked by the caller (demux_ambient_fit_bad_args, fit_args.hpp)
int demux_ambient_fit_run(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int n_cand, const int32_t* cand,
                          double rho_max, double* rho_hat, double* ll_hat, double* ll_zero, double* info, int32_t* status,
                          int32_t* n_steps, float* kernel_ms);
// demux_alpha_fit.hip: the fit of muxgl_demux_alpha_fit to the host, rows of the handle's own cells; the arguments are
// checked by the caller (demux_alpha_fit_bad_args, fit_args.hpp)
int demux_alpha_fit_run(muxgl_handle* h, const muxgl_demux_params* p, int n_cand, const int32_t* pair, double alpha_max,
                        double* alpha_hat, double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status,
                        int32_t* n_steps, float* kernel_ms);
// demux_ambient.hip: usable reads by marker and allele of the handle's own cells whose mask byte is set (cell_mask: host
// [C] or NULL), to n_ref / n_alt (host [S])
int pileup_allele_counts_run(muxgl_handle* h, const uint8_t* cell_mask, int64_t* n_ref, int64_t* n_alt);
struct demux_incl_out {  // muxgl_demux_inclusion's outputs (host; any may be NULL), rows of the handle's own cells
  double *incl, *tot, *dbl;
  int32_t *partner, *alpha_idx, *first;
};
int demux_inclusion_run(muxgl_handle* h, const muxgl_demux_params* p, const demux_incl_out& out);  // demux_incl.hip
int demux_entry_pg_launch(muxgl_handle* h, const muxgl_demux_params* p, double* d_pg, bool gen_stream = false,
                          bool by_record = false);
int demux_ring_lin_launch(muxgl_handle* h, const muxgl_demux_params* p, const wave_item* items, int64_t n_items,
                          const double* gm, int na, const ring_sel& sel, double* llw, const double* pgt = nullptr,
                          bool pg_by_record = false);
void demux_ring_release(muxgl_handle* h);
void demux_panel_release(muxgl_handle* h);  // muxgl_api.hip: the GP tensor and what was made from it; V = 0
int demux_row_plan(muxgl_handle* h);
int demux_row_launch(muxgl_handle* h, const muxgl_demux_params* p);
void demux_row_free(muxgl_handle* h);
int demux_row_build(muxgl_handle* h, muxgl_row_state** st, int64_t c0, int64_t c1, int ch);
int demux_oct_launch(muxgl_handle* h, const muxgl_demux_params* p);
int demux_oct_split_info(const muxgl_handle* h, int64_t* out);  // muxgl_demux_oct_split
int demux_row2_launch(muxgl_handle* h, const muxgl_demux_params* p);  // (demux_row2.hip)
double row2_part_bytes(const muxgl_row_state* st);  // chunk partials of the two-per-lane row kernels (demux_row2.hip)
int demux_call16_launch(muxgl_handle* h, const muxgl_demux_params* p);
int fmx_oct_estep_launch(muxgl_handle* h, muxgl_row_state* st, int64_t c0, int64_t nc);
int fmx_row2_estep_launch(muxgl_handle* h, muxgl_row_state* st, int64_t c0, int64_t nc);
int demux_wave_plan(muxgl_handle* h, const int64_t* cell_ptr);
int demux_wave_launch(muxgl_handle* h, const muxgl_demux_params* p);
const int32_t* demux_wave_order(const muxgl_handle* h);  // cells, longest first (device)
int demux_wave_items(const muxgl_handle* h, const wave_item** items, int64_t* n_items, const wave_cut** cuts,
                     int64_t* n_cuts, int64_t* n_over);  // work units of the wave kernels (device)
int fmx_wave_estep_launch(muxgl_handle* h, int64_t c0, int64_t nc);  // 32 < K <= 255
int64_t fmx_wave_fll_rows(const muxgl_handle* h);  // rows of d_fll: C + extra parts of long cells
int fmx_stream_estep_launch(muxgl_handle* h, const muxgl_fmx_params* p, int64_t c0, int64_t nc);  // fmx_stream.hip
int fmx_stream_call_launch(muxgl_handle* h, int64_t c0, int64_t c1, double lsp, double ldp);
int fmx_stream_rows(muxgl_handle* h, const std::vector<int32_t>& cells, double* rows);  // deep-tie rows, host
// what every demuxlet call on a panel asks first: 0, or 1 with h's message set.  The two "is it set" facts are the caller's:
// a handle knows them as d_cell_ptr and d_gp, a device group as have_pileup and V
static inline int demux_preconditions(muxgl_handle* h, const muxgl_demux_params* p, bool have_pileup, bool have_gp) {
  if (!p) MUXGL_FAIL(h, "demux params NULL");
  if (p->n_alpha < 1 || p->n_alpha > MUXGL_MAX_ALPHA) MUXGL_FAIL(h, "n_alpha=%d outside [1,%d]", p->n_alpha, MUXGL_MAX_ALPHA);
  if (!have_pileup) MUXGL_FAIL(h, "no pileup set (muxgl_set_pileup)");
  if (!have_gp) MUXGL_FAIL(h, "no GP tensor set (muxgl_demux_set_gp)");
  return 0;
}
// fmx_refusal.hpp's rule on the state of m (the handle itself, or a member of its group): 0, or 1 with h's message set
static inline int fmx_refuse(muxgl_handle* h, const muxgl_handle* m, const char* who, const char* what) {
  char why[256];
  if (fmx_table_refusal(who, what, m->d_cell_ptr != nullptr, m->fmx_prepared, m->K, m->fmx_sng_state, why, sizeof(why)))
    MUXGL_FAIL(h, "%s", why);
  return 0;
}
// fmx_unknown.hip: the first row of gp0[S][3] that is no probability triple (muxgl_fmx_unknown's rule), or -1
int64_t fmx_unknown_bad_prior(const double* gp0, int64_t S);
// fmx_ambient.hip: muxgl_fmx_ambient's checks of its arguments, on the host: 0, or 1 with the reason written to `why`
int fmx_ambient_bad_args(const double* amb_af, int64_t S, int32_t n_rho, const double* rho, double* ll_amb, char* why,
                         size_t why_len);
// (the same for muxgl_fmx_ambient_fit and muxgl_fmx_alpha_fit: fmx_ambient_fit_bad_args, fmx_alpha_fit_bad_args, fit_args.hpp)
void fmx_wave_streams_release(muxgl_handle* h);  // the linear/general entry streams and their rank table
int demux_ensure_ll(muxgl_handle* h, const muxgl_demux_params* p);  // standard LL tensor allocated and zeroed
int demux_call_wave_launch(muxgl_handle* h, const muxgl_demux_params* p);
void demux_wave_free(muxgl_handle* h);
int demux_gp_neutral_rows(muxgl_handle* h, int V);  // d_gp rows of markers without genotypes := (1,0,0) (demux_wave.hip)
void demux_row_release(muxgl_row_state** st);
int plan_build_chunks(muxgl_handle* h, muxgl_row_state* st, int64_t cb, int64_t ce, int ch);  // chunk tables (plan_kernels.hip)
int plan_build_qent(muxgl_handle* h);       // packed entry records of the quad kernel, on the device (plan_kernels.hip)
int quad_launch_order(muxgl_handle* h, const row_chunk* d_chunks, const int32_t* d_nlin, int64_t n, int32_t** order,
                      int64_t cut = 0);  // cut > 0: the chunks of cells below `cut` first
int plan_build_lin(muxgl_handle* h);        // d_lin (plan_kernels.hip)
int plan_build_bit_streams(muxgl_handle* h, const uint32_t* bits, int64_t** rank, fmx_grec** rec_set, fmx_grec** rec_clr,
                           int64_t* n_set);
void plan_lin_streams_release(muxgl_handle* h);
int plan_build_snp_major(muxgl_handle* h);  // d_entry_cell, d_snp_ptr, d_snp_entry, d_snp_cell (plan_kernels.hip)

// handle plumbing shared by muxgl_api.hip and muxgl_group.hip
int muxgl_handle_create(int device, int32_t flags, hipStream_t shared_stream, muxgl_handle** out, std::string* err);
int muxgl_validate_pileup(muxgl_handle* h, int64_t C, int64_t S, int64_t nnz, int64_t R, const int64_t* cell_ptr,
                          const int32_t* entry_snp, const int64_t* entry_rptr, int64_t* maxlen_out);
int muxgl_set_pileup_role(muxgl_handle* h, int role, int64_t C, int64_t S, int64_t nnz, int64_t R, const int64_t* cell_ptr,
                          const int32_t* entry_snp, const int64_t* entry_rptr, const uint8_t* reads, bool trusted = false);
int fmx_attach_column_slab(muxgl_handle* h, int64_t C_total, int64_t c0, int64_t s0, int64_t s1, int64_t nnz_s, int64_t R_s,
                           const int64_t* cell_ptr_s, const int32_t* entry_snp_s, const int64_t* entry_rptr_s,
                           const uint8_t* reads_s, bool trusted);
int fmx_cluster_counts_device(muxgl_handle* m);  // m->d_ccnt := read counts of the cluster pileups (stream-ordered)
int fmx_snp_major_full(muxgl_handle* h);  // d_segls / d_secnt on first use (freemuxlet-old)
int fmx_phase_gp(muxgl_handle* h, const muxgl_fmx_params* p);
int fmx_phase_estep(muxgl_handle* h, const muxgl_fmx_params* p);
int fmx_anchor_launch(muxgl_handle* h, const muxgl_fmx_params* p);  // fmx_anchor.hip: the anchored columns of d_cgp
int fmx_set_anchors_on(muxgl_handle* h, int32_t n_anchor, const int32_t* donor, const uint8_t* mode, bool member);
int fmx_get_cluster_gp_on(muxgl_handle* h, int32_t k0, int32_t k1, double* out);
int fmx_phase_mstep(muxgl_handle* h);
int fmx_mstep_stream_launch(muxgl_handle* h);  // K <= 64 (fmx_mstep.hip)
// fmx_exact.hip: near-tie calls settled in the reference's arithmetic (steps A, B, C; all three on one handle)
int fmx_exact_snps(muxgl_handle* h, std::vector<int32_t>* snps);
int fmx_exact_rows(muxgl_handle* h, const muxgl_fmx_params* p, const int32_t* snps, int64_t n, double* rows, uint8_t* owned);
int fmx_exact_finish(muxgl_handle* h, const muxgl_fmx_params* p, const int32_t* snps, int64_t n, const double* rows,
                     int64_t* deltas, int32_t* reassigned);
int fmx_exact_resolve(muxgl_handle* h, const muxgl_fmx_params* p, bool* reassigned);
void fmx_exact_release(muxgl_handle* h);

// device groups (muxgl_group.hip): every entry point of the C-ABI forwards here when h->group is set
int group_create(const muxgl_config* cfg, muxgl_handle** out, std::string* err);
void group_destroy(muxgl_handle* h);
int group_set_pileup(muxgl_handle* h, int64_t C, int64_t S, int64_t nnz, int64_t R, const int64_t* cell_ptr,
                     const int32_t* entry_snp, const int64_t* entry_rptr, const uint8_t* reads);
int group_demux_set_gp(muxgl_handle* h, int32_t V, const double* gp, const uint8_t* has_gp);
int group_demux_run(muxgl_handle* h, const muxgl_demux_params* p, muxgl_demux_cell* out, double* full_ll);
int group_demux_singlets(muxgl_handle* h, const muxgl_demux_params* p, double* sng);
int group_demux_inclusion(muxgl_handle* h, const muxgl_demux_params* p, const demux_incl_out& out);
int group_demux_unknown(muxgl_handle* h, const muxgl_demux_params* p, const double* gp0, double* ll_ju, double* ll_uj,
                        double* ll_uu, float* kernel_ms);
int group_demux_ambient(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int32_t n_rho, const double* rho,
                        double* ll_amb, float* kernel_ms);
int group_pileup_allele_counts(muxgl_handle* h, const uint8_t* cell_mask, int64_t* n_ref, int64_t* n_alt);
int group_demux_ambient_fit(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int32_t n_cand,
                            const int32_t* cand, double rho_max, double* rho_hat, double* ll_hat, double* ll_zero, double* info,
                            int32_t* status, int32_t* n_steps, float* kernel_ms);
int group_demux_alpha_fit(muxgl_handle* h, const muxgl_demux_params* p, int32_t n_cand, const int32_t* pair, double alpha_max,
                          double* alpha_hat, double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status,
                          int32_t* n_steps, float* kernel_ms);
const muxgl_demux_cell* group_demux_results(const muxgl_handle* h);
int group_demux_get_entry_pg(muxgl_handle* h, double* pg);
int group_fmx_prepare(muxgl_handle* h, const double* af, double* cell_llk0, double* cell_llk2, int32_t* cell_nsnps,
                      int32_t* cell_nreads);
int group_fmx_get_entry_gls(muxgl_handle* h, double* gls, int32_t* counts);
int group_fmx_set_clusters(muxgl_handle* h, int32_t K, const int32_t* clust);
int group_fmx_set_anchors(muxgl_handle* h, int32_t n_anchor, const int32_t* donor, const uint8_t* mode);
int group_fmx_get_cluster_gp(muxgl_handle* h, int32_t k0, int32_t k1, double* out);
int group_fmx_iterate(muxgl_handle* h, const muxgl_fmx_params* p, muxgl_fmx_cell* out, int32_t* nsingle, int32_t* namb,
                      int32_t* nchanged, double* full_ll);
int group_fmx_get_cluster_pileup(muxgl_handle* h, double* gls, int32_t* counts);
int group_fmx_singlets(muxgl_handle* h, double* sng);
int group_fmx_inclusion(muxgl_handle* h, const muxgl_fmx_params* p, double* incl, double* tot, double* dbl, int32_t* partner);
int group_fmx_unknown(muxgl_handle* h, const double* gp0, double* ll_ju, double* ll_u, double* ll_uu, float* kernel_ms);
int group_fmx_ambient(muxgl_handle* h, const double* amb_af, int32_t n_rho, const double* rho, double* ll_amb, float* kernel_ms);
int group_fmx_ambient_fit(muxgl_handle* h, const double* amb_af, int32_t n_cand, const int32_t* cand, double rho_max,
                          double* rho_hat, double* ll_hat, double* ll_zero, double* info, int32_t* status, int32_t* n_steps,
                          float* kernel_ms);
int group_fmx_alpha_fit(muxgl_handle* h, int32_t n_cand, const int32_t* pair, double alpha_max, double* alpha_hat,
                        double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status, int32_t* n_steps,
                        float* kernel_ms);
void group_fmx_exact_stats(const muxgl_handle* h, int64_t* cells, int64_t* changed, int64_t* unresolved);
void group_peer_stats(const muxgl_handle* h, int32_t* out);
int group_get_timing(const muxgl_handle* h, float* ms);
#define MUXGL_NOT_FOR_GROUPS(h, who) \
  if ((h)->group) MUXGL_FAIL(h, who ": not available on a device group (use a one-device handle)")
