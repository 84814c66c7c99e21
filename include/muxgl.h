/*
 * muxgl.h -- C-ABI of libmuxgl, the MI355X (gfx950) genotype-likelihood engine behind popscle's
 *            demuxlet / freemuxlet hot path.
 *
 * popscle has no plugin/FFI surface: the hot loops are inline in cmdCramDemuxlet / cmdCramFreemux2.  The drop-in
 * boundary is therefore the data hand-over between `scl.load_from_plp(...)` returning
 * (cmd_cram_demuxlet.cpp:122, cmd_cram_freemux2.cpp:87) and the `hprintf` row writers
 * (cmd_cram_demuxlet.cpp:993-1013, cmd_cram_freemux2.cpp:608-665).  Each entry point below names the reference
 * lines it replaces.  INTEGRATION.md shows the glue a popscle maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C, no exceptions across the ABI; every call returns 0 on success, nonzero on failure, and
 *     muxgl_last_error(h) (or muxgl_last_error(NULL) after a failed muxgl_create) describes the failure.  This
 *     replaces the reference's error() -> throw pexception -> abort (Error.cpp:29-43).
 *   - the library needs a HIP device; there is NO CPU fallback.  muxgl_create fails if no gfx950 device is usable.
 *   - all pointer arguments are HOST pointers borrowed for the duration of the call unless the name ends in _dev.
 *   - every call is synchronous: results are complete when it returns (the EM phases of a handle created with
 *     MUXGL_FLAG_ASYNC_PHASES excepted).  The reference is single-threaded and so is each handle: use one handle per
 *     thread / process, on one device or on a device group (muxgl_config).
 *
 * Packed pileup (what sc_dropseq_lib_t holds after load_from_plp, sc_drop_seq.h:130-184, flattened):
 *   cell_ptr   int64[C+1]   entries of cell c = [cell_ptr[c], cell_ptr[c+1])   <- cell_umis[c] (std::map order =
 *                           ascending SNP id, sc_drop_seq.h:165)
 *   entry_snp  int32[nnz]   SNP id of the entry                                <- cell_umis[c] keys
 *   entry_rptr int64[nnz+1] reads of entry e = [entry_rptr[e], entry_rptr[e+1]) <- sc_snp_droplet_t iteration order
 *   reads      uint8[R]     bit7 allele (0 ref, 1 alt), bits0-6 capped BQ; MUXGL_READ_OTHER = allele "2"
 *                           <- (allele<<24 | bq<<16 | count) words of sc_drop_seq.h:23-27
 */
#ifndef MUXGL_H
#define MUXGL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUXGL_VERSION 3
#define MUXGL_READ_OTHER 0xFF
#define MUXGL_MAX_ALPHA 16
#define MUXGL_MAX_DEVICES 16
/* demuxlet: largest V of muxgl_demux_set_gp.  The scans name a doublet by its int32 position (j V + k) n_alpha + n, so
 * V * V * n_alpha < 2^31: 11585 samples (2^31 / 16 alphas, square root); muxgl_demux_run checks the product for its grid */
#define MUXGL_MAX_SAMPLES 11585
/* freemuxlet: largest K of muxgl_fmx_greedy_init and muxgl_fmx_set_clusters.  The serial greedy start
 * (fmx_greedy_kernel, one workgroup of 1024 threads) holds one stripe of Kp clusters, K rounded up to a power of two, in
 * its threads: Kp <= 1024.  Beyond 255 clusters the EM takes the streamed E-step (see muxgl_fmx_iterate). */
#define MUXGL_MAX_CLUSTERS 1024

enum { MUXGL_SNG = 0, MUXGL_DBL = 1, MUXGL_AMB = 2 };

/* muxgl_config.flags */
#define MUXGL_FLAG_FORCE_TILE_SWEEP 1 /* never take the V<=16 row/oct kernels (lets tests cover the general tile sweep) */
#define MUXGL_FLAG_FORCE_ROW_KERNEL 2  /* never take the default-grid oct kernels (V, K <= 16: lets tests cover the row
                                          kernels behind them) */
#define MUXGL_FLAG_FORCE_WAVE_KERNEL 4 /* demuxlet: take the wave kernels for V <= 16 too, and the ring of 32 instead of the
                                          two-per-lane row kernel at 17..32 samples; freemuxlet: never take the
                                          two-per-lane row kernel at 17..32 clusters (test coverage) */
#define MUXGL_FLAG_FORCE_BATCHED_GREEDY 8 /* (no effect since the batched greedy-init kernels became the default for K <= 64;
                                             MUXGL_FLAG_FORCE_TILE_SWEEP selects the serial kernel) */
#define MUXGL_FLAG_DEMUX_ONLY 16   /* device group: the caller will only run demuxlet, so muxgl_set_pileup need not cut
                                      the SNP-major column slabs freemuxlet's ordered M-step works on */
#define MUXGL_FLAG_ASYNC_PHASES 32 /* muxgl_fmx_iter_gp / _estep / _mstep return once their kernels are enqueued on the
                                      handle's stream (muxgl_stream); muxgl_fmx_iter_fetch and every other call still
                                      return with the stream drained.  For callers that order their own collectives
                                      against that stream (popscle_amd/freemuxlet.py) */
#define MUXGL_FLAG_NO_LINEAR_ENTRIES 64 /* sweep every entry through the general three-term form, also those whose
                                          likelihoods are linear in the genotypes (one usable read) and would take the
                                          one-moment form of the oct (V, K <= 16) and wave (V, K > 32) kernels
                                          (lets tests compare the two) */
#define MUXGL_FLAG_NO_PIVOT_SUMS 256 /* freemuxlet E-step beyond 32 clusters: the pair sums of the non-linear entries as the
                                        three-term sums instead of around the lane's smallest term (lets tests compare the
                                        two forms) */
#define MUXGL_FLAG_GROUP_PROBE_SELF 1024 /* device group: muxgl_create also walks the pairs of members that share a device when
                                           it enables peer access (tests: the refusal path on a one-GPU box) */
/* (128 was MUXGL_FLAG_MSTEP_LDS_STATES until round 6: the M-step variant with the cluster states in LDS is retired) */
#define MUXGL_FLAG_FORCE_STREAMED_CALL 2048 /* demuxlet beyond 32 samples: take the streamed call (demux_stream.hip), which
                                            jobs with more than 255 samples take anyway (lets tests compare it with the
                                            other paths) */
#define MUXGL_FLAG_FORCE_STREAMED_ESTEP 4096 /* freemuxlet beyond 32 clusters: take the streamed E-step (fmx_stream.hip),
                                             which jobs with more than 255 clusters take anyway (lets tests compare it with
                                             the other paths) */
#define MUXGL_FLAG_SPLIT_GENERAL_SWEEP 512 /* demuxlet beyond 32 samples: sweep the entries with more than one usable read in
                                             launches of their own on top of the linear entries' slab (round 3's scheme)
                                             instead of in the same launch with the same accumulators (lets tests
                                             compare the two) */

typedef struct muxgl_handle muxgl_handle;

/* One handle drives one device (n_devices <= 1) or a device group (n_devices > 1): the same entry points, with the
 * cells of the pileup cut into n_devices contiguous ranges (demuxlet: no exchange; freemuxlet: E-step by cells, ordered
 * M-step by SNPs, two all-gathers per EM iteration as peer-to-peer copies over xGMI).  The reference's own way to use
 * several workers is the same cut at file level (--group-list, README.md:168; sc_drop_seq.cpp:93-101,164-170).  A
 * device may be named more than once (virtual ranks on one GPU: tests). */
typedef struct {
  int32_t struct_size; /* sizeof(muxgl_config) of the header the caller was built against (MUXGL_CONFIG_INIT sets it):
                          muxgl_create rejects any other value instead of reading past a shorter struct */
  int32_t device_id; /* HIP device ordinal this handle runs on (n_devices == 0) */
  int32_t flags;     /* MUXGL_FLAG_* bits, normally 0 */
  int32_t n_devices; /* 0: device_id; >= 1: device_ids[0 .. n_devices) */
  int32_t device_ids[MUXGL_MAX_DEVICES];
} muxgl_config;
#define MUXGL_CONFIG_INIT {(int32_t)sizeof(muxgl_config), 0, 0, 0, {0}}

/* demuxlet parameters: --alpha grid and --doublet-prior (cmd_cram_demuxlet.cpp:32,62-63,85-89) */
typedef struct {
  int32_t n_alpha;
  int32_t _pad;
  double alpha[MUXGL_MAX_ALPHA];
  double doublet_prior;
} muxgl_demux_params;

#define MUXGL_CELL_DEEP_SNG 2
#define MUXGL_CELL_DEEP_DBL 4

/* per-cell demuxlet result: every quantity cmd_cram_demuxlet.cpp:788-991 derives and :993-1013 prints.
 * Sample indices are positions in the GP tensor's V axis; -1 = none.  valid=0: the cell has no entries and the
 * reference prints no row (:653). */
typedef struct {
  int32_t valid; /* bit 0: the cell has entries (0: the reference prints no row, :653).  muxgl_demux_run also sets
                    MUXGL_CELL_DEEP_SNG / MUXGL_CELL_DEEP_DBL where the THIRD-largest log-likelihood of the singlet /
                    doublet scan is within rounding reach of the runner-up (three or more hypotheses contend): read and
                    cleared by muxgl_demux_exact_calls, which then recomputes every hypothesis of that scan */
  int32_t nsnps;
  int32_t type, next_type;
  int32_t sBest, sNext;
  int32_t dBest1, dBest2, dBestA;
  int32_t dNext1, dNext2, dNextA;
  int32_t jBest, kBest, aBest;
  int32_t jNext, kNext, aNext;
  double sngBestLLK, sngNextLLK, dblBestLLK, dblNextLLK;
  double sumLLK, sngLLK;
  double bestLLK, nextLLK;
  double bestPP, sngPP, sngOnlyPP;
} muxgl_demux_cell;

/* freemuxlet parameters: --doublet-prior, --geno-error (cmd_cram_freemux2.cpp:19-20) */
typedef struct {
  double doublet_prior;
  double geno_error;
} muxgl_fmx_params;

/* per-cell freemuxlet state/result (cmd_cram_freemux2.cpp:345-367, printed at :660-665) */
typedef struct {
  int32_t type;  /* 0 SNG, 1 DBL, 2 AMB, -1 never classified */
  int32_t clust; /* clusts[i]: jBest for SNG after an iteration, else -1 */
  int32_t jBest, kBest, jNext, kNext;
  int32_t sBest, sNext, dBest1, dBest2, dNext1, dNext2;
  double bestLLK, nextLLK;
  double sngBestLLK, sngNextLLK, dblBestLLK, dblNextLLK;
  double bestPP, sngPP, sngOnlyPP, sumLLK;
  double sngThirdLLK, dblThirdLLK; /* third-largest log-likelihood of each scan (-1e300: none), see muxgl_demux_cell */
} muxgl_fmx_cell;

/* kernel timings of the most recent *_run / *_iterate call, milliseconds, measured with hipEvents recorded on the
 * stream the kernels were launched on */
enum {
  MUXGL_T_DEMUX_REDUCE = 0, /* row and default-grid paths: chunk partials folded per cell (default grid: and the call).
                               Where the default-grid path runs its cells as two groups on two streams (below,
                               muxgl_demux_oct_split) the first group's share runs underneath the second group's sweep:
                               the slot is then what remained of the step's device time behind the end of the last
                               sweep, i.e. the exposed part (to the end of the later of the two finishes, which run
                               on a stream each and are joined by the host before muxgl_demux_run returns) */
  MUXGL_T_DEMUX_SWEEP = 1,  /* per-entry likelihoods (a4,a5) fused with the sample-pair x alpha sweep (a6); with two cell
                               groups: from the start of the step to the end of the later of the two sweeps (the later
                               of two elapsed times, taken on the host).  SWEEP and REDUCE never overlap */
  MUXGL_T_DEMUX_CALL = 2,  /* evidence sums, best/next scans, call (a7-a9) */
  MUXGL_T_DEMUX_D2H = 3,   /* per-cell records to host */
  MUXGL_T_FMX_ENTRY = 4,   /* entry 9-GL pileup + cell scores (b1,b2) */
  MUXGL_T_FMX_GP = 5,      /* cluster genotype posterior tensor */
  MUXGL_T_FMX_ESTEP = 6,   /* E-step pair sweep (b6) */
  MUXGL_T_FMX_CALL = 7,    /* scans + re-assignment (b7,b8 classification) */
  MUXGL_T_FMX_MSTEP = 8,   /* ordered clamped merge (b5,b8) */
  MUXGL_T_FMXOLD_PAIR = 9, /* freemuxlet-old: pairwise droplet distance matrix (c1) */
  MUXGL_T_FMXOLD_VOTE = 10, /* freemuxlet-old: one voting pass (c1) */
  MUXGL_T_FMX_ESTEP_SWEEP = 11, /* the pair-sweep kernel(s) alone, inside MUXGL_T_FMX_ESTEP (which also brackets the
                                   relayout of the cluster posteriors and the reduction of the chunk partials) */
  MUXGL_T_DEMUX_SINGLETS = 12,  /* muxgl_demux_singlets: entry weights + sample sweep (with a table cut into several
                                   batches also the copies between them) */
  MUXGL_T_FMX_SINGLETS = 13,    /* muxgl_fmx_singlets: (packing of the entry diagonals +) cluster sweep (with a table cut
                                   into several batches also the copies between them) */
  MUXGL_T_DEMUX_INCLUSION = 14, /* muxgl_demux_inclusion: entry likelihoods + pair sweep + marginal fold + finish (with a
                                   state cut into several batches of cells also the copies between them) */
  MUXGL_T_FMX_INCLUSION = 15,   /* muxgl_fmx_inclusion: pair sweep + marginal fold + finish (with a state cut into
                                   several batches of cells also the copies between them) */
  MUXGL_T_COUNT = 16
};

/* ---- lifetime ------------------------------------------------------------------------------------------------ */
int muxgl_create(const muxgl_config* cfg, muxgl_handle** out);
void muxgl_destroy(muxgl_handle* h);
const char* muxgl_last_error(const muxgl_handle* h);
int muxgl_version(void);

/* device group: what muxgl_create found when it enabled direct peer copies between its members' devices: out[3] = ordered
 * pairs of members on distinct devices (with MUXGL_FLAG_GROUP_PROBE_SELF: all ordered pairs), pairs with peer access
 * enabled, pairs left on the runtime's staged copy (no peer access between the two devices, or MUXGL_GROUP_NO_PEER=1 in
 * the environment).  Either way the copies are hipMemcpyPeerAsync and the results the same. */
int muxgl_group_peer_stats(const muxgl_handle* h, int32_t* out);

/* ---- pileup hand-over: replaces the in-memory result of sc_dropseq_lib_t::load_from_plp
 *      (sc_drop_seq.cpp:103-384; containers sc_drop_seq.h:130-184).  Copies to device memory.
 *      A new pileup drops everything that was made for the previous one: the GP tensor of muxgl_demux_set_gp (every
 *      demuxlet call and muxgl_fmx_match_donors fail with "no GP tensor set" until it is handed over again for the new
 *      SNP set), the grid of the last muxgl_demux_run, and the freemuxlet state from muxgl_fmx_prepare on. ---------- */
int muxgl_set_pileup(muxgl_handle* h, int64_t C, int64_t S, int64_t nnz, int64_t R, const int64_t* cell_ptr,
                     const int32_t* entry_snp, const int64_t* entry_rptr, const uint8_t* reads);

/* ---- demuxlet ------------------------------------------------------------------------------------------------ */
/* genotype-probability tensor gp[S][V][3] (sc_snp_t::gps, sc_drop_seq.h:29-37, built at sc_drop_seq.cpp:287-315) and
 * has_gp[S] (0 <=> gps == NULL, sc_drop_seq.cpp:258-282).  1 <= V <= MUXGL_MAX_SAMPLES (and V * V * n_alpha < 2^31 for
 * the grid of muxgl_demux_run).  Beyond 255 samples muxgl_demux_run takes the streamed call, which does not produce
 * full_ll. */
int muxgl_demux_set_gp(muxgl_handle* h, int32_t V, const double* gp, const uint8_t* has_gp);

/* replaces the per-cell loop cmd_cram_demuxlet.cpp:636-991.  out: NULL or [C].  full_ll: NULL or [C][V][V][n_alpha]
 * receiving llksAB for the entries the reference ever reads: (j,0,0) and (j,k!=j,n>=1); other slots are 0.
 * The streamed call (V > 255, MUXGL_FLAG_FORCE_STREAMED_CALL at V > 32, or a job whose [C][V][V][n_alpha] tensor does not
 * fit the device) folds the hypotheses into the scans as it goes and never holds the tensor: there full_ll must be NULL
 * (the call fails, naming the reason, otherwise).  Its device memory beyond the pileup and the per-entry likelihoods is a
 * slab budget, 4 GiB or a third of the device's memory if less; MUXGL_DEMUX_SLAB_MB=<n> in the environment sets it. */
int muxgl_demux_run(muxgl_handle* h, const muxgl_demux_params* p, muxgl_demux_cell* out, double* full_ll);

/* sng[C][V] = llksAB[(j,0,0)] of cmd_cram_demuxlet.cpp:733-747 for every droplet and sample.  Needs muxgl_set_pileup
 * and muxgl_demux_set_gp, not a previous muxgl_demux_run; any V up to MUXGL_MAX_SAMPLES; one device or a device group.
 * This is the table the reference's disabled .single / .sing2 writers print (:580, :839-848): what full_ll[c][j][0][0]
 * holds on the paths that have it.  The slot is (j, k = 0, n = 0) whatever alpha[0] is, and the per-entry likelihoods are
 * normalised over the whole grid (:686-725), so the call takes the same parameters as muxgl_demux_run (doublet_prior is
 * not read).  A droplet without entries gets a row of zeros.  The device holds three weights per entry and a slab of the
 * table (the streamed call's budget: 4 GiB or a third of the device, MUXGL_DEMUX_SLAB_MB); a larger table is swept in
 * batches of cells, each copied out before the next.  The table is bit-identical from run to run, for any budget, on one
 * device and on a group.  The records, timings and state of muxgl_demux_run stay as they are (the call's own kernel time
 * is MUXGL_T_DEMUX_SINGLETS of muxgl_get_timing; it counts as a collecting call of muxgl_get_timing_sum). */
int muxgl_demux_singlets(muxgl_handle* h, const muxgl_demux_params* p, double* sng);

/* Per droplet c and sample s: how much evidence there is that s is in the droplet at all, and with whom s pairs best --
 * the row and column marginals of the pair matrix the reference's disabled .pair writer prints (cmd_cram_demuxlet.cpp:
 * 852-877).  Over the hypotheses that carry prior mass in :804-821,
 *   H   = { (j,k,n) : j != k, n >= 1, and k < j where alpha[n] == 0.5 },   value LL(j,k,n) = llksAB[(j,k,n)]
 *   H_s = { h in H : j == s or k == s }
 * incl[C][V]  = log( exp(LL(s,0,0) + lsp) + sum_{h in H_s} exp(LL(h) + prior(h)) ), lsp = log_single_prior and prior =
 *               log_doublet_prior1 (alpha != 0.5) / log_doublet_prior2 (alpha == 0.5) exactly as :793-795
 * tot[C]      = log of the same sum over all singlets and all of H, WITHOUT the reference's -1e-300 seed (:791), so
 *               exp(incl - tot) is the posterior that s is in the droplet (sumLLK of the record = logAdd(-1e-300, tot))
 * dbl[C][V]   = max_{h in H_s} LL(h)   (-1e300 when H_s is empty: V == 1 or a grid without a doublet alpha)
 * partner, alpha_idx, first [C][V]: the other sample of that hypothesis, its n, and 1 if s is j / 0 if s is k
 *               (-1, -1, -1 when H_s is empty).  Ties: value descending, then scan position (j V + k) A + n ascending.
 * Any out pointer may be NULL.  A droplet without entries gets LL = 0 for every hypothesis, like the singlet table.
 * Needs muxgl_set_pileup and muxgl_demux_set_gp, not a previous muxgl_demux_run; every grid muxgl_demux_run accepts
 * (also one without a doublet alpha); 1 <= V <= MUXGL_MAX_SAMPLES with V * V * n_alpha < 2^31; one device or a device
 * group (every member fills the rows of its own cells).  The tables are the device's arithmetic throughout (products of
 * factors, one log per hypothesis: equal to the reference's sums of logs to ~1e-11); near ties in `partner` are decided
 * by those values and the order above, not re-resolved in exact arithmetic.
 * The device holds the per-entry likelihoods ([nnz][n_alpha][9]) and, within the streamed call's budget (4 GiB or a third
 * of the device, MUXGL_DEMUX_SLAB_MB), a slab of the pair sweep plus the state and the outputs of a batch of whole cells
 * (60 bytes per cell and sample); the batch is finished and copied out before the next; nothing proportional to C x V^2.
 * It fails when one cell's state and one 64 x 64 block of the sweep exceed the budget.  All six outputs are bit-identical
 * from call to call, for any budget, on one device, on a group and through the sharded driver.  The records, full_ll,
 * timings and state of muxgl_demux_run stay as they are (the call's own kernel time is MUXGL_T_DEMUX_INCLUSION of
 * muxgl_get_timing; it counts as a collecting call of muxgl_get_timing_sum). */
int muxgl_demux_inclusion(muxgl_handle* h, const muxgl_demux_params* p, double* incl, double* tot, double* dbl,
                          int32_t* partner, int32_t* alpha_idx, int32_t* first);

/* Every droplet against a donor that is NOT in the panel: the half-unspecified and unspecified doublet likelihoods the
 * reference accumulates and never prints (llksA0 / llks00, cmd_cram_demuxlet.cpp:749-773; the commented-out header of
 * :628 still lists their columns).  With pG_e[n][l][m] the per-entry likelihood of :655-725, normalised over the whole
 * grid (so the call takes the parameters of muxgl_demux_run; doublet_prior is not read), u[s][.] the unknown donor's
 * genotype prior at marker s, and the sums over the entries e of droplet c whose marker s_e has genotypes:
 *   ll_ju[C][V][n_alpha]: ll_ju[c][j][n] = sum_e log sum_l sum_m gp[s_e][j][l] * u[s_e][m] * pG_e[n][l][m]
 *                         (llksA0: sample j with share 1 - alpha[n], the unknown donor with share alpha[n])
 *   ll_uj[C][V][n_alpha]: ll_uj[c][k][n] = sum_e log sum_l sum_m u[s_e][l] * gp[s_e][k][m] * pG_e[n][l][m]
 *                         (the other orientation, which the reference does not form: the same hypothesis as ll_ju only
 *                         where alpha[n] == 0.5)
 *   ll_uu[C][n_alpha]:    ll_uu[c][n]    = sum_e log sum_l sum_m u[s_e][l] * u[s_e][m] * pG_e[n][l][m]      (llks00)
 * gp0 == NULL: u is the reference's panel mean (:428-440), the rows gp[s][0..V-1] added in sample order, then divided by
 * V, computed on the device.  gp0 != NULL: the caller's prior [S][3] (Hardy-Weinberg from an allele frequency, say);
 * the values in rows of markers without genotypes do not matter.  A marker without genotypes contributes a factor of
 * exactly 1 everywhere (:733), a droplet without entries gets zeros, and slot n = 0 is kept like every other slot (the
 * singlet slot of :799,806).  Needs muxgl_set_pileup and muxgl_demux_set_gp, not a previous muxgl_demux_run; any V up
 * to MUXGL_MAX_SAMPLES (there is no pair grid: V * V * n_alpha may exceed 2^31) and any n_alpha up to MUXGL_MAX_ALPHA; one
 * device or a device group (every member fills the rows of its own cells).  Any subset of the three tables may be NULL;
 * with all three NULL the call fails, naming the reason, and the handle stays usable.  kernel_ms (NULL allowed) receives
 * the hipEvent time of the call's kernels, from a pair of events the call makes for itself (a group: the slowest
 * member's): the records, full_ll, timing slots and state of muxgl_demux_run stay as they are.
 * Device memory: nothing proportional to nnz x n_alpha is held for the whole pileup.  The cells are swept in batches of
 * whole cells whose 6 n_alpha weights per entry, slab rows and table rows fit the streamed call's budget (4 GiB or a
 * third of the device, MUXGL_DEMUX_SLAB_MB); each batch is copied out before the next; the call fails, naming the
 * reason, when one cell alone exceeds the budget.  All three tables are bit-identical from call to call, for any budget,
 * for any subset of requested tables, on one device, on a group and through the sharded driver. */
int muxgl_demux_unknown(muxgl_handle* h, const muxgl_demux_params* p, const double* gp0 /* NULL, or [S][3] */,
                        double* ll_ju /* NULL or [C][V][n_alpha] */, double* ll_uj /* NULL or [C][V][n_alpha] */,
                        double* ll_uu /* NULL or [C][n_alpha] */, float* kernel_ms /* NULL or one float */);

/* The usable reads (every read byte but MUXGL_READ_OTHER) of the pileup by marker and allele, over the droplets whose
 * byte of cell_mask is not 0 (cell_mask == NULL: over all of them): n_ref[s] / n_alt[s] = reads of marker s with bit 7
 * clear / set.  A device kernel over the entries with integer adds: exact, and the same whatever the order.  Needs only
 * muxgl_set_pileup; one device or a device group (every member counts its own droplets, the counts are added on the
 * host).  It reads the pileup and changes no state.  What it is for: the ALT fraction of the pool's free-floating RNA,
 * amb_af of muxgl_demux_ambient, from all droplets or from the nearly empty ones. */
int muxgl_pileup_allele_counts(muxgl_handle* h, const uint8_t* cell_mask /* NULL = all, or [C] */,
                               int64_t* n_ref /* [S] */, int64_t* n_alt /* [S] */);

/* Every droplet as ONE cell of sample j plus a share rho of ambient RNA: the hypothesis the reference lacks (its only
 * reading of a singlet from a high-soup prep is "j plus one other donor", a doublet with a partner picked nearly at
 * random).  The ambient RNA is no donor: its ALT fraction at marker s is the pool's, amb_af[s], any number in [0, 1],
 * where a second donor's genotype m of cmd_cram_demuxlet.cpp:655-725 stands, as 2 * amb_af[s]:
 *   p(l, f, rho)    = 0.5 * l + (2 * f - l) * 0.5 * rho
 *   a_e[r][l]       = product over the usable reads of entry e of (pR * (1 - p) + pA * p),  p = p(l, amb_af[s_e], rho[r])
 *   w_e[r][l]       = (a_e[r][l] / q_max_e + 1e-10) / (1 + 1e-10)
 *   ll_amb[c][j][r] = sum over the entries e of droplet c whose marker has genotypes of
 *                     log( sum_l gp[s_e][j][l] * w_e[r][l] )
 * q_max_e is the entry's scale under the alpha grid of p: the number that scales pG_e in muxgl_demux_run,
 * muxgl_demux_singlets and muxgl_demux_unknown with that grid (doublet_prior is not read).  The ambient products take
 * part in no maximum, they are only divided by the grid's; a / q_max may exceed 1 by a modest factor where the best p
 * of an entry is not on the grid.  ll_amb is therefore on the scale of the log-likelihoods of the records and of the
 * singlet table, and may be subtracted from dblBestLLK or from a row of muxgl_demux_singlets.  Three identities:
 *   amb_af in {0, 0.5, 1} and rho[r] == alpha[n]: w_e[r][l] = pG_e[n][l][2 f], and ll_amb[c][j][r] is the reference's
 *     llksAB[(j, V, n)] on the panel with one donor appended whose row at marker s is one-hot at genotype 2 * amb_af[s];
 *   rho[r] == 0: the column is the table of muxgl_demux_singlets with the same grid;
 *   rho[r] == 1: p is amb_af, the column is the same for every sample ("nothing but soup").
 * The rho reported for a droplet by a caller is the maximum over the grid rho[]; muxgl_demux_ambient_fit (below) gives
 * the continuous estimate with its observed information.
 * A marker without genotypes contributes a factor of exactly 1 (:733), a droplet without entries gets zeros.  Needs
 * muxgl_set_pileup and muxgl_demux_set_gp, not a previous muxgl_demux_run; any V up to MUXGL_MAX_SAMPLES; 1 <= n_rho <=
 * MUXGL_MAX_ALPHA; every rho and every amb_af[s] of a marker with genotypes finite and in [0, 1] (the values of markers
 * without genotypes do not matter); one device or a device group (every member fills the rows of its own cells).  It
 * fails, naming the reason and leaving the handle usable, without a pileup or a GP tensor, with ll_amb == NULL, with
 * n_rho or n_alpha out of range, with a rho or an amb_af out of range or not finite, and when one cell alone exceeds
 * the budget.  kernel_ms (NULL allowed) receives the hipEvent time of the call's kernels, from a pair of events the call
 * makes for itself (a group: the slowest member's): the records, full_ll, plans, timing slots and cached grid of
 * muxgl_demux_run and every freemuxlet state stay as they are.
 * Device memory: nothing proportional to nnz x n_rho is held for the whole pileup.  The cells are swept in batches of
 * whole cells whose 3 n_rho weights per entry, slab rows and table rows fit the streamed call's budget (4 GiB or a third
 * of the device, MUXGL_DEMUX_SLAB_MB); each batch is copied out before the next.  The table is bit-identical from call
 * to call, for any budget, for any split of rho[] over several calls, on one device, on a group and through the
 * sharded driver. */
int muxgl_demux_ambient(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af /* [S] */, int32_t n_rho,
                        const double* rho /* [n_rho] */, double* ll_amb /* [C][V][n_rho] */,
                        float* kernel_ms /* NULL or one float */);

/* The ambient share of muxgl_demux_ambient as a per-droplet maximum-likelihood estimate, for n_cand candidate samples per
 * droplet (cand[c][k] = a sample, or -1 to skip the slot).  With w_e[l](rho) exactly as above (the reference's per-read
 * term of cmd_cram_demuxlet.cpp:655-725 with p = 0.5 * l + (2 * f - l) * 0.5 * rho of :673, divided by q_max_e of the alpha
 * grid of p, + 1e-10, / (1 + 1e-10)):
 *   LL(rho) = sum over the entries e of droplet c whose marker has genotypes of log( sum_l gp[s_e][j][l] * w_e[l](rho) )
 * Every read's factor is linear in rho, so an entry's product is a polynomial in rho and LL', LL'' are analytic: the
 * product rule along the reads, no division, no finite difference.  Per (c, k), each array [C][n_cand]:
 *   rho_hat  the maximiser of LL on [0, rho_max]: LL is taken at the nine points i * rho_max / 8, the best of them (ties
 *            to the lowest index) with its two neighbours, clipped to [0, rho_max], is the bracket, and rho_hat is the
 *            maximiser of LL inside the bracket, found by a safeguarded Newton iteration on LL' (the Newton step where
 *            LL'' < 0 and the step stays strictly inside the bracket, bisection otherwise; the bracket shrinks by the sign
 *            of LL' at every step; it stops after a Newton step <= 1e-9, or when the bracket or a bisection step is <= 1e-9 -- after
 *            one last Newton step from there where one is possible -- or after 48 steps);
 *   ll_hat   LL(rho_hat);   ll_zero  LL(0), the candidate's entry of muxgl_demux_singlets;   info  -LL''(rho_hat);
 *   status   0 interior and converged; 1 at the lower bound (rho_hat == 0.0 exactly and LL'(0) <= 0); 2 at the upper
 *            bound (rho_hat == rho_max exactly and LL'(rho_max) >= 0); 3 step cap reached (the values are those of the
 *            best point evaluated, by LL); 4 slot skipped (cand < 0: all outputs 0); 5 droplet without a scored entry (all outputs 0);
 *   n_steps  the evaluations of (LL, LL', LL'') after the one at the best coarse point (0 at a bound).
 * The caller's standard error of rho_hat is info^(-1/2) where status is 0 and info > 0; at status 1 or 2 the estimate
 * sits on a bound and has NO standard error (info is still -LL'' there, for what it is worth).  The likelihood ratio
 * against rho = 0 is 2 * (ll_hat - ll_zero).
 * Needs muxgl_set_pileup and muxgl_demux_set_gp, not a previous muxgl_demux_run; any V up to MUXGL_MAX_SAMPLES; 1 <= n_cand
 * <= MUXGL_MAX_FIT_CAND; 0 < rho_max <= 1, finite; every cand in [-1, V); amb_af as for muxgl_demux_ambient; any of the six outputs may
 * be NULL, not all; one device or a device group (every member fits its own cells).  It fails, naming the reason and
 * leaving the handle usable, without a pileup or a GP tensor, with every output NULL, with cand == NULL, and with n_cand,
 * n_alpha, rho_max, a candidate or an amb_af out of range or not finite.  kernel_ms (NULL allowed) receives the hipEvent
 * time of the call's one kernel, from a pair of events the call makes for itself (a group: the slowest member's).  The
 * call reads state and changes none: records, full_ll, plans, timing slots and the cached grid stay as they are.
 * Device memory: the inputs, cand and the outputs.  Nothing proportional to nnz is allocated, so no slab budget applies
 * and MUXGL_DEMUX_SLAB_MB is not read.  The whole fit of a (droplet, candidate) runs in one wave of one launch with every
 * reduction tree fixed by the droplet alone: the outputs are bit-identical from call to call, for any order, grouping or
 * repetition of candidates, for any subset of outputs, on one device, on a group and through the sharded driver. */
#define MUXGL_MAX_FIT_CAND 16 /* candidates per droplet of muxgl_demux_ambient_fit */
int muxgl_demux_ambient_fit(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af /* [S] */,
                            int32_t n_cand, const int32_t* cand /* [C][n_cand], sample or -1 */, double rho_max,
                            double* rho_hat, double* ll_hat, double* ll_zero, double* info,   /* each [C][n_cand] or NULL */
                            int32_t* status, int32_t* n_steps,                                /* [C][n_cand] or NULL */
                            float* kernel_ms);

/* The mixing share of a doublet as a per-droplet maximum-likelihood estimate, for n_cand pairs of samples per droplet
 * (pair[c][slot] = (j, k), or (-1, -1) to skip the slot).  muxgl_demux_run scores a pair only at the alphas of its grid,
 * one V x V sweep per point; this call fits alpha for the pairs a caller names.  With j the first sample and alpha the
 * share of k, the reference's own doublet term (cmd_cram_demuxlet.cpp:655-746):
 *   p(l, m, alpha) = 0.5 * l + (m - l) * 0.5 * alpha                                                        (:673)
 *   a_e[l][m]      = product over the usable reads of entry e of (pR * (1 - p) + pA * p)
 *   w_e[l][m]      = (a_e[l][m] / q_max_e + 1e-10) / (1 + 1e-10), q_max_e the entry's scale under the alpha grid of p
 *   LL(alpha)      = sum over the entries e of droplet c whose marker has genotypes of
 *                    log( sum_l sum_m (gp[s_e][j][l] * gp[s_e][k][m]) * w_e[l][m] )                         (:738-746)
 * Every read's factor is linear in alpha (dt/dalpha = (pA - pR) (m - l) 0.5, exactly 0 on the diagonal l == m), so an
 * entry's product is a polynomial in alpha and LL', LL'' are analytic: the product rule along the reads, no division, no
 * finite difference.  At every alpha[n] of the grid LL is the reference's llksAB[j][k][n]; alpha = 0 is sample j alone and
 * alpha = 1 sample k alone, so both singlets nest in the model.  Per (c, slot), each array [C][n_cand]:
 *   alpha_hat, ll_hat, info, status, n_steps   by the rules of muxgl_demux_ambient_fit above, with alpha in the place of
 *            rho: the nine points i * alpha_max / 8, the best of them (ties to the lowest index) with its two neighbours
 *            as the bracket, safeguarded Newton on LL', the same stops, 48 steps; status 0 interior, 1 at the lower bound
 *            (alpha_hat == 0.0 exactly), 2 at the upper (alpha_hat == alpha_max exactly), 3 step cap, 4 slot skipped (an
 *            index < 0: all outputs 0), 5 droplet without a scored entry (all outputs 0);
 *   ll_zero  LL(0): sample j alone, the reference's llksAB[j][k][n] for alpha[n] == 0, within rounding of j's entry of
 *            muxgl_demux_singlets;
 *   ll_top   LL(alpha_max), coarse point 8: with alpha_max == 1 sample k alone, with alpha_max == alpha[n] the reference's
 *            llksAB[j][k][n].  At status 2 ll_hat == ll_top bit for bit, at status 1 ll_hat == ll_zero.
 * The caller's standard error of alpha_hat is info^(-1/2) where status is 0 and info > 0; on a bound there is
 * NO standard error.  With alpha_max == 1 the likelihood ratio against "one cell" is 2 * (ll_hat - max(ll_zero, ll_top)).
 * Needs muxgl_set_pileup and muxgl_demux_set_gp, not a previous muxgl_demux_run; any V up to MUXGL_MAX_SAMPLES (no full_ll
 * tensor, no 255-sample limit); 1 <= n_cand <= MUXGL_MAX_FIT_CAND; 0 < alpha_max <= 1, finite; every index in [-1, V);
 * j == k is allowed (the reference's slot (j, j, n)); any of the seven outputs may be NULL, not all; one device or a
 * device group (every member fits its own cells).  It fails, naming the reason and leaving the handle usable, without a
 * pileup or a GP tensor, with every output NULL, with pair == NULL, with n_cand, n_alpha, alpha_max or an index out of
 * range, and with a slot of exactly one negative index.  kernel_ms (NULL allowed) receives the hipEvent time of the
 * call's one kernel, from a pair of events the call makes for itself (a group: the slowest member's).  The call reads
 * state and changes none: records, full_ll, plans, timing slots and the cached grid stay as they are.
 * Device memory: pair and the outputs.  Nothing proportional to nnz is allocated, so no slab budget applies and
 * MUXGL_DEMUX_SLAB_MB is not read.  The whole fit of a (droplet, slot) runs in one wave of one launch with every
 * reduction tree fixed by the droplet alone: the outputs are bit-identical from call to call, for any order, grouping or
 * repetition of slots, for any subset of outputs, on one device, on a group and through the sharded driver. */
int muxgl_demux_alpha_fit(muxgl_handle* h, const muxgl_demux_params* p,
                          int32_t n_cand, const int32_t* pair /* [C][n_cand][2]: (j, k), or (-1, -1) to skip */,
                          double alpha_max,
                          double* alpha_hat, double* ll_hat, double* ll_zero, double* ll_top, double* info, /* each [C][n_cand] or NULL */
                          int32_t* status, int32_t* n_steps,                                                /* [C][n_cand] or NULL */
                          float* kernel_ms);

/* The usable reads of the pileup as a histogram: the number of reads per (marker, read byte) over the droplets whose byte
 * of cell_mask is not 0 (cell_mask == NULL: over all of them), as records with keys[i] = marker * 256 + byte, strictly
 * ascending, and counts[i] > 0; MUXGL_READ_OTHER never appears.  Every read with the same key has the same likelihood
 * under any model of the marker, so this exact integer statistic is all muxgl_demux_soup_mix needs of the reads.
 * Size query as muxgl_fmx_exact_snps: with keys == counts == NULL only *n is written; with room for cap records the call
 * fails, naming the reason, when cap < *n.  A device pass over the entries (one key per usable read, a radix sort, a
 * run-length pass; 32 bytes of device memory per usable read of the chosen droplets): integer work only, so the records
 * are the same for any order of the droplets.  Summed per (marker, bit 7 of the byte) they are muxgl_pileup_allele_counts
 * exactly.  Needs only muxgl_set_pileup; one device or a device group (every member counts its own droplets and the
 * sorted lists are merged on the host with integer adds).  It reads the pileup and changes no state. */
int muxgl_pileup_read_hist(muxgl_handle* h, const uint8_t* cell_mask /* NULL = all, or [C] */, int64_t* keys /* NULL or [cap] */,
                           int64_t* counts /* NULL or [cap] */, int64_t cap, int64_t* n);

/* The soup as a mixture of the donors: the ALT fraction of the pool's free-floating RNA at marker s is a weighted mean of
 * the donors' genotype dosages, with shares pi that are the same at every marker -- M unknowns where the count route
 * (muxgl_pileup_allele_counts) estimates S.  The components are the V samples of the panel and, with with_unknown != 0,
 * component V: a donor missing from the VCF, whose genotype prior per marker is the panel mean as muxgl_demux_unknown
 * forms it (gp0 == NULL) or the caller's gp0[S][3].  M = V + (with_unknown ? 1 : 0).  With (g0, g1, g2) = gp[s][v][0..2]:
 *   r_v(s) = g0 + g1 / 2,   a_v(s) = g1 / 2 + g2               (rows need not sum to one)
 *   R(s) = sum_v pi_v r_v(s),   A(s) = sum_v pi_v a_v(s)
 *   D(s, b) = pR * R(s) + pA * A(s)       (pR, pA of read byte b from the Phred table as muxgl_demux_run takes them:
 *                                          a REF read has pR = Mat, pA = Err / 3, an ALT read the other way round)
 *   LL(pi) = sum over the records of n * log D
 *   grad_v = (1 / N) * sum_s [ r_v(s) * sum_b n * pR / D + a_v(s) * sum_b n * pA / D ],   one EM step: pi'_v = pi_v * grad_v
 * over the records (marker s, byte b, count n) of a read histogram (muxgl_pileup_read_hist) whose marker has genotypes
 * and R(s) + A(s) > 0 at the start; N is their total count.  keys == NULL: the histogram of the handle's own pileup under
 * cell_mask; else the caller's n_rec records (cell_mask must be NULL).  LL is concave in pi and the EM is monotone; it
 * keeps sum pi = 1 up to rounding and is not renormalised; at the maximum grad_v == 1 where pi_v > 0 and <= 1 where
 * pi_v == 0.  The start is pi0 divided by its sum (added in component order), or 1 / M everywhere (pi0 == NULL).
 * For i = 0 .. n_iter_max: LL and grad at the current pi, ll[i] = LL; stop if i == n_iter_max (status 1); else step, and
 * stop after a step with max_v |pi'_v - pi_v| <= tol (status 0): LL and grad are then taken once more at the final pi
 * and stored in ll[i + 1].  grad and amb_af always belong to the returned pi; the unused tail of ll is NaN; n_iter = the
 * steps taken.  n_iter_max == 0 only evaluates the start: the call is a scorer of a given pi as well.  Status 2: no
 * record takes part; pi is the start, ll[0] and grad are 0.  amb_af[s] = A(s) / (R(s) + A(s)) at the returned pi, 0.5 at
 * a marker without genotypes (the ambient calls do not read those) or with R + A == 0.  n_reads = N.
 * Needs muxgl_set_pileup and muxgl_demux_set_gp, not a previous muxgl_demux_run; any V up to MUXGL_MAX_SAMPLES.  Any output
 * may be NULL, not all.  It fails, naming the reason and leaving the handle usable: without a pileup or a GP tensor; with
 * keys that are not strictly ascending, out of range or carry byte 0xFF; with a count <= 0; with a pi0 that has a negative
 * or non-finite entry or sums to 0; with a gp0 entry that is negative or non-finite; with n_iter_max < 0 or tol negative
 * or not finite; with every output NULL.  kernel_ms (NULL allowed) receives the hipEvent time between the call's first
 * and last kernel (the 16-byte read-back of LL and the step after every iteration included).  The call reads state and
 * changes none: records, full_ll, plans, timing slots, the cached grid and every freemuxlet state stay as they are;
 * nothing is cached on the handle.  Device memory: the histogram, 24 bytes per active marker, one row of M doubles per
 * 256 active markers, and [S][3] with the unknown component.  Every rounded sum has a tree fixed by the histogram and M
 * alone: the outputs are bit-identical from call to call, for the handle's own pileup against the same histogram passed
 * in, for any order of the droplets, on one device, on a group (one member fits, from the merged histogram) and through
 * the sharded driver. */
int muxgl_demux_soup_mix(muxgl_handle* h, const uint8_t* cell_mask /* NULL = all, or [C] */, int64_t n_rec,
                         const int64_t* keys /* NULL, or [n_rec] */, const int64_t* counts /* [n_rec] with keys */,
                         int32_t with_unknown, const double* gp0 /* NULL or [S][3] */, const double* pi0 /* NULL or [M] */,
                         int32_t n_iter_max, double tol,
                         double* pi /* [M] */, double* grad /* [M] */, double* ll /* [n_iter_max + 1] */,
                         double* amb_af /* [S] */, int32_t* n_iter, int64_t* n_reads, int32_t* status,
                         float* kernel_ms /* NULL or one float */);

/* The calls rounding noise could decide, settled in the reference's own arithmetic -- HOST pass, no device work, no
 * handle (popscle_amd/host/exact_calls.hpp).  The kernels' log-likelihoods equal the reference's to ~1e-12, not to the last
 * bit, and every decision of cmd_cram_demuxlet.cpp:827-837,883-906,925-988 compares two of them.  For the cells of
 * cells[C] (records of muxgl_demux_run) where a comparison's margin is within 1e-9 x max(1, |LL|) this call recomputes the
 * contested hypotheses on the host as the reference does (IEEE doubles in its operation order, glibc log) and rewrites the
 * record from those numbers:
 *   - the best (or next) doublet is an alpha = 0.5 pair: the reference evaluates (j,k) and (k,j) with transposed
 *     summation orders (:738-746) and reports whichever came out larger as DBL.BEST.GUESS, the other as runner-up;
 *     muxgl_demux_run names the pair (lo, hi).  Every such cell is looked at (two hypotheses);
 *   - best and next of a scan, or a +2 threshold, within reach: the named hypotheses are recomputed and compared;
 *   - next and third of a scan within reach (MUXGL_CELL_DEEP_* in `valid`): every hypothesis of that scan is recomputed.
 * Integer fields and the log-likelihoods of recomputed hypotheses then equal the reference's exactly; sumLLK / sngLLK
 * stay as the device summed them.  The pileup and gp / has_gp are the arrays handed to muxgl_set_pileup /
 * muxgl_demux_set_gp.  nthreads host threads (cells are independent).
 * stats: NULL or int64[6] = cells looked at, mirrored pairs put into (hi, lo) order, mirrored pairs whose two orders tied
 * exactly, cells with a near tie other than the mirror, cells that needed every hypothesis of a scan, cells whose call
 * changed beyond the order of a mirrored pair. */
int muxgl_demux_exact_calls(int64_t C, int32_t V, const int64_t* cell_ptr, const int32_t* entry_snp,
                            const int64_t* entry_rptr, const uint8_t* reads, const double* gp, const uint8_t* has_gp,
                            const muxgl_demux_params* p, muxgl_demux_cell* cells, int32_t nthreads, int64_t* stats);

/* pinned host view of the last run's [C] records (valid until the next run or destroy) */
const muxgl_demux_cell* muxgl_demux_results(const muxgl_handle* h);

/* What the most recent muxgl_demux_run did on the default-grid path (V <= 32, alpha {0, 0.5}), for tests and tuning:
 * info[0] = the first cell of the second cell group of the plan (0: one group), info[1] = the cell groups that run used
 * (1 or 2; 1 as well when the LL tensor was asked for, and always under MUXGL_FLAG_NO_LINEAR_ENTRIES, whose plan has no
 * launch order), info[2] = the sweep units the device holds at once (one residency round), info[3] = the plan's units.
 * The boundary follows from info[2] and the plan; the environment variable MUXGL_OCT_SPLIT=<cell index>, read when the
 * plan is built (first run after muxgl_set_pileup / muxgl_demux_set_gp), places it explicitly, 0 forces one group.
 * Records do not depend on it.  Zeros before the first run, on other paths' plans and for a device group. */
int muxgl_demux_oct_split(const muxgl_handle* h, int64_t* info);

/* per-entry pGs[nnz][n_alpha*9] of the last run (cmd_cram_demuxlet.cpp:655-725), for parity tests */
int muxgl_demux_get_entry_pg(muxgl_handle* h, double* pg);

/* ---- freemuxlet ---------------------------------------------------------------------------------------------- */
/* b1+b2: calculate_snp_droplet_pileup for every entry (sc_drop_seq.cpp:452-509) and the per-cell singlet scores
 * (cmd_cram_freemux2.cpp:117-160).  af[S] from the .var.gz AF column.  Outputs [C], any may be NULL.
 * The reference sorts the cells by llk2 - llk0 (ties by index, sc_drop_seq.h:190-198) and the greedy start walks them in
 * that order, so where two cells' scores are within 1e-9 x max(1, |llk|) of each other -- droplets of single-read entries
 * score 0 +- rounding noise -- the last bits decide.  When both cell_llk0 and cell_llk2 are asked for on a handle that
 * holds the whole pileup, the sums of every such cell are therefore recomputed exactly as the reference forms them (IEEE
 * operations in its order on the device, glibc log on the host, score_exact.hpp); all other cells keep the device's sums
 * (equal to ~1e-13); a device group does the same, each member for its cells.  A slabbed handle (one rank of a sharded run:
 * it sees only its own cells) returns the device's sums for all of them. */
int muxgl_fmx_prepare(muxgl_handle* h, const double* af, double* cell_llk0, double* cell_llk2, int32_t* cell_nsnps,
                      int32_t* cell_nreads);

/* of the last muxgl_fmx_prepare: the number of cells whose sums were recomputed in the reference's arithmetic */
int muxgl_fmx_score_stats(const muxgl_handle* h, int64_t* exact_scores);

/* entry pileups (for parity checks and callers that want them): gls[nnz][9],
 * counts[nnz][3] = nreads,nref,nalt.  Either may be NULL. */
int muxgl_fmx_get_entry_gls(muxgl_handle* h, double* gls, int32_t* counts);

/* b3+b4: sort cells by singlet score (descending, ties by id descending: cmd_cram_freemux2.cpp:184-189 with the
 * comparator sc_drop_seq.h:187-198) and run the greedy initial clustering (:217-261, distance =
 * sc_dropseq_lib_t::calculate_droplet_clust_distance, sc_drop_seq.cpp:544-578).  scores[C] = cell_scores (llk2-llk0,
 * possibly shuffled by --randomize-singlet-score on the caller side).  The procedure is sequential over cells by
 * construction (each assignment changes the cluster pileups the next cell is scored against): the cells are sorted on
 * the host; the device then decides them in batches of 32, each batch as a fixpoint of the sequential rule (guess from
 * the state at the start of the batch, replay of the predecessors' merges at shared SNPs, iterate until no guess
 * changes), or, beyond 64 clusters or where the batched kernel cannot be resident, with one persistent workgroup walking
 * the cells in order (fmx_greedy.hip).  The kernels form their scores in another association than the reference's
 * (products instead of sums of logs), equal to ~1e-13 relative: a decision whose margin over the runner-up is within
 * 1e-9 x max(1, |score|) is therefore not taken by them but by greedy_exact.hpp, which recomputes that step's K distances
 * in the reference's own arithmetic (IEEE operations in the reference's order on the device, glibc log on the host) given
 * the earlier decisions -- all such steps of a pass in one launch.  Where it overrules the kernel, the steps behind it that
 * cover a SNP of a cell whose decision changed are decided again the same way against the corrected assignments, in
 * order; every other step stands (it read none of the states that changed).  Only if that walk outlasts twice the pass
 * itself is the pass repeated with the decisions so far pinned.  A score of exactly 0 counts as the
 * structural tie of clusters sharing no SNP with the cell only when both of its products are empty.  The result is the
 * reference's clustering, not an approximation of it (muxgl_fmx_greedy_stats reports how often the exact path was taken).
 * One device, whole pileup: not available on a device group or a slabbed handle.
 * clust_out[C] receives the cluster id, or -1 for cells skipped by frac_init_clust / singlet_score_thres. */
int muxgl_fmx_greedy_init(muxgl_handle* h, int32_t K, const double* scores, double frac_init_clust,
                          double singlet_score_thres, int32_t* clust_out);

/* of the last muxgl_fmx_greedy_init: steps whose margin was a near tie and went through the exact path, and how many of
 * those it decided differently from the kernel (each such step repeats the run once).  Either pointer may be NULL. */
int muxgl_fmx_greedy_stats(const muxgl_handle* h, int64_t* near_ties, int64_t* overruled);

/* initial clusters (after --init-cluster or greedy init): builds the cluster pileups in ascending cell id
 * (cmd_cram_freemux2.cpp:277-288) and resets types/jBest/kBest (:263-265,349-350).  clust[C], -1 = unassigned. */
int muxgl_fmx_set_clusters(muxgl_handle* h, int32_t K, const int32_t* clust);

/* Anchored clusters: a pool of which only some donors are genotyped.  Clusters 0 .. n_anchor-1 take their genotype
 * posteriors from the panel of muxgl_demux_set_gp instead of from their cluster pileups: cluster i reads column donor[i].
 * n_anchor = 0 (donor may be NULL) removes the anchors.  The other clusters are learned from the droplets as ever, in the
 * same EM; with K = n_anchor the run is a genotype-driven assignment in freemuxlet's arithmetic.
 *
 * From the next posterior phase on (muxgl_fmx_iterate, muxgl_fmx_iter_gp) the row [s][i] of an anchored cluster that every
 * E-step path, the exact near-tie path and the three tables muxgl_fmx_singlets / _inclusion / _unknown read is
 *   - at a marker with genotypes (has_gp[s]): the panel row gp[s][donor[i]] as given -- the loader has applied its error
 *     model; geno_error is not mixed in again;
 *   - at a marker without: the row of a cluster without cells (HWE at af[s], mixed with itself by geno_error), so an
 *     anchored donor without any genotype behaves bit for bit like an empty cluster.
 * Clusters >= n_anchor are untouched and the priors of a singlet and a doublet use the whole K.  donor may name a column
 * twice: such clusters tie exactly and the scan order decides, as it does for clusters without cells.
 *
 * The M-step is unchanged: singlets still merge into an anchored cluster's pileup.  muxgl_fmx_get_cluster_pileup,
 * muxgl_fmx_match_donors, muxgl_fmx_cluster_pairs and a written cluster VCF therefore keep describing the DROPLETS assigned
 * to a cluster; for an anchored cluster that is a check on the panel's genotypes, not what the next E-step reads.
 *
 * The anchors belong to the cluster state: muxgl_fmx_set_clusters, muxgl_fmx_prepare, muxgl_set_pileup and
 * muxgl_demux_set_gp (the panel they index goes) drop them, as do muxgl_fmx_set_column_slab and a muxgl_fmx_set_shard
 * range that is not the whole job.  This call -- also the removal -- makes the three tables
 * unavailable until the next E-step and has the near-tie cells settled again.  Call it after muxgl_fmx_set_clusters.
 * Refused, with the handle left as it was: no clusters set; n_anchor outside [0, K]; n_anchor > 0 without a panel, with
 * donor == NULL or with a donor outside [0, V); a handle with a caller's own slabs (muxgl_fmx_set_column_slab) or shard
 * (muxgl_fmx_set_shard with less than the whole job).  Device groups are supported. */
int muxgl_fmx_set_anchors(muxgl_handle* h, int32_t n_anchor, const int32_t* donor /* [n_anchor], each in [0, V) */);

/* Anchors with a mode each: muxgl_fmx_set_anchors is this call with mode == NULL (all HELD), and after it every anchored
 * cluster is HELD again.  The same refusals and the same state effects; a mode other than the two below is refused too,
 * with the handle -- its anchors and their modes included -- left as it was.
 *
 * MUXGL_ANCHOR_HELD   the panel row IS the posterior row, as described above.
 * MUXGL_ANCHOR_PRIOR  the panel row is the PRIOR of the posterior the droplets form ("learn the genotypes with the donor
 *   VCF as prior"): for low-pass or imputed panels, RNA-derived calls, flat GP / PL rows.  Cluster i with v = donor[i] is a
 *   free cluster whose Hardy-Weinberg triple inside the product of cmd_cram_freemux2.cpp:402-415 is the panel row:
 *     - at a marker with genotypes, with w = gp[s][v][0..2] and d = (gls[0], gls[4], gls[8]) of the cluster's own pileup:
 *       q_g = w_g d_g / sum_g w_g d_g, then, if geno_error > 0, q_g <- (1 - e) q_g + e p_g with p the Hardy-Weinberg triple
 *       at af[s].  A zero in w is a zero in q before the mix.  d is positive, so the sum vanishes only for a row w without
 *       a positive entry; such a row (or one holding a NaN) is used as given, as for a HELD cluster;
 *     - at a marker without, the row of the free cluster with this pileup, bit for bit.
 *   A PRIOR cluster whose panel rows equal the Hardy-Weinberg triples bit for bit, or without genotypes anywhere, is a free
 *   cluster bit for bit, on every E-step path and on the exact near-tie path.  The M-step, the priors of a singlet and a
 *   doublet and the state rules are those of a HELD cluster; HELD and PRIOR clusters mix freely. */
#define MUXGL_ANCHOR_HELD 0
#define MUXGL_ANCHOR_PRIOR 1
int muxgl_fmx_set_anchors_mode(muxgl_handle* h, int32_t n_anchor, const int32_t* donor /* [n_anchor] */,
                               const uint8_t* mode /* [n_anchor] MUXGL_ANCHOR_*, or NULL = all HELD */);

/* The posterior rows [s][k][0..2] of clusters k0 <= k < k1 that the last posterior phase (muxgl_fmx_iterate,
 * muxgl_fmx_iter_gp) wrote and its E-step read -- free, HELD and PRIOR clusters alike; for a PRIOR cluster the genotypes
 * as the droplets refined them.  out: [S][k1 - k0][3].  Reads state and changes none.  Refused: no clusters set; before
 * the first posterior phase after muxgl_fmx_set_clusters; a range outside [0, K].  On a sharded handle the rows outside its
 * own SNP range are what the caller's exchange put there.  Device groups are supported. */
int muxgl_fmx_get_cluster_gp(muxgl_handle* h, int32_t k0, int32_t k1, double* out /* [S][k1-k0][3] */);

/* one EM iteration, cmd_cram_freemux2.cpp:375-597: E-step, scans, re-assignment, ordered M-step.
 * out: NULL or [C].  full_ll: NULL or [C][K(K+1)/2].
 * The streamed E-step (K > 255, MUXGL_FLAG_FORCE_STREAMED_ESTEP at K > 32, or a K <= 255 job whose [C][K(K+1)/2] table
 * does not fit 0.9 x the device's memory) sweeps the pair matrix in 64 x 64 blocks of clusters, a group of
 * (cells x blocks) at a time, and keeps only what the call reads per cell: its device memory does not depend on C x K^2
 * (a slab budget of 4 GiB or a third of device memory; MUXGL_FMX_SLAB_MB in the environment overrides it).  It keeps no
 * [C][K(K+1)/2] table, so full_ll must be NULL there: otherwise the call fails with an error. */
int muxgl_fmx_iterate(muxgl_handle* h, const muxgl_fmx_params* p, muxgl_fmx_cell* out, int32_t* nsingle, int32_t* namb,
                      int32_t* nchanged, double* full_ll);

/* sng[C][K] = llks[j(j+1)/2 + j] of cmd_cram_freemux2.cpp:448-455 for every droplet and cluster, as the LAST E-step of this
 * handle formed them: sng[c][j] = sum over the entries e of c of log(egl_e[0] q[s_e][j][0] + egl_e[4] q[s_e][j][1] +
 * egl_e[8] q[s_e][j][2]), egl_e the entry likelihoods of muxgl_fmx_prepare and q the cluster genotype posteriors that
 * E-step read (MUXGL_BUF_CGP, geno_error mixed in, :402-415) -- so the call takes no parameters.  This is the number
 * sngBestLLK / sngNextLLK are scanned from (:485-497) and the diagonal of full_ll where that table exists; it does not need
 * the table, runs at any K up to MUXGL_MAX_CLUSTERS whichever E-step path ran, on one device, a device group and a slabbed or
 * sharded handle (per-cell output covers the handle's own cells, as muxgl_fmx_iter_fetch's records do; every member of a
 * group sweeps its own cells).  The M-step and the near-tie path behind an E-step leave the posteriors alone, so the table
 * belongs to the records of the same iteration: call it after muxgl_fmx_iterate, or after muxgl_fmx_iter_estep (and whatever
 * follows it) and before the next muxgl_fmx_iter_gp.  It fails, naming the reason, before the first E-step since
 * muxgl_fmx_set_clusters, after a posterior phase without its E-step, for a NULL output, without a pileup and without
 * muxgl_fmx_prepare; the handle stays usable.  A droplet without entries gets a row of zeros.
 * The table is the device's arithmetic throughout (products of factors, one log per cell part and cluster: equal to the
 * reference's sums of logs to ~1e-11): the records of a near-tie cell carry the values the exact path recomputed in the
 * reference's arithmetic (muxgl_fmx_exact_stats), the table keeps the device's for those cells too.
 * It reads state and changes none: records, counters, assignments, cluster pileups and the near-tie bookkeeping stay as
 * they are.  The device holds a slab of the table (the streamed E-step's budget: 4 GiB or a third of the device,
 * MUXGL_FMX_SLAB_MB); a larger table is swept in batches of cells, each copied out before the next; nothing proportional to
 * C x K^2.  The table is bit-identical from call to call, for any budget, on one device, on a group and through the sharded
 * driver.  Under MUXGL_FLAG_ASYNC_PHASES it returns with the stream drained, like every non-phase call.  Its kernel time
 * is MUXGL_T_FMX_SINGLETS of muxgl_get_timing (the slots of the last iteration keep their values); it counts as a
 * collecting call of muxgl_get_timing_sum. */
int muxgl_fmx_singlets(muxgl_handle* h, double* sng);

/* Per droplet c and cluster s: how much evidence there is that s is in the droplet at all, and with which cluster s pairs
 * best -- the row and column marginals of the triangle llks[] of cmd_cram_freemux2.cpp:383-456 as the LAST E-step of this
 * handle formed it (the reference keeps only the best and the next doublet of a droplet, :469-513).  The hypotheses are
 * those of the scans :469-498: a singlet (j, j) with log_single_prior (lsp, :379), a doublet (j, k), k < j, with
 * log_double_prior (ldp, :380); LL(j, k) = llks[j(j+1)/2 + k].  For cluster s, H_s = { (s, k) : k < s } + { (j, s) : j > s }.
 * incl[C][K]    = log( exp(LL(s,s) + lsp) + sum_{h in H_s} exp(LL(h) + ldp) )
 * tot[C]        = log of the same sum over all singlets and all doublets: the record's sumLLK (whose seed of -1e300 adds
 *                 nothing), so exp(incl - tot) is the posterior that s is in the droplet
 * dbl[C][K]     = max_{h in H_s} LL(h)   (-1e300 when H_s is empty, K == 1, or holds no finite value)
 * partner[C][K] = the other cluster of that hypothesis (-1: none).  Ties: value descending, then position
 *                 p = hi(hi+1)/2 + lo ascending, the order of the scans.  s is the first (higher) cluster of the pair
 *                 exactly when partner < s.
 * Any out pointer may be NULL (all four: the call succeeds and writes nothing).  p->doublet_prior is read; geno_error is
 * not (it is already mixed into the posteriors the E-step read).  A hypothesis whose LL is -inf (a cluster whose posterior
 * rows were never filled) adds nothing to a sum and never wins dbl; a sum without a finite term is -inf, never NaN.  A
 * droplet without entries has LL = 0 for every hypothesis.
 * State rules, refusals and guarantees are muxgl_fmx_singlets': the tables belong to the records of the same iteration
 * (call it after muxgl_fmx_iterate, or after muxgl_fmx_iter_estep and before the next muxgl_fmx_iter_gp); it fails, naming
 * the reason, before the first E-step since muxgl_fmx_set_clusters, after a posterior phase without its E-step, for NULL
 * p, without a pileup and without muxgl_fmx_prepare, and the handle stays usable; it reads state and changes none
 * (records, counters, assignments, cluster pileups and the near-tie bookkeeping stay as they are).  1 <= K <=
 * MUXGL_MAX_CLUSTERS whichever E-step path ran; one device, a device group (every member fills the rows of its own cells)
 * and a slabbed or sharded handle (per-cell outputs cover the handle's own cells).
 * The values are the device's arithmetic throughout: the streamed E-step's sweep (products of factors, one log per cell
 * part and hypothesis, equal to the reference's sums of logs to ~1e-11), also where another E-step path made the records.
 * Near ties in `partner` are decided by those values and the order above, not re-resolved in exact arithmetic; the
 * records of a near-tie cell carry the exact path's values, the tables keep the device's for those cells too.
 * Within the streamed E-step's budget (4 GiB or a third of the device, MUXGL_FMX_SLAB_MB) the device holds a slab of the pair
 * sweep plus the state and the outputs of a batch of whole cells (52 bytes per cell and cluster); a batch is finished and
 * copied out before the next; nothing proportional to C x K^2.  It fails, naming the variable, when one cell's state and
 * one 64 x 64 block of the sweep exceed the budget.  All four outputs are bit-identical from call to call, for any budget,
 * on one device, on a group and through the sharded driver.  Under MUXGL_FLAG_ASYNC_PHASES it returns with the stream
 * drained.  Its kernel time is MUXGL_T_FMX_INCLUSION of muxgl_get_timing (the slots of the last iteration keep their
 * values); it counts as a collecting call of muxgl_get_timing_sum. */
int muxgl_fmx_inclusion(muxgl_handle* h, const muxgl_fmx_params* p, double* incl, double* tot, double* dbl,
                        int32_t* partner);

/* Every droplet against a donor that NO cluster holds -- a donor spread over clusters that are not theirs because
 * --nsample is too small, or one with too few cells for the greedy start to give them a cluster.  A cluster without cells
 * has a pileup of ones and its posterior row at a marker is the Hardy-Weinberg triple gp0s of cmd_cram_freemux2.cpp:388-390:
 * the reference run with K + 2 clusters, two of them empty, holds these numbers in its llks[] triangle.  With g = egl_e[9]
 * the entry likelihoods of muxgl_fmx_prepare, q[s][j][.] the cluster posteriors the last E-step read (MUXGL_BUF_CGP,
 * geno_error mixed in), u[s][.] the unknown donor's genotype prior at marker s, and the sums over the entries e of droplet
 * c in entry order:
 *   ll_ju[C][K]: ll_ju[c][j] = sum_e log sum_g1 sum_g2 g[3 g1 + g2] * u[s_e][g1] * q[s_e][j][g2]
 *                (cluster j plus the unknown donor: slot (K, j), :440-446, the unknown donor the higher-numbered cluster)
 *   ll_u[C]:     ll_u[c]     = sum_e log sum_g g[4 g] * u[s_e][g]                     (the unknown donor alone: slot (K, K))
 *   ll_uu[C]:    ll_uu[c]    = sum_e log sum_g1 sum_g2 g[3 g1 + g2] * u[s_e][g1] * u[s_e][g2]
 *                (two unknown donors: slot (K + 1, K))
 * gp0 == NULL: u[s] = ((1-af)(1-af), 2 af (1-af), af af), formed exactly as :388-390 from the af of muxgl_fmx_prepare, on
 * the device.  gp0 != NULL: the caller's rows [S][3] (a specific donor's genotypes, say).  Every row must be a probability
 * triple -- entries in [0, 1], sum within 1e-6 of 1; this is checked on the host before any device work and the call
 * fails naming the first offending marker.  The reference's empty cluster goes through the division by its sum and the
 * geno_error mixing with itself (:406-415) and equals u only to an ulp; the call uses u as defined here.
 * With gp0 == NULL, ll_u and ll_uu are the quantities behind cell_llk2 / cell_llk0 of muxgl_fmx_prepare; the call forms
 * them itself (so they exist for a caller's prior and on a slabbed rank), and they are the device's sums (products of
 * factors, one log per cell part), not the exactly recomputed ones muxgl_fmx_prepare returns for near-tied cells.
 * State rules and refusals are muxgl_fmx_singlets': call it after muxgl_fmx_iterate, or after muxgl_fmx_iter_estep and
 * before the next muxgl_fmx_iter_gp; it fails, naming the reason, before the first E-step since muxgl_fmx_set_clusters,
 * after a posterior phase without its E-step, without a pileup and without muxgl_fmx_prepare, and the handle stays usable.
 * It reads state and changes none: records, counters, assignments, cluster pileups, MUXGL_BUF_CGP, the near-tie
 * bookkeeping and whether the other table calls may run stay as they are; it caches nothing on the handle.  Under
 * MUXGL_FLAG_ASYNC_PHASES it returns with the stream drained.
 * 1 <= K <= MUXGL_MAX_CLUSTERS whichever E-step path ran; one device, a device group (every member fills the rows of its
 * own cells) and a slabbed or sharded handle (the outputs cover the handle's own cells).
 * Any subset of the three outputs may be NULL; with all three NULL the call fails, naming the reason, and the handle stays
 * usable.  A droplet without entries gets zeros.  A factor of exactly 0 (a one-hot gp0 against posterior rows that were
 * never filled) gives -inf, never NaN.
 * kernel_ms (NULL allowed) receives the hipEvent time of the call's kernels, from a pair of events the call makes for
 * itself (a group: the slowest member's): no timing slot of muxgl_get_timing is touched and the call is not a collecting
 * call of muxgl_get_timing_sum.
 * Device memory: the cells are swept in batches of whole cells whose 40 bytes of weights per entry, slab rows (K + 2
 * doubles per cell part) and table rows fit the streamed E-step's budget (4 GiB or a third of the device,
 * MUXGL_FMX_SLAB_MB); each batch is copied out before the next; the call fails, naming the variable, when one cell alone
 * exceeds the budget.  The outputs are bit-identical from call to call, for any MUXGL_FMX_SLAB_MB, for any subset of
 * outputs, on one device, on a group and through the sharded driver, and for a gp0 holding the Hardy-Weinberg rows formed
 * with the expressions above against the NULL call. */
int muxgl_fmx_unknown(muxgl_handle* h, const double* gp0 /* NULL or [S][3] */,
                      double* ll_ju /* NULL or [C][K] */, double* ll_u /* NULL or [C] */,
                      double* ll_uu /* NULL or [C] */, float* kernel_ms /* NULL or one float */);

/* Every droplet as ONE cell of cluster j plus a share rho of ambient RNA: the reading freemuxlet lacks (a clean singlet
 * from a high-soup prep comes out as a doublet of its own cluster with a partner picked nearly at random), the counterpart
 * of muxgl_demux_ambient.  The ambient RNA is no donor: its ALT fraction at marker s is the pool's, amb_af[s], any number
 * in [0, 1], and its share any rho in [0, 1].  This is calculate_snp_droplet_pileup (sc_drop_seq.cpp:452-509, alpha =
 * 0.5) with three ambient elements per rho carried along the entry's nine:
 *   p(l, f, rho) = 0.5 * l + (2 * f - l) * 0.5 * rho                                (f = amb_af[s_e])
 *   per usable read of entry e, in read order (a byte of MUXGL_READ_OTHER is skipped, :468):
 *       nine[i] *= mat * frac_i + e4                                               (:483-491)
 *       a[r][l] *= mat * (ALT read ? p : 1 - p) + e4,   p = p(l, f, rho[r])
 *       t = nine[0] + ... + nine[8]; nine and a are all divided by t               (:493-494)
 *   after the reads every element of nine and of a below 1e-6 becomes 1e-6 (:498-501, sc_drop_seq.h:14),
 *       T = sum of the floored nine, w_e[r][l] = a[r][l] / T                       (:502-504)
 *   ll_amb[c][j][r] = sum over the entries e of droplet c, in entry order, of
 *                     log( q[s_e][j][0] * w_e[r][0] + q[s_e][j][1] * w_e[r][1] + q[s_e][j][2] * w_e[r][2] )
 * q[s][j][.] are the cluster posteriors the last E-step read (MUXGL_BUF_CGP, geno_error mixed in).  The ambient elements
 * take part in none of the sums t and T: those are the numbers behind the entry likelihoods of muxgl_fmx_prepare, so
 * ll_amb is on the scale of the log-likelihoods of .clust1.samples.gz and of muxgl_fmx_singlets, and may be subtracted
 * from bestLLK or dblBestLLK.  Every marker contributes (freemuxlet has no has_gp).  Three identities:
 *   amb_af in {0, 0.5, 1} and rho[r] == 0.5: p = (l + 2 f) / 4 exactly, w_e[r][l] is the entry likelihood gls[3 l + 2 f],
 *     and ll_amb[c][j][r] is the reference's doublet slot (j, X) for a cluster X whose posterior row at marker s is one-hot
 *     at genotype 2 * amb_af[s];
 *   rho[r] == 0: w_e[r][l] = gls[4 l], the column is the table of muxgl_fmx_singlets;
 *   rho[r] == 1: p is amb_af, the column is the same for every cluster (up to the rounding of q's row sums).
 * The rho reported for a droplet by a caller is the maximum over the grid rho[]; muxgl_fmx_ambient_fit (below) gives the
 * continuous estimate with its observed information.
 * State rules and refusals are muxgl_fmx_unknown's under this call's name: call it after muxgl_fmx_iterate, or after
 * muxgl_fmx_iter_estep and before the next muxgl_fmx_iter_gp.  It also fails, naming the reason and leaving the handle
 * usable, with ll_amb, amb_af or rho NULL, with n_rho outside [1, 16], naming the first rho and then the first marker
 * whose value is not a finite number in [0, 1], and when one cell alone exceeds the budget (naming MUXGL_FMX_SLAB_MB).
 * It reads state and changes none: records, counters, assignments, cluster pileups, MUXGL_BUF_CGP and whether the other
 * table calls may run stay as they are; it caches nothing on the handle.  kernel_ms (NULL allowed) receives the hipEvent
 * time of the call's kernels, from a pair of events the call makes for itself (a group: the slowest member's): no timing
 * slot of muxgl_get_timing is touched.  With C == 0 the call succeeds and writes nothing; a droplet without entries gets
 * zeros.  1 <= K <= MUXGL_MAX_CLUSTERS whichever E-step path ran; one device, a device group (every member fills the rows
 * of its own cells) and a slabbed or sharded handle (the output covers the handle's own cells).
 * Device memory: nothing proportional to nnz x n_rho is held for the whole pileup.  The cells are swept in batches of
 * whole cells whose 24 bytes of weights per entry and rho, slab rows and table rows fit the streamed E-step's budget
 * (4 GiB or a third of the device, MUXGL_FMX_SLAB_MB); each batch is copied out before the next.  The table is
 * bit-identical from call to call, for any budget, for any split of rho[] over several calls, on one device, on a group
 * and through the sharded driver. */
int muxgl_fmx_ambient(muxgl_handle* h, const double* amb_af /* [S] */, int32_t n_rho, const double* rho /* [n_rho] */,
                      double* ll_amb /* [C][K][n_rho] */, float* kernel_ms /* NULL or one float */);

/* The ambient share of muxgl_fmx_ambient as a per-droplet maximum-likelihood estimate, for n_cand candidate clusters per
 * droplet (cand[c][k] = a cluster, or -1 to skip the slot): the counterpart of muxgl_demux_ambient_fit.  The model is
 * muxgl_fmx_ambient's, unchanged; with a[l](rho), T and q exactly as above,
 *   LL(rho) = sum over ALL entries e of droplet c of log( q[s_e][j][0] * w_e[0] + q[s_e][j][1] * w_e[1] + q[s_e][j][2] * w_e[2] ),
 *   w_e[l] = max(a[l](rho), 1e-6) / T.
 * Every read's ambient factor is linear in rho with slope v = +-mat * (2 * f - l) * 0.5 (+ for an ALT read), so a[l] is a
 * polynomial in rho and its derivatives follow from the product rule along the reads (a'' = a'' * fac + 2 * a' * v; a' =
 * a' * fac + a * v; a = a * fac; all three divided by the read's t).  The 1e-6 floor makes LL piecewise: where a[l] < 1e-6
 * the element is the constant 1e-6 and its derivatives are 0 -- the derivative of the floored function on that piece.  LL
 * is continuous; where an element crosses the floor LL' jumps, always upward (max(a, 1e-6) is convex in a), so a maximum of
 * LL never sits on such a kink and the search, which narrows its bracket by the sign of LL' alone, closes on a smooth zero
 * of LL'.  An upward jump can also start a second rise of LL inside the bracket of the coarse points; therefore, where an
 * element is below the floor at one of the bracket's three coarse points and not at another, LL is first taken on the 65
 * points lo + (hi - lo) * i / 64 of that bracket and the best of them (ties to the lowest index) with its two neighbours
 * becomes the bracket; status 1 / 2 then need that point to be 0 / rho_max.  Per (c, k), each array [C][n_cand]: rho_hat, ll_hat, ll_zero (the candidate's entry of muxgl_fmx_singlets),
 * info, status and n_steps mean what they mean for muxgl_demux_ambient_fit, found by the same search (the nine coarse
 * points i * rho_max / 8, the bracket around the best, the bound tests, the safeguarded Newton iteration on LL' with the
 * stops 1e-9, one last Newton step, 48 steps), with the statuses
 *   0 interior and converged; 1 at the lower bound; 2 at the upper bound; 3 step cap reached; 4 slot skipped (cand < 0: all
 *   outputs 0); 5 droplet without entries (all outputs 0); 6 LL at a coarse point is not finite -- a posterior row of
 *   exactly 0 at one of the droplet's markers makes a factor 0: rho_hat = 0, ll_hat = ll_zero = -inf, info = 0, n_steps = 0;
 *   no NaN is written.
 * The standard error of rho_hat is info^(-1/2) where status is 0 and info > 0; on a bound there is none.  The likelihood
 * ratio against rho = 0 is 2 * (ll_hat - ll_zero).
 * State rules are muxgl_fmx_ambient's under this call's name: call it after muxgl_fmx_iterate, or after
 * muxgl_fmx_iter_estep and before the next muxgl_fmx_iter_gp.  1 <= n_cand <= MUXGL_MAX_FIT_CAND; 0 < rho_max <= 1, finite;
 * every cand in [-1, K); every amb_af[s] a finite number in [0, 1]; any of the six outputs may be NULL, not all.  Every
 * refusal names its reason and leaves the handle usable.  Any K up to MUXGL_MAX_CLUSTERS on every E-step path, with
 * anchors held or as priors; one device, a device group (every member fits its own cells) and a slabbed or sharded handle
 * (the outputs cover the handle's own cells).  With C == 0 the call succeeds and writes nothing.  It reads state and
 * changes none and touches no timing slot; kernel_ms (NULL allowed) receives the hipEvent time of the call's one kernel
 * from events of its own (a group: the slowest member's).
 * Device memory: the inputs, cand and the outputs.  The entry likelihoods are recomputed on every pass; nothing
 * proportional to nnz is allocated, so no slab budget applies and MUXGL_FMX_SLAB_MB is not read.  The whole fit of a
 * (droplet, candidate) runs in one wave of one launch with every reduction tree fixed by the droplet alone: the outputs
 * are bit-identical from call to call, for any order, grouping or repetition of candidates, for any subset of outputs, on
 * one device, on a group and through the sharded driver. */
int muxgl_fmx_ambient_fit(muxgl_handle* h, const double* amb_af /* [S] */, int32_t n_cand,
                          const int32_t* cand /* [C][n_cand], cluster or -1 */, double rho_max,
                          double* rho_hat, double* ll_hat, double* ll_zero, double* info, /* [C][n_cand] or NULL */
                          int32_t* status, int32_t* n_steps, float* kernel_ms);

/* The mixing share alpha of a freemuxlet doublet as a per-droplet maximum-likelihood estimate, for n_cand slots per droplet
 * (pair[c][t] = (j, k), two clusters, or (-1, -1) to skip the slot; j == k is allowed): the counterpart of
 * muxgl_demux_alpha_fit.  The reference fixes the share at one half (calculate_snp_droplet_pileup(..., 0.5),
 * sc_drop_seq.cpp:452-509; the pair loop is cmd_cram_freemux2.cpp:394-455), so a 15 : 85 doublet is scored as a 50 : 50 one.
 * Here alpha is the share of k.  The genotype pair (l, m), l from j and m from k, element l * 3 + m
 * (sc_drop_seq.cpp:472-480), has
 *   p(l, m, alpha) = 0.5 * l + (m - l) * 0.5 * alpha      the ALT-read probability; one fma; exact at alpha = 0, 0.5, 1
 *   x = ALT read ? p : 1 - p
 *   per usable read:  a[l][m] *= (mat * x + e4);  then a[l][m] *= 1 / t     t = the read's sum of the REFERENCE nine (alpha = 0.5)
 *   after the reads:  a[l][m] = max(a[l][m], 1e-6);  w[l][m] = a[l][m] * (1 / T)    T = the final sum of the floored reference nine
 *   D_e = sum_l sum_m (q[s_e][j][l] * q[s_e][k][m]) * w_e[l][m]     q = the posteriors the last E-step read (MUXGL_BUF_CGP)
 *   LL(alpha) = sum over ALL entries e of droplet c of log D_e
 * The reference renormalises its nine after every read by a sum that depends on alpha, so its function called with
 * another alpha is on another scale per alpha and is no likelihood in alpha: the six off-diagonal elements take the read's
 * 1 / t and the final 1 / T of the alpha = 0.5 nine and take part in neither sum, as the ambient elements of
 * muxgl_fmx_ambient do; the three diagonal elements do not depend on alpha.  At alpha = 0.5 LL is the reference's
 * llks[j * (j + 1) / 2 + k] of the last E-step (k < j); at alpha = 0 every element (l, m) is the diagonal element (l, l) and
 * LL is cluster j's entry of muxgl_fmx_singlets, at alpha = 1 cluster k's (sum_m q[m] = 1 to rounding): both singlets nest.
 * Every read's factor is linear in alpha with slope v = +-mat * (m - l) * 0.5 (+ for an ALT read), so the derivatives
 * follow from the product rule along the reads as for muxgl_fmx_ambient_fit; a floored element is the constant 1e-6 with
 * derivatives 0.  D' and D'' are summed with (l, m) next to (m, l), without a fused step: exactly 0 where the two
 * posterior rows hold the same numbers.  Each element is a product of positive linear factors, above the floor on an
 * interval, and the coefficients q * q are >= 0: LL' jumps only upward at a crossing, a maximum never sits on a kink, and
 * a bracket in which an element changes sides is first scanned on 65 points, as for muxgl_fmx_ambient_fit.
 * Per (c, t), each array [C][n_cand]: alpha_hat, ll_hat = LL(alpha_hat), ll_zero = LL(0), ll_top = LL(alpha_max), info =
 * -LL''(alpha_hat), status and n_steps, found by muxgl_fmx_ambient_fit's search on [0, alpha_max], with its statuses
 *   0 interior and converged; 1 at the lower bound (ll_hat == ll_zero bit for bit); 2 at the upper bound (ll_hat == ll_top
 *   bit for bit); 3 step cap reached; 4 slot skipped (all outputs 0); 5 droplet without entries (all outputs 0); 6 LL at a
 *   coarse point is not finite -- a posterior row of exactly 0: alpha_hat = 0, ll_hat = ll_zero = ll_top = -inf, info = 0,
 *   n_steps = 0; no NaN is written.
 * The standard error of alpha_hat is info^(-1/2) where status is 0 and info > 0.
 * State rules are muxgl_fmx_ambient's under this call's name: call it after muxgl_fmx_iterate, or after
 * muxgl_fmx_iter_estep and before the next muxgl_fmx_iter_gp.  1 <= n_cand <= MUXGL_MAX_FIT_CAND; 0 < alpha_max <= 1,
 * finite; every index in [-1, K); a slot with exactly one negative index, pair == NULL and every output NULL are refused.
 * Every refusal names its reason and leaves the handle usable.  Any K up to MUXGL_MAX_CLUSTERS on every E-step path, with
 * anchors held or as priors; one device, a device group (every member fits its own cells) and a slabbed or sharded handle
 * (the outputs cover the handle's own cells).  With C == 0 the call succeeds and writes nothing.  It reads state and
 * changes none and touches no timing slot; kernel_ms (NULL allowed) receives the hipEvent time of the call's one kernel
 * from events of its own (a group: the slowest member's).
 * Device memory: the inputs, pair and the outputs.  Nothing proportional to nnz is allocated, so no slab budget applies and
 * MUXGL_FMX_SLAB_MB is not read.  The whole fit of a (droplet, slot) runs in one wave of one launch with every reduction
 * tree fixed by the droplet alone: the outputs are bit-identical from call to call, for any order, grouping or repetition
 * of slots, for any subset of outputs, on one device, on a group and through the sharded driver. */
int muxgl_fmx_alpha_fit(muxgl_handle* h, int32_t n_cand, const int32_t* pair /* [C][n_cand][2]: (j, k) or (-1, -1) */,
                        double alpha_max,
                        double* alpha_hat, double* ll_hat, double* ll_zero, double* ll_top, double* info, /* [C][n_cand] or NULL */
                        int32_t* status, int32_t* n_steps, float* kernel_ms);

/* Near-tie calls of the EM iterations since muxgl_fmx_set_clusters.  The kernels' log-likelihoods equal the reference's to
 * ~1e-12, not to the last bit; a cell where a comparison of cmd_cram_freemux2.cpp:469-497,521-584 has a margin within
 * 1e-9 x max(1, |LL|) is therefore not decided by them but listed, and its contested hypotheses are recomputed in the
 * reference's own arithmetic (cluster states as ordered clamped chains from the read bytes, IEEE operations in the
 * reference's order on the device, glibc log on the host: fmx_exact.hip); record, assignment and counters are patched
 * and the M-step runs again when an assignment changed.  muxgl_fmx_iterate does all of that itself, on one device and on a
 * device group.  near_tie_cells = cells that went through that path, calls_changed = how many of them it decided
 * differently from the kernels, unresolved = listed cells a caller of the sharded phases left open (see below).  Any
 * pointer may be NULL. */
int muxgl_fmx_exact_stats(const muxgl_handle* h, int64_t* near_tie_cells, int64_t* calls_changed, int64_t* unresolved);

/* The same for the sharded phases (muxgl_fmx_iter_*): a listed cell's SNPs are spread over the ranks' M-step ranges, so the
 * caller carries two small exchanges in the iterations where the job-wide count of listed cells (the fourth counter of
 * MUXGL_BUF_STAT after the all-reduce, or the sum of muxgl_fmx_exact_pending over the ranks) is not zero -- after
 * muxgl_fmx_iter_estep + muxgl_fmx_iter_fetch and BEFORE anything overwrites the assignments of the previous iteration
 * the chains are built from (the library keeps its own copy, taken when the E-step started):
 *   1. muxgl_fmx_exact_snps on every rank: the SNPs its listed cells cover (call with out = NULL for the count, then
 *      with room); the caller unites the lists (ascending, unique);
 *   2. muxgl_fmx_exact_rows on every rank with the united list: rows[n][K][3] and owned[n] are filled for the SNPs of the
 *      rank's own M-step range; the caller gathers every row from its owner;
 *   3. muxgl_fmx_exact_finish on every rank with the complete rows: settles the rank's listed cells, patches records,
 *      assignments (also in MUXGL_BUF_CLUST) and the rank's counters; deltas[3] = what it added to (nsingle, namb,
 *      nchanged), *reassigned != 0: an assignment changed.
 * Then the assignments are exchanged again and, if any rank reports a reassignment, muxgl_fmx_iter_mstep is repeated on
 * all.  popscle_amd/freemuxlet.py run_em is the reference driver. */
int muxgl_fmx_exact_pending(const muxgl_handle* h, int64_t* cells);
/* A settled cell is not listed again while its inputs last: the library keeps the exact scan results per cell and
 * fmx_call_kernel takes them from there as long as no assignment has changed anywhere since (a converged job pays nothing
 * for its near ties).  muxgl_fmx_iterate knows that from its own counters; a caller of the phases says so after every
 * iteration with the JOB-WIDE number of changed cells (after the exact path) -- without this call every E-step starts
 * afresh, which is always correct. */
int muxgl_fmx_exact_hint(muxgl_handle* h, int32_t nchanged_jobwide);
int muxgl_fmx_exact_snps(muxgl_handle* h, int32_t* out, int64_t cap, int64_t* n);
int muxgl_fmx_exact_rows(muxgl_handle* h, const muxgl_fmx_params* p, const int32_t* snps, int64_t n, double* rows,
                         uint8_t* owned);
int muxgl_fmx_exact_finish(muxgl_handle* h, const muxgl_fmx_params* p, const int32_t* snps, int64_t n, const double* rows,
                           int64_t* deltas, int32_t* reassigned);

/* cluster pileups for the .clust1.vcf.gz writer (cmd_cram_freemux2.cpp:608-658): gls[K][S][9], counts[K][S][3] */
int muxgl_fmx_get_cluster_pileup(muxgl_handle* h, double* gls, int32_t* counts);

/* Which cluster is which donor: the cluster pileups scored against the donors' genotypes, demuxlet's singlet likelihood
 * (cmd_cram_demuxlet.cpp:733-747) with a cluster in the place of a droplet.  With gls[K][S][9], counts[K][S][3]
 * exactly as muxgl_fmx_get_cluster_pileup returns them at the moment of the call, gp[S][V][3] / has_gp[S] of
 * muxgl_demux_set_gp and af[S] of muxgl_fmx_prepare:
 *   U(k)      = { s : has_gp[s] != 0 and counts[k][s][0] > 0 }
 *   L_g       = gls[k][s][4 g], g = 0, 1, 2   (the diagonal, as the E-step reads it, cmd_cram_freemux2.cpp:402-404)
 *   ll[K][V]  = sum over s in U(k) of log(L_0 gp[s][v][0] + L_1 gp[s][v][1] + L_2 gp[s][v][2])
 *   ll0[K]    = sum over s in U(k) of log(L_0 (1-af)(1-af) + L_1 2 af (1-af) + L_2 af af)   (gp0s of :388-390: an unrelated
 *               individual), so ll[k][v] - ll0[k] is the log Bayes factor "cluster k is donor v" against "somebody from
 *               the population": positive for a match
 *   nsnps[K]  = |U(k)|
 * A cluster without cells has U = {}: ll = ll0 = 0, nsnps = 0.  A factor that is exactly 0 makes that score -inf, never
 * NaN.  Membership in U is decided by has_gp and the read count, never by the content of a gp row (the device copy holds
 * (1,0,0) in the rows of markers without genotypes).  Any output may be NULL (all three: the call succeeds and writes
 * nothing).  kernel_ms (NULL allowed) receives the hipEvent time of the call's kernels, from a pair of events the call
 * creates and destroys itself: no slot of muxgl_get_timing / muxgl_get_timing_sum is touched and the call is not a
 * collecting one.
 * It needs muxgl_set_pileup, muxgl_fmx_prepare, muxgl_fmx_set_clusters (from then on the pileups exist) and
 * muxgl_demux_set_gp (after the muxgl_set_pileup in force) on the same handle, and scores the pileups as they are now:
 * after muxgl_fmx_set_clusters the initial ones, after muxgl_fmx_iterate what .clust1.vcf.gz prints.  1 <= K <=
 * MUXGL_MAX_CLUSTERS, 1 <= V <= MUXGL_MAX_SAMPLES.  One device, whole pileup: it fails, naming the reason and leaving the
 * handle usable, on a device group, a slabbed handle and a handle whose muxgl_fmx_set_shard range is not everything (their
 * cluster pileups are cut by SNP range, and ranges summed in rank order would round differently), for a NULL handle and
 * when one of the four prerequisites is missing.
 * It reads state and changes none: records, counters, assignments, cluster pileups, MUXGL_BUF_CGP, the near-tie
 * bookkeeping and whether muxgl_fmx_singlets / muxgl_fmx_inclusion may run stay bit for bit what they were.  Under
 * MUXGL_FLAG_ASYNC_PHASES it returns with the stream drained.
 * The values are the device's arithmetic (products of factors, one log per cluster, donor and part of 2048 consecutive
 * SNPs, the parts added in ascending SNP order: equal to the sums of logs to ~1e-11).  Device memory beyond the inputs is
 * per cluster of a batch: those logs, the read counts of its S markers and its results; batches of clusters are sized to
 * the streamed E-step's budget (4 GiB or a third of the device, MUXGL_FMX_SLAB_MB) and each is copied out before the next;
 * nothing proportional to K x S x V.  All three outputs are bit-identical from call to call and for any budget. */
int muxgl_fmx_match_donors(muxgl_handle* h, double* ll /*[K][V]*/, double* ll0 /*[K]*/, int32_t* nsnps /*[K]*/, float* kernel_ms);

/* Did the run split one donor over two clusters: every pair of cluster pileups scored as "one individual" against "two
 * unrelated individuals", the pairwise Bayes factor of freemuxlet-old (cmd_cram_freemuxlet.cpp:186-221, dropD.llk2, .llk0,
 * .nsnps) with clusters in the place of droplets.  The pair a > b is stored at a (a - 1) / 2 + b, the indexing of
 * muxgl_dropd.  With gls[K][S][9], counts[K][S][3] exactly as muxgl_fmx_get_cluster_pileup returns them at the moment of
 * the call and af[S] of muxgl_fmx_prepare:
 *   U(k)       = { s : counts[k][s][0] > 0 },  L_k,g = gls[k][s][4 g],  p = ((1-af)^2, 2 af (1-af), af^2)   (gps, :200-203)
 *   nsnps[a,b] = |U(a) n U(b)|
 *   llk2[a,b]  = sum over s in U(a) n U(b) of log( sum_g p_g L_a,g L_b,g )                         (lk2 of :206)
 *   llk0[a,b]  = sum over the same s of log( sum_gi sum_gj p_gi p_gj L_a,gi L_b,gj )               (lk0 of :208), formed as
 *                (sum_g p_g L_a,g) (sum_g p_g L_b,g)
 * llk2 - llk0 is the log Bayes factor "a and b are one donor" against "two unrelated donors": positive for a split donor
 * (the reference's threshold is --bf-thres, 5.41).
 * The rules of muxgl_fmx_match_donors carry over word for word.  A cluster without cells has U = {}: each of its pairs
 * gets 0, 0, 0.  K = 1 has no pair and the call succeeds.  No NaN and no +inf; a factor that is exactly 0 gives -inf,
 * which cannot arise for af in [0, 1] because the merge clamps every pileup element to 1e-6.  Any output may be NULL (all
 * three: the call succeeds and writes nothing).  kernel_ms (NULL allowed) receives the hipEvent time of the call's
 * kernels, from a pair of events the call creates and destroys itself: no slot of muxgl_get_timing /
 * muxgl_get_timing_sum is touched and the call is not a collecting one.
 * It needs muxgl_set_pileup, muxgl_fmx_prepare and muxgl_fmx_set_clusters on the same handle (no GP tensor), and scores
 * the pileups as they are now.  One device, whole pileup: it fails, naming the reason and leaving the handle usable, on a
 * device group, a slabbed handle and a handle whose muxgl_fmx_set_shard range is not everything (their cluster pileups are
 * cut by SNP range, and ranges summed in rank order would round differently), for a NULL handle and when one of the three
 * prerequisites is missing.
 * It reads state and changes none: records, counters, assignments, cluster pileups, MUXGL_BUF_CGP, the near-tie
 * bookkeeping and whether muxgl_fmx_singlets / muxgl_fmx_inclusion may run stay bit for bit what they were.  Under
 * MUXGL_FLAG_ASYNC_PHASES it returns with the stream drained.
 * The values are the device's arithmetic (products of factors, one log per pair, product and part of 2048 consecutive
 * SNPs, the parts added in ascending SNP order).  Device memory beyond the inputs: one membership bit per (SNP, cluster),
 * one block of 64 partner clusters packed as 1536 S bytes, the triangle of results (20 bytes per pair), and per row cluster
 * of a batch the logs and counts of its parts, batches sized to the streamed E-step's budget (MUXGL_FMX_SLAB_MB); nothing
 * proportional to K x K x S.  All three outputs are bit-identical from call to call, for any budget and tile size
 * (MUXGL_FMX_PAIRS_TILE). */
int muxgl_fmx_cluster_pairs(muxgl_handle* h, double* llk2 /*[K(K-1)/2]*/, double* llk0 /*[K(K-1)/2]*/,
                            int32_t* nsnps /*[K(K-1)/2]*/, float* kernel_ms);

/* ---- freemuxlet-old (`popscle freemuxlet-old`, cmd_cram_freemuxlet.cpp): the parts that differ from freemux2.  The
 *      entry pileups, scores and the EM loop are the calls above (geno_error = 0 except in the tenth and last
 *      iteration, no early stop: cmd_cram_freemuxlet.cpp:457,485,500); what is particular to the old command is its
 *      initial clustering from a pairwise droplet distance matrix.  rand() and std::random_shuffle stay with the
 *      caller, which passes the visiting orders and the vote jitters in the reference's drawing order. ------------- */

/* dropD (sc_drop_seq.h:45-52) of the cell pair a > b, stored at a(a-1)/2 + b */
typedef struct {
  int32_t nsnps, nread1, nread2, _pad;
  double llk0, llk2;
} muxgl_dropd;

/* pairwise distance matrix, cmd_cram_freemuxlet.cpp:176-221, after muxgl_fmx_prepare.  The device keeps one vote sign
 * per ordered pair (+1: llk2 - llk0 > bf_thres, -1: llk0 - llk2 > bf_thres, :273-278,312-313; C^2 bytes).
 * full: NULL or [C(C-1)/2] records (what --aux-files prints to .ldist.gz, :264, and what parity tests compare). */
int muxgl_fmxold_pair_dist(muxgl_handle* h, double bf_thres, muxgl_dropd* full);

/* the sign matrix as [C][C] bytes (tests) */
int muxgl_fmxold_get_signs(muxgl_handle* h, int8_t* out);

/* first-pass voting, cmd_cram_freemuxlet.cpp:245-291.  order[C] = drops_srted (muxgl_fmx_greedy_init's sort order:
 * score descending, ties by id descending); jitter[n_visited][K] = the values `rand()/(RAND_MAX+1.)/1000.` drawn for
 * the visited cells (:257-259).  clust_out[C]: cluster, or -1 for cells beyond frac_init_clust; ccounts: NULL or [K].
 * K <= 64. */
int muxgl_fmxold_vote_init(muxgl_handle* h, int32_t K, const int32_t* order, const double* jitter,
                           double frac_init_clust, int32_t* clust_out, int32_t* ccounts);

/* one refinement pass, cmd_cram_freemuxlet.cpp:297-343 (one value of `iter`).  order[C] = orand after
 * std::random_shuffle (:301-302), jitter[C][K] in visiting order.  clust_inout[C] is updated in place; changed and
 * ccounts[K] as the reference reports them (:346-349). */
int muxgl_fmxold_vote_refine(muxgl_handle* h, int32_t K, const int32_t* order, const double* jitter,
                             int32_t keep_init_missing, int32_t* clust_inout, int32_t* changed, int32_t* ccounts);

/* ---- sharded EM: one handle per rank (one process per GPU, popscle_amd/freemuxlet.py; a device group does the same
 *      inside one process, see muxgl_config).  Rank r owns a cell range [c0,c1) for the E-step / scans / re-assignment
 *      and a SNP range [s0,s1) for the cluster GP rows and the ordered M-step (a chain per (cluster, SNP) in ascending
 *      cell id with a clamp after every merge, sc_drop_seq.h:77-101: not an associative reduction, so exactly one rank
 *      evaluates it).  One iteration =
 *          iter_gp -> all-gather MUXGL_BUF_CGP slices [s0*K*3, s1*K*3) -> iter_estep -> all-gather MUXGL_BUF_CLUST
 *          slices [c0,c1) (+ sum of the three counters) -> iter_mstep.
 *      The collectives are the caller's (RCCL over xGMI via torch.distributed in this repo); muxgl_fmx_buffer exposes
 *      the device buffers they run on, muxgl_stream the stream the phases are enqueued on.  Both buffers have
 *      MUXGL_XCHG_PAD units of slack behind them, so equal slices of ceil(n / ranks) units can be gathered in place.
 *      With the full ranges the phases reproduce muxgl_fmx_iterate bit for bit.
 *
 *      What a rank holds, two ways:
 *        a) slabs -- muxgl_set_pileup(row slab: the rank's cells [c0,c1) with every SNP, cells renumbered from 0) then
 *           muxgl_fmx_set_column_slab(column slab: all C_total cells, only the entries with s0 <= SNP < s1, SNP ids
 *           unchanged), then muxgl_fmx_prepare / muxgl_fmx_set_clusters(clust[C_total]) / the phases.  Device memory
 *           and H2D traffic are 2/ranks of the pileup.  Per-cell outputs (prepare's scores, iter_fetch's records) cover
 *           the rank's own cells [C = c1-c0]; MUXGL_BUF_CLUST is job-wide [C_total], MUXGL_BUF_CGP is [S][K][3];
 *           muxgl_fmx_get_cluster_pileup returns the rows of [s0,s1) and zeros elsewhere.
 *        b) the whole pileup on every rank + muxgl_fmx_set_shard(c0,c1,s0,s1) after muxgl_fmx_prepare (simple, but every
 *           rank uploads and keeps everything; kept for callers that hold the whole pileup anyway). ------------------- */
enum { MUXGL_BUF_CGP = 0 /* f64[S][K][3] */, MUXGL_BUF_CLUST = 1 /* i32[C_total] */, MUXGL_BUF_CELLS = 2 /* muxgl_fmx_cell[C] */,
       MUXGL_BUF_STAT = 3 /* i32[4]: nsingle, namb, nchanged of the local cell range */ };
#define MUXGL_XCHG_PAD 64
int muxgl_fmx_set_column_slab(muxgl_handle* h, int64_t C_total, int64_t c0, int64_t s0, int64_t s1, int64_t nnz_s,
                              int64_t R_s, const int64_t* cell_ptr_s /*[C_total+1]*/, const int32_t* entry_snp_s,
                              const int64_t* entry_rptr_s, const uint8_t* reads_s);
int muxgl_fmx_set_shard(muxgl_handle* h, int64_t c0, int64_t c1, int64_t s0, int64_t s1);
int muxgl_fmx_iter_gp(muxgl_handle* h, const muxgl_fmx_params* p);
int muxgl_fmx_iter_estep(muxgl_handle* h, const muxgl_fmx_params* p);
int muxgl_fmx_iter_mstep(muxgl_handle* h);
/* counters of the last E-step and, when out / full_ll are given, the records / E-step tensor of the own cells.  With
 * out == NULL and full_ll == NULL it waits for the counters only (work enqueued behind the E-step keeps running). */
int muxgl_fmx_iter_fetch(muxgl_handle* h, muxgl_fmx_cell* out, int32_t* nsingle, int32_t* namb, int32_t* nchanged,
                         double* full_ll);
int muxgl_fmx_buffer(muxgl_handle* h, int32_t which, void** dev_ptr, int64_t* n_elems);
int muxgl_memcpy_dev(muxgl_handle* h, void* dst_dev, const void* src_dev, int64_t bytes);
/* the hipStream_t every kernel of this handle is enqueued on (NULL for a device group) */
void* muxgl_stream(const muxgl_handle* h);

/* ---- measurement --------------------------------------------------------------------------------------------- */
/* ms[MUXGL_T_COUNT]: hipEvent durations of the kernels of the most recent run/iterate call (0 where not run) */
int muxgl_get_timing(const muxgl_handle* h, float* ms);
/* ms_sum[MUXGL_T_COUNT]: the same durations summed since the last reset -- every event bracket is added exactly once,
 * whichever entry point collects it -- and `calls`, the number of collecting calls: one per muxgl_demux_run /
 * muxgl_fmx_iterate, and with the phased API one per phase that reads its brackets back (iter_gp, iter_estep,
 * iter_mstep; under MUXGL_FLAG_ASYNC_PHASES only an iter_fetch that drains the stream).  Either pointer may be NULL;
 * reset != 0 clears both afterwards.  For loops that time many calls without a fetch per call.  One-device handles. */
int muxgl_get_timing_sum(muxgl_handle* h, double* ms_sum, int64_t* calls, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
