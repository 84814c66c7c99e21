// fmx_singlets.hip -- muxgl_fmx_singlets: the [C][K] table of singlet log-likelihoods, llks[j(j+1)/2 + j] of
// cmd_cram_freemux2.cpp:448-455 for every droplet and every cluster (the numbers sngBestLLK / sngNextLLK are scanned from,
// :485-497), as the last E-step of the handle formed them.
//
//   sng[c][j] = sum over the entries e of c of log( egl_e[0] q[s_e][j][0] + egl_e[4] q[s_e][j][1] + egl_e[8] q[s_e][j][2] )
//
// egl_e: the nine entry likelihoods of muxgl_fmx_prepare (d_egls); q: the cluster genotype posteriors the last E-step read
// (d_cgp, [S][K][3], geno_error mixed in, :402-415).  Nothing between that E-step and the next posterior phase writes
// d_cgp: the M-step (fmx_mstep.hip) rewrites the cluster pileups, the exact path (fmx_exact.hip) builds its own rows,
// a device group's and the sharded driver's exchanges after the E-step move assignments only.  h->fmx_sng_state says
// whether d_cgp still is what an E-step read (fmx_kernels.hip sets it).
//
// Two kernels (the design of demux_singlets.hip; the entry's weights are the diagonal of its likelihoods, so there is
// no weight kernel):
//   * fsg_sweep_kernel, lane = cluster: f = q_0 d_0 + q_1 d_1 + q_2 d_2 per (entry, cluster), multiplied into a product
//     kept as mantissa x 2^exponent (prodacc), one log per (cell part, cluster).  A wave is one work unit: a part of a
//     cell x a block of 64 clusters, the entry wave-uniform (its diagonal comes through scalar loads).  Below 64 clusters
//     a wave holds G = 64 / KH entries side by side (KH = K rounded up to a power of two, lane = (entry slot, cluster))
//     and the G partial products of a cluster are multiplied in a fixed butterfly at the end.
//   * table_join_kernel (table_call.hpp): the logs of the parts of a long cell, added in entry order.
// Which cell goes into which batch, its cut into parts (the equal parts of the wave plan, as fmx_stream.hip's
// sweep_block cuts a cell) and the order of the work items are table_plan.hpp's; the host body that drives the plan is
// table_call.hpp's table_batches, whose customer this unit is (one bracket in its timing slot).  The cut depends on the cell alone and
// every reduction tree is fixed: the table is bit-identical from call to call, for any slab budget, on one device, on a
// group and through the sharded driver.
//
// The diagonal is read straight from d_egls (3 of 9 doubles at a 72-byte stride; DESIGN.md 4.2c has the measurement
// against a packed [nnz][3] copy, a path that is gone).
//
// Memory: a slab of the table (the streamed E-step's budget: 4 GiB or a third of the device, MUXGL_FMX_SLAB_MB) and the
// work items.  When the table exceeds the budget the cells are swept in batches (table_call.hpp has the protocol).
// Nothing proportional to C x K^2.
#include <algorithm>
#include <vector>

#include "table_call.hpp"

namespace {

// Entries per lane between two renormalisations, all of their loads in flight.  The smallest factor this path can see:
// a factor is a combination sum_l q_l d_l of the entry's diagonal with a posterior triple that sums to 1 (within a few
// ulp, with or without the geno_error mixing of :402-415: a single q_l may be tiny or exactly 0 at geno_error = 0, their
// sum may not), so f >= min_l d_l, and every entry likelihood leaves calculate_snp_droplet_pileup clamped to
// MIN_NORM_GL = 1e-6 and divided by a sum <= 1 + 9e-6 (sc_drop_seq.cpp:498-504): f >= 9.9999e-7 > 2^-20.  A mantissa
// in [0.5, 1) times N such factors is >= 2^(-1 - 20 N): normal up to N = 51.  Eight is what the registers hold in
// flight at <= 128 VGPRs; it leaves 2^-161.  A factor of exactly 0 (posterior rows that were never filled) makes the
// product 0 and the log -inf, the reference's log(0) chain; frexp(0) = 0, so no NaN on the way.
constexpr int FSG_UNR = 8;

using fsg_item = table_plan::item;  // the entries [e0, e1) of one cell, result row `row` of the slab

// grid: ceil(n_items * nblk / 4) workgroups of four waves; wave u <-> (item u / nblk, cluster block u % nblk), so the
// waves of a workgroup walk the same entries and read neighbouring pieces of the same posterior rows.
// diag is d_egls, [nnz][9], the diagonal at 0, 4, 8.
template <int KH>
__global__ void __launch_bounds__(256)
    fsg_sweep_kernel(int64_t n_units, int nblk, const fsg_item* __restrict__ items, const int32_t* __restrict__ entry_snp,
                     const double* __restrict__ diag, const double* __restrict__ cgp, int K, double* __restrict__ slab) {
  constexpr int G = 64 / KH;  // entries side by side in a wave
  constexpr int DS = 9, D1 = 4, D2 = 8;
  const int64_t u = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (u >= n_units) return;
  const int64_t it = u / nblk;
  const int blk = (int)(u - it * nblk);
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / KH;  // entry slot of the lane
  const int j = G == 1 ? blk * 64 + lane : lane % KH;
  const bool jl = j < K;
  const size_t jo = (size_t)(jl ? j : K - 1) * 3;
  const int64_t e0 = items[it].e0, e1 = items[it].e1;
  const size_t K3 = (size_t)K * 3;

  double acc = 1.0;
  int32_t ex = 0;
  for (int64_t eb = e0; eb < e1; eb += (int64_t)FSG_UNR * G) {
    double f[FSG_UNR];
#pragma unroll
    for (int i = 0; i < FSG_UNR; ++i) {
      const int64_t e = eb + (int64_t)i * G + sub;
      const bool ok = e < e1;
      const int64_t ec = ok ? e : e1 - 1;  // (a slot past the end reads the last entry again and counts as 1)
      const double* d = diag + (size_t)ec * DS;
      const double* q = cgp + (size_t)entry_snp[ec] * K3 + jo;
      const double v = fma(q[2], d[D2], fma(q[1], d[D1], q[0] * d[0]));  // :448-451
      f[i] = ok ? v : 1.0;
    }
#pragma unroll
    for (int i = 0; i < FSG_UNR; ++i) acc *= f[i];
    prodacc_renorm(acc, ex);
  }
  if (G > 1) {  // the G partial products of a cluster, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
    for (int off = KH; off < 64; off <<= 1) {
      acc *= __shfl_xor(acc, off, 64);
      ex += __shfl_xor(ex, off, 64);
    }
  }
  if (jl && sub == 0) slab[(size_t)items[it].row * K + j] = prodacc_log(acc, ex);
}

template <int KH>
void launch_sweep(muxgl_handle* h, int64_t n_items, int nblk, const fsg_item* d_items, double* d_slab) {
  const int64_t n_units = n_items * nblk;
  hipLaunchKernelGGL((fsg_sweep_kernel<KH>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, nblk,
                     d_items, h->d_entry_snp, h->d_egls, h->d_cgp, h->K, d_slab);
}

int fmx_singlets_run(muxgl_handle* h, double* sng) {
  const int K = h->K, nblk = (K + 63) / 64, KH = lane_width(K);
  const table_call call = {"muxgl_fmx_singlets", "MUXGL_FMX_SLAB_MB", table_plan::equal_begin, (double)nblk, 0.0, 0.0,
                           table_plan::shape(K, "clusters"), ""};
  table_batches<table_plan::cut> tb;
  if (tb.plan(h, call, [K](int64_t, int64_t np) { return table_plan::singlet_bytes(np, K); })) return 1;

  dev_tmp<double> d_slab;
  if (dev_alloc(h, &d_slab.p, (size_t)tb.bt.max_rows * K)) return 1;
  tic(h, MUXGL_T_FMX_SINGLETS);
  return tb.run(h, table_slot_timer{MUXGL_T_FMX_SINGLETS},
      [&](const table_batch<table_plan::cut>& b) {
#define CALL_S(W) launch_sweep<W>(h, b.n_items, nblk, b.d_items, d_slab.p)
        DISPATCH_WIDTH(KH, CALL_S);
#undef CALL_S
        HIPCHK(h, hipGetLastError());
        return table_join(h, b, K, d_slab.p);
      },
      [&](const table_batch<table_plan::cut>& b) {
        HIPCHK(h, hipMemcpyAsync(sng + (size_t)b.c0 * K, d_slab.p, sizeof(double) * (size_t)b.nc() * K, hipMemcpyDeviceToHost, h->stream));
        return 0;
      });
}

}  // namespace

extern "C" int muxgl_fmx_singlets(muxgl_handle* h, double* sng) {
  if (!h) return 1;
  if (h->group) return group_fmx_singlets(h, sng);
  HIPCHK(h, hipSetDevice(h->device));
  if (fmx_refuse(h, h, "muxgl_fmx_singlets", "the table belongs")) return 1;
  if (!sng) MUXGL_FAIL(h, "muxgl_fmx_singlets: NULL output");
  if (h->C == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing: the slots of the last iteration keep their values)
  if (fmx_singlets_run(h, sng)) return 1;
  collect_timing(h);
  return 0;
}
