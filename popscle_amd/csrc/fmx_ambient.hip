// fmx_ambient.hip -- muxgl_fmx_ambient: every droplet scored as ONE cell of cluster j plus a share rho of ambient RNA, the
// freemuxlet counterpart of demux_ambient.hip.  The ambient RNA is no donor: where the second cluster's genotype stands in
// calculate_snp_droplet_pileup (sc_drop_seq.cpp:452-509, alpha = 0.5), its "genotype" at marker s is twice the pool's ALT
// fraction f[s], any number in [0, 2], and its share is rho instead of one half.  Per entry e, with the nine products of
// the reference carried along unchanged:
//
//   p(l, f, rho)    = 0.5 l + (2 f - l) 0.5 rho                 formed as fma(2 f - l, 0.5 rho, 0.5 l)
//   per usable read, in read order:
//       nine[i] *= mat frac_i + e4                              :483-491, as fmx_entry_kernel forms them
//       a[r][l] *= mat (ALT read ? p : 1 - p) + e4
//       t = nine[0] + ... + nine[8];  nine and a are all multiplied by 1 / t            :493-494
//   after the reads every element of nine and of a below 1e-6 becomes 1e-6 (:498-501, sc_drop_seq.h:14)
//       T = sum of the floored nine;  w_e[r][l] = a[r][l] (1 / T)                        :502-504
//   ll_amb[c][j][r] = sum over the entries e of droplet c of
//                     log( (q[s_e][j][0] w_e[r][0] + q[s_e][j][1] w_e[r][1]) + q[s_e][j][2] w_e[r][2] )
//
// q is d_cgp, the posteriors the last E-step read (muxgl_fmx_singlets' rule).  The ambient products take part in none of
// the sums t and T: those are the numbers behind d_egls, so the table is on the scale of the records' log-likelihoods.
// With f in {0, 1/2, 1} and rho = 0.5, p is (l + 2 f) / 4 exactly and w_e[l] is the entry's gls[3 l + 2 f]; with rho = 0
// w_e[l] is gls[4 l] (the singlet table); with rho = 1 p is f for every l.
//   * fam_weight_kernel, lane = entry: the nine exactly as fmx_entry_kernel forms them (the same operations in the same
//     order, its reciprocal-multiply included) and beside them 3 x RC ambient products through the same reads.  The rhos
//     are swept in passes of RC (4, 8 or 16); every pass repeats the nine identically and every ambient product belongs
//     to one rho, so the passes change no bit: 24 bytes per entry and rho.
//   * fam_sweep_kernel, lane = cluster of a 64-cluster block: one dot q_j . w_e[r] per (entry, cluster, rho), multiplied
//     into a product kept as mantissa x 2^exponent, one log per (cell part, cluster, rho).  A wave is one work unit: a
//     part of a cell (at most 2048 entries) x a block x a chunk of CH <= 4 rhos.  Every accumulator belongs to one rho,
//     so this chunking changes no bit either.  Below 64 clusters a wave holds G = 64 / KH entries side by side,
//     multiplied in a fixed xor butterfly at the end.
//   * fam_emit_kernel: the logs of the parts of a cell added in entry order and written in the caller's layout.
// Which cell goes into which batch, its cut into parts (the equal parts of the wave plan, as muxgl_fmx_singlets cuts a
// cell) and the order of the work items are table_plan.hpp's.  The cut of a cell depends on the cell alone and every
// reduction tree is fixed: the table is bit-identical from call to call, for any budget, for any split of the rhos over
// calls, on one device, on a group and through the sharded driver.
//
// Memory: nothing proportional to nnz x n_rho is held for the whole pileup.  Cells are swept in batches of whole cells
// whose weights ([entries][n_rho][3]), slab rows and table rows (table_plan::fmx_ambient_bytes) fit the streamed E-step's
// budget (4 GiB or a third of the device, MUXGL_FMX_SLAB_MB); each batch is copied out before the next.  The call caches
// nothing on the handle.
#include <algorithm>
#include <cmath>
#include <vector>

#include "table_call.hpp"

namespace {

constexpr double kMinNormGL = 1e-6;  // sc_drop_seq.h:14
constexpr int FAM_MAX_RHO = 16;

struct fam_grid {
  double a[FAM_MAX_RHO];
};
using fam_item = table_plan::item;  // the entries [e0, e1) of one cell, result row `row` of the slab
// the further parts of a cell: its value = slab[cell row] + slab[first] + ... + slab[first + count - 1], in this order
using fam_cell = table_plan::cell;

// wt[(e - eb0)][r][0..2] = w_e[r][l], for the entries [eb0, eb1) of a batch
template <int RC>
__global__ void __launch_bounds__(256)
    fam_weight_kernel(int64_t eb0, int64_t eb1, int NR, const int32_t* __restrict__ entry_snp,
                      const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                      const double* __restrict__ lut_g, fam_grid rh, const double* __restrict__ af, double* __restrict__ wt) {
  __shared__ double lut[256];
  lut[threadIdx.x] = lut_g[threadIdx.x];
  __syncthreads();
  const int64_t e = eb0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= eb1) return;
  double* o = wt + (size_t)(e - eb0) * NR * 3;
  const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
  // p = fma(2 f - l, 0.5 rho, 0.5 l): exactly 0 at (l = 0, f = 0) and exactly 1 at (l = 2, f = 1), so those corners
  // carry e4 and mat + e4 themselves, as gls[0] and gls[8] do
  const double f = af[entry_snp[e]];
  const double tf = f + f;
  const double tf1 = tf - 1.0, tf2 = tf - 2.0;
  for (int rb = 0; rb < NR; rb += RC) {
    double gls[9], am[RC * 3];
#pragma unroll
    for (int i = 0; i < 9; ++i) gls[i] = 1.0;
#pragma unroll
    for (int i = 0; i < RC * 3; ++i) am[i] = 1.0;
    for (int64_t r = r0; r < r1; ++r) {
      const uint32_t b = reads[r];
      if (b == MUXGL_READ_OTHER) continue;  // :468
      const uint32_t al = b >> 7, bq = b & 0x7f;
      const double mat = lut[128 + bq], e4 = lut[bq] / 4.;
      // the nine, operation for operation those of fmx_entry_kernel (:472-494)
      const double fr[9] = {1.0, .75, .5, .75, .5, .25, .5, .25, 0.0};
      double tmp = 0.0;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double fi = (al == 0) ? fr[i] : fr[8 - i];
        gls[i] *= (mat * fi + e4);
        tmp += gls[i];
      }
      const double inv = 1.0 / tmp;
#pragma unroll
      for (int i = 0; i < 9; ++i) gls[i] *= inv;
#pragma unroll
      for (int k = 0; k < RC; ++k) {
        const double hr = 0.5 * rh.a[rb + k];  // (rb + k < 16: a slot past the end holds the last rho again)
        const double p0 = tf * hr, p1 = fma(tf1, hr, 0.5), p2 = fma(tf2, hr, 1.0);
        const double x0 = (al == 0) ? 1.0 - p0 : p0;
        const double x1 = (al == 0) ? 1.0 - p1 : p1;
        const double x2 = (al == 0) ? 1.0 - p2 : p2;
        am[k * 3 + 0] *= (mat * x0 + e4);
        am[k * 3 + 1] *= (mat * x1 + e4);
        am[k * 3 + 2] *= (mat * x2 + e4);
      }
#pragma unroll
      for (int i = 0; i < RC * 3; ++i) am[i] *= inv;
    }
    double tmp = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (gls[i] < kMinNormGL) gls[i] = kMinNormGL;  // :498-501
      tmp += gls[i];
    }
    const double inv = 1.0 / tmp;
#pragma unroll
    for (int k = 0; k < RC; ++k)
      if (rb + k < NR) {
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          double a = am[k * 3 + l];
          if (a < kMinNormGL) a = kMinNormGL;
          o[(rb + k) * 3 + l] = a * inv;
        }
      }
  }
}

// Entries per lane between two renormalisations, all of their loads in flight.  The smallest factor this path can see:
// every weight w_e[r][l] is floored at MIN_NORM_GL = 1e-6 and divided by T, the sum of the nine floored likelihoods, which
// is <= 1 + 9e-6 (sc_drop_seq.cpp:498-504): w >= 9.9999e-7 > 2^-20.  A factor is a combination sum_l q_l w_l of the
// weights with a posterior triple that sums to 1 (within a few ulp, with or without the geno_error mixing of :402-415: a
// single q_l may be tiny or exactly 0 at geno_error = 0, their sum may not), so f >= min_l w_l > 2^-20.  A mantissa in
// [0.5, 1) times N such factors is >= 2^(-1 - 20 N): normal up to N = 51; eight leave 2^-161.  Upwards an
// ambient product can exceed the nine's maximum only by the modest factor by which the best p of the entry is off the
// reference's grid, per read, and an entry has at most a few hundred reads: no overflow of a double in eight factors.
// A factor of exactly 0 (posterior rows that were never filled) makes the product 0 and the log -inf; frexp(0) = 0, so
// no NaN on the way.
//
// grid: ceil(n_units / 4) workgroups of four waves; wave unit <-> (item, cluster block, rho chunk), the chunk fastest,
// so the waves of a workgroup walk the same entries and read the same or neighbouring pieces of the posterior rows.
// slab[row][r][K]
template <int KH, int CH>
__global__ void __launch_bounds__(256)
    fam_sweep_kernel(int64_t n_units, int nblk, int nch, int NR, const fam_item* __restrict__ items,
                     const int32_t* __restrict__ entry_snp, int64_t eb0, const double* __restrict__ wt,
                     const double* __restrict__ cgp, int K, double* __restrict__ slab) {
  constexpr int G = 64 / KH;            // entries side by side in a wave
  // entries per lane between two renormalisations (see above: 8 are safe), as many as 128 VGPRs hold in flight: below 64
  // clusters the weights come through vector loads, and four rhos of four entries would take 134.  Every lane walks the
  // entries sub, sub + G, ... of its part whatever UNR is, and a renormalisation moves powers of two only: UNR changes no bit
  constexpr int UNR = CH == 1 ? 8 : (CH == 4 && KH < 64) ? 3 : 4;
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int ch = (int)(unit % nch);
  const int64_t rest = unit / nch;
  const int blk = (int)(rest % nblk);
  const int64_t it = rest / nblk;
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / KH;  // entry slot of the lane
  const int j = G == 1 ? blk * 64 + lane : lane % KH;
  const bool jl = j < K;
  const size_t jo = (size_t)(jl ? j : K - 1) * 3;
  const size_t K3 = (size_t)K * 3;
  const int64_t e0 = items[it].e0, e1 = items[it].e1;
  int rr[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) rr[c] = ch * CH + c < NR ? ch * CH + c : NR - 1;  // (a slot past the end repeats the last rho)

  double acc[CH];
  int32_t ex[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    acc[c] = 1.0;
    ex[c] = 0;
  }
  for (int64_t eb = e0; eb < e1; eb += (int64_t)UNR * G) {
    double f[UNR][CH];
#pragma unroll
    for (int i = 0; i < UNR; ++i) {
      const int64_t e = eb + (int64_t)i * G + sub;
      const bool ok = e < e1;
      const int64_t ec = ok ? e : e1 - 1;  // (a slot past the end reads the last entry again and counts as 1)
      const double* q = cgp + (size_t)entry_snp[ec] * K3 + jo;
      const double q0 = q[0], q1 = q[1], q2 = q[2];
      const double* we = wt + (size_t)(ec - eb0) * NR * 3;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const double* w = we + rr[c] * 3;
        const double v = fma(q2, w[2], fma(q1, w[1], q0 * w[0]));
        f[i][c] = ok ? v : 1.0;
      }
    }
#pragma unroll
    for (int i = 0; i < UNR; ++i)
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] *= f[i][c];
#pragma unroll
    for (int c = 0; c < CH; ++c) prodacc_renorm(acc[c], ex[c]);
  }
  if (G > 1) {  // the G partial products of a cluster, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
    for (int off = KH; off < 64; off <<= 1)
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        acc[c] *= __shfl_xor(acc[c], off, 64);
        ex[c] += __shfl_xor(ex[c], off, 64);
      }
  }
  if (jl && sub == 0) {
    double* out = slab + (size_t)items[it].row * NR * K + j;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (ch * CH + c < NR) out[(size_t)rr[c] * K] = prodacc_log(acc[c], ex[c]);
  }
}

// lane = (cell, cluster, rho), rho fastest: out[nc][K][NR]
__global__ void __launch_bounds__(256)
    fam_emit_kernel(int64_t nc, const fam_cell* __restrict__ cells, int K, int NR, const double* __restrict__ slab,
                    double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc * K * NR) return;
  const int r = (int)(i % NR);
  const int j = (int)((i / NR) % K);
  const int64_t c = i / ((int64_t)NR * K);
  const size_t rs = (size_t)NR * K, off = (size_t)r * K + j;
  const fam_cell ct = cells[c];
  double s = slab[(size_t)c * rs + off];
  for (int64_t k = 0; k < ct.count; ++k) s += slab[(size_t)(ct.first + k) * rs + off];
  out[i] = s;
}

struct fam_batch {  // what one launch of the three kernels needs
  int64_t eb0, eb1, n_items, nc;
  const fam_item* d_items;
  const fam_cell* d_cells;
  double *d_wt, *d_slab, *d_out;
  const double* d_af;
};

template <int RC>
void launch_weights(muxgl_handle* h, int NR, const fam_grid& rh, const fam_batch& b) {
  hipLaunchKernelGGL((fam_weight_kernel<RC>), dim3((unsigned)((b.eb1 - b.eb0 + 255) / 256)), dim3(256), 0, h->stream, b.eb0,
                     b.eb1, NR, h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, rh, b.d_af, b.d_wt);
}

// rhos per pass of the weight kernel: as many as the call has, rounded up to 4, 8 or 16
int weights_dispatch(muxgl_handle* h, int NR, const fam_grid& rh, const fam_batch& b) {
  if (NR > 8)
    launch_weights<16>(h, NR, rh, b);
  else if (NR > 4)
    launch_weights<8>(h, NR, rh, b);
  else
    launch_weights<4>(h, NR, rh, b);
  HIPCHK(h, hipGetLastError());
  return 0;
}

template <int KH, int CH>
void launch_sweep(muxgl_handle* h, int NR, int nch, const fam_batch& b) {
  const int nblk = (h->K + 63) / 64;
  const int64_t n_units = b.n_items * nblk * nch;
  hipLaunchKernelGGL((fam_sweep_kernel<KH, CH>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, nblk,
                     nch, NR, b.d_items, h->d_entry_snp, b.eb0, b.d_wt, h->d_cgp, h->K, b.d_slab);
}

template <int CH>
void sweep_dispatch_kh(muxgl_handle* h, int NR, int nch, const fam_batch& b) {
  int KH = 64;
  while (KH > 1 && KH / 2 >= h->K) KH /= 2;
#define CALL_S(W) launch_sweep<W, CH>(h, NR, nch, b)
  DISPATCH_WIDTH(KH, CALL_S);
#undef CALL_S
}

int sweep_dispatch(muxgl_handle* h, int CH, int NR, int nch, const fam_batch& b) {
  switch (CH) {
    case 1: sweep_dispatch_kh<1>(h, NR, nch, b); break;
    case 2: sweep_dispatch_kh<2>(h, NR, nch, b); break;
    case 3: sweep_dispatch_kh<3>(h, NR, nch, b); break;
    default: sweep_dispatch_kh<4>(h, NR, nch, b); break;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

int fmx_ambient_run(muxgl_handle* h, const double* amb_af, int NR, const double* rho, double* ll_amb, float* kernel_ms) {
  const int K = h->K;
  const int64_t C = h->C, S = h->S;
  std::vector<int64_t> cell_ptr((size_t)C + 1);
  HIPCHK(h, hipMemcpyAsync(cell_ptr.data(), h->d_cell_ptr, sizeof(int64_t) * (size_t)(C + 1), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));

  // batches of whole cells whose device bytes fit the budget (table_plan.hpp)
  const size_t budget = dev_slab_budget("MUXGL_FMX_SLAB_MB");
  auto bytes_of = [&](int64_t len, int64_t np) { return table_plan::fmx_ambient_bytes(len, np, NR, K); };
  const table_plan::batches bt = table_plan::plan(cell_ptr.data(), C, budget, bytes_of);
  if (bt.over >= 0) {
    const int64_t len = cell_ptr[(size_t)bt.over + 1] - cell_ptr[(size_t)bt.over];
    MUXGL_FAIL(h, "muxgl_fmx_ambient: droplet %lld alone (%lld entries x %d rhos x %d clusters: %.1f MB) exceeds the budget "
                  "of %.1f MB (raise MUXGL_FMX_SLAB_MB)",
               (long long)(h->cell_base + bt.over), (long long)len, NR, K,
               (double)bytes_of(len, table_plan::parts(len)) / 1048576.0, (double)budget / 1048576.0);
  }
  const int nblk = (K + 63) / 64;
  const int nch = (NR + 3) / 4, CH = (NR + nch - 1) / nch;  // chunks of the rhos, rhos per chunk (1..4)
  if (table_plan::exceeds_one_launch((double)bt.max_rows * nblk * nch, 4.0) ||
      table_plan::exceeds_one_launch((double)bt.max_cells * K * NR, 256.0))
    MUXGL_FAIL(h, "muxgl_fmx_ambient: a batch of %lld rows x %d clusters x %d rhos exceeds one launch (lower MUXGL_FMX_SLAB_MB)",
               (long long)bt.max_rows, K, NR);
  fam_grid rh;
  for (int i = 0; i < FAM_MAX_RHO; ++i) rh.a[i] = i < NR ? rho[i] : rho[NR - 1];  // (a slot past the end is not written)

  dev_tmp<double> d_af, d_wt, d_slab, d_out;
  dev_tmp<fam_item> d_items;
  dev_tmp<fam_cell> d_cells;
  if (dev_alloc(h, &d_af.p, (size_t)S)) return 1;
  if (dev_alloc(h, &d_wt.p, (size_t)bt.max_entries * NR * 3)) return 1;
  if (dev_alloc(h, &d_slab.p, (size_t)bt.max_rows * NR * K)) return 1;
  if (dev_alloc(h, &d_out.p, (size_t)bt.max_cells * K * NR)) return 1;
  if (dev_alloc(h, &d_items.p, (size_t)bt.max_rows)) return 1;
  if (dev_alloc(h, &d_cells.p, (size_t)bt.max_cells)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, "muxgl_fmx_ambient")) return 1;

  if (S > 0) HIPCHK(h, hipMemcpyAsync(d_af.p, amb_af, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, h->stream));
  std::vector<fam_item> items;
  std::vector<fam_cell> cells;
  int64_t c0 = 0;
  for (const int64_t c1 : bt.end) {
    const int64_t nc = c1 - c0;
    table_plan::fill(cell_ptr.data(), c0, c1, table_plan::equal_begin, items, nullptr, &cells);
    const fam_batch b = {cell_ptr[(size_t)c0], cell_ptr[(size_t)c1], (int64_t)items.size(), nc, d_items.p, d_cells.p,
                         d_wt.p, d_slab.p, d_out.p, d_af.p};
    if (table_upload(h, items, d_items.p, cells, d_cells.p)) return 1;
    if (ev.start(h)) return 1;
    if (b.eb1 > b.eb0 && weights_dispatch(h, NR, rh, b)) return 1;
    if (sweep_dispatch(h, CH, NR, nch, b)) return 1;
    {
      const int64_t n = nc * K * NR;
      hipLaunchKernelGGL(fam_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, nc, d_cells.p, K, NR,
                         d_slab.p, d_out.p);
      HIPCHK(h, hipGetLastError());
    }
    if (ev.stop(h)) return 1;
    HIPCHK(h, hipMemcpyAsync(ll_amb + (size_t)c0 * K * NR, d_out.p, sizeof(double) * (size_t)nc * K * NR, hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ev.add();
    c0 = c1;
  }
  return 0;
}

}  // namespace

// why the handle cannot give the table now (NULL: it can): fmx_unknown_refusal's rules under this call's name; shared with
// the device group
const char* fmx_ambient_refusal(const muxgl_handle* h) {
  if (!h->d_cell_ptr) return "muxgl_fmx_ambient: no pileup set (muxgl_set_pileup)";
  if (!h->fmx_prepared) return "muxgl_fmx_ambient: call muxgl_fmx_prepare first";
  if (h->K < 1) return "muxgl_fmx_ambient: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)";
  if (h->fmx_sng_state == FMX_SNG_NONE)
    return "muxgl_fmx_ambient: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep first)";
  if (h->fmx_sng_state != FMX_SNG_READY)
    return "muxgl_fmx_ambient: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; the table "
           "belongs to an E-step's own posteriors: call it before the next iteration's posterior phase";
  return nullptr;
}

// the caller's arguments, on the host, before any device work: 0, or 1 with the reason in `why` (the handle's message is
// the caller's to set, so that a group's handle carries it)
int fmx_ambient_bad_args(const double* amb_af, int64_t S, int32_t n_rho, const double* rho, double* ll_amb, char* why,
                         size_t why_len) {
  if (!ll_amb) return snprintf(why, why_len, "muxgl_fmx_ambient: NULL output"), 1;
  if (n_rho < 1 || n_rho > FAM_MAX_RHO)
    return snprintf(why, why_len, "muxgl_fmx_ambient: n_rho=%d outside [1,%d]", n_rho, FAM_MAX_RHO), 1;
  if (!rho || !amb_af) return snprintf(why, why_len, "muxgl_fmx_ambient: %s is NULL", rho ? "amb_af" : "rho"), 1;
  for (int r = 0; r < n_rho; ++r)
    if (!(std::isfinite(rho[r]) && rho[r] >= 0.0 && rho[r] <= 1.0))
      return snprintf(why, why_len, "muxgl_fmx_ambient: rho[%d] (%g) is not a finite number in [0, 1]", r, rho[r]), 1;
  for (int64_t s = 0; s < S; ++s)
    if (!(std::isfinite(amb_af[s]) && amb_af[s] >= 0.0 && amb_af[s] <= 1.0))
      return snprintf(why, why_len, "muxgl_fmx_ambient: amb_af of marker %lld (%g) is not a finite number in [0, 1]",
                      (long long)s, amb_af[s]),
             1;
  return 0;
}

extern "C" int muxgl_fmx_ambient(muxgl_handle* h, const double* amb_af, int32_t n_rho, const double* rho, double* ll_amb,
                                 float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (h->group) return group_fmx_ambient(h, amb_af, n_rho, rho, ll_amb, kernel_ms);
  HIPCHK(h, hipSetDevice(h->device));
  if (const char* why = fmx_ambient_refusal(h)) MUXGL_FAIL(h, "%s", why);
  char why[256];
  if (fmx_ambient_bad_args(amb_af, h->S, n_rho, rho, ll_amb, why, sizeof(why))) MUXGL_FAIL(h, "%s", why);
  if (h->C == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  // (no clear_timing, no timing slot: records, timings and every other state of the handle keep their values)
  return fmx_ambient_run(h, amb_af, n_rho, rho, ll_amb, kernel_ms);
}
