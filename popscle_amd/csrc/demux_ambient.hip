// demux_ambient.hip -- muxgl_demux_ambient: every droplet scored as ONE cell of sample j plus a share rho of ambient RNA,
// and muxgl_pileup_allele_counts, which makes the ambient profile.  The ambient RNA is no donor: where the second donor's
// genotype m stands in cmd_cram_demuxlet.cpp:673, its "genotype" at marker s is twice the pool's ALT fraction f[s], any
// number in [0, 2].  Over the entries e of droplet c whose marker has genotypes:
//
//   p(l, f, rho)    = 0.5 l + (2 f - l) 0.5 rho                                   (the reference's own expression, :673)
//   a_e[r][l]       = prod over the usable reads of (pR (1 - p) + pA p),   p = p(l, f[s_e], rho[r])
//   w_e[r][l]       = (a_e[r][l] / q_max_e + 1e-10) / (1 + 1e-10)        q_max_e: the maximum of the alpha grid's products
//   ll_amb[c][j][r] = sum_e log( sum_l gp[s_e][j][l] w_e[r][l] )
//
// The ambient products take part in no maximum: they are only divided by the grid's, so the table is on the scale of the
// records' log-likelihoods and of the singlet table.  The design is that of demux_unknown.hip with one weight triple per
// (entry, rho) and one orientation:
//   * amb_weight_kernel, lane = entry: the NA x 9 products of the grid as row_entry_pg<NA> forms them (grid_walk of
//     demux_entry.hpp: the same operations in the same order, so q_max is the same number) and beside them 3 x RC ambient
//     products through the same reads; both rescaled every 32 reads by the grid's maximum only.  The rhos are swept in
//     chunks of RC (4, 8 or 16 by the size of the grid, to hold the register count); every chunk repeats the grid
//     products identically and every ambient product belongs to one rho, so the chunking changes no bit.  A marker
//     without genotypes gets ones: its row of gp is (1, 0, 0), so its factor is exactly 1 and the sweep has no branch.
//   * amb_sweep_kernel, lane = sample column of a 64-column block: one dot gp_j . w_e[r] per (entry, column, rho),
//     multiplied into a product kept as mantissa x 2^exponent, one log per (cell part, column, rho).  A wave is one work
//     unit: a part of a cell (at most 2048 entries) x a block x a chunk of CH <= 4 rhos.  Every accumulator belongs to
//     one rho, so this chunking changes no bit either.  Below 64 columns a wave holds G = 64 / VH entries side by side,
//     multiplied in a fixed butterfly at the end.
//   * amb_emit_kernel: the logs of the parts of a cell added in entry order and written in the caller's layout.
//   * amb_count_kernel, lane = entry: the usable reads of the entry by allele, added to its marker's two counters with
//     integer atomics (exact, and the same in any order); the entry's droplet, for the mask, by bisection of cell_ptr.
// Which cell goes into which batch, its cut into parts (fixed parts of 2048 entries) and the order of the work items
// are table_plan.hpp's.  The cut of a cell depends on the cell alone and every reduction tree is fixed: the table is
// bit-identical from call to call, for any budget, for any split of the rhos over calls, on one device, on a group and
// through the sharded driver.
//
// Memory: nothing proportional to nnz x n_rho is held for the whole pileup.  Cells are swept in batches of whole cells
// whose weights ([entries][n_rho][3]), slab rows and output rows (table_plan::ambient_bytes) fit the streamed call's
// budget (4 GiB or a third of the device, MUXGL_DEMUX_SLAB_MB); each batch is copied out before the next.
#include <algorithm>
#include <cmath>
#include <vector>

#include "demux_entry.hpp"
#include "table_call.hpp"

namespace {

using amb_grid = demux_grid;  // the alpha grid, and the call's rhos in the same sixteen slots
using amb_item = table_plan::item;  // the entries [e0, e1) of one cell, result row `row` of the slab
// the further parts of a cell: its value = slab[cell row] + slab[first] + ... + slab[first + count - 1], in this order
using amb_cell = table_plan::cell;

// wt[(e - eb0)][r][0..2] = w_e[r][l], for the entries [eb0, eb1) of a batch
template <int NA, int RC>
__global__ void __launch_bounds__(256)
    amb_weight_kernel(int64_t eb0, int64_t eb1, int NR, const int32_t* __restrict__ entry_snp,
                      const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                      const double* __restrict__ lut_g, amb_grid al, amb_grid rh, const double* __restrict__ af,
                      const uint8_t* __restrict__ has_gp, double* __restrict__ wt) {
  __shared__ double lut[384];
  for (int i = threadIdx.x; i < 384; i += 256) lut[i] = lut_g[i];
  __syncthreads();
  const int64_t e = eb0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= eb1) return;
  const int32_t s = entry_snp[e];
  double* o = wt + (size_t)(e - eb0) * NR * 3;
  if (!has_gp[s]) {  // (no genotypes: the reference skips the marker, :733)
    for (int i = 0; i < NR * 3; ++i) o[i] = 1.0;
    return;
  }
  const int64_t r0 = entry_rptr[e], r1 = entry_rptr[e + 1];
  // p = 0.5 l + (2 f - l) 0.5 rho: exactly 0 at (l = 0, f = 0) and exactly 1 at (l = 2, f = 1), as in the reference, so
  // those corners carry pR and pA themselves (see row_entry_pg on what a rounded corner costs at base quality 93)
  const double tf = af[s] + af[s];
  const double tf1 = tf - 1.0, tf2 = tf - 2.0;
  for (int rb = 0; rb < NR; rb += RC) {
    double pG[NA * 9], am[RC * 3];
#pragma unroll
    for (int i = 0; i < RC * 3; ++i) am[i] = 1.0;
    // the grid's walk (demux_entry.hpp), without the hoist barrier; the ambient products follow the grid's rescale
    const double mx = grid_walk<NA, RC * 3, false>(reads, r0, r1, al.a, lut, pG, am, [&](double pR, double pA, double) {
#pragma unroll
      for (int k = 0; k < RC; ++k) {
        const double hr = 0.5 * rh.a[rb + k];  // (rb + k < 16: a slot past the end holds the last rho again)
        const double p0 = tf * hr, p1 = fma(tf1, hr, 0.5), p2 = fma(tf2, hr, 1.0);
        am[k * 3 + 0] *= fma(pA, p0, pR * (1.0 - p0));
        am[k * 3 + 1] *= fma(pA, p1, pR * (1.0 - p1));
        am[k * 3 + 2] *= fma(pA, p2, pR * (1.0 - p2));
      }
    });
    const double c = 1.0 / (1.0 + 1e-10);
    const double sc = c / mx, t = 1e-10 * c;
#pragma unroll
    for (int k = 0; k < RC; ++k)
      if (rb + k < NR) {
        o[(rb + k) * 3 + 0] = fma(am[k * 3 + 0], sc, t);
        o[(rb + k) * 3 + 1] = fma(am[k * 3 + 1], sc, t);
        o[(rb + k) * 3 + 2] = fma(am[k * 3 + 2], sc, t);
      }
  }
}

// grid: ceil(n_units / 4) workgroups of four waves; wave unit <-> (item, column block, rho chunk), the chunk fastest,
// so the waves of a workgroup walk the same entries and read the same or neighbouring pieces of the genotype rows.
// slab[row][r][V]
template <int VH, int CH>
__global__ void __launch_bounds__(256)
    amb_sweep_kernel(int64_t n_units, int nblk, int nch, int NR, const amb_item* __restrict__ items,
                     const int32_t* __restrict__ entry_snp, int64_t eb0, const double* __restrict__ wt,
                     const double* __restrict__ gp, int V, double* __restrict__ slab) {
  constexpr int G = 64 / VH;            // entries side by side in a wave
  constexpr int UNR = CH == 1 ? 8 : 4;  // entries per lane between two renormalisations, their loads in flight: a factor
                                        // is >= ~1e-11 for triples that sum to ~1, eight cannot underflow
  const int64_t unit = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= n_units) return;
  const int ch = (int)(unit % nch);
  const int64_t rest = unit / nch;
  const int blk = (int)(rest % nblk);
  const int64_t it = rest / nblk;
  const int lane = threadIdx.x & 63;
  const int sub = G == 1 ? 0 : lane / VH;  // entry slot of the lane
  const int j = G == 1 ? blk * 64 + lane : lane % VH;
  const bool jl = j < V;
  const size_t jo = (size_t)(jl ? j : V - 1) * 3;
  const size_t V3 = (size_t)V * 3;
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
      const double* g = gp + (size_t)entry_snp[ec] * V3 + jo;
      const double g0 = g[0], g1 = g[1], g2 = g[2];
      const double* we = wt + (size_t)(ec - eb0) * NR * 3;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const double* w = we + rr[c] * 3;
        const double v = fma(g2, w[2], fma(g1, w[1], g0 * w[0]));
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
  if (G > 1) {  // the G partial products of a column, in a fixed butterfly (a product commutes: both lanes get the same bits)
#pragma unroll
    for (int off = VH; off < 64; off <<= 1)
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        acc[c] *= __shfl_xor(acc[c], off, 64);
        ex[c] += __shfl_xor(ex[c], off, 64);
      }
  }
  if (jl && sub == 0) {
    double* out = slab + (size_t)items[it].row * NR * V + j;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (ch * CH + c < NR) out[(size_t)rr[c] * V] = prodacc_log(acc[c], ex[c]);
  }
}

// lane = (cell, sample, rho), rho fastest: out[nc][V][NR]
__global__ void __launch_bounds__(256)
    amb_emit_kernel(int64_t nc, const amb_cell* __restrict__ cells, int V, int NR, const double* __restrict__ slab,
                    double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nc * V * NR) return;
  const int r = (int)(i % NR);
  const int j = (int)((i / NR) % V);
  const int64_t c = i / ((int64_t)NR * V);
  const size_t rs = (size_t)NR * V, off = (size_t)r * V + j;
  const amb_cell ct = cells[c];
  double s = slab[(size_t)c * rs + off];
  for (int64_t k = 0; k < ct.count; ++k) s += slab[(size_t)(ct.first + k) * rs + off];
  out[i] = s;
}

// cnt[s][0] / [s][1] += the entry's usable reads with bit 7 clear / set; mask: one byte per cell, or NULL
__global__ void __launch_bounds__(256)
    amb_count_kernel(int64_t nnz, int64_t C, const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                     const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                     const uint8_t* __restrict__ mask, unsigned long long* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  if (mask) {  // the cell of the entry: the last c with cell_ptr[c] <= e (empty cells share a start with their successor)
    int64_t lo = 0, hi = C;  // invariant: cell_ptr[lo] <= e < cell_ptr[hi]
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (cell_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    if (!mask[lo]) return;
  }
  unsigned long long n0 = 0, n1 = 0;
  for (int64_t r = entry_rptr[e]; r < entry_rptr[e + 1]; ++r) {
    const uint32_t b = reads[r];
    if (b == MUXGL_READ_OTHER) continue;
    if (b >> 7) ++n1; else ++n0;
  }
  unsigned long long* o = cnt + (size_t)entry_snp[e] * 2;
  if (n0) atomicAdd(o, n0);
  if (n1) atomicAdd(o + 1, n1);
}

struct amb_batch {  // what one launch of the three kernels needs
  int64_t eb0, eb1, n_items, nc;
  const amb_item* d_items;
  const amb_cell* d_cells;
  double *d_wt, *d_slab, *d_out;
  const double* d_af;
};

template <int NA, int RC>
int launch_weights(muxgl_handle* h, int NR, const amb_grid& al, const amb_grid& rh, const amb_batch& b) {
  hipLaunchKernelGGL((amb_weight_kernel<NA, RC>), dim3((unsigned)((b.eb1 - b.eb0 + 255) / 256)), dim3(256), 0, h->stream,
                     b.eb0, b.eb1, NR, h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, al, rh, b.d_af, h->d_has_gp,
                     b.d_wt);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// rhos per pass of the weight kernel: as many as the call has, rounded up to 4, 8 or 16, within what a lane holds beside
// the grid's NA x 9 products (NA <= 4: 16, NA <= 8: 8, above: 4)
template <int NA>
int launch_weights_rc(muxgl_handle* h, int NR, const amb_grid& al, const amb_grid& rh, const amb_batch& b) {
  constexpr int CAP = NA <= 4 ? 16 : NA <= 8 ? 8 : 4;
  if constexpr (CAP >= 16)
    if (NR > 8) return launch_weights<NA, 16>(h, NR, al, rh, b);
  if constexpr (CAP >= 8)
    if (NR > 4) return launch_weights<NA, 8>(h, NR, al, rh, b);
  return launch_weights<NA, 4>(h, NR, al, rh, b);
}

int weights_dispatch(muxgl_handle* h, int A, int NR, const amb_grid& al, const amb_grid& rh, const amb_batch& b) {
#define CALL_W(N) launch_weights_rc<N>(h, NR, al, rh, b)
  DISPATCH_NA(A, CALL_W);
#undef CALL_W
}

template <int VH, int CH>
void launch_sweep(muxgl_handle* h, int NR, int nch, const amb_batch& b) {
  const int nblk = (h->V + 63) / 64;
  const int64_t n_units = b.n_items * nblk * nch;
  hipLaunchKernelGGL((amb_sweep_kernel<VH, CH>), dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, h->stream, n_units, nblk,
                     nch, NR, b.d_items, h->d_entry_snp, b.eb0, b.d_wt, h->d_gp, h->V, b.d_slab);
}

template <int CH>
void sweep_dispatch_vh(muxgl_handle* h, int NR, int nch, const amb_batch& b) {
  int VH = 64;
  while (VH > 1 && VH / 2 >= h->V) VH /= 2;
#define CALL_S(W) launch_sweep<W, CH>(h, NR, nch, b)
  DISPATCH_WIDTH(VH, CALL_S);
#undef CALL_S
}

int sweep_dispatch(muxgl_handle* h, int CH, int NR, int nch, const amb_batch& b) {
  switch (CH) {
    case 1: sweep_dispatch_vh<1>(h, NR, nch, b); break;
    case 2: sweep_dispatch_vh<2>(h, NR, nch, b); break;
    case 3: sweep_dispatch_vh<3>(h, NR, nch, b); break;
    default: sweep_dispatch_vh<4>(h, NR, nch, b); break;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // namespace

int demux_ambient_bad_rho(int n_rho, const double* rho) {
  for (int r = 0; r < n_rho; ++r)
    if (!(std::isfinite(rho[r]) && rho[r] >= 0.0 && rho[r] <= 1.0)) return r;
  return -1;
}

// the ambient profile: a fraction wherever a marker has genotypes
int demux_ambient_check_af(muxgl_handle* h, const double* amb_af, const char* who) {
  const int64_t S = h->S;
  std::vector<uint8_t> has_gp((size_t)S);
  if (S > 0) HIPCHK(h, hipMemcpyAsync(has_gp.data(), h->d_has_gp, (size_t)S, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int64_t s = 0; s < S; ++s)
    if (has_gp[(size_t)s] && !(std::isfinite(amb_af[s]) && amb_af[s] >= 0.0 && amb_af[s] <= 1.0))
      MUXGL_FAIL(h, "%s: amb_af of marker %lld (%g) is not a finite number in [0, 1]", who, (long long)s, amb_af[s]);
  return 0;
}

int demux_ambient_run(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int NR, const double* rho,
                      double* ll_amb, float* kernel_ms) {
  const int V = h->V, A = p->n_alpha;
  const int64_t C = h->C, S = h->S;
  if (demux_ambient_check_af(h, amb_af, "muxgl_demux_ambient")) return 1;
  std::vector<int64_t> cell_ptr((size_t)C + 1);
  HIPCHK(h, hipMemcpyAsync(cell_ptr.data(), h->d_cell_ptr, sizeof(int64_t) * (size_t)(C + 1), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));

  // batches of whole cells whose device bytes fit the budget (table_plan.hpp)
  const size_t budget = dev_slab_budget("MUXGL_DEMUX_SLAB_MB");
  auto bytes_of = [&](int64_t len, int64_t np) { return table_plan::ambient_bytes(len, np, NR, V); };
  const table_plan::batches bt = table_plan::plan(cell_ptr.data(), C, budget, bytes_of);
  if (bt.over >= 0) {
    const int64_t len = cell_ptr[(size_t)bt.over + 1] - cell_ptr[(size_t)bt.over];
    MUXGL_FAIL(h, "muxgl_demux_ambient: droplet %lld alone (%lld entries x %d rhos x %d samples: %.1f MB) exceeds the "
                  "budget of %.1f MB (raise MUXGL_DEMUX_SLAB_MB)",
               (long long)(h->cell_base + bt.over), (long long)len, NR, V,
               (double)bytes_of(len, table_plan::parts(len)) / 1048576.0, (double)budget / 1048576.0);
  }
  const int nblk = (V + 63) / 64;
  const int nch = (NR + 3) / 4, CH = (NR + nch - 1) / nch;  // chunks of the rhos, rhos per chunk (1..4)
  if (table_plan::exceeds_one_launch((double)bt.max_rows * nblk * nch, 4.0) ||
      table_plan::exceeds_one_launch((double)bt.max_cells * V * NR, 256.0))
    MUXGL_FAIL(h, "muxgl_demux_ambient: a batch of %lld rows x %d samples x %d rhos exceeds one launch (lower MUXGL_DEMUX_SLAB_MB)",
               (long long)bt.max_rows, V, NR);
  const amb_grid al = demux_grid_of(p);
  amb_grid rh;
  for (int i = 0; i < MUXGL_MAX_ALPHA; ++i) rh.a[i] = i < NR ? rho[i] : rho[NR - 1];  // (a repeated rho is not written)

  dev_tmp<double> d_af, d_wt, d_slab, d_out;
  dev_tmp<amb_item> d_items;
  dev_tmp<amb_cell> d_cells;
  if (dev_alloc(h, &d_af.p, (size_t)S)) return 1;
  if (dev_alloc(h, &d_wt.p, (size_t)bt.max_entries * NR * 3)) return 1;
  if (dev_alloc(h, &d_slab.p, (size_t)bt.max_rows * NR * V)) return 1;
  if (dev_alloc(h, &d_out.p, (size_t)bt.max_cells * V * NR)) return 1;
  if (dev_alloc(h, &d_items.p, (size_t)bt.max_rows)) return 1;
  if (dev_alloc(h, &d_cells.p, (size_t)bt.max_cells)) return 1;
  call_events ev;  // (the handle's timing slots keep their values)
  if (ev.create(h, kernel_ms, "muxgl_demux_ambient")) return 1;

  if (S > 0) HIPCHK(h, hipMemcpyAsync(d_af.p, amb_af, sizeof(double) * (size_t)S, hipMemcpyHostToDevice, h->stream));
  std::vector<amb_item> items;
  std::vector<amb_cell> cells;
  int64_t c0 = 0;
  for (const int64_t c1 : bt.end) {
    const int64_t nc = c1 - c0;
    table_plan::fill(cell_ptr.data(), c0, c1, table_plan::fixed_begin, items, nullptr, &cells);
    const amb_batch b = {cell_ptr[(size_t)c0], cell_ptr[(size_t)c1], (int64_t)items.size(), nc, d_items.p, d_cells.p,
                         d_wt.p, d_slab.p, d_out.p, d_af.p};
    if (table_upload(h, items, d_items.p, cells, d_cells.p)) return 1;
    if (ev.start(h)) return 1;
    if (b.eb1 > b.eb0 && weights_dispatch(h, A, NR, al, rh, b)) return 1;
    if (sweep_dispatch(h, CH, NR, nch, b)) return 1;
    {
      const int64_t n = nc * V * NR;
      hipLaunchKernelGGL(amb_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, nc, d_cells.p, V, NR,
                         d_slab.p, d_out.p);
      HIPCHK(h, hipGetLastError());
    }
    if (ev.stop(h)) return 1;
    HIPCHK(h, hipMemcpyAsync(ll_amb + (size_t)c0 * V * NR, d_out.p, sizeof(double) * (size_t)nc * V * NR, hipMemcpyDeviceToHost,
                             h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ev.add();
    c0 = c1;
  }
  return 0;
}

int pileup_allele_counts_run(muxgl_handle* h, const uint8_t* cell_mask, int64_t* n_ref, int64_t* n_alt) {
  const int64_t S = h->S, C = h->C;
  dev_tmp<unsigned long long> d_cnt;
  dev_tmp<uint8_t> d_mask;
  if (dev_alloc(h, &d_cnt.p, (size_t)S * 2)) return 1;
  if (S > 0) HIPCHK(h, hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long) * (size_t)S * 2, h->stream));
  if (cell_mask && C > 0) {
    if (dev_alloc(h, &d_mask.p, (size_t)C)) return 1;
    HIPCHK(h, hipMemcpyAsync(d_mask.p, cell_mask, (size_t)C, hipMemcpyHostToDevice, h->stream));
  }
  if (h->nnz > 0) {
    hipLaunchKernelGGL(amb_count_kernel, dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, h->stream, h->nnz, C,
                       h->d_cell_ptr, h->d_entry_snp, h->d_entry_rptr, h->d_reads, cell_mask ? d_mask.p : nullptr, d_cnt.p);
    HIPCHK(h, hipGetLastError());
  }
  std::vector<unsigned long long> cnt((size_t)S * 2);
  if (S > 0)
    HIPCHK(h, hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(unsigned long long) * (size_t)S * 2, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int64_t s = 0; s < S; ++s) {
    n_ref[s] = (int64_t)cnt[(size_t)s * 2];
    n_alt[s] = (int64_t)cnt[(size_t)s * 2 + 1];
  }
  return 0;
}
