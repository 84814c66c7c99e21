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
//   * the sweep (lane = sample column of a 64-column block, one dot gp_j . w_e[r] per (entry, column, rho)), the emit
//     kernel and the host run (on table_call.hpp's batch loop) are ambient_table.hpp's, shared with fmx_ambient.hip;
//     what they guarantee -- no bit depends on the chunking, the budget, the split of the rhos or the devices -- is
//     written there.  This unit cuts a long cell into fixed parts of 2048 entries and sweeps inside the streamed call's
//     budget (4 GiB or a third of the device, MUXGL_DEMUX_SLAB_MB).
//   * amb_count_kernel, lane = entry: the usable reads of the entry by allele, added to its marker's two counters with
//     integer atomics (exact, and the same in any order); the entry's droplet, for the mask, by bisection of cell_ptr.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ambient_table.hpp"
#include "demux_entry.hpp"

namespace {

static_assert(AMBIENT_MAX_RHO == MUXGL_MAX_ALPHA, "the call's rhos take the sixteen slots of an alpha grid");

// entries per lane between two renormalisations of the sweep, their loads in flight: a factor is >= ~1e-11 for triples
// that sum to ~1, eight cannot underflow
struct amb_sweep {
  static constexpr int unr(int /*VH*/, int CH) { return CH == 1 ? 8 : 4; }
};

// wt[(e - eb0)][r][0..2] = w_e[r][l], for the entries [eb0, eb1) of a batch
template <int NA, int RC>
__global__ void __launch_bounds__(256)
    amb_weight_kernel(int64_t eb0, int64_t eb1, int NR, const int32_t* __restrict__ entry_snp,
                      const int64_t* __restrict__ entry_rptr, const uint8_t* __restrict__ reads,
                      const double* __restrict__ lut_g, demux_grid al, ambient_rhos rh, const double* __restrict__ af,
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

template <int NA, int RC>
int launch_weights(muxgl_handle* h, int NR, const demux_grid& al, const ambient_rhos& rh, const ambient_batch& b) {
  hipLaunchKernelGGL((amb_weight_kernel<NA, RC>), dim3((unsigned)((b.eb1 - b.eb0 + 255) / 256)), dim3(256), 0, h->stream,
                     b.eb0, b.eb1, NR, h->d_entry_snp, h->d_entry_rptr, h->d_reads, h->d_lut, al, rh, b.d_af, h->d_has_gp,
                     b.d_wt);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// rhos per pass of the weight kernel: as many as the call has, rounded up to 4, 8 or 16, within what a lane holds beside
// the grid's NA x 9 products (NA <= 4: 16, NA <= 8: 8, above: 4)
template <int NA>
int launch_weights_rc(muxgl_handle* h, int NR, const demux_grid& al, const ambient_rhos& rh, const ambient_batch& b) {
  constexpr int CAP = NA <= 4 ? 16 : NA <= 8 ? 8 : 4;
  if constexpr (CAP >= 16)
    if (NR > 8) return launch_weights<NA, 16>(h, NR, al, rh, b);
  if constexpr (CAP >= 8)
    if (NR > 4) return launch_weights<NA, 8>(h, NR, al, rh, b);
  return launch_weights<NA, 4>(h, NR, al, rh, b);
}

int weights_dispatch(muxgl_handle* h, int A, int NR, const demux_grid& al, const ambient_rhos& rh, const ambient_batch& b) {
#define CALL_W(N) launch_weights_rc<N>(h, NR, al, rh, b)
  DISPATCH_NA(A, CALL_W);
#undef CALL_W
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
  if (demux_ambient_check_af(h, amb_af, "muxgl_demux_ambient")) return 1;  // (first, and with no cell too)
  const ambient_call call = {"muxgl_demux_ambient", h->V, "samples", h->d_gp, "MUXGL_DEMUX_SLAB_MB", table_plan::fixed_begin};
  const demux_grid al = demux_grid_of(p);
  return ambient_table_run<amb_sweep>(h, call, amb_af, NR, rho, ll_amb, kernel_ms,
                                      [&](const ambient_rhos& rh, const ambient_batch& b) {
                                        return weights_dispatch(h, p->n_alpha, NR, al, rh, b);
                                      });
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
