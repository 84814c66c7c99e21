// soup_mix.hip -- muxgl_pileup_read_hist and muxgl_demux_soup_mix: the soup (the pool's free-floating RNA) fitted as a
// mixture of the donors of the panel.  Its ALT fraction at marker s is a weighted mean of the donors' genotype dosages with
// weights pi that are the same at every marker; the reads of the nearly empty droplets determine them.  The components are
// the V samples of the panel and, optionally, component V: a donor missing from the VCF, whose genotype prior per marker
// is the panel mean as muxgl_demux_unknown forms it (rows added in sample order, one division) or the caller's [S][3].
//
//   r_v(s) = g0 + g1 / 2,  a_v(s) = g1 / 2 + g2            (g0, g1, g2 = gp[s][v][0..2]; rows need not sum to one)
//   R(s) = sum_v pi_v r_v(s),  A(s) = sum_v pi_v a_v(s)
//   D(s, b) = pR R(s) + pA A(s)                              (pR, pA of read byte b as demux_entry.hpp takes them from the
//                                                             Phred table; a sum of non-negative terms, never pR + d * ...)
//   LL(pi) = sum n log D,   grad_v = (1 / N) sum_s [ r_v(s) sum_b n pR / D + a_v(s) sum_b n pA / D ],   pi'_v = pi_v grad_v
//
// The reads enter only through their histogram: n usable reads per (marker, byte), an exact integer statistic.
//   * hist_count_kernel / hist_fill_kernel, lane = entry: the usable reads of the entries of the chosen droplets become
//     keys marker * 256 + byte; a radix sort and a run-length pass (heads, a scan, one store per run) make the records.
//     Integer work only: the same records for any order of the droplets.
//   * soup_mix_reads_kernel<W>: a wave takes 64 / W markers side by side (W = the components rounded up to a power of two,
//     64 from 33 on; beyond 64 a lane takes the components lane, lane + 64, ... in this order).  A lane reads its row of
//     the panel as it lies (24 contiguous bytes), R and A come from a fixed butterfly over the W lanes, and the first lane
//     of the slot walks the marker's records in key order for sum n pR / D, sum n pA / D and sum n log D (pos_log).
//   * soup_mix_update_kernel: the transposed product, lane = component.  A workgroup walks a block of
//     soup_mix_plan::UPDATE_BLOCK active markers for 64 components -- four waves, a quarter of the block each in marker
//     order, the quarters added in order -- and writes one partial row.
//   * soup_mix_finish_kernel: adds the block partials in block order, forms grad, pi' and the largest step, and adds the
//     blocks' LL the same way.
// Every rounded sum has a tree fixed by the histogram and the number of components alone, so the outputs are bit-identical
// from call to call, for the handle's own pileup against the same histogram passed in, for any order of the droplets, on
// one device, on a group (the members' histograms are merged with integer adds and one member fits) and through the
// sharded driver.  Temporaries are dev_tmp; nothing is cached on the handle and no state changes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"
#include "soup_mix_plan.hpp"

namespace {

namespace sp = soup_mix_plan;

// ---- the histogram ------------------------------------------------------------------------------------------------------

// cnt[e] = usable reads of entry e where its droplet's mask byte is set (mask NULL: everywhere); cnt[nnz] = 0
__global__ void __launch_bounds__(256)
    hist_count_kernel(int64_t nnz, int64_t C, const int64_t* __restrict__ cell_ptr, const int64_t* __restrict__ entry_rptr,
                      const uint8_t* __restrict__ reads, const uint8_t* __restrict__ mask, int64_t* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e > nnz) return;
  int64_t n = 0;
  bool on = e < nnz;
  if (on && mask) {  // the cell of the entry: the last c with cell_ptr[c] <= e (as amb_count_kernel, demux_ambient.hip)
    int64_t lo = 0, hi = C;
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (cell_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    on = mask[lo] != 0;
  }
  if (on)
    for (int64_t r = entry_rptr[e]; r < entry_rptr[e + 1]; ++r) n += reads[r] != MUXGL_READ_OTHER;
  cnt[e] = n;
}

// keys[off[e] ...] = marker * 256 + byte of the usable reads of entry e (off: the scan of cnt)
__global__ void __launch_bounds__(256)
    hist_fill_kernel(int64_t nnz, const int32_t* __restrict__ entry_snp, const int64_t* __restrict__ entry_rptr,
                     const uint8_t* __restrict__ reads, const int64_t* __restrict__ off, int64_t* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  int64_t o = off[e];
  const int64_t o1 = off[e + 1];
  if (o == o1) return;
  const int64_t base = (int64_t)entry_snp[e] * 256;
  for (int64_t r = entry_rptr[e]; r < entry_rptr[e + 1] && o < o1; ++r) {
    const uint32_t b = reads[r];
    if (b != MUXGL_READ_OTHER) keys[o++] = base + b;
  }
}

// head[i] = 1 where a run of equal keys begins; head[T] = 0
__global__ void __launch_bounds__(256) hist_head_kernel(int64_t T, const int64_t* __restrict__ k, int64_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > T) return;
  head[i] = (i < T && (i == 0 || k[i] != k[i - 1])) ? 1 : 0;
}

// run j (idx: the scan of head): its key and its first position
__global__ void __launch_bounds__(256)
    hist_emit_kernel(int64_t T, const int64_t* __restrict__ k, const int64_t* __restrict__ idx, int64_t* __restrict__ ukey,
                     int64_t* __restrict__ ustart) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  if (i == 0 || k[i] != k[i - 1]) {
    ukey[idx[i]] = k[i];
    ustart[idx[i]] = i;
  }
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// in-place exclusive scan of n int64 (rocPRIM's temporary as plan_kernels.hip takes it)
int scan_i64(muxgl_handle* h, int64_t* d, size_t n) {
  size_t tb = 0;
  void* tmp = nullptr;
  HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, d, d, (int64_t)0, n, rocprim::plus<int64_t>(), h->stream));
  HIPCHK(h, dev_malloc_retry(&tmp, tb ? tb : 1));
  hipError_t e = rocprim::exclusive_scan(tmp, tb, d, d, (int64_t)0, n, rocprim::plus<int64_t>(), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) MUXGL_FAIL(h, "muxgl_pileup_read_hist: scan failed: %s", hipGetErrorString(e));
  return 0;
}

// the histogram of the handle's own droplets under cell_mask (host [C] or NULL), as sorted records on the host
int read_hist_run(muxgl_handle* h, const uint8_t* cell_mask, std::vector<int64_t>* keys, std::vector<int64_t>* counts) {
  keys->clear();
  counts->clear();
  const int64_t nnz = h->nnz, C = h->C;
  if (nnz == 0 || C == 0) return 0;
  dev_tmp<uint8_t> d_mask;
  dev_tmp<int64_t> d_off, d_keys, d_sorted, d_idx, d_ukey, d_ustart;
  if (cell_mask) {
    if (dev_alloc(h, &d_mask.p, (size_t)C)) return 1;
    HIPCHK(h, hipMemcpyAsync(d_mask.p, cell_mask, (size_t)C, hipMemcpyHostToDevice, h->stream));
  }
  if (dev_alloc(h, &d_off.p, (size_t)nnz + 1)) return 1;
  hipLaunchKernelGGL(hist_count_kernel, dim3(blocks_of(nnz + 1)), dim3(256), 0, h->stream, nnz, C, h->d_cell_ptr,
                     h->d_entry_rptr, h->d_reads, cell_mask ? d_mask.p : nullptr, d_off.p);
  HIPCHK(h, hipGetLastError());
  if (scan_i64(h, d_off.p, (size_t)nnz + 1)) return 1;
  int64_t T = 0;
  HIPCHK(h, hipMemcpyAsync(&T, d_off.p + nnz, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (T == 0) return 0;
  if (dev_alloc(h, &d_keys.p, (size_t)T) || dev_alloc(h, &d_sorted.p, (size_t)T)) return 1;
  hipLaunchKernelGGL(hist_fill_kernel, dim3(blocks_of(nnz)), dim3(256), 0, h->stream, nnz, h->d_entry_snp, h->d_entry_rptr,
                     h->d_reads, d_off.p, d_keys.p);
  HIPCHK(h, hipGetLastError());
  unsigned bits = 9;  // the byte and the marker's bits
  while (bits < 63 && ((int64_t)1 << (bits - 8)) < h->S) ++bits;
  {
    size_t tb = 0;
    void* tmp = nullptr;
    HIPCHK(h, rocprim::radix_sort_keys(nullptr, tb, d_keys.p, d_sorted.p, (size_t)T, 0u, bits, h->stream));
    HIPCHK(h, dev_malloc_retry(&tmp, tb ? tb : 1));
    hipError_t e = rocprim::radix_sort_keys(tmp, tb, d_keys.p, d_sorted.p, (size_t)T, 0u, bits, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) MUXGL_FAIL(h, "muxgl_pileup_read_hist: sort failed: %s", hipGetErrorString(e));
  }
  dev_free(&d_keys.p);
  if (dev_alloc(h, &d_idx.p, (size_t)T + 1)) return 1;
  hipLaunchKernelGGL(hist_head_kernel, dim3(blocks_of(T + 1)), dim3(256), 0, h->stream, T, d_sorted.p, d_idx.p);
  HIPCHK(h, hipGetLastError());
  if (scan_i64(h, d_idx.p, (size_t)T + 1)) return 1;
  int64_t nrun = 0;
  HIPCHK(h, hipMemcpyAsync(&nrun, d_idx.p + T, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (dev_alloc(h, &d_ukey.p, (size_t)nrun) || dev_alloc(h, &d_ustart.p, (size_t)nrun)) return 1;
  hipLaunchKernelGGL(hist_emit_kernel, dim3(blocks_of(T)), dim3(256), 0, h->stream, T, d_sorted.p, d_idx.p, d_ukey.p,
                     d_ustart.p);
  HIPCHK(h, hipGetLastError());
  keys->resize((size_t)nrun);
  counts->resize((size_t)nrun);
  HIPCHK(h, hipMemcpyAsync(keys->data(), d_ukey.p, sizeof(int64_t) * (size_t)nrun, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(counts->data(), d_ustart.p, sizeof(int64_t) * (size_t)nrun, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int64_t j = 0; j < nrun; ++j)  // first positions -> lengths
    (*counts)[(size_t)j] = (j + 1 < nrun ? (*counts)[(size_t)j + 1] : T) - (*counts)[(size_t)j];
  return 0;
}

// the members' sorted lists merged: equal keys' counts added (integers: exact in any order)
void merge_hist(std::vector<int64_t>* keys, std::vector<int64_t>* counts, const std::vector<int64_t>& k2,
                const std::vector<int64_t>& c2) {
  std::vector<int64_t> k, c;
  k.reserve(keys->size() + k2.size());
  c.reserve(keys->size() + k2.size());
  size_t i = 0, j = 0;
  while (i < keys->size() || j < k2.size()) {
    if (j == k2.size() || (i < keys->size() && (*keys)[i] < k2[j])) {
      k.push_back((*keys)[i]);
      c.push_back((*counts)[i++]);
    } else if (i == keys->size() || k2[j] < (*keys)[i]) {
      k.push_back(k2[j]);
      c.push_back(c2[j++]);
    } else {
      k.push_back(k2[j]);
      c.push_back((*counts)[i++] + c2[j++]);
    }
  }
  keys->swap(k);
  counts->swap(c);
}

// the histogram of a handle or of a group (every member counts its own droplets)
int read_hist_any(muxgl_handle* h, const uint8_t* cell_mask, std::vector<int64_t>* keys, std::vector<int64_t>* counts) {
  if (!h->group) {
    HIPCHK(h, hipSetDevice(h->device));
    return read_hist_run(h, cell_mask, keys, counts);
  }
  muxgl_group* g = h->group;
  keys->clear();
  counts->clear();
  std::vector<int64_t> k2, c2;
  for (int r = 0; r < g->n; ++r) {
    muxgl_handle* m = g->m[(size_t)r];
    if (hipSetDevice(m->device) != hipSuccess || read_hist_run(m, cell_mask ? cell_mask + g->cb[(size_t)r] : nullptr, &k2, &c2)) {
      char buf[64];
      snprintf(buf, sizeof(buf), "device group member %d (device %d): ", r, m->device);
      h->err = std::string(buf) + m->err;
      return 1;
    }
    merge_hist(keys, counts, k2, c2);
  }
  return 0;
}

// ---- the fit ------------------------------------------------------------------------------------------------------------

struct mix_panel {
  const double* gp;  // [S][V][3]
  const double* u;   // [S][3], component V (NULL without it)
  int V, M;
};

// u = the panel mean of cmd_cram_demuxlet.cpp:428-440, the rows added in sample order, one division: the operations of
// unk_mean_kernel (demux_unknown.hip) in their order
__global__ void __launch_bounds__(256)
    soup_mean_kernel(int64_t S, const double* __restrict__ gp, const uint8_t* __restrict__ has_gp, int V, double* __restrict__ u) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  double a0 = 1.0, a1 = 0.0, a2 = 0.0;
  if (has_gp[s]) {
    const double* g = gp + (size_t)s * V * 3;
    a0 = a1 = a2 = 0.0;
    for (int j = 0; j < V; ++j) {
      a0 += g[3 * j];
      a1 += g[3 * j + 1];
      a2 += g[3 * j + 2];
    }
    const double nv = (double)V;
    a0 /= nv;
    a1 /= nv;
    a2 /= nv;
  }
  u[3 * s] = a0;
  u[3 * s + 1] = a1;
  u[3 * s + 2] = a2;
}

__device__ __forceinline__ const double* mix_row(const mix_panel& p, int64_t s, int v) {
  return v < p.V ? p.gp + ((size_t)s * p.V + v) * 3 : p.u + (size_t)s * 3;
}

// R(s), A(s) in every lane of the slot of W lanes that holds marker s; li = the lane's place in its slot
template <int W>
__device__ __forceinline__ void mix_RA(const mix_panel& p, const double* __restrict__ pi, int64_t s, int li, double& R, double& A) {
  double r = 0.0, a = 0.0;
  for (int v = li; v < p.M; v += W) {
    const double* g = mix_row(p, s, v);
    const double g0 = g[0], hg = 0.5 * g[1], g2 = g[2], w = pi[v];
    r = fma(w, g0 + hg, r);
    a = fma(w, hg + g2, a);
  }
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
    r += __shfl_xor(r, off, 64);
    a += __shfl_xor(a, off, 64);
  }
  R = r;
  A = a;
}

// Over the n markers of a list (marker[i]; marker == NULL: marker i itself), 64 / W per wave.
//   ra != NULL: ra[i] = R + A at pi, nothing else (the cut of the active markers)
//   af != NULL: af[i] = A / (R + A), 0.5 at a marker without genotypes or with R + A == 0 (the fitted profile)
//   else:       wR[i] = sum_b n pR / D, wA[i] = sum_b n pA / D, ll[i] = sum_b n log D over the marker's records, in key order
template <int W>
__global__ void __launch_bounds__(256)
    soup_mix_reads_kernel(int64_t n, const int32_t* __restrict__ marker, const int64_t* __restrict__ rec_ptr,
                          const uint8_t* __restrict__ rec_byte, const double* __restrict__ rec_n, const double* __restrict__ lut,
                          mix_panel p, const double* __restrict__ pi, const uint8_t* __restrict__ has_gp, double* __restrict__ wR,
                          double* __restrict__ wA, double* __restrict__ ll, double* __restrict__ ra, double* __restrict__ af) {
  constexpr int G = 64 / W;
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave * G >= n) return;  // (wave-uniform)
  const int64_t slot = wave * G + lane / W;
  const bool live = slot < n;
  const int64_t i = live ? slot : n - 1;  // a slot past the end repeats the last marker: every lane takes part in the butterfly
  const int64_t s = marker ? (int64_t)marker[i] : i;
  double R, A;
  mix_RA<W>(p, pi, s, lane % W, R, A);
  if (!live || lane % W != 0) return;
  if (ra) {
    ra[i] = R + A;
    return;
  }
  if (af) {
    const double t = R + A;
    af[i] = (has_gp[s] && t > 0.0) ? A / t : 0.5;
    return;
  }
  double sR = 0.0, sA = 0.0, sl = 0.0;
  for (int64_t k = rec_ptr[i]; k < rec_ptr[i + 1]; ++k) {
    const uint32_t b = rec_byte[k];
    const uint32_t al = b >> 7, bq = b & 0x7f;
    const double e3 = lut[256 + bq], mt = lut[128 + bq];  // Err / 3, Mat (demux_entry.hpp)
    const double pR = al == 0 ? mt : e3;
    const double pA = al == 0 ? e3 : mt;
    const double D = fma(pA, A, pR * R);  // two non-negative terms
    const double cn = rec_n[k];
    const double q = cn / D;
    sR = fma(q, pR, sR);
    sA = fma(q, pA, sA);
    sl = fma(cn, pos_log(D, 0.0), sl);
  }
  wR[i] = sR;
  wA[i] = sA;
  ll[i] = sl;
}

// part[blk][v] = the transposed product over the active markers i of block blk: r_v wR[i] + a_v wA[i], added in marker
// order inside each quarter of the block (UPDATE_BLOCK / 4 markers, one wave each), the four quarters then added in
// order; ll_part[blk] = ll[i] added the same way.  A quarter past the end adds an exact 0.  grid (blocks, ceil(M / 64)),
// four waves per workgroup, lane = component
__global__ void __launch_bounds__(256)
    soup_mix_update_kernel(int64_t n_act, const int32_t* __restrict__ marker, mix_panel p, const double* __restrict__ wR,
                           const double* __restrict__ wA, const double* __restrict__ ll, double* __restrict__ part,
                           double* __restrict__ ll_part) {
  constexpr int QUARTER = sp::UPDATE_BLOCK / 4;
  __shared__ double s_acc[4][64];
  __shared__ double s_ll[4];
  const int64_t blk = blockIdx.x;
  const int wv = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int v = (int)blockIdx.y * 64 + lane;
  const int64_t b1 = (blk + 1) * sp::UPDATE_BLOCK < n_act ? (blk + 1) * sp::UPDATE_BLOCK : n_act;
  const int64_t i0 = blk * sp::UPDATE_BLOCK + (int64_t)wv * QUARTER;
  const int64_t i1 = i0 + QUARTER < b1 ? i0 + QUARTER : b1;
  double acc = 0.0;
  if (v < p.M) {
#pragma unroll 4
    for (int64_t i = i0; i < i1; ++i) {
      const double* g = mix_row(p, (int64_t)marker[i], v);
      const double g0 = g[0], hg = 0.5 * g[1], g2 = g[2];
      acc = fma(hg + g2, wA[i], fma(g0 + hg, wR[i], acc));
    }
  }
  s_acc[wv][lane] = acc;
  if (blockIdx.y == 0 && lane == 0) {
    double l = 0.0;
    for (int64_t i = i0; i < i1; ++i) l += ll[i];
    s_ll[wv] = l;
  }
  __syncthreads();
  if (wv == 0 && v < p.M) part[(size_t)blk * p.M + v] = ((s_acc[0][lane] + s_acc[1][lane]) + s_acc[2][lane]) + s_acc[3][lane];
  if (blockIdx.y == 0 && threadIdx.x == 0) ll_part[blk] = ((s_ll[0] + s_ll[1]) + s_ll[2]) + s_ll[3];
}

// grad_v = (sum over the blocks, in order, of part[blk][v]) / N, pi'_v = pi_v grad_v; scal[0] = LL (the blocks' added in
// order), scal[1] = max_v |pi'_v - pi_v| (a NaN wins, so a broken fit never looks converged).  One workgroup.
__global__ void __launch_bounds__(256)
    soup_mix_finish_kernel(int64_t nblk, int M, double N, const double* __restrict__ part, const double* __restrict__ ll_part,
                           const double* __restrict__ pi, double* __restrict__ pi_next, double* __restrict__ grad,
                           double* __restrict__ scal) {
  __shared__ double smax[256];
  double mx = 0.0;
  for (int v = threadIdx.x; v < M; v += 256) {
    double g = 0.0;
    for (int64_t b = 0; b < nblk; ++b) g += part[(size_t)b * M + v];
    const double gr = g / N;
    const double w = pi[v], wn = w * gr;
    grad[v] = gr;
    pi_next[v] = wn;
    const double d = fabs(wn - w);
    mx = (d > mx || d != d) ? d : mx;
  }
  smax[threadIdx.x] = mx;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const double a = smax[threadIdx.x], b = smax[threadIdx.x + off];
      smax[threadIdx.x] = (a != a) ? a : ((b > a || b != b) ? b : a);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double l = 0.0;
    for (int64_t b = 0; b < nblk; ++b) l += ll_part[b];
    scal[0] = l;
    scal[1] = smax[0];
  }
}

struct reads_launch {
  int64_t n;
  const int32_t* marker;
  const int64_t* rec_ptr;
  const uint8_t* rec_byte;
  const double* rec_n;
  const double* pi;
  double *wR, *wA, *ll, *ra, *af;
};

template <int W>
void launch_reads_w(muxgl_handle* h, const mix_panel& p, const reads_launch& a) {
  const int64_t waves = sp::waves(a.n, p.M);
  hipLaunchKernelGGL((soup_mix_reads_kernel<W>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, h->stream, a.n, a.marker,
                     a.rec_ptr, a.rec_byte, a.rec_n, h->d_lut, p, a.pi, h->d_has_gp, a.wR, a.wA, a.ll, a.ra, a.af);
}

int launch_reads(muxgl_handle* h, const mix_panel& p, const reads_launch& a) {
  if (a.n == 0) return 0;
#define CALL_R(W) launch_reads_w<W>(h, p, a)
  DISPATCH_WIDTH(sp::lane_width(p.M), CALL_R);
#undef CALL_R
  HIPCHK(h, hipGetLastError());
  return 0;
}

struct mix_out {
  double *pi, *grad, *ll, *amb_af;
  int32_t *n_iter, *status;
  int64_t* n_reads;
};

template <class T>
int to_device(muxgl_handle* h, dev_tmp<T>* d, const std::vector<T>& v) {
  if (dev_alloc(h, &d->p, v.size())) return 1;
  if (!v.empty()) HIPCHK(h, hipMemcpyAsync(d->p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, h->stream));
  return 0;
}

// the fit on one handle from a checked histogram; pi: the start, already divided by its sum
int soup_mix_run(muxgl_handle* h, int64_t n_rec, const int64_t* keys, const int64_t* counts, bool with_unknown,
                 const double* gp0, std::vector<double> pi, int32_t n_iter_max, double tol, const mix_out& out,
                 float* kernel_ms) {
  const int64_t S = h->S;
  const int M = h->V + (with_unknown ? 1 : 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<uint8_t> has_gp((size_t)S);
  if (S > 0) HIPCHK(h, hipMemcpyAsync(has_gp.data(), h->d_has_gp, (size_t)S, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const sp::marker_list cand = sp::candidates(n_rec, keys, counts, has_gp.data());

  call_events ev;
  if (ev.create(h, kernel_ms, "muxgl_demux_soup_mix")) return 1;
  dev_tmp<double> d_u, d_pi0, d_pi1, d_grad, d_scal, d_ra, d_wR, d_wA, d_ll, d_part, d_llp, d_recn, d_af;
  dev_tmp<int32_t> d_marker;
  dev_tmp<int64_t> d_recptr;
  dev_tmp<uint8_t> d_recb;
  mix_panel p = {h->d_gp, nullptr, h->V, M};
  if (ev.start(h)) return 1;
  if (with_unknown) {
    if (dev_alloc(h, &d_u.p, (size_t)S * 3)) return 1;
    if (gp0) {
      if (S > 0) HIPCHK(h, hipMemcpyAsync(d_u.p, gp0, sizeof(double) * (size_t)S * 3, hipMemcpyHostToDevice, h->stream));
    } else if (S > 0) {
      hipLaunchKernelGGL(soup_mean_kernel, dim3(blocks_of(S)), dim3(256), 0, h->stream, S, h->d_gp, h->d_has_gp, h->V, d_u.p);
      HIPCHK(h, hipGetLastError());
    }
    p.u = d_u.p;
  }
  if (to_device(h, &d_pi0, pi) || dev_alloc(h, &d_pi1.p, (size_t)M) || dev_alloc(h, &d_grad.p, (size_t)M) ||
      dev_alloc(h, &d_scal.p, 2))
    return 1;

  // the active markers: the candidates with R + A > 0 at the start
  sp::marker_list act;
  if (!cand.marker.empty()) {
    std::vector<double> ra(cand.marker.size());
    if (to_device(h, &d_marker, cand.marker) || dev_alloc(h, &d_ra.p, ra.size())) return 1;
    reads_launch a = {(int64_t)ra.size(), d_marker.p, nullptr, nullptr, nullptr, d_pi0.p, nullptr, nullptr, nullptr, d_ra.p, nullptr};
    if (launch_reads(h, p, a)) return 1;
    HIPCHK(h, hipMemcpyAsync(ra.data(), d_ra.p, sizeof(double) * ra.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    act = sp::active(cand, ra.data(), counts);
  } else {
    act.rec_ptr.push_back(0);
  }
  const int64_t n_act = (int64_t)act.marker.size();
  const int64_t nblk = sp::update_blocks(n_act);
  const double N = (double)act.n_reads;

  std::vector<double> ll((size_t)n_iter_max + 1, nan), grad((size_t)M, 0.0);
  int32_t status = 2, n_iter = 0;
  double* d_cur = d_pi0.p;
  double* d_nxt = d_pi1.p;
  if (n_act > 0) {
    std::vector<uint8_t> recb(act.rec.size());
    std::vector<double> recn(act.rec.size());
    for (size_t k = 0; k < act.rec.size(); ++k) {
      recb[k] = (uint8_t)(keys[act.rec[k]] & 0xFF);
      recn[k] = (double)counts[act.rec[k]];
    }
    if (to_device(h, &d_marker, act.marker) || to_device(h, &d_recptr, act.rec_ptr) || to_device(h, &d_recb, recb) ||
        to_device(h, &d_recn, recn))
      return 1;
    if (dev_alloc(h, &d_wR.p, (size_t)n_act) || dev_alloc(h, &d_wA.p, (size_t)n_act) || dev_alloc(h, &d_ll.p, (size_t)n_act) ||
        dev_alloc(h, &d_part.p, (size_t)nblk * M) || dev_alloc(h, &d_llp.p, (size_t)nblk))
      return 1;
    // LL and grad at d_cur, pi' into d_nxt, (LL, step) to the host
    double scal[2];
    auto evaluate = [&]() -> int {
      reads_launch a = {n_act, d_marker.p, d_recptr.p, d_recb.p, d_recn.p, d_cur, d_wR.p, d_wA.p, d_ll.p, nullptr, nullptr};
      if (launch_reads(h, p, a)) return 1;
      hipLaunchKernelGGL(soup_mix_update_kernel, dim3((unsigned)nblk, (unsigned)((M + 63) / 64)), dim3(256), 0, h->stream, n_act,
                         d_marker.p, p, d_wR.p, d_wA.p, d_ll.p, d_part.p, d_llp.p);
      HIPCHK(h, hipGetLastError());
      hipLaunchKernelGGL(soup_mix_finish_kernel, dim3(1), dim3(256), 0, h->stream, nblk, M, N, d_part.p, d_llp.p, d_cur, d_nxt,
                         d_grad.p, d_scal.p);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(scal, d_scal.p, sizeof(scal), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      return 0;
    };
    for (int32_t i = 0;; ++i) {
      if (evaluate()) return 1;
      ll[(size_t)i] = scal[0];
      if (i == n_iter_max) {
        status = 1;
        break;
      }
      std::swap(d_cur, d_nxt);  // the step
      n_iter = i + 1;
      if (scal[1] <= tol) {  // converged: LL and grad once more, at the final pi
        if (evaluate()) return 1;
        ll[(size_t)i + 1] = scal[0];
        status = 0;
        break;
      }
    }
    HIPCHK(h, hipMemcpyAsync(grad.data(), d_grad.p, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(pi.data(), d_cur, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, h->stream));
  } else {
    ll[0] = 0.0;  // no record takes part: pi is the start, LL and grad are 0
  }
  std::vector<double> af;
  if (out.amb_af && S > 0) {
    af.resize((size_t)S);
    if (dev_alloc(h, &d_af.p, (size_t)S)) return 1;
    reads_launch a = {S, nullptr, nullptr, nullptr, nullptr, d_cur, nullptr, nullptr, nullptr, nullptr, d_af.p};
    if (launch_reads(h, p, a)) return 1;
    HIPCHK(h, hipMemcpyAsync(af.data(), d_af.p, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, h->stream));
  }
  if (ev.stop(h)) return 1;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ev.add();
  if (out.pi) memcpy(out.pi, pi.data(), sizeof(double) * (size_t)M);
  if (out.grad) memcpy(out.grad, grad.data(), sizeof(double) * (size_t)M);
  if (out.ll) memcpy(out.ll, ll.data(), sizeof(double) * ll.size());
  if (out.amb_af && S > 0) memcpy(out.amb_af, af.data(), sizeof(double) * (size_t)S);
  if (out.n_iter) *out.n_iter = n_iter;
  if (out.status) *out.status = status;
  if (out.n_reads) *out.n_reads = act.n_reads;
  return 0;
}

}  // namespace

int muxgl_pileup_read_hist(muxgl_handle* h, const uint8_t* cell_mask, int64_t* keys, int64_t* counts, int64_t cap, int64_t* n) {
  if (!h) return 1;
  if (!n) MUXGL_FAIL(h, "muxgl_pileup_read_hist: n is NULL");
  if (!(h->group ? h->group->have_pileup : h->d_cell_ptr != nullptr))
    MUXGL_FAIL(h, "muxgl_pileup_read_hist: no pileup set (muxgl_set_pileup)");
  if ((keys == nullptr) != (counts == nullptr)) MUXGL_FAIL(h, "muxgl_pileup_read_hist: keys and counts go together");
  std::vector<int64_t> k, c;
  if (read_hist_any(h, cell_mask, &k, &c)) return 1;
  *n = (int64_t)k.size();
  if (keys) {
    if (cap < *n) MUXGL_FAIL(h, "muxgl_pileup_read_hist: room for %lld records, %lld needed", (long long)cap, (long long)*n);
    if (!k.empty()) {
      memcpy(keys, k.data(), sizeof(int64_t) * k.size());
      memcpy(counts, c.data(), sizeof(int64_t) * c.size());
    }
  }
  return 0;
}

int muxgl_demux_soup_mix(muxgl_handle* h, const uint8_t* cell_mask, int64_t n_rec, const int64_t* keys, const int64_t* counts,
                         int32_t with_unknown, const double* gp0, const double* pi0, int32_t n_iter_max, double tol,
                         double* pi, double* grad, double* ll, double* amb_af, int32_t* n_iter, int64_t* n_reads,
                         int32_t* status, float* kernel_ms) {
  if (!h) return 1;
  if (kernel_ms) *kernel_ms = 0.f;
  const char* who = "muxgl_demux_soup_mix";
  muxgl_group* g = h->group;
  if (!(g ? g->have_pileup : h->d_cell_ptr != nullptr)) MUXGL_FAIL(h, "%s: no pileup set (muxgl_set_pileup)", who);
  if (!(g ? g->V >= 1 : h->d_gp != nullptr)) MUXGL_FAIL(h, "%s: no GP tensor set (muxgl_demux_set_gp)", who);
  const int64_t S = g ? g->S : h->S;
  const int V = g ? g->V : h->V;
  const int M = V + (with_unknown ? 1 : 0);
  if (!pi && !grad && !ll && !amb_af && !n_iter && !n_reads && !status) MUXGL_FAIL(h, "%s: every output is NULL", who);
  if (n_iter_max < 0) MUXGL_FAIL(h, "%s: n_iter_max=%d is negative", who, n_iter_max);
  if (!(std::isfinite(tol) && tol >= 0.0)) MUXGL_FAIL(h, "%s: tol (%g) is not a finite number >= 0", who, tol);
  if (keys) {
    if (cell_mask) MUXGL_FAIL(h, "%s: a histogram was passed in, so cell_mask must be NULL", who);
    if (n_rec < 0 || (n_rec > 0 && !counts)) MUXGL_FAIL(h, "%s: n_rec=%lld / counts do not describe a histogram", who, (long long)n_rec);
    int64_t at = 0;
    switch (sp::check_hist(n_rec, keys, counts, S, &at)) {
      case sp::HIST_UNSORTED: MUXGL_FAIL(h, "%s: keys are not strictly ascending at record %lld", who, (long long)at);
      case sp::HIST_MARKER: MUXGL_FAIL(h, "%s: key %lld of record %lld names no marker in [0, %lld)", who, (long long)keys[at], (long long)at, (long long)S);
      case sp::HIST_BYTE: MUXGL_FAIL(h, "%s: record %lld carries byte 0xFF (MUXGL_READ_OTHER is no usable read)", who, (long long)at);
      case sp::HIST_COUNT: MUXGL_FAIL(h, "%s: count %lld of record %lld is not above 0", who, (long long)counts[at], (long long)at);
      default: break;
    }
  }
  std::vector<double> start((size_t)M, 1.0 / (double)M);
  if (pi0) {
    double sum = 0.0;
    for (int v = 0; v < M; ++v) {
      if (!(std::isfinite(pi0[v]) && pi0[v] >= 0.0)) MUXGL_FAIL(h, "%s: pi0[%d] (%g) is negative or not finite", who, v, pi0[v]);
      sum += pi0[v];
    }
    if (!(sum > 0.0 && std::isfinite(sum))) MUXGL_FAIL(h, "%s: pi0 sums to %g", who, sum);
    for (int v = 0; v < M; ++v) start[(size_t)v] = pi0[v] / sum;
  }
  if (gp0)
    for (int64_t i = 0; i < S * 3; ++i)
      if (!(std::isfinite(gp0[i]) && gp0[i] >= 0.0))
        MUXGL_FAIL(h, "%s: gp0 of marker %lld (%g) is negative or not finite", who, (long long)(i / 3), gp0[i]);
  // (no clear_timing, no timing slot: the call reads state and changes none)
  std::vector<int64_t> own_k, own_c;
  if (!keys) {
    if (read_hist_any(h, cell_mask, &own_k, &own_c)) return 1;
    n_rec = (int64_t)own_k.size();
    keys = own_k.data();
    counts = own_c.data();
  }
  const mix_out out = {pi, grad, ll, amb_af, n_iter, status, n_reads};
  muxgl_handle* m = g ? g->m[0] : h;  // a group fits on one member, from the merged histogram
  HIPCHK(h, hipSetDevice(m->device));
  if (soup_mix_run(m, n_rec, keys, counts, with_unknown != 0, gp0, start, n_iter_max, tol, out, kernel_ms)) {
    if (m != h) h->err = "device group member 0: " + m->err;
    return 1;
  }
  return 0;
}
