// fmx_stream.hip -- the streamed freemuxlet E-step and call: up to MUXGL_MAX_CLUSTERS clusters, device memory independent
// of C x K^2.
//
// Every other E-step writes the whole [C][K(K+1)/2] table d_fll, which the call kernel then scans (263 KB a cell at
// K = 256, 4.2 MB at K = 1024).  The call only needs a few numbers per cell: the best, next and third value of each scan
// and the two evidence sums.  So here the pair matrix is walked in 64 x 64 blocks of clusters (X >= Y), a GROUP of
// (cells x blocks) at a time whose slab fits a fixed budget; after each group a fold kernel merges the slab into a running
// state per cell, and the slab is reused.  A last kernel makes the call from that state with the tail every freemuxlet call
// kernel ends in (fmx_call_finish.inc).  The design of demux_stream.hip, with the entry's nine genotype-pair likelihoods in
// the role of pG; the two share the groups and the block list (stream_plan.hpp) and the state and its fold
// (stream_fold.hpp).  The sweep kernel, its launch and block_hyps are in fmx_stream_sweep.hpp, which fmx_incl.hip includes
// too.
//
// Reference being replaced: cmd_cram_freemux2.cpp:383-456 (E-step), :458-513 (scans), :515-584 (re-assignment).
//
// Arithmetic.  Each hypothesis is the factor and the product order of the wave E-step (fmx_wave.hip), in a plainer
// mapping, so that a job below 256 clusters gets the wave path's log-likelihoods bit for bit on this path:
//   * diagonal block X = Y: lane j holds cluster 64X + j; wave w takes the rotations t = 8w + 1 .. 8w + 8 of the wave
//     kernel (partner 64X + ((j - t) mod 64), rotation 32 written by the higher lane only), so every pair is formed by the
//     lane and in the orientation the wave kernel forms it.  With linear entries (MUXGL_FLAG_NO_LINEAR_ENTRIES unset) those
//     come first, in the one-moment form c0 + c1 (E_j + E_k), then the others; without MUXGL_FLAG_NO_PIVOT_SUMS the others'
//     pair sums are taken around the lane's smallest u.  Slot t - 1 of the block's slab holds rotation t, slot 32 the
//     singlet (the diagonal of glis);
//   * off-diagonal block X > Y: lane j holds cluster 64X + j and wave w the partners 64Y + 16w .. 64Y + 16w + 15, every
//     entry in entry order through the three-term sum; slot k holds partner 64Y + k;
//   * a cell of more than 2048 entries is cut into the parts of the wave plan (demux_wave_plan): one product per part,
//     their logs added in entry order, as fmx_wave_combine_kernel does.  The sweep walks a cell's parts itself, so nothing
//     else is needed for long cells.
// Products are mantissa x 2^exponent with one log per (cell, hypothesis); the renormalisation points do not change a bit
// (scaling by powers of two is exact, and pos_log takes the exponent apart itself).
//
// State per cell (stream_fold.hpp, which also says why records are bit-identical whatever the budget): fmx_top2 of the
// singlet and of the doublet scan (value, position p = j(j+1)/2 + k, and the third value), the evidence sums of all
// hypotheses with their priors and of the singlets without.  Order: value descending, then position ascending
// (fmx_better) -- the order fmx_top2_push and the reference's strict `>` updates leave.
#include <algorithm>
#include <vector>

#include "fmx_call_body.hpp"
#include "fmx_stream_sweep.hpp"
#include "stream_fold.hpp"

namespace {

constexpr int32_t NO_POS = 0x7fffffff;

// the lists of the state and their butterfly: xor pairings
struct fmx_top2_ops {
  using list = fmx_top2;
  static __device__ __forceinline__ fmx_top2 empty() { return fmx_top2{-1e300, -1e300, NO_POS, NO_POS, -1e300}; }
  static __device__ __forceinline__ fmx_top2 merge(fmx_top2 a, const fmx_top2& b) {  // a first
    fmx_top2_push(a, b.v1, b.p1);
    fmx_top2_push(a, b.v2, b.p2);
    a.v3 = fmax(a.v3, b.v3);  // (b.v1 >= b.v2 >= b.v3 are all in the union: b.v3 can be its third at best)
    return a;
  }
  template <int M>
  static __device__ __forceinline__ fmx_top2 partner(const fmx_top2& t) {
    return fmx_top2{__shfl_xor(t.v1, M, 64), __shfl_xor(t.v2, M, 64), __shfl_xor(t.p1, M, 64), __shfl_xor(t.p2, M, 64),
                    __shfl_xor(t.v3, M, 64)};
  }
  template <int M>
  static __device__ __forceinline__ double partner(double x) { return __shfl_xor(x, M, 64); }
};
using fmx_stream_state = stream_fold::stream_state<fmx_top2_ops>;
constexpr int STATE_DOUBLES = (int)(sizeof(fmx_stream_state) / sizeof(double));
static_assert(sizeof(fmx_stream_state) % sizeof(double) == 0, "the state is kept in a double buffer");

// Fold of one group: one workgroup per cell of the group (stream_fold::fold_blocks)
__global__ void __launch_bounds__(256)
    fmx_stream_fold_kernel(int64_t c0, int32_t b0, int32_t nb, const int32_t* __restrict__ blocks, int K,
                           double log_single_prior, double log_double_prior, const double* __restrict__ slab,
                           fmx_stream_state* __restrict__ state) {
  const int j = threadIdx.x & 63, w = threadIdx.x >> 6;
  stream_fold::fold_blocks(nb, state + (c0 + blockIdx.x), [&](int z, fmx_stream_state& t) {
    const int bz = blocks[b0 + z];
    const int X = bz >> 16, Y = bz & 0xffff;
    const double* in = slab + ((size_t)blockIdx.x * nb + z) * SLAB;
    block_hyps(X, Y, w, j, K, in, [&](int p, double v, bool singlet) {
      if (singlet) {
        fmx_top2_push(t.sng, v, p);
        t.all.push(v + log_single_prior);
        t.sgl.push(v);
      } else {
        fmx_top2_push(t.dbl, v, p);
        t.all.push(v + log_double_prior);
      }
    });
  });
}

__device__ __forceinline__ int row_of(int p) {
  int r = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= p) ++r;
  while (r * (r + 1) / 2 > p) --r;
  return r;
}

// the call of cells [c0, c1) from their states (state[i - c0]): one lane per cell
template <bool FMX_WIDE_PREV>
__global__ void __launch_bounds__(64)
    fmx_stream_call_kernel(int64_t c0, int64_t c1, double log_single_prior, double log_double_prior,
                           const fmx_stream_state* __restrict__ state, muxgl_fmx_cell* __restrict__ cells,
                           int32_t* __restrict__ clust, int32_t* __restrict__ stat, int32_t* __restrict__ prev_state,
                           int32_t* __restrict__ flagged, const int32_t* __restrict__ xc_epoch,
                           const fmx_xc* __restrict__ xc, int32_t epoch) {
  const int64_t i = c0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c1) return;
  const fmx_stream_state s = state[i - c0];
  int32_t sBest = -1, sNext = -1, dBest1 = -1, dBest2 = -1, dNext1 = -1, dNext2 = -1;
  double sngBestLLK = -1e300, sngNextLLK = -1e300, dblBestLLK = -1e300, dblNextLLK = -1e300;
  double sumLLK = -1e300, sngLLK = -1e300;
  if (s.all.S > 0.0) sumLLK = s.all.M + log(s.all.S);
  if (s.sgl.S > 0.0) sngLLK = s.sgl.M + log_single_prior + log(s.sgl.S);
  if (s.sng.p1 != NO_POS) sBest = row_of(s.sng.p1), sngBestLLK = s.sng.v1;
  if (s.sng.p2 != NO_POS) sNext = row_of(s.sng.p2), sngNextLLK = s.sng.v2;
  if (s.dbl.p1 != NO_POS) dBest1 = row_of(s.dbl.p1), dBest2 = s.dbl.p1 - dBest1 * (dBest1 + 1) / 2, dblBestLLK = s.dbl.v1;
  if (s.dbl.p2 != NO_POS) dNext1 = row_of(s.dbl.p2), dNext2 = s.dbl.p2 - dNext1 * (dNext1 + 1) / 2, dblNextLLK = s.dbl.v2;
  double sngThird = s.sng.v3, dblThird = s.dbl.v3;
#include "fmx_call_finish.inc"
}

// rows[x][p] = the E-step's value of hypothesis p of cell x of the batch, from a sweep over all blocks
__global__ void __launch_bounds__(256)
    fmx_stream_rows_kernel(int32_t nb, const int32_t* __restrict__ blocks, int K, const double* __restrict__ slab,
                           double* __restrict__ rows) {
  const int z = blockIdx.y;
  const int bz = blocks[z];
  const int X = bz >> 16, Y = bz & 0xffff;
  const int j = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double* in = slab + ((size_t)blockIdx.x * nb + z) * SLAB;
  double* row = rows + (size_t)blockIdx.x * ((size_t)K * (K + 1) / 2);
  block_hyps(X, Y, w, j, K, in, [&](int p, double v, bool) { row[p] = v; });
}


}  // namespace

// E-step of the cell shard [c0, c0 + nc) into the per-cell states (h->d_fss); the call follows in fmx_stream_call_launch
int fmx_stream_estep_launch(muxgl_handle* h, const muxgl_fmx_params* p, int64_t c0, int64_t nc) {
  const int K = h->K;
  const std::vector<int32_t> blocks = block_list(K);
  const int64_t nb_all = (int64_t)blocks.size();
  const size_t per = (size_t)SLAB * sizeof(double);  // one (cell, block) of the slab
  // (sized here, before anything is enqueued)
  const auto [gc, gb] = stream_plan::cut_groups(nc, nb_all, per, dev_slab_budget("MUXGL_FMX_SLAB_MB"));
  const size_t slab_n = (size_t)gc * gb * SLAB, st_n = (size_t)nc * STATE_DOUBLES;
  if (h->fblocks_k != K) {
    if (dev_alloc(h, &h->d_fblocks, blocks.size())) return 1;
    HIPCHK(h, hipMemcpyAsync(h->d_fblocks, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, h->stream));
    h->fblocks_k = K;
  }
  if (h->fslab_cap < slab_n) {
    if (dev_alloc(h, &h->d_fslab, slab_n)) return 1;
    h->fslab_cap = slab_n;
  }
  if (h->fss_cap < st_n) {
    if (dev_alloc(h, &h->d_fss, st_n)) return 1;
    h->fss_cap = st_n;
  }
  fmx_stream_state* st = reinterpret_cast<fmx_stream_state*>(h->d_fss);
  hipLaunchKernelGGL(stream_fold::stream_init_kernel<fmx_top2_ops>, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0,
                     h->stream, nc, st);
  HIPCHK(h, hipGetLastError());
  const double lsp = log((1.0 - p->doublet_prior) / K);          // cmd_cram_freemux2.cpp:379
  const double ldp = log(p->doublet_prior / K / (K - 1) * 2.0);  // :380
  tic(h, MUXGL_T_FMX_ESTEP_SWEEP);
  for (int64_t g0 = 0; g0 < nc; g0 += gc) {
    const int64_t ng = std::min(gc, nc - g0);
    for (int64_t b0 = 0; b0 < nb_all; b0 += gb) {  // blocks in order: stream_fold.hpp (determinism)
      const int32_t nb = (int32_t)std::min(gb, nb_all - b0);
      if (sweep_launch(h, c0 + g0, nullptr, ng, (int32_t)b0, nb, h->d_fblocks, h->d_fslab)) return 1;
      hipLaunchKernelGGL(fmx_stream_fold_kernel, dim3((unsigned)ng), dim3(256), 0, h->stream, g0, (int32_t)b0, nb,
                         h->d_fblocks, K, lsp, ldp, h->d_fslab, st);
      HIPCHK(h, hipGetLastError());
    }
  }
  toc(h, MUXGL_T_FMX_ESTEP_SWEEP);
  return 0;
}

int fmx_stream_call_launch(muxgl_handle* h, int64_t c0, int64_t c1, double lsp, double ldp) {
  const int64_t nc = c1 - c0;
  const fmx_stream_state* st = reinterpret_cast<const fmx_stream_state*>(h->d_fss);
#define CALL(WIDE)                                                                                                   \
  hipLaunchKernelGGL(fmx_stream_call_kernel<WIDE>, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, h->stream, c0, c1, \
                     lsp, ldp, st, h->d_fcells, h->d_clust, h->d_fstat, h->d_prev_state, h->d_flagged, h->d_xc_epoch,  \
                     h->d_xc, h->xs_epoch)
  if (h->K > 255) CALL(true);
  else CALL(false);
#undef CALL
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The E-step's rows [n][K(K+1)/2] of the cells cells[0..n) (host ids), into rows (host), for the exact pass's deep ties
// (fmx_exact.hip): swept again over all blocks, in batches whose slab fits the budget.  Uses the cluster posteriors of the
// running iteration (d_cgp), as the E-step did.
int fmx_stream_rows(muxgl_handle* h, const std::vector<int32_t>& cells, double* rows) {
  const int K = h->K;
  const size_t npairs = (size_t)K * (K + 1) / 2;
  const int64_t n = (int64_t)cells.size();
  if (n == 0) return 0;
  const std::vector<int32_t> blocks = block_list(K);
  const int32_t nb = (int32_t)blocks.size();
  const size_t per_cell = (size_t)nb * SLAB * sizeof(double) + npairs * sizeof(double);
  const int64_t batch =
      std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(dev_slab_budget("MUXGL_FMX_SLAB_MB") / per_cell)));
  dev_tmp<int32_t> d_blocks, d_cells;
  dev_tmp<double> d_slab, d_rows;
  if (dev_alloc(h, &d_blocks.p, blocks.size()) || dev_alloc(h, &d_cells.p, (size_t)n) ||
      dev_alloc(h, &d_slab.p, (size_t)batch * nb * SLAB) || dev_alloc(h, &d_rows.p, (size_t)batch * npairs))
    return 1;
  HIPCHK(h, hipMemcpyAsync(d_blocks.p, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_cells.p, cells.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  for (int64_t x0 = 0; x0 < n; x0 += batch) {
    const int64_t m = std::min(batch, n - x0);
    if (sweep_launch(h, x0, d_cells.p, m, 0, nb, d_blocks.p, d_slab.p)) return 1;
    hipLaunchKernelGGL(fmx_stream_rows_kernel, dim3((unsigned)m, (unsigned)nb), dim3(256), 0, h->stream, nb, d_blocks.p, K,
                       d_slab.p, d_rows.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(rows + (size_t)x0 * npairs, d_rows.p, sizeof(double) * (size_t)m * npairs,
                             hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return 0;
}
