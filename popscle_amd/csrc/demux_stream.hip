// demux_stream.hip -- the streamed demuxlet call: any number of samples, device memory independent of C x V^2.
//
// The other paths materialise every hypothesis of a cell before the call reads them: the wave path's result slabs
// ([C][64 x 64 blocks][A][4096]) and, beyond 64 samples, the [C][V][V][A] tensor gathered from them.  The call only needs
// a few numbers per cell -- the top of each scan and two evidence sums -- so here the pair matrix is walked in 64 x 64
// blocks, a GROUP of (cells x blocks) at a time whose slab fits a fixed budget, and after each group a fold kernel merges
// the slab into a running state per cell; the slab is then reused.  A last kernel makes the call from that state with
// demux_call_decide (demux_call_body.hpp), the code every other call kernel ends in.
//
// Reference being replaced: cmd_cram_demuxlet.cpp:733-747 (pair sweep), :788-991 (evidence, scans, call).
//
// Why not the wave kernels of demux_wave.hip on these blocks: they would need to be edited (their entry points, plan and
// work units live in that file's anonymous namespace), and the machine code of the headline paths must not change.  The
// sweep here is the same arithmetic -- u = g_j . pG per (entry, alpha), then g_k . u per hypothesis, as a product in
// mantissa / exponent form with one log per hypothesis -- in a plainer mapping: lane = sample j of the block, the wave's
// KT partner samples k are wave-uniform (scalar loads), all alphas of the grid in one launch.
//
// State per cell (stream_state): the top-two (value, scan position) of the singlet and of the doublet scan plus the third
// value of each (muxgl_call::top2), and the evidence sums as (largest term, sum relative to it) for sumLLK and sngLLK.
// Ordering rule: value descending, then scan position ascending (muxgl_call::key_before), which is what the reference's
// update rule (bv < v, then nv < v) leaves; it is a total order, so the top-two do not depend on grouping.  Scan
// positions: j for singlets, (j V + k) A + n for doublets.  An alpha = 0.5 pair is listed once, as (lo, hi), with the
// value computed in the (hi, lo) orientation; demux_call_decide names its mirror the runner-up.
// Determinism: a block's partial is reduced in a fixed tree, and a cell's partials are merged into its state in block
// order, whatever the budget cuts: records are bit-identical across budgets (tests/test_demux_many_samples_gpu.py).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "demux_call_body.hpp"

namespace {

using namespace muxgl_call;

constexpr int SBLK = 64;                     // samples per side of a block of the pair matrix
constexpr int SLAB_DOUBLES = SBLK * SBLK;    // per alpha and block: [k][j]

struct stream_state {
  top2 sng, dbl;
  double M, S, Ms, Ss;  // evidence: largest term, sum of exp(term - M); the same for the singlet terms
};

// merge of two partials (a first in block order: the LSE merge is one fixed expression, so the order fixes the bits)
__device__ __forceinline__ stream_state merge_state(const stream_state& a, const stream_state& b) {
  stream_state r;
  r.sng = top2_merge<true>(a.sng, b.sng);
  r.dbl = top2_merge<true>(a.dbl, b.dbl);
  r.M = fmax(a.M, b.M);
  r.S = (a.S > 0.0 ? a.S * exp_nonpos(a.M - r.M) : 0.0) + (b.S > 0.0 ? b.S * exp_nonpos(b.M - r.M) : 0.0);
  r.Ms = fmax(a.Ms, b.Ms);
  r.Ss = (a.Ss > 0.0 ? a.Ss * exp_nonpos(a.Ms - r.Ms) : 0.0) + (b.Ss > 0.0 ? b.Ss * exp_nonpos(b.Ms - r.Ms) : 0.0);
  return r;
}

__device__ __forceinline__ stream_state empty_state() {
  stream_state s;
  s.sng = top2{-1e300, -1e300, -1, -1, -1e300};
  s.dbl = s.sng;
  s.M = s.Ms = -__builtin_huge_val();
  s.S = s.Ss = 0.0;
  return s;
}

// one more term of a running (largest term, sum relative to it)
__device__ __forceinline__ void lse_push(double& M, double& S, double t) {
  if (!(t > -__builtin_huge_val())) return;  // exp(-inf) adds nothing
  if (t > M) {
    S = (S > 0.0 ? S * exp_nonpos(M - t) : 0.0) + 1.0;
    M = t;
  } else {
    S += exp_nonpos(t - M);
  }
}

__global__ void __launch_bounds__(256) stream_init_kernel(int64_t n, stream_state* __restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st[i] = empty_state();
}

// Sweep of one group: grid = (cells of the group, 64 / (4 KT) sub-tiles, blocks of the group).  Lane j of wave w owns
// sample jbase + j and the KT partners kbase + 4 KT y + KT w + i; NA >= A - 1 accumulators per pair (alphas 1 .. A - 1),
// and lanes of the sub-tile holding k = 0 also the singlet slot (j, 0, alpha 0) (:806,828).
// slab[cell - c0][block of group][n][k][j].  Markers without genotypes are skipped (:733), wave-uniformly.
template <int NA, int KT>
__global__ void __launch_bounds__(256)
    stream_sweep_kernel(int64_t c0, int32_t b0, const int32_t* __restrict__ blocks, int nblk,
                        const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ entry_snp,
                        const double* __restrict__ pg, const uint8_t* __restrict__ has_gp, const double* __restrict__ gp,
                        int V, int nAlpha, double* __restrict__ slab) {
  const int64_t c = c0 + blockIdx.x;
  const int64_t e0 = cell_ptr[c], e1 = cell_ptr[c + 1];
  if (e0 == e1) return;
  const int b = blocks[b0 + (int)blockIdx.z];
  const int X = b / nblk, Y = b - X * nblk;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = SBLK * X + lane;
  const int kk0 = 4 * KT * (int)blockIdx.y + KT * w;  // first partner of the wave, inside the block
  const int kb = SBLK * Y + kk0;
  const bool jl = j < V;
  const bool with_singlet = kb == 0;  // wave-uniform
  const int V3 = V * 3;
  const int PG = nAlpha * 9;
  const int jo = (jl ? j : V - 1) * 3;
  int ko[KT];  // (no sample: any valid row; the fold never reads those slots)
#pragma unroll
  for (int i = 0; i < KT; ++i) ko[i] = (kb + i < V ? kb + i : V - 1) * 3;

  double acc[KT][NA], accS = 1.0;
  int32_t ex[KT][NA], exS = 0;
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[i][a] = 1.0, ex[i][a] = 0;

  int cnt = 0;
  for (int64_t e = e0; e < e1; ++e) {
    const int32_t s = entry_snp[e];
    if (!has_gp[s]) continue;
    const double* row = gp + (size_t)s * V3;
    const double* q = pg + (size_t)e * PG;
    const double g0 = jl ? row[jo] : 1.0, g1 = jl ? row[jo + 1] : 0.0, g2 = jl ? row[jo + 2] : 0.0;
    double u[NA][3];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const double* qa = q + (size_t)(a + 1 < nAlpha ? a + 1 : 0) * 9;
#pragma unroll
      for (int m = 0; m < 3; ++m) u[a][m] = fma(g2, qa[6 + m], fma(g1, qa[3 + m], g0 * qa[m]));
    }
    if (with_singlet) {  // llksAB[j][0][0]: alpha 0 against sample 0's triple
      const double v0 = fma(g2, q[6], fma(g1, q[3], g0 * q[0]));
      const double v1 = fma(g2, q[7], fma(g1, q[4], g0 * q[1]));
      const double v2 = fma(g2, q[8], fma(g1, q[5], g0 * q[2]));
      accS *= fma(row[2], v2, fma(row[1], v1, row[0] * v0));
    }
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      const double h0 = row[ko[i]], h1 = row[ko[i] + 1], h2 = row[ko[i] + 2];
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[i][a] *= fma(h2, u[a][2], fma(h1, u[a][1], h0 * u[a][0]));  // :738-746
    }
    if (++cnt == 16) {  // every factor is >= ~1e-11: sixteen of them cannot underflow
      cnt = 0;
#pragma unroll
      for (int i = 0; i < KT; ++i)
#pragma unroll
        for (int a = 0; a < NA; ++a) prodacc_renorm(acc[i][a], ex[i][a]);
      prodacc_renorm(accS, exS);
    }
  }

  double* out = slab + ((size_t)blockIdx.x * gridDim.z + blockIdx.z) * nAlpha * SLAB_DOUBLES;
#pragma unroll
  for (int i = 0; i < KT; ++i)
#pragma unroll
    for (int a = 0; a < NA; ++a)
      if (a + 1 < nAlpha) out[((size_t)(a + 1) * SBLK + kk0 + i) * SBLK + lane] = prodacc_log(acc[i][a], ex[i][a]);
  if (with_singlet) out[lane] = prodacc_log(accS, exS);  // slot (n = 0, k = 0)
}

template <int M>
__device__ __forceinline__ stream_state state_partner(const stream_state& s) {
  stream_state o;
  o.sng = top2_partner<M, true>(s.sng);
  o.dbl = top2_partner<M, true>(s.dbl);
  o.M = lane_partner<M>(s.M);
  o.S = lane_partner<M>(s.S);
  o.Ms = lane_partner<M>(s.Ms);
  o.Ss = lane_partner<M>(s.Ss);
  return o;
}

// Fold of one group: one workgroup per cell of the group; the group's blocks in order, each reduced over the workgroup
// in a fixed tree (thread -> wave butterfly -> the four waves in order) and merged into the cell's state.
__global__ void __launch_bounds__(256)
    stream_fold_kernel(int64_t c0, int32_t b0, int32_t nb, const int32_t* __restrict__ blocks, int nblk,
                       const int64_t* __restrict__ cell_ptr, int V, int nAlpha, call_alpha al,
                       const double* __restrict__ slab, stream_state* __restrict__ state) {
  __shared__ stream_state parts[4];
  const int64_t c = c0 + blockIdx.x;
  if (cell_ptr[c] == cell_ptr[c + 1]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  stream_state st = state[c];  // (read by every thread, written by thread 0 at the end)
  for (int z = 0; z < nb; ++z) {
    const int b = blocks[b0 + z];
    const int X = b / nblk, Y = b - X * nblk;
    const int j = SBLK * X + lane;
    const double* in = slab + ((size_t)blockIdx.x * nb + z) * nAlpha * SLAB_DOUBLES;
    stream_state t = empty_state();
    if (j < V) {
      if (Y == 0 && w == 0) {  // singlet of sample j (:806,828)
        const double v = in[lane];
        top2_insert(t.sng, v, j);
        const double term = v + al.log_single_prior;
        lse_push(t.M, t.S, term);
        lse_push(t.Ms, t.Ss, term);
      }
      for (int kq = 16 * w; kq < 16 * w + 16; ++kq) {
        const int k = SBLK * Y + kq;
        if (k >= V || k == j) continue;
        for (int n = 1; n < nAlpha; ++n) {
          const double v = in[((size_t)n * SBLK + kq) * SBLK + lane];
          if (al.a[n] == 0.5) {  // (hi, lo) orientation only, listed as (lo, hi): see the header
            if (k > j) continue;
            lse_push(t.M, t.S, v + al.log_doublet_prior2);  // :812-815
            top2_insert(t.dbl, v, (k * V + j) * nAlpha + n);
          } else {
            lse_push(t.M, t.S, v + al.log_doublet_prior1);
            top2_insert(t.dbl, v, (j * V + k) * nAlpha + n);
          }
        }
      }
    }
    wave_for<0, 6>([&](auto sc) {
      constexpr int m = 1 << decltype(sc)::value;
      t = merge_state(t, state_partner<m>(t));
    });
    if (lane == 0) parts[w] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      stream_state r = merge_state(merge_state(parts[0], parts[1]), merge_state(parts[2], parts[3]));
      st = merge_state(st, r);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) state[c] = st;
}

// the call from the state: one lane per cell (demux_call_decide's note)
__global__ void __launch_bounds__(64)
    stream_call_kernel(int64_t C, const int64_t* __restrict__ cell_ptr, int V, int nAlpha, call_alpha al,
                       const stream_state* __restrict__ state, muxgl_demux_cell* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const stream_state& s = state[c];
  const call_partial cp{s.sng, s.dbl, s.M, s.S, s.Ms, s.Ss};
  demux_call_decide(cp, (int32_t)(cell_ptr[c + 1] - cell_ptr[c]), V, nAlpha, al, out + c);
}

template <int NA, int KT>
void launch_sweep(muxgl_handle* h, int64_t c0, int64_t nc, int32_t b0, int32_t nb, const int32_t* d_blocks, int nblk,
                  const double* d_pg, int A, double* d_slab) {
  hipLaunchKernelGGL((stream_sweep_kernel<NA, KT>), dim3((unsigned)nc, (unsigned)(SBLK / (4 * KT)), (unsigned)nb),
                     dim3(256), 0, h->stream, c0, b0, d_blocks, nblk, h->d_cell_ptr, h->d_entry_snp, d_pg, h->d_has_gp,
                     h->d_gp, h->V, A, d_slab);
}

int sweep_dispatch(muxgl_handle* h, int64_t c0, int64_t nc, int32_t b0, int32_t nb, const int32_t* d_blocks, int nblk,
                   const double* d_pg, int A, double* d_slab) {
  const int na = A - 1;  // alphas 1 .. A - 1 (A >= 2)
#define SW(NA, KT) launch_sweep<NA, KT>(h, c0, nc, b0, nb, d_blocks, nblk, d_pg, A, d_slab)
  if (na <= 1) SW(1, 16);
  else if (na <= 2) SW(2, 8);
  else if (na <= 4) SW(4, 8);
  else if (na <= 6) SW(6, 4);
  else if (na <= 8) SW(8, 4);
  else if (na <= 12) SW(12, 2);
  else SW(15, 2);
#undef SW
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // namespace

// slab budget in bytes: MUXGL_DEMUX_SLAB_MB, else 4 GiB bounded by a third of the device's memory (the handle cache's cap)
static size_t stream_budget() {
  if (const char* s = getenv("MUXGL_DEMUX_SLAB_MB")) {
    const long long mb = atoll(s);
    if (mb > 0) return (size_t)mb << 20;
  }
  size_t fr = 0, tot = 0;
  size_t b = (size_t)4 << 30;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot > 0) b = std::min(b, tot / 3);
  return b;
}

int demux_stream_launch(muxgl_handle* h, const muxgl_demux_params* p) {
  const int V = h->V, A = p->n_alpha;
  if (A < 2) MUXGL_FAIL(h, "streamed demuxlet call: the alpha grid needs a doublet alpha (n_alpha >= 2)");
  if ((double)V * V * A >= 2147483648.0)
    MUXGL_FAIL(h, "streamed demuxlet call: V=%d with %d alphas exceeds the int32 scan positions (V*V*n_alpha < 2^31)", V, A);
  if (h->want_full_ll)
    MUXGL_FAIL(h, "muxgl_demux_run: full_ll is not available on the streamed path (V=%d; more than 255 samples, a job whose "
                  "[C][V][V][A] tensor does not fit the device, or MUXGL_FLAG_FORCE_STREAMED_CALL): pass full_ll = NULL", V);
  const int nblk = (V + SBLK - 1) / SBLK;
  bool all_sym = true;
  for (int n = 1; n < A; ++n) all_sym = all_sym && p->alpha[n] == 0.5;
  // blocks that hold a hypothesis the call reads: with alpha = 0.5 only the (hi, lo) orientation, and the singlets in Y = 0
  std::vector<int32_t> blocks;
  for (int X = 0; X < nblk; ++X)
    for (int Y = 0; Y < nblk; ++Y)
      if (!all_sym || X >= Y) blocks.push_back(X * nblk + Y);
  const int64_t nb_all = (int64_t)blocks.size();
  const size_t per = (size_t)A * SLAB_DOUBLES * sizeof(double);  // one (cell, block) of the slab
  const size_t budget = std::max(stream_budget(), per);
  // groups: all cells x as many blocks as fit; if one block of every cell does not fit, one block x as many cells as fit
  int64_t gb, gc;
  if ((size_t)h->C * per <= budget) {
    gc = h->C;
    gb = std::min<int64_t>(nb_all, (int64_t)(budget / ((size_t)h->C * per)));
  } else {
    gb = 1;
    gc = (int64_t)(budget / per);
  }
  gb = std::min<int64_t>(gb, 65535);
  gc = std::min<int64_t>(gc, (int64_t)1 << 30);

  int32_t* d_blocks = nullptr;
  double* d_pg = nullptr;
  double* d_slab = nullptr;
  stream_state* d_state = nullptr;
  auto run = [&]() -> int {
    if (dev_alloc(h, &d_blocks, blocks.size())) return 1;
    if (dev_alloc(h, &d_pg, (size_t)h->nnz * A * 9)) return 1;
    if (dev_alloc(h, &d_slab, (size_t)gc * gb * A * SLAB_DOUBLES)) return 1;
    if (dev_alloc(h, &d_state, (size_t)h->C)) return 1;
    HIPCHK(h, hipMemcpyAsync(d_blocks, blocks.data(), sizeof(int32_t) * blocks.size(), hipMemcpyHostToDevice, h->stream));
    tic(h, MUXGL_T_DEMUX_SWEEP);
    if (demux_entry_pg_launch(h, p, d_pg)) return 1;
    hipLaunchKernelGGL(stream_init_kernel, dim3((unsigned)((h->C + 255) / 256)), dim3(256), 0, h->stream, h->C, d_state);
    HIPCHK(h, hipGetLastError());
    const call_alpha al = make_call_alpha(p, V);
    for (int64_t c0 = 0; c0 < h->C; c0 += gc) {
      const int64_t nc = std::min(gc, h->C - c0);
      for (int64_t b0 = 0; b0 < nb_all; b0 += gb) {  // blocks in order: see the header (determinism)
        const int32_t nb = (int32_t)std::min(gb, nb_all - b0);
        if (sweep_dispatch(h, c0, nc, (int32_t)b0, nb, d_blocks, nblk, d_pg, A, d_slab)) return 1;
        hipLaunchKernelGGL(stream_fold_kernel, dim3((unsigned)nc), dim3(256), 0, h->stream, c0, (int32_t)b0, nb, d_blocks,
                           nblk, h->d_cell_ptr, V, A, al, d_slab, d_state);
        HIPCHK(h, hipGetLastError());
      }
    }
    toc(h, MUXGL_T_DEMUX_SWEEP);
    tic(h, MUXGL_T_DEMUX_CALL);
    hipLaunchKernelGGL(stream_call_kernel, dim3((unsigned)((h->C + 63) / 64)), dim3(64), 0, h->stream, h->C, h->d_cell_ptr,
                       V, A, al, d_state, h->d_dcells);
    HIPCHK(h, hipGetLastError());
    toc(h, MUXGL_T_DEMUX_CALL);
    return 0;
  };
  const int rc = run();
  dev_free(&d_blocks);
  dev_free(&d_pg);
  dev_free(&d_slab);
  dev_free(&d_state);
  return rc;
}
