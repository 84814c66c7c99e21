// fmx_anchor.hip -- freemuxlet with some clusters anchored to genotyped donors (muxgl_fmx_set_anchors[_mode]).
//
// A pool whose genotype panel is incomplete: clusters 0 .. n_anchor-1 take their genotype posteriors from the panel of
// muxgl_demux_set_gp, the others learn theirs from the droplets, in one EM.  Every E-step path and the three per-droplet
// tables read the posteriors from d_cgp [S][K][3], which fmx_cgp_kernel writes from the cluster pileups; anchoring is a
// second writer of the anchored columns, launched right behind it by fmx_phase_gp, and its twin in the exact path
// (rows_kernel, fmx_exact.hip; both through fmx_anchor_row.hpp).  Nothing else changes: the priors use the whole K and the
// M-step still merges the singlets of an anchored cluster into its pileup.
//
// An anchored cluster has a mode.  MUXGL_ANCHOR_HELD: the panel row is the posterior, and the pileup is a check on the
// panel's genotypes, not an input of the next E-step.  MUXGL_ANCHOR_PRIOR: the panel row is the PRIOR of the posterior the
// droplets form -- a free cluster whose Hardy-Weinberg triple in the product is the panel row (fmx_prior_row) --, so a
// vague or wrong genotype is refined by the droplets.  The PRIOR columns are a third writer, behind the second.
//
//   fmx_anchor_kernel  lane <-> (SNP of the handle's M-step range, anchored cluster): 24 bytes read or three divisions,
//                      24 bytes written; no LDS, no scratch
//   fmx_prior_kernel   lane <-> (SNP of the handle's M-step range, PRIOR cluster): the three diagonal doubles of the
//                      cluster's pileup row ([K][S][9], 72-byte stride: fmx_cgp_kernel's own reads) and 24 bytes of panel,
//                      three divisions, 24 bytes written; no LDS, no scratch
#include <vector>

#include "common.hpp"
#include "fmx_anchor_row.hpp"

namespace {

__global__ void __launch_bounds__(256)
    fmx_anchor_kernel(int64_t s0, int64_t s1, int K, int n_anchor, int V, const int32_t* __restrict__ donor,
                      const double* __restrict__ af, const double* __restrict__ gp, const uint8_t* __restrict__ has_gp,
                      double geno_error, double* __restrict__ cgp) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (s1 - s0) * n_anchor) return;
  const int64_t s = s0 + tid / n_anchor;
  const int i = (int)(tid % n_anchor);
  double o[3];
  fmx_anchor_row<false>(has_gp[s] != 0, gp + ((size_t)s * V + donor[i]) * 3, af[s], geno_error, o);
  double* out = cgp + ((size_t)s * K + i) * 3;
  out[0] = o[0];
  out[1] = o[1];
  out[2] = o[2];
}

// prior[j] < n_anchor <= K is the j-th PRIOR cluster, donor[prior[j]] < V its column of the panel
__global__ void __launch_bounds__(256)
    fmx_prior_kernel(int64_t S, int64_t s0, int64_t s1, int K, int n_prior, int V, const int32_t* __restrict__ prior,
                     const int32_t* __restrict__ donor, const double* __restrict__ af, const double* __restrict__ cgls,
                     const double* __restrict__ gp, const uint8_t* __restrict__ has_gp, double geno_error,
                     double* __restrict__ cgp) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (s1 - s0) * n_prior) return;
  const int64_t s = s0 + tid / n_prior;
  const int k = prior[tid % n_prior];
  const double* g = cgls + ((size_t)k * S + s) * 9;
  double o[3];
  fmx_prior_row<false>(has_gp[s] != 0, gp + ((size_t)s * V + donor[k]) * 3, g[0], g[4], g[8], af[s], geno_error, o);
  double* out = cgp + ((size_t)s * K + k) * 3;
  out[0] = o[0];
  out[1] = o[1];
  out[2] = o[2];
}

}  // namespace

// the anchored columns of d_cgp for the SNPs of the handle's M-step range, on the handle's stream (fmx_phase_gp, behind
// fmx_cgp_kernel): all of them as HELD, then the PRIOR ones again from the pileups of the M-step's owner
int fmx_anchor_launch(muxgl_handle* h, const muxgl_fmx_params* p) {
  const muxgl_handle* m = h->col ? h->col : h;
  const int64_t n = (m->fs1 - m->fs0) * h->n_anchor;
  if (n <= 0) return 0;
  if (!h->d_anchor || !h->d_gp || !h->d_has_gp || h->V < 1 || h->n_anchor > h->K)
    MUXGL_FAIL(h, "internal: anchors without their panel");  // (whoever drops the panel drops the anchors: fmx_anchors_drop)
  hipLaunchKernelGGL(fmx_anchor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, m->fs0, m->fs1, h->K,
                     h->n_anchor, h->V, h->d_anchor, h->d_af, h->d_gp, h->d_has_gp, p->geno_error, h->d_cgp);
  const int64_t np = (m->fs1 - m->fs0) * h->n_prior;
  if (np <= 0) return 0;
  if (!h->d_prior || !m->d_cgls || h->n_prior > h->n_anchor) MUXGL_FAIL(h, "internal: PRIOR anchors without their list");
  hipLaunchKernelGGL(fmx_prior_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, h->S, m->fs0, m->fs1,
                     h->K, h->n_prior, h->V, h->d_prior, h->d_anchor, h->d_af, m->d_cgls, h->d_gp, h->d_has_gp,
                     p->geno_error, h->d_cgp);
  return 0;
}

// muxgl_fmx_set_anchors_mode on one handle.  member: the handle is a device group's (its slabs are the library's own cut
// and every member holds the whole panel); a caller's own slabs or shard are refused
int fmx_set_anchors_on(muxgl_handle* h, int32_t n_anchor, const int32_t* donor, const uint8_t* mode, bool member) {
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->fmx_prepared || h->K < 1) MUXGL_FAIL(h, "muxgl_fmx_set_anchors: no clusters set (call muxgl_fmx_set_clusters first)");
  if (n_anchor < 0 || n_anchor > h->K)
    MUXGL_FAIL(h, "muxgl_fmx_set_anchors: n_anchor=%d outside [0, K=%d]", n_anchor, h->K);
  if (!member && h->col)
    MUXGL_FAIL(h, "muxgl_fmx_set_anchors: the handle holds slabs (muxgl_fmx_set_column_slab); anchors need a handle with "
                  "the whole job, or a device group");
  if (!member && (h->fc0 != 0 || h->fc1 != h->C || h->fs0 != 0 || h->fs1 != h->S))
    MUXGL_FAIL(h, "muxgl_fmx_set_anchors: the handle is sharded (muxgl_fmx_set_shard); anchors need a handle with the "
                  "whole job, or a device group");
  std::vector<int32_t> prior;
  if (n_anchor > 0) {
    if (h->V < 1 || !h->d_gp || !h->d_has_gp)
      MUXGL_FAIL(h, "muxgl_fmx_set_anchors: no genotype panel set (muxgl_demux_set_gp)");
    if (!donor) MUXGL_FAIL(h, "muxgl_fmx_set_anchors: donor is NULL with n_anchor=%d", n_anchor);
    for (int32_t i = 0; i < n_anchor; ++i)
      if (donor[i] < 0 || donor[i] >= h->V)
        MUXGL_FAIL(h, "muxgl_fmx_set_anchors: donor[%d]=%d outside [0, V=%d)", i, donor[i], h->V);
    for (int32_t i = 0; mode && i < n_anchor; ++i) {
      if (mode[i] != MUXGL_ANCHOR_HELD && mode[i] != MUXGL_ANCHOR_PRIOR)
        MUXGL_FAIL(h, "muxgl_fmx_set_anchors: mode[%d]=%d is neither MUXGL_ANCHOR_HELD (0) nor MUXGL_ANCHOR_PRIOR (1)", i,
                   (int)mode[i]);
      if (mode[i] == MUXGL_ANCHOR_PRIOR) prior.push_back(i);
    }
    // (pageable sources: the copies have left the caller's arrays when the call returns)
    std::vector<uint8_t> md((size_t)n_anchor, (uint8_t)MUXGL_ANCHOR_HELD);
    if (mode) md.assign(mode, mode + n_anchor);
    if (dev_alloc(h, &h->d_anchor, (size_t)n_anchor)) return 1;
    if (dev_alloc(h, &h->d_anchor_mode, (size_t)n_anchor)) return 1;
    if (!prior.empty() && dev_alloc(h, &h->d_prior, prior.size())) return 1;
    HIPCHK(h, hipMemcpyAsync(h->d_anchor, donor, sizeof(int32_t) * (size_t)n_anchor, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_anchor_mode, md.data(), (size_t)n_anchor, hipMemcpyHostToDevice, h->stream));
    if (!prior.empty())
      HIPCHK(h, hipMemcpyAsync(h->d_prior, prior.data(), sizeof(int32_t) * prior.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  h->n_anchor = n_anchor;
  h->n_prior = (int32_t)prior.size();
  // the posteriors of the next E-step are others than the last one's: no table of the last E-step, and the near-tie cells
  // settled under the old posteriors are settled again
  h->fmx_sng_state = FMX_SNG_NONE;
  h->xs_keep = false;
  ++h->xs_epoch;
  return 0;
}

// muxgl_fmx_get_cluster_gp on one handle: columns [k0, k1) of d_cgp as the last posterior phase left them
int fmx_get_cluster_gp_on(muxgl_handle* h, int32_t k0, int32_t k1, double* out) {
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->fmx_prepared || h->K < 1) MUXGL_FAIL(h, "muxgl_fmx_get_cluster_gp: no clusters set (call muxgl_fmx_set_clusters first)");
  if (!h->cgp_valid || !h->d_cgp)
    MUXGL_FAIL(h, "muxgl_fmx_get_cluster_gp: no posterior phase has run for these clusters (muxgl_fmx_iterate, muxgl_fmx_iter_gp)");
  if (k0 < 0 || k1 < k0 || k1 > h->K) MUXGL_FAIL(h, "muxgl_fmx_get_cluster_gp: [%d, %d) outside [0, K=%d]", k0, k1, h->K);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (k1 == k0 || h->S == 0) return 0;
  if (!out) MUXGL_FAIL(h, "muxgl_fmx_get_cluster_gp: NULL output");
  const size_t w = sizeof(double) * 3 * (size_t)(k1 - k0);
  HIPCHK(h, hipMemcpy2D(out, w, h->d_cgp + (size_t)k0 * 3, sizeof(double) * 3 * (size_t)h->K, w, (size_t)h->S,
                        hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int muxgl_fmx_set_anchors_mode(muxgl_handle* h, int32_t n_anchor, const int32_t* donor, const uint8_t* mode) {
  if (!h) return 1;
  if (h->group) return group_fmx_set_anchors(h, n_anchor, donor, mode);
  return fmx_set_anchors_on(h, n_anchor, donor, mode, false);
}

extern "C" int muxgl_fmx_set_anchors(muxgl_handle* h, int32_t n_anchor, const int32_t* donor) {
  return muxgl_fmx_set_anchors_mode(h, n_anchor, donor, nullptr);
}

extern "C" int muxgl_fmx_get_cluster_gp(muxgl_handle* h, int32_t k0, int32_t k1, double* out) {
  if (!h) return 1;
  if (h->group) return group_fmx_get_cluster_gp(h, k0, k1, out);
  return fmx_get_cluster_gp_on(h, k0, k1, out);
}
