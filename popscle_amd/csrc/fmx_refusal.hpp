// fmx_refusal.hpp -- when a freemuxlet call that reads the last E-step's posteriors (muxgl_fmx_singlets, _inclusion,
// _unknown, _ambient, _ambient_fit) cannot run, and what it says then.  Plain C++ (no HIP), so that
// tests/test_fmx_refusal.py compiles it on its own and holds the texts.
#pragma once
#include <cstddef>
#include <cstdio>

// muxgl_handle::fmx_sng_state: no E-step since muxgl_fmx_set_clusters; d_cgp holds the posteriors the last E-step read;
// a posterior phase has rewritten them since
enum { FMX_SNG_NONE = 0, FMX_SNG_READY = 1, FMX_SNG_STALE = 2 };

// 0: the call may run.  1: it may not, and `why` holds the reason under the call's name `who`; `what` is the call's
// result as the subject of the last rule ("the table belongs", "the tables belong", "the fit belongs").  The rules, in
// this order: a pileup is set, muxgl_fmx_prepare has run, clusters are set, an E-step has run since, and no posterior
// phase has rewritten d_cgp after it.
inline int fmx_table_refusal(const char* who, const char* what, bool have_pileup, bool prepared, int K, int sng_state,
                             char* why, size_t n) {
  if (!have_pileup) return snprintf(why, n, "%s: no pileup set (muxgl_set_pileup)", who), 1;
  if (!prepared) return snprintf(why, n, "%s: call muxgl_fmx_prepare first", who), 1;
  if (K < 1)
    return snprintf(why, n, "%s: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)", who), 1;
  if (sng_state == FMX_SNG_NONE)
    return snprintf(why, n, "%s: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep first)",
                    who),
           1;
  if (sng_state != FMX_SNG_READY)
    return snprintf(why, n,
                    "%s: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; %s to an E-step's "
                    "own posteriors: call it before the next iteration's posterior phase",
                    who, what),
           1;
  return 0;
}
