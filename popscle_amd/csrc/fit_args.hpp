// fit_args.hpp -- what the four per-droplet fits (muxgl_demux_ambient_fit, muxgl_demux_alpha_fit, muxgl_fmx_ambient_fit,
// muxgl_fmx_alpha_fit) refuse in their arguments, and what they say then: checked on the host before any device work, by
// the call itself and, once for all members, by its group driver (muxgl_group.hip).  Plain C++ (no HIP), so that
// tests/test_fit_args.py compiles it on its own and holds the texts.  Every rule returns 0, or 1 with the reason in `why`.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/muxgl.h"

namespace ambient_fit {

// the arguments every fit checks alike before its indices.  null_arg: the name of a pointer argument that is NULL, or
// NULL; bound: the name of x_max ("rho_max", "alpha_max")
inline int bad_head(const char* who, int32_t n_cand, const char* null_arg, const char* bound, double x_max, bool any_out,
                    char* why, size_t n) {
  if (!any_out) return snprintf(why, n, "%s: every output is NULL", who), 1;
  if (n_cand < 1 || n_cand > MUXGL_MAX_FIT_CAND)
    return snprintf(why, n, "%s: n_cand=%d outside [1,%d]", who, n_cand, MUXGL_MAX_FIT_CAND), 1;
  if (null_arg) return snprintf(why, n, "%s: %s is NULL", who, null_arg), 1;
  if (!(std::isfinite(x_max) && x_max > 0.0 && x_max <= 1.0))
    return snprintf(why, n, "%s: %s (%g) is not a finite number in (0, 1]", who, bound, x_max), 1;
  return 0;
}

// the arguments of the two ambient fits.  what: "sample" or "cluster", n_what of them
inline int bad_args(const char* who, const char* what, const double* amb_af, int32_t n_cand, const int32_t* cand, int64_t C,
                    int n_what, double rho_max, bool any_out, char* why, size_t n) {
  if (bad_head(who, n_cand, !cand ? "cand" : !amb_af ? "amb_af" : nullptr, "rho_max", rho_max, any_out, why, n)) return 1;
  for (int64_t i = 0; i < C * n_cand; ++i)
    if (cand[i] < -1 || cand[i] >= n_what)
      return snprintf(why, n, "%s: cand[%lld][%d] (%d) is neither -1 nor a %s in [0,%d)", who, (long long)(i / n_cand),
                      (int)(i % n_cand), cand[i], what, n_what), 1;
  return 0;
}

// the arguments of the two mixing-share fits: a slot is a pair of indices, both -1 (skipped) or both a `what`
inline int pair_bad_args(const char* who, const char* what, int32_t n_cand, const int32_t* pair, int64_t C, int n_what,
                         double alpha_max, bool any_out, char* why, size_t n) {
  if (bad_head(who, n_cand, pair ? nullptr : "pair", "alpha_max", alpha_max, any_out, why, n)) return 1;
  for (int64_t i = 0; i < C * n_cand; ++i) {
    const int32_t j = pair[2 * i], k = pair[2 * i + 1];
    for (int t = 0; t < 2; ++t)
      if (pair[2 * i + t] < -1 || pair[2 * i + t] >= n_what)
        return snprintf(why, n, "%s: pair[%lld][%d][%d] (%d) is neither -1 nor a %s in [0,%d)", who, (long long)(i / n_cand),
                        (int)(i % n_cand), t, pair[2 * i + t], what, n_what), 1;
    if ((j < 0) != (k < 0))
      return snprintf(why, n, "%s: pair[%lld][%d] (%d, %d) has exactly one negative index", who, (long long)(i / n_cand),
                      (int)(i % n_cand), j, k), 1;
  }
  return 0;
}

}  // namespace ambient_fit

// ---- the four calls' rules (demuxlet's amb_af is checked against the handle's has_gp by demux_ambient_check_af) ----
inline int demux_ambient_fit_bad_args(const double* amb_af, int32_t n_cand, const int32_t* cand, int64_t C, int V,
                                      double rho_max, bool any_out, char* why, size_t n) {
  return ambient_fit::bad_args("muxgl_demux_ambient_fit", "sample", amb_af, n_cand, cand, C, V, rho_max, any_out, why, n);
}

inline int demux_alpha_fit_bad_args(int32_t n_cand, const int32_t* pair, int64_t C, int V, double alpha_max, bool any_out,
                                    char* why, size_t n) {
  return ambient_fit::pair_bad_args("muxgl_demux_alpha_fit", "sample", n_cand, pair, C, V, alpha_max, any_out, why, n);
}

inline int fmx_ambient_fit_bad_args(const double* amb_af, int64_t S, int32_t n_cand, const int32_t* cand, int64_t C, int K,
                                    double rho_max, bool any_out, char* why, size_t n) {
  if (ambient_fit::bad_args("muxgl_fmx_ambient_fit", "cluster", amb_af, n_cand, cand, C, K, rho_max, any_out, why, n)) return 1;
  for (int64_t s = 0; s < S; ++s)
    if (!(std::isfinite(amb_af[s]) && amb_af[s] >= 0.0 && amb_af[s] <= 1.0))
      return snprintf(why, n, "muxgl_fmx_ambient_fit: amb_af of marker %lld (%g) is not a finite number in [0, 1]", (long long)s,
                      amb_af[s]), 1;
  return 0;
}

inline int fmx_alpha_fit_bad_args(int32_t n_cand, const int32_t* pair, int64_t C, int K, double alpha_max, bool any_out,
                                  char* why, size_t n) {
  return ambient_fit::pair_bad_args("muxgl_fmx_alpha_fit", "cluster", n_cand, pair, C, K, alpha_max, any_out, why, n);
}
