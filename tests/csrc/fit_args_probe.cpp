// Stand-alone host program over popscle_amd/csrc/fit_args.hpp for tests/test_fit_args.py (no device code): every case of
// the four fits' argument rules, one line "<call>\t<case>\t<return code>\t<text>" each.  C = 2 droplets, n_cand = 2,
// 5 samples or clusters, 3 markers.
#include <cmath>
#include <cstring>

#include "fit_args.hpp"

namespace {

constexpr int64_t C = 2, S = 3;
constexpr int N = 5;

struct args {
  bool any_out = true;
  int32_t n_cand = 2;
  bool null_slot = false, null_af = false;
  double bound = 0.5;
  int32_t slot[8] = {0, 1, -1, -1, 4, 4, 2, 0};  // (as pairs: (0,1) (-1,-1) (4,4) (2,0); as candidates the first four)
  double af[3] = {0.0, 0.25, 1.0};
};

void run(const char* name, const args& a) {
  const int32_t* slot = a.null_slot ? nullptr : a.slot;
  const double* af = a.null_af ? nullptr : a.af;
  for (int call = 0; call < 4; ++call) {
    char why[256];
    memset(why, 0, sizeof(why));
    int rc = 0;
    if (call == 0) rc = demux_ambient_fit_bad_args(af, a.n_cand, slot, C, N, a.bound, a.any_out, why, sizeof(why));
    if (call == 1) rc = demux_alpha_fit_bad_args(a.n_cand, slot, C, N, a.bound, a.any_out, why, sizeof(why));
    if (call == 2) rc = fmx_ambient_fit_bad_args(af, S, a.n_cand, slot, C, N, a.bound, a.any_out, why, sizeof(why));
    if (call == 3) rc = fmx_alpha_fit_bad_args(a.n_cand, slot, C, N, a.bound, a.any_out, why, sizeof(why));
    static const char* const who[4] = {"demux_ambient_fit", "demux_alpha_fit", "fmx_ambient_fit", "fmx_alpha_fit"};
    printf("%s\t%s\t%d\t%s\n", who[call], name, rc, why);
  }
}

}  // namespace

int main() {
  args a;
  run("ok", a);
  a = args(), a.any_out = false, a.n_cand = 0, a.null_slot = true;  // (the first rule asked)
  run("no_output", a);
  a = args(), a.n_cand = 0, a.null_slot = true;
  run("n_cand_0", a);
  a = args(), a.n_cand = MUXGL_MAX_FIT_CAND + 1, a.null_slot = true;
  run("n_cand_over", a);
  a = args(), a.null_slot = true, a.null_af = true, a.bound = 0.0;  // (cand before amb_af, both before the bound)
  run("null_slot", a);
  a = args(), a.null_af = true, a.bound = 0.0;
  run("null_af", a);
  a = args(), a.bound = 0.0, a.slot[0] = -2;  // (the bound before the indices)
  run("bound_0", a);
  a = args(), a.bound = 1.5;
  run("bound_1.5", a);
  a = args(), a.bound = NAN;
  run("bound_nan", a);
  a = args(), a.bound = 1.0;
  run("bound_1", a);
  a = args(), a.slot[3] = -2;
  run("index_-2", a);
  a = args(), a.slot[2] = N, a.slot[3] = N;
  run("index_n", a);
  a = args(), a.slot[6] = -1;  // (pair [1][1] = (-1, 0); as candidates past the end, never read)
  run("one_negative", a);
  a = args(), a.slot[3] = -2, a.af[1] = -0.5;  // (the indices before freemuxlet's amb_af)
  run("index_before_af", a);
  a = args(), a.af[1] = 1.5;
  run("af_1.5", a);
  a = args(), a.af[2] = NAN;
  run("af_nan", a);
  a = args(), a.af[0] = -0.25;
  run("af_negative", a);
  return 0;
}
