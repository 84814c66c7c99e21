// muxgl_group.hip -- a device group behind one muxgl handle (muxgl_config.n_devices > 1).
//
// The reference parallelises by cutting the barcodes into groups and running one process per group (--group-list,
// README.md:168; sc_drop_seq.cpp:93-101,164-170).  A device group is the same cut inside the library:
//   * demuxlet (cmd_cram_demuxlet.cpp:636-1013 carries no cross-cell state): member r holds the cells [cb[r], cb[r+1])
//     (contiguous, balanced by entries) and a replica of the GP tensor; no exchange; the records are concatenated.
//   * freemuxlet: member r holds its ROW slab (its cells, every SNP: E-step, scans, re-assignment) and its COLUMN slab
//     (every cell, the SNPs [sb[r], sb[r+1]): cluster pileups, posteriors and the ordered clamped merge, which is a
//     chain per (cluster, SNP) in ascending cell id -- sc_drop_seq.h:77-101 -- and therefore owned by exactly one
//     member).  Per EM iteration two all-gathers: the cluster-GP rows f64[S][K][3] after the posterior phase and the
//     assignments i32[C] after the E-step.  xGMI is point to point, so each all-gather is N-1 direct peer copies per
//     member (hipMemcpyPeerAsync, pulled on the destination's stream behind an event of the source's stream); nothing is
//     staged through the host and no host thread waits inside an iteration: one thread enqueues the whole iteration on
//     all devices, then drains them.
// The hand-over calls (slicing, validation, H2D) run one host thread per member.
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "common.hpp"
#include "score_exact.hpp"

namespace {

// f(r) for every member on its own host thread; the first failure's message becomes the group's
template <class F>
int for_members(muxgl_handle* h, F f) {
  muxgl_group* g = h->group;
  std::vector<int> rc((size_t)g->n, 0);
  std::vector<std::thread> th;
  for (int r = 0; r < g->n; ++r) th.emplace_back([&, r]() { rc[(size_t)r] = f(r); });
  for (auto& t : th) t.join();
  for (int r = 0; r < g->n; ++r)
    if (rc[(size_t)r]) {
      char buf[64];
      snprintf(buf, sizeof(buf), "device group member %d (device %d): ", r, g->m[(size_t)r]->device);
      h->err = std::string(buf) + g->m[(size_t)r]->err;
      return 1;
    }
  return 0;
}

// The members of a fit call, each on its own cells: run(member, o, at, ms) with o = the member's first cell x n_cand and
// at(q) = q + o, or NULL for an output the caller does not want.  kernel_ms: the slowest member's.
template <class Run>
int fit_members(muxgl_handle* h, int32_t n_cand, float* kernel_ms, Run run) {
  muxgl_group* g = h->group;
  std::vector<float> ms((size_t)g->n, 0.f);
  if (for_members(h, [&](int r) {
        const size_t o = (size_t)g->cb[(size_t)r] * (size_t)n_cand;
        return run(g->m[(size_t)r], o, [o](auto* q) { return q ? q + o : nullptr; }, kernel_ms ? &ms[(size_t)r] : nullptr);
      }))
    return 1;
  if (kernel_ms) *kernel_ms = *std::max_element(ms.begin(), ms.end());
  return 0;
}

// The members of a table call, each on its own cells: run(member, at, ms) with at(q, w) = q + the member's first cell x w
// (w: the output's values per cell), or NULL for an output the caller does not want.  kernel_ms: the slowest member's.
// slot >= 0: the call reports through that timing slot of a handle, and the group's is the members' maximum.
template <class Run>
int table_members(muxgl_handle* h, int slot, float* kernel_ms, Run run) {
  muxgl_group* g = h->group;
  std::vector<float> ms((size_t)g->n, 0.f);
  if (for_members(h, [&](int r) {
        const size_t c = (size_t)g->cb[(size_t)r];
        return run(g->m[(size_t)r], [c](auto* q, size_t w) { return q ? q + c * w : nullptr; },
                   kernel_ms ? &ms[(size_t)r] : nullptr);
      }))
    return 1;
  if (kernel_ms) *kernel_ms = *std::max_element(ms.begin(), ms.end());
  if (slot >= 0) {
    g->ms[slot] = 0.f;
    for (auto* m : g->m) g->ms[slot] = std::max(g->ms[slot], m->ms[slot]);
  }
  return 0;
}

// fmx_refusal.hpp's rule for a group: the group's own two facts first, then the state of every member
int fmx_group_refuse(muxgl_handle* h, const char* who, const char* what) {
  muxgl_group* g = h->group;
  char why[256];
  if (fmx_table_refusal(who, what, g->have_pileup, g->prepared, 1, FMX_SNG_READY, why, sizeof(why))) MUXGL_FAIL(h, "%s", why);
  for (const muxgl_handle* m : g->m)
    if (fmx_refuse(h, m, who, what)) return 1;
  return 0;
}

void max_timing(muxgl_group* g) {
  for (int i = 0; i < MUXGL_T_COUNT; ++i) {
    g->ms[i] = 0.f;
    for (auto* m : g->m) g->ms[i] = std::max(g->ms[i], m->ms[i]);
  }
}

// n contiguous ranges over `items` units with near-equal weight: cut i at the first prefix sum >= total * i / n
std::vector<int64_t> cuts_by_prefix(const int64_t* prefix /*[items+1]*/, int64_t items, int n) {
  std::vector<int64_t> cut((size_t)n + 1, 0);
  const int64_t total = prefix[items];
  for (int i = 1; i < n; ++i) {
    const int64_t target = (int64_t)((__int128)total * i / n);
    int64_t c = std::lower_bound(prefix, prefix + items + 1, target) - prefix;
    cut[(size_t)i] = std::min(std::max(c, cut[(size_t)i - 1]), items);
  }
  cut[(size_t)n] = items;
  return cut;
}

}  // namespace

int group_create(const muxgl_config* cfg, muxgl_handle** out, std::string* err) {
  muxgl_handle* h = new muxgl_handle();
  muxgl_group* g = new muxgl_group();
  h->group = g;
  h->flags = cfg->flags;
  h->device = cfg->device_ids[0];
  g->n = cfg->n_devices;
  for (int r = 0; r < g->n; ++r) {
    muxgl_handle* m = nullptr;
    if (muxgl_handle_create(cfg->device_ids[r], cfg->flags & ~(MUXGL_FLAG_DEMUX_ONLY | MUXGL_FLAG_ASYNC_PHASES), nullptr,
                            &m, err)) {
      muxgl_destroy(h);
      return 1;
    }
    g->m.push_back(m);
  }
  // Direct peer copies between distinct devices.  Whatever goes wrong here -- no peer access between two devices, access
  // already enabled by another handle -- leaves hipMemcpyPeerAsync on its staged path, which is still correct, and must
  // not leave a sticky error behind for the next HIP call.  MUXGL_GROUP_NO_PEER=1 skips the enabling altogether (the
  // staged path on a box that does have peer access); MUXGL_FLAG_GROUP_PROBE_SELF also walks the pairs of members that
  // share a device (virtual ranks on one GPU: hipDeviceEnablePeerAccess(self) fails -- the error path, on any box).
  g->peer_pairs = g->peer_enabled = g->peer_refused = 0;
  const bool no_peer = getenv("MUXGL_GROUP_NO_PEER") != nullptr;
  const bool probe_self = (cfg->flags & MUXGL_FLAG_GROUP_PROBE_SELF) != 0;
  for (int a = 0; a < g->n; ++a)
    for (int b = 0; b < g->n; ++b) {
      const int da = g->m[(size_t)a]->device, db = g->m[(size_t)b]->device;
      if (a == b || (da == db && !probe_self)) continue;
      ++g->peer_pairs;
      int can = 0;
      hipError_t e = hipDeviceCanAccessPeer(&can, da, db);
      if (e != hipSuccess) (void)hipGetLastError();
      if (e == hipSuccess && da == db) can = 1;  // (probe: the runtime answers 0 for a device and itself; ask it to enable anyway)
      if (e == hipSuccess && can && !no_peer && hipSetDevice(da) == hipSuccess) {
        e = hipDeviceEnablePeerAccess(db, 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) ++g->peer_enabled;
        else ++g->peer_refused;
        if (e != hipSuccess) (void)hipGetLastError();
      } else {
        ++g->peer_refused;
      }
    }
  g->ev_gp.assign((size_t)g->n, nullptr);
  g->ev_es.assign((size_t)g->n, nullptr);
  for (int r = 0; r < g->n; ++r) {
    hipError_t e = hipSetDevice(g->m[(size_t)r]->device);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_gp[(size_t)r], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ev_es[(size_t)r], hipEventDisableTiming);
    if (e != hipSuccess) {
      *err = std::string("muxgl_create: device group events: ") + hipGetErrorString(e);
      muxgl_destroy(h);
      return 1;
    }
  }
  *out = h;
  return 0;
}

void group_destroy(muxgl_handle* h) {
  muxgl_group* g = h->group;
  if (!g) return;
  for (size_t r = 0; r < g->m.size(); ++r) {
    (void)hipSetDevice(g->m[r]->device);
    if (g->m[r]->stream) (void)hipStreamSynchronize(g->m[r]->stream);
  }
  for (size_t r = 0; r < g->ev_gp.size(); ++r) {
    if (g->ev_gp[r]) (void)hipEventDestroy(g->ev_gp[r]);
    if (g->ev_es[r]) (void)hipEventDestroy(g->ev_es[r]);
  }
  for (auto* m : g->m) muxgl_destroy(m);
  free(g->h_dcells);
  delete g;
  h->group = nullptr;
}

int group_set_pileup(muxgl_handle* h, int64_t C, int64_t S, int64_t nnz, int64_t R, const int64_t* cell_ptr,
                     const int32_t* entry_snp, const int64_t* entry_rptr, const uint8_t* reads) {
  muxgl_group* g = h->group;
  if (C < 0 || S < 0 || nnz < 0 || R < 0) MUXGL_FAIL(h, "muxgl_set_pileup: negative size");
  if (!cell_ptr || !entry_rptr || (nnz > 0 && !entry_snp) || (R > 0 && !reads))
    MUXGL_FAIL(h, "muxgl_set_pileup: NULL array");
  if (S > INT32_MAX || C > INT32_MAX) MUXGL_FAIL(h, "muxgl_set_pileup: C or S exceeds int32");
  host_timer tm;
  int64_t maxlen = 0;
  if (muxgl_validate_pileup(h, C, S, nnz, R, cell_ptr, entry_snp, entry_rptr, &maxlen)) return 1;
  tm.lap("group set_pileup: validation");
  g->have_pileup = g->have_cols = g->prepared = false;
  g->C = C;
  g->S = S;
  g->nnz = nnz;
  g->R = R;
  g->K = 0;
  g->V = h->V = 0;  // the members drop their panel with their pileup (demux_panel_release) ...
  g->n_alpha = 0;   // ... and the grid of the last run
  // cells: contiguous ranges balanced by entries (the work unit of every sweep)
  g->cb = cuts_by_prefix(cell_ptr, C, g->n);
  g->eb.assign((size_t)g->n + 1, 0);
  for (int r = 0; r <= g->n; ++r) g->eb[(size_t)r] = cell_ptr[g->cb[(size_t)r]];
  // SNPs: contiguous ranges balanced by entries per SNP (the length of the merge chains), +1 so that bare SNPs spread
  const bool cols = !(h->flags & MUXGL_FLAG_DEMUX_ONLY);
  g->sb.assign((size_t)g->n + 1, 0);
  g->sb[(size_t)g->n] = S;
  if (cols) {
    unsigned hw = std::thread::hardware_concurrency();
    int T = (int)(hw ? (hw > 16 ? 16 : hw) : 1);
    if (nnz < (1 << 20)) T = 1;
    std::vector<std::vector<int32_t>> part((size_t)T, std::vector<int32_t>((size_t)S, 0));
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
      th.emplace_back([&, t]() {
        int32_t* cnt = part[(size_t)t].data();
        for (int64_t e = nnz * t / T; e < nnz * (t + 1) / T; ++e) ++cnt[entry_snp[e]];
      });
    for (auto& x : th) x.join();
    std::vector<int64_t> pre((size_t)S + 1, 0);
    for (int64_t s = 0; s < S; ++s) {
      int64_t c = 1;
      for (int t = 0; t < T; ++t) c += part[(size_t)t][(size_t)s];
      pre[(size_t)s + 1] = pre[(size_t)s] + c;
    }
    g->sb = cuts_by_prefix(pre.data(), S, g->n);
    tm.lap("group set_pileup: SNP coverage + cuts");
  }
  const int rc = for_members(h, [&](int r) -> int {
    muxgl_handle* m = g->m[(size_t)r];
    const int64_t c0 = g->cb[(size_t)r], c1 = g->cb[(size_t)r + 1], nc = c1 - c0;
    const int64_t e0 = g->eb[(size_t)r], e1 = g->eb[(size_t)r + 1], ne = e1 - e0;
    const int64_t r0 = entry_rptr[e0], r1 = entry_rptr[e1];
    {  // row slab: the member's cells, every SNP; pointers rebased, payload arrays handed over in place
      std::vector<int64_t> cp((size_t)nc + 1), rp((size_t)ne + 1);
      for (int64_t i = 0; i <= nc; ++i) cp[(size_t)i] = cell_ptr[c0 + i] - e0;
      for (int64_t i = 0; i <= ne; ++i) rp[(size_t)i] = entry_rptr[e0 + i] - r0;
      if (muxgl_set_pileup_role(m, MUXGL_ROLE_FULL, nc, S, ne, r1 - r0, cp.data(), entry_snp + e0, rp.data(),
                                reads + r0, true))
        return 1;
    }
    if (!cols) return 0;
    // column slab: every cell, the entries with s0 <= SNP < s1 -- a contiguous run of each cell's ascending SNP ids
    const int32_t s0 = (int32_t)g->sb[(size_t)r], s1 = (int32_t)g->sb[(size_t)r + 1];
    std::vector<int64_t> cps((size_t)C + 1, 0), lo((size_t)C);
    int64_t nr = 0;
    for (int64_t c = 0; c < C; ++c) {
      const int32_t* b = entry_snp + cell_ptr[c];
      const int32_t* e = entry_snp + cell_ptr[c + 1];
      const int32_t* a = std::lower_bound(b, e, s0);
      const int32_t* z = std::lower_bound(a, e, s1);
      lo[(size_t)c] = a - entry_snp;
      cps[(size_t)c + 1] = cps[(size_t)c] + (z - a);
      nr += entry_rptr[z - entry_snp] - entry_rptr[a - entry_snp];
    }
    const int64_t ns = cps[(size_t)C];
    std::vector<int32_t> es((size_t)ns);
    std::vector<int64_t> rps((size_t)ns + 1);
    std::vector<uint8_t> rd((size_t)nr);
    int64_t rpos = 0;
    for (int64_t c = 0; c < C; ++c) {
      const int64_t a = lo[(size_t)c], k = cps[(size_t)c + 1] - cps[(size_t)c], o = cps[(size_t)c];
      if (!k) continue;
      memcpy(es.data() + o, entry_snp + a, sizeof(int32_t) * (size_t)k);
      const int64_t ra = entry_rptr[a];
      for (int64_t i = 0; i < k; ++i) rps[(size_t)(o + i)] = rpos + (entry_rptr[a + i] - ra);
      const int64_t nb = entry_rptr[a + k] - ra;
      if (nb) memcpy(rd.data() + rpos, reads + ra, (size_t)nb);
      rpos += nb;
    }
    rps[(size_t)ns] = rpos;
    return fmx_attach_column_slab(m, C, c0, s0, s1, ns, nr, cps.data(), es.data(), rps.data(), rd.data(), true);
  });
  if (rc) return 1;
  tm.lap("group set_pileup: slabs cut and handed over");
  free(g->h_dcells);
  g->h_dcells = (muxgl_demux_cell*)calloc((size_t)(C ? C : 1), sizeof(muxgl_demux_cell));
  if (!g->h_dcells) MUXGL_FAIL(h, "muxgl_set_pileup: out of host memory");
  g->have_pileup = true;
  g->have_cols = cols;
  h->C = C;
  h->S = S;
  h->nnz = nnz;
  h->R = R;
  return 0;
}

int group_demux_set_gp(muxgl_handle* h, int32_t V, const double* gp, const uint8_t* has_gp) {
  muxgl_group* g = h->group;
  if (!g->have_pileup) MUXGL_FAIL(h, "muxgl_demux_set_gp: call muxgl_set_pileup first");
  if (for_members(h, [&](int r) { return muxgl_demux_set_gp(g->m[(size_t)r], V, gp, has_gp); })) return 1;
  g->V = V;
  h->V = V;
  g->n_alpha = 0;  // (as the members' have_dp: muxgl_demux_get_entry_pg wants a run on this panel)
  return 0;
}

int group_demux_run(muxgl_handle* h, const muxgl_demux_params* p, muxgl_demux_cell* out, double* full_ll) {
  muxgl_group* g = h->group;
  if (!g->have_pileup || g->V < 1) MUXGL_FAIL(h, "muxgl_demux_run: no pileup / GP tensor set");
  if (!p) MUXGL_FAIL(h, "demux params NULL");
  if (p->n_alpha < 1 || p->n_alpha > MUXGL_MAX_ALPHA) MUXGL_FAIL(h, "n_alpha=%d outside [1,%d]", p->n_alpha, MUXGL_MAX_ALPHA);
  const size_t per_cell = (size_t)g->V * g->V * p->n_alpha;
  if (for_members(h, [&](int r) {
        muxgl_handle* m = g->m[(size_t)r];
        const int64_t c0 = g->cb[(size_t)r];
        if (muxgl_demux_run(m, p, g->h_dcells + c0, full_ll ? full_ll + (size_t)c0 * per_cell : nullptr)) return 1;
        return 0;
      }))
    return 1;
  g->n_alpha = p->n_alpha;
  if (out && g->C) memcpy(out, g->h_dcells, sizeof(muxgl_demux_cell) * (size_t)g->C);
  max_timing(g);
  return 0;
}

// every member sweeps its own cells and writes their rows of the caller's [C][V] table
int group_demux_singlets(muxgl_handle* h, const muxgl_demux_params* p, double* sng) {
  muxgl_group* g = h->group;
  if (demux_preconditions(h, p, g->have_pileup, g->V >= 1)) return 1;
  if (!sng) MUXGL_FAIL(h, "muxgl_demux_singlets: NULL output");
  return table_members(h, MUXGL_T_DEMUX_SINGLETS, nullptr, [&](muxgl_handle* m, auto at, float*) {
    return muxgl_demux_singlets(m, p, at(sng, (size_t)g->V));
  });
}

// every member folds its own cells and writes their rows of the caller's tables
int group_demux_inclusion(muxgl_handle* h, const muxgl_demux_params* p, const demux_incl_out& out) {
  muxgl_group* g = h->group;
  if (demux_preconditions(h, p, g->have_pileup, g->V >= 1)) return 1;
  const size_t V = (size_t)g->V;
  return table_members(h, MUXGL_T_DEMUX_INCLUSION, nullptr, [&](muxgl_handle* m, auto at, float*) {
    return muxgl_demux_inclusion(m, p, at(out.incl, V), at(out.tot, 1), at(out.dbl, V), at(out.partner, V), at(out.alpha_idx, V),
                                 at(out.first, V));
  });
}

// every member sweeps its own cells and writes their rows of the caller's tables; kernel_ms: the slowest member's
int group_demux_unknown(muxgl_handle* h, const muxgl_demux_params* p, const double* gp0, double* ll_ju, double* ll_uj,
                        double* ll_uu, float* kernel_ms) {
  muxgl_group* g = h->group;
  if (demux_preconditions(h, p, g->have_pileup, g->V >= 1)) return 1;
  if (!ll_ju && !ll_uj && !ll_uu) MUXGL_FAIL(h, "muxgl_demux_unknown: all three outputs are NULL");
  const size_t A = (size_t)p->n_alpha, VA = (size_t)g->V * A;
  return table_members(h, -1, kernel_ms, [&](muxgl_handle* m, auto at, float* ms) {
    return muxgl_demux_unknown(m, p, gp0, at(ll_ju, VA), at(ll_uj, VA), at(ll_uu, A), ms);
  });
}

// every member sweeps its own cells and writes their rows of the caller's table; kernel_ms: the slowest member's
int group_demux_ambient(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int32_t n_rho, const double* rho,
                        double* ll_amb, float* kernel_ms) {
  muxgl_group* g = h->group;
  if (demux_preconditions(h, p, g->have_pileup, g->V >= 1)) return 1;
  if (!ll_amb) MUXGL_FAIL(h, "muxgl_demux_ambient: NULL output");
  if (n_rho < 1 || n_rho > MUXGL_MAX_ALPHA) MUXGL_FAIL(h, "muxgl_demux_ambient: n_rho=%d outside [1,%d]", n_rho, MUXGL_MAX_ALPHA);
  if (!rho || !amb_af) MUXGL_FAIL(h, "muxgl_demux_ambient: %s is NULL", rho ? "amb_af" : "rho");
  if (const int r = demux_ambient_bad_rho(n_rho, rho); r >= 0)
    MUXGL_FAIL(h, "muxgl_demux_ambient: rho[%d] (%g) is not a finite number in [0, 1]", r, rho[r]);
  // (every member checks amb_af against its copy of has_gp)
  return table_members(h, -1, kernel_ms, [&](muxgl_handle* m, auto at, float* ms) {
    return muxgl_demux_ambient(m, p, amb_af, n_rho, rho, at(ll_amb, (size_t)g->V * (size_t)n_rho), ms);
  });
}

// every member fits its own cells and writes their rows of the caller's arrays; kernel_ms: the slowest member's
int group_demux_ambient_fit(muxgl_handle* h, const muxgl_demux_params* p, const double* amb_af, int32_t n_cand,
                            const int32_t* cand, double rho_max, double* rho_hat, double* ll_hat, double* ll_zero, double* info,
                            int32_t* status, int32_t* n_steps, float* kernel_ms) {
  muxgl_group* g = h->group;
  if (demux_preconditions(h, p, g->have_pileup, g->V >= 1)) return 1;
  char why[256];
  if (demux_ambient_fit_bad_args(amb_af, n_cand, cand, g->C, g->V, rho_max,
                                 rho_hat || ll_hat || ll_zero || info || status || n_steps, why, sizeof(why)))
    MUXGL_FAIL(h, "%s", why);
  // (every member checks amb_af against its copy of has_gp)
  return fit_members(h, n_cand, kernel_ms, [&](muxgl_handle* m, size_t o, auto at, float* ms) {
    return muxgl_demux_ambient_fit(m, p, amb_af, n_cand, cand + o, rho_max, at(rho_hat), at(ll_hat), at(ll_zero), at(info),
                                   at(status), at(n_steps), ms);
  });
}

// every member fits its own cells and writes their rows of the caller's arrays; kernel_ms: the slowest member's
int group_demux_alpha_fit(muxgl_handle* h, const muxgl_demux_params* p, int32_t n_cand, const int32_t* pair, double alpha_max,
                          double* alpha_hat, double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status,
                          int32_t* n_steps, float* kernel_ms) {
  muxgl_group* g = h->group;
  if (demux_preconditions(h, p, g->have_pileup, g->V >= 1)) return 1;
  char why[256];
  if (demux_alpha_fit_bad_args(n_cand, pair, g->C, g->V, alpha_max,
                               alpha_hat || ll_hat || ll_zero || ll_top || info || status || n_steps, why, sizeof(why)))
    MUXGL_FAIL(h, "%s", why);
  return fit_members(h, n_cand, kernel_ms, [&](muxgl_handle* m, size_t o, auto at, float* ms) {
    return muxgl_demux_alpha_fit(m, p, n_cand, pair + 2 * o, alpha_max, at(alpha_hat), at(ll_hat), at(ll_zero), at(ll_top),
                                 at(info), at(status), at(n_steps), ms);
  });
}

// every member counts the reads of its own cells; the counts are added here (integers: exact in any order)
int group_pileup_allele_counts(muxgl_handle* h, const uint8_t* cell_mask, int64_t* n_ref, int64_t* n_alt) {
  muxgl_group* g = h->group;
  if (!g->have_pileup) MUXGL_FAIL(h, "muxgl_pileup_allele_counts: no pileup set (muxgl_set_pileup)");
  if (!n_ref || !n_alt) MUXGL_FAIL(h, "muxgl_pileup_allele_counts: NULL output");
  const size_t S = (size_t)g->S;
  std::vector<int64_t> part((size_t)g->n * 2 * S);
  if (for_members(h, [&](int r) {
        int64_t* q = part.data() + (size_t)r * 2 * S;
        return muxgl_pileup_allele_counts(g->m[(size_t)r], cell_mask ? cell_mask + g->cb[(size_t)r] : nullptr, q, q + S);
      }))
    return 1;
  for (size_t s = 0; s < S; ++s) n_ref[s] = n_alt[s] = 0;
  for (int r = 0; r < g->n; ++r) {
    const int64_t* q = part.data() + (size_t)r * 2 * S;
    for (size_t s = 0; s < S; ++s) {
      n_ref[s] += q[s];
      n_alt[s] += q[S + s];
    }
  }
  return 0;
}

const muxgl_demux_cell* group_demux_results(const muxgl_handle* h) { return h->group->h_dcells; }

int group_demux_get_entry_pg(muxgl_handle* h, double* pg) {
  muxgl_group* g = h->group;
  if (g->n_alpha < 1) MUXGL_FAIL(h, "muxgl_demux_get_entry_pg: no previous muxgl_demux_run");
  if (!pg) MUXGL_FAIL(h, "muxgl_demux_get_entry_pg: NULL output");
  return for_members(h, [&](int r) {
    if (g->eb[(size_t)r + 1] == g->eb[(size_t)r]) return 0;  // a member without entries has nothing to report
    return muxgl_demux_get_entry_pg(g->m[(size_t)r], pg + (size_t)g->eb[(size_t)r] * g->n_alpha * 9);
  });
}

int group_fmx_prepare(muxgl_handle* h, const double* af, double* cell_llk0, double* cell_llk2, int32_t* cell_nsnps,
                      int32_t* cell_nreads) {
  muxgl_group* g = h->group;
  if (!g->have_pileup) MUXGL_FAIL(h, "muxgl_fmx_prepare: no pileup set (muxgl_set_pileup)");
  if (!g->have_cols)
    MUXGL_FAIL(h, "muxgl_fmx_prepare: the group was created with MUXGL_FLAG_DEMUX_ONLY (no column slabs were cut)");
  if (for_members(h, [&](int r) {
        const int64_t c0 = g->cb[(size_t)r];
        return muxgl_fmx_prepare(g->m[(size_t)r], af, cell_llk0 ? cell_llk0 + c0 : nullptr,
                                 cell_llk2 ? cell_llk2 + c0 : nullptr, cell_nsnps ? cell_nsnps + c0 : nullptr,
                                 cell_nreads ? cell_nreads + c0 : nullptr);
      }))
    return 1;
  // cells whose scores come within rounding reach of each other (in the whole job's order): the reference's own sums, each
  // from the member that holds the cell (score_exact.hpp) -- the group returns what a one-device handle returns
  h->fmx_exact_scores = 0;
  if (cell_llk0 && cell_llk2) {
    std::vector<std::vector<int64_t>> cps((size_t)g->n);
    auto exact_sums = [&](const std::vector<int32_t>& cells) -> int {
      size_t a = 0;
      for (int r = 0; r < g->n && a < cells.size(); ++r) {
        const int64_t c0 = g->cb[(size_t)r], c1 = g->cb[(size_t)r + 1];
        size_t b = a;
        while (b < cells.size() && cells[b] < c1) ++b;
        if (b > a) {
          muxgl_handle* m = g->m[(size_t)r];
          std::vector<int32_t> local(cells.begin() + (long)a, cells.begin() + (long)b);
          for (int32_t& c : local) c -= (int32_t)c0;
          if (hipSetDevice(m->device) != hipSuccess || (cps[(size_t)r].empty() && score_exact::fetch_cell_ptr(m, &cps[(size_t)r])) ||
              score_exact::compute(m, local, cps[(size_t)r], cell_llk0 + c0, cell_llk2 + c0)) {
            h->err = "device group member: " + m->err;
            return 1;
          }
        }
        a = b;
      }
      return 0;
    };
    if (score_exact::settle_with(g->C, cell_llk0, cell_llk2, &h->fmx_exact_scores, &h->err, exact_sums)) return 1;
  }
  g->prepared = true;
  g->K = 0;
  max_timing(g);
  return 0;
}

int group_fmx_get_entry_gls(muxgl_handle* h, double* gls, int32_t* counts) {
  muxgl_group* g = h->group;
  if (!g->prepared) MUXGL_FAIL(h, "muxgl_fmx_get_entry_gls: call muxgl_fmx_prepare first");
  return for_members(h, [&](int r) {
    const size_t e0 = (size_t)g->eb[(size_t)r];
    return muxgl_fmx_get_entry_gls(g->m[(size_t)r], gls ? gls + e0 * 9 : nullptr, counts ? counts + e0 * 3 : nullptr);
  });
}

void group_peer_stats(const muxgl_handle* h, int32_t* out) {
  out[0] = h->group->peer_pairs, out[1] = h->group->peer_enabled, out[2] = h->group->peer_refused;
}

void group_fmx_exact_stats(const muxgl_handle* h, int64_t* cells, int64_t* changed, int64_t* unresolved) {
  *cells = *changed = *unresolved = 0;
  for (muxgl_handle* m : h->group->m) {
    *cells += m->fmx_exact_cells;
    *changed += m->fmx_exact_changed;
    *unresolved += m->fmx_exact_unresolved;
  }
}

int group_fmx_set_clusters(muxgl_handle* h, int32_t K, const int32_t* clust) {
  muxgl_group* g = h->group;
  if (!g->prepared) MUXGL_FAIL(h, "muxgl_fmx_set_clusters: call muxgl_fmx_prepare first");
  if (for_members(h, [&](int r) { return muxgl_fmx_set_clusters(g->m[(size_t)r], K, clust); })) return 1;
  g->K = K;
  h->K = K;
  max_timing(g);
  return 0;
}

// every member holds the whole panel and writes the anchored columns of its own SNP range (fmx_anchor.hip); the
// all-gather of the posterior rows in group_fmx_iterate carries them with the rest
int group_fmx_set_anchors(muxgl_handle* h, int32_t n_anchor, const int32_t* donor, const uint8_t* mode) {
  muxgl_group* g = h->group;
  if (!g->prepared || g->K < 1) MUXGL_FAIL(h, "muxgl_fmx_set_anchors: no clusters set (call muxgl_fmx_set_clusters first)");
  // (checked here once, so that the group's handle carries the plain message and no member is left with other anchors
  //  than the rest)
  if (n_anchor < 0 || n_anchor > g->K) MUXGL_FAIL(h, "muxgl_fmx_set_anchors: n_anchor=%d outside [0, K=%d]", n_anchor, g->K);
  if (n_anchor > 0) {
    if (g->V < 1) MUXGL_FAIL(h, "muxgl_fmx_set_anchors: no genotype panel set (muxgl_demux_set_gp)");
    if (!donor) MUXGL_FAIL(h, "muxgl_fmx_set_anchors: donor is NULL with n_anchor=%d", n_anchor);
    for (int32_t i = 0; i < n_anchor; ++i)
      if (donor[i] < 0 || donor[i] >= g->V)
        MUXGL_FAIL(h, "muxgl_fmx_set_anchors: donor[%d]=%d outside [0, V=%d)", i, donor[i], g->V);
    for (int32_t i = 0; mode && i < n_anchor; ++i)
      if (mode[i] != MUXGL_ANCHOR_HELD && mode[i] != MUXGL_ANCHOR_PRIOR)
        MUXGL_FAIL(h, "muxgl_fmx_set_anchors: mode[%d]=%d is neither MUXGL_ANCHOR_HELD (0) nor MUXGL_ANCHOR_PRIOR (1)", i,
                   (int)mode[i]);
  }
  return for_members(h, [&](int r) { return fmx_set_anchors_on(g->m[(size_t)r], n_anchor, donor, mode, true); });
}

// after muxgl_fmx_iterate every member holds all the posterior rows (its own and the pulled ones): the first member's
int group_fmx_get_cluster_gp(muxgl_handle* h, int32_t k0, int32_t k1, double* out) {
  muxgl_group* g = h->group;
  if (!g->prepared || g->K < 1) MUXGL_FAIL(h, "muxgl_fmx_get_cluster_gp: no clusters set (call muxgl_fmx_set_clusters first)");
  muxgl_handle* m = g->m[0];
  if (fmx_get_cluster_gp_on(m, k0, k1, out)) {
    h->err = m->err;
    return 1;
  }
  return 0;
}

// One EM iteration (cmd_cram_freemux2.cpp:375-597) on the group.  Everything is enqueued from this thread; the devices
// wait for each other through events only.  Buffer hazards: a member's posterior rows are rewritten by its next
// posterior phase, which sits behind its M-step, which sits behind its assignment pulls, which wait for every member's
// E-step -- and a member's E-step sits behind its pulls of those rows; the assignment slices likewise.
int group_fmx_iterate(muxgl_handle* h, const muxgl_fmx_params* p, muxgl_fmx_cell* out, int32_t* nsingle, int32_t* namb,
                      int32_t* nchanged, double* full_ll) {
  muxgl_group* g = h->group;
  if (!p) MUXGL_FAIL(h, "muxgl_fmx_iterate: params NULL");
  if (!g->prepared || g->K < 1) MUXGL_FAIL(h, "muxgl_fmx_iterate: call muxgl_fmx_prepare and muxgl_fmx_set_clusters first");
  const int n = g->n, K = g->K;
  const size_t row = (size_t)K * 3;
  if (full_ll)
    for (int r = 0; r < n; ++r)
      if (g->m[(size_t)r]->fmx_streamed)
        MUXGL_FAIL(h, "muxgl_fmx_iterate: full_ll is not available on the streamed E-step (K=%d; more than 255 clusters, a "
                      "job whose [C][K(K+1)/2] table does not fit the device, or MUXGL_FLAG_FORCE_STREAMED_ESTEP): pass "
                      "full_ll = NULL", K);
#define GCHK(m, call)                                                                                     \
  do {                                                                                                    \
    hipError_t _e = (call);                                                                               \
    if (_e != hipSuccess)                                                                                 \
      MUXGL_FAIL(h, "device group, device %d: %s failed: %s", (m)->device, #call, hipGetErrorString(_e)); \
  } while (0)
  auto phase_fail = [&](muxgl_handle* m) {
    h->err = m->err;
    return 1;
  };
  for (int r = 0; r < n; ++r) {  // cluster genotype posteriors of the own SNP range
    muxgl_handle* m = g->m[(size_t)r];
    GCHK(m, hipSetDevice(m->device));
    clear_timing(m);
    if (fmx_phase_gp(m, p)) return phase_fail(m);
    GCHK(m, hipEventRecord(g->ev_gp[(size_t)r], m->stream));
  }
  for (int r = 0; r < n; ++r) {  // all-gather of the posterior rows, then the E-step of the own cells
    muxgl_handle* m = g->m[(size_t)r];
    GCHK(m, hipSetDevice(m->device));
    for (int o = 0; o < n; ++o) {
      if (o == r) continue;
      muxgl_handle* src = g->m[(size_t)o];
      const int64_t s0 = g->sb[(size_t)o], s1 = g->sb[(size_t)o + 1];
      if (s1 <= s0) continue;
      GCHK(m, hipStreamWaitEvent(m->stream, g->ev_gp[(size_t)o], 0));
      GCHK(m, hipMemcpyPeerAsync(m->d_cgp + (size_t)s0 * row, m->device, src->d_cgp + (size_t)s0 * row, src->device,
                                 sizeof(double) * (size_t)(s1 - s0) * row, m->stream));
    }
    if (fmx_phase_estep(m, p)) return phase_fail(m);
    GCHK(m, hipEventRecord(g->ev_es[(size_t)r], m->stream));
  }
  for (int r = 0; r < n; ++r) {  // all-gather of the assignments, then the ordered merge of the own SNP range
    muxgl_handle* m = g->m[(size_t)r];
    GCHK(m, hipSetDevice(m->device));
    for (int o = 0; o < n; ++o) {
      if (o == r) continue;
      muxgl_handle* src = g->m[(size_t)o];
      const int64_t c0 = g->cb[(size_t)o], c1 = g->cb[(size_t)o + 1];
      if (c1 <= c0) continue;
      GCHK(m, hipStreamWaitEvent(m->stream, g->ev_es[(size_t)o], 0));
      GCHK(m, hipMemcpyPeerAsync(m->col->d_clust + c0, m->device, src->col->d_clust + c0, src->device,
                                 sizeof(int32_t) * (size_t)(c1 - c0), m->stream));
    }
    if (fmx_phase_mstep(m)) return phase_fail(m);
  }
  // Near-tie calls (fmx_exact.hip): the members' listed cells are settled in the reference's arithmetic -- the SNP lists
  // united, every row computed by the member whose M-step range holds the SNP, the rows handed to all -- and, when an
  // assignment changed, the assignments are pulled and the ordered merge is run once more.
  int64_t listed = 0;
  for (int r = 0; r < n; ++r) {
    muxgl_handle* m = g->m[(size_t)r];
    GCHK(m, hipSetDevice(m->device));
    GCHK(m, hipStreamSynchronize(m->stream));
    listed += m->h_fstat[3];
  }
  if (listed > 0) {
    std::vector<int32_t> uni;
    for (int r = 0; r < n; ++r) {
      muxgl_handle* m = g->m[(size_t)r];
      GCHK(m, hipSetDevice(m->device));
      std::vector<int32_t> sn;
      if (fmx_exact_snps(m, &sn)) return phase_fail(m);
      uni.insert(uni.end(), sn.begin(), sn.end());
    }
    std::sort(uni.begin(), uni.end());
    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
    const int64_t nu = (int64_t)uni.size();
    std::vector<double> rows((size_t)nu * row);
    std::vector<uint8_t> owned((size_t)nu, 0);
    for (int r = 0; r < n; ++r) {
      muxgl_handle* m = g->m[(size_t)r];
      GCHK(m, hipSetDevice(m->device));
      if (fmx_exact_rows(m, p, uni.data(), nu, rows.data(), owned.data())) return phase_fail(m);
    }
    for (int64_t i = 0; i < nu; ++i)
      if (!owned[(size_t)i]) MUXGL_FAIL(h, "device group: no member's M-step range holds SNP %d", uni[(size_t)i]);
    bool reassigned = false;
    for (int r = 0; r < n; ++r) {
      muxgl_handle* m = g->m[(size_t)r];
      GCHK(m, hipSetDevice(m->device));
      int64_t dl[3];
      int32_t re = 0;
      if (fmx_exact_finish(m, p, uni.data(), nu, rows.data(), dl, &re)) return phase_fail(m);
      for (int i = 0; i < 3; ++i) m->h_fstat[i] += (int32_t)dl[i];
      m->h_fstat[3] = 0;
      reassigned = reassigned || re != 0;
    }
    if (reassigned) {
      for (int r = 0; r < n; ++r) {  // (finish drained every member's stream: no events needed for these pulls)
        muxgl_handle* m = g->m[(size_t)r];
        GCHK(m, hipSetDevice(m->device));
        for (int o = 0; o < n; ++o) {
          if (o == r) continue;
          muxgl_handle* src = g->m[(size_t)o];
          const int64_t c0 = g->cb[(size_t)o], c1 = g->cb[(size_t)o + 1];
          if (c1 <= c0) continue;
          GCHK(m, hipMemcpyPeerAsync(m->col->d_clust + c0, m->device, src->col->d_clust + c0, src->device,
                                     sizeof(int32_t) * (size_t)(c1 - c0), m->stream));
        }
        if (fmx_phase_mstep(m)) return phase_fail(m);
      }
    }
  }
  const size_t npairs = (size_t)K * (K + 1) / 2;
  int32_t st[3] = {0, 0, 0};
  for (int r = 0; r < n; ++r) {
    muxgl_handle* m = g->m[(size_t)r];
    const int64_t c0 = g->cb[(size_t)r], nc = g->cb[(size_t)r + 1] - c0;
    GCHK(m, hipSetDevice(m->device));
    if (out && nc)
      GCHK(m, hipMemcpyAsync(m->h_fcells, m->d_fcells, sizeof(muxgl_fmx_cell) * (size_t)nc, hipMemcpyDeviceToHost, m->stream));
    GCHK(m, hipStreamSynchronize(m->stream));
    collect_timing(m);
    if (out && nc) memcpy(out + c0, m->h_fcells, sizeof(muxgl_fmx_cell) * (size_t)nc);
    for (int i = 0; i < 3; ++i) st[i] += m->h_fstat[i];
    if (full_ll && nc)
      GCHK(m, hipMemcpy(full_ll + (size_t)c0 * npairs, m->d_fll, sizeof(double) * (size_t)nc * npairs, hipMemcpyDeviceToHost));
  }
#undef GCHK
  for (muxgl_handle* m : g->m) m->xs_keep = st[2] == 0;  // (fmx_exact.hip: the settled cells' table stays valid while nothing moves)
  if (nsingle) *nsingle = st[0];
  if (namb) *namb = st[1];
  if (nchanged) *nchanged = st[2];
  max_timing(g);
  return 0;
}

// gls[K][S][9], counts[K][S][3]: every member contributes the rows of its SNP range
int group_fmx_get_cluster_pileup(muxgl_handle* h, double* gls, int32_t* counts) {
  muxgl_group* g = h->group;
  if (g->K < 1) MUXGL_FAIL(h, "muxgl_fmx_get_cluster_pileup: no clusters set");
  for (int r = 0; r < g->n; ++r) {
    muxgl_handle* m = g->m[(size_t)r];
    muxgl_handle* c = m->col;
    const int64_t s0 = g->sb[(size_t)r], s1 = g->sb[(size_t)r + 1];
    HIPCHK(h, hipSetDevice(m->device));
    HIPCHK(h, hipStreamSynchronize(m->stream));
    if (s1 <= s0) continue;
    if (gls)
      HIPCHK(h, hipMemcpy2D(gls + (size_t)s0 * 9, sizeof(double) * 9 * (size_t)g->S, c->d_cgls + (size_t)s0 * 9,
                            sizeof(double) * 9 * (size_t)g->S, sizeof(double) * 9 * (size_t)(s1 - s0), (size_t)g->K,
                            hipMemcpyDeviceToHost));
    if (counts) {
      if (fmx_cluster_counts_device(c)) {
        h->err = c->err;
        return 1;
      }
      HIPCHK(h, hipStreamSynchronize(m->stream));
      HIPCHK(h, hipMemcpy2D(counts + (size_t)s0 * 3, sizeof(int32_t) * 3 * (size_t)g->S, c->d_ccnt + (size_t)s0 * 3,
                            sizeof(int32_t) * 3 * (size_t)g->S, sizeof(int32_t) * 3 * (size_t)(s1 - s0), (size_t)g->K,
                            hipMemcpyDeviceToHost));
    }
  }
  return 0;
}

// every member sweeps its own cells and writes their rows of the caller's [C][K] table
int group_fmx_singlets(muxgl_handle* h, double* sng) {
  muxgl_group* g = h->group;
  if (fmx_group_refuse(h, "muxgl_fmx_singlets", "the table belongs")) return 1;
  if (!sng) MUXGL_FAIL(h, "muxgl_fmx_singlets: NULL output");
  return table_members(h, MUXGL_T_FMX_SINGLETS, nullptr, [&](muxgl_handle* m, auto at, float*) {
    return muxgl_fmx_singlets(m, at(sng, (size_t)g->K));
  });
}

// every member sweeps its own cells and writes their rows of the caller's tables; kernel_ms: the slowest member's
int group_fmx_unknown(muxgl_handle* h, const double* gp0, double* ll_ju, double* ll_u, double* ll_uu, float* kernel_ms) {
  muxgl_group* g = h->group;
  if (fmx_group_refuse(h, "muxgl_fmx_unknown", "the tables belong")) return 1;
  if (!ll_ju && !ll_u && !ll_uu) MUXGL_FAIL(h, "muxgl_fmx_unknown: all three outputs are NULL");
  if (gp0) {  // (once here, so that the group's handle carries the message; the members find nothing)
    const int64_t bad = fmx_unknown_bad_prior(gp0, g->S);
    if (bad >= 0)
      MUXGL_FAIL(h, "muxgl_fmx_unknown: gp0 row of marker %lld (%g, %g, %g) is not a probability triple (entries in [0, 1], "
                    "sum within 1e-6 of 1)",
                 (long long)bad, gp0[3 * bad], gp0[3 * bad + 1], gp0[3 * bad + 2]);
  }
  return table_members(h, -1, kernel_ms, [&](muxgl_handle* m, auto at, float* ms) {
    return muxgl_fmx_unknown(m, gp0, at(ll_ju, (size_t)g->K), at(ll_u, 1), at(ll_uu, 1), ms);
  });
}

// every member sweeps its own cells and writes their rows of the caller's table; kernel_ms: the slowest member's
int group_fmx_ambient(muxgl_handle* h, const double* amb_af, int32_t n_rho, const double* rho, double* ll_amb, float* kernel_ms) {
  muxgl_group* g = h->group;
  if (fmx_group_refuse(h, "muxgl_fmx_ambient", "the table belongs")) return 1;
  char why[256];  // (once here, so that the group's handle carries the message; the members find nothing)
  if (fmx_ambient_bad_args(amb_af, g->S, n_rho, rho, ll_amb, why, sizeof(why))) MUXGL_FAIL(h, "%s", why);
  return table_members(h, -1, kernel_ms, [&](muxgl_handle* m, auto at, float* ms) {
    return muxgl_fmx_ambient(m, amb_af, n_rho, rho, at(ll_amb, (size_t)g->K * (size_t)n_rho), ms);
  });
}

// every member fits its own cells and writes their rows of the caller's arrays; kernel_ms: the slowest member's
int group_fmx_ambient_fit(muxgl_handle* h, const double* amb_af, int32_t n_cand, const int32_t* cand, double rho_max,
                          double* rho_hat, double* ll_hat, double* ll_zero, double* info, int32_t* status, int32_t* n_steps,
                          float* kernel_ms) {
  muxgl_group* g = h->group;
  if (fmx_group_refuse(h, "muxgl_fmx_ambient_fit", "the fit belongs")) return 1;
  char why[256];  // (once here, so that the group's handle carries the message; the members find nothing)
  if (fmx_ambient_fit_bad_args(amb_af, g->S, n_cand, cand, g->C, g->K, rho_max,
                               rho_hat || ll_hat || ll_zero || info || status || n_steps, why, sizeof(why)))
    MUXGL_FAIL(h, "%s", why);
  return fit_members(h, n_cand, kernel_ms, [&](muxgl_handle* m, size_t o, auto at, float* ms) {
    return muxgl_fmx_ambient_fit(m, amb_af, n_cand, cand + o, rho_max, at(rho_hat), at(ll_hat), at(ll_zero), at(info),
                                 at(status), at(n_steps), ms);
  });
}

// every member fits its own cells and writes their rows of the caller's arrays; kernel_ms: the slowest member's
int group_fmx_alpha_fit(muxgl_handle* h, int32_t n_cand, const int32_t* pair, double alpha_max, double* alpha_hat,
                        double* ll_hat, double* ll_zero, double* ll_top, double* info, int32_t* status, int32_t* n_steps,
                        float* kernel_ms) {
  muxgl_group* g = h->group;
  if (fmx_group_refuse(h, "muxgl_fmx_alpha_fit", "the fit belongs")) return 1;
  char why[256];  // (once here, so that the group's handle carries the message; the members find nothing)
  if (fmx_alpha_fit_bad_args(n_cand, pair, g->C, g->K, alpha_max,
                             alpha_hat || ll_hat || ll_zero || ll_top || info || status || n_steps, why, sizeof(why)))
    MUXGL_FAIL(h, "%s", why);
  return fit_members(h, n_cand, kernel_ms, [&](muxgl_handle* m, size_t o, auto at, float* ms) {
    return muxgl_fmx_alpha_fit(m, n_cand, pair + 2 * o, alpha_max, at(alpha_hat), at(ll_hat), at(ll_zero), at(ll_top), at(info),
                               at(status), at(n_steps), ms);
  });
}

// every member folds its own cells and writes their rows of the caller's tables
int group_fmx_inclusion(muxgl_handle* h, const muxgl_fmx_params* p, double* incl, double* tot, double* dbl, int32_t* partner) {
  muxgl_group* g = h->group;
  if (!p) MUXGL_FAIL(h, "muxgl_fmx_inclusion: fmx params NULL");
  if (fmx_group_refuse(h, "muxgl_fmx_inclusion", "the tables belong")) return 1;
  const size_t K = (size_t)g->K;
  return table_members(h, MUXGL_T_FMX_INCLUSION, nullptr, [&](muxgl_handle* m, auto at, float*) {
    return muxgl_fmx_inclusion(m, p, at(incl, K), at(tot, 1), at(dbl, K), at(partner, K));
  });
}

int group_get_timing(const muxgl_handle* h, float* ms) {
  memcpy(ms, h->group->ms, sizeof(float) * MUXGL_T_COUNT);
  return 0;
}
