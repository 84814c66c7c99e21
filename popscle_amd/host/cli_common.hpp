// cli_common.hpp -- what the commands of the front end share besides the writers (table_writers.hpp): the flag groups with
// their checks, the hand-over of a pileup, the ambient profile, the reference's random numbers, and the steps the two
// freemuxlet commands have in common.
#pragma once

#include "../csrc/anchor_plan.hpp"
#include "table_writers.hpp"

namespace pa {

inline void check(muxgl_handle* h, int rc, const char* what) {
  if (rc != 0) fatal("%s failed: %s", what, muxgl_last_error(h));
}

struct CommonFlags {
  std::string plpPrefix, outPrefix, groupList;
  LoadOptions lo;
  int32_t device = 0;
  std::string devices;  // --devices 0,1,2,...: a device group (muxgl_config.n_devices), the in-process counterpart of
                        // running one popscle per --group-list chunk (README.md:168)
  void add(Args& a) {
    a.add_string("plp", &plpPrefix);
    a.add_string("out", &outPrefix);
    a.add_int("cap-BQ", &lo.capBQ);
    a.add_int("min-BQ", &lo.minBQ);
    a.add_string("group-list", &lo.groupList);
    a.add_int("min-total", &lo.minRead);
    a.add_int("min-umi", &lo.minUMI);
    a.add_int("min-snp", &lo.minSNP);
    a.add_int("device", &device);
    a.add_string("devices", &devices);
  }
  // the handle the command computes on: one device, or the group named by --devices
  muxgl_config config(int32_t flags) const {
    muxgl_config cfg = MUXGL_CONFIG_INIT;
    cfg.device_id = device;
    cfg.flags = flags;
    if (!devices.empty()) {
      size_t pos = 0;
      while (pos <= devices.size()) {
        const size_t comma = std::min(devices.find(',', pos), devices.size());
        const std::string tok = devices.substr(pos, comma - pos);
        if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos)
          fatal("--devices expects a comma-separated list of device ordinals, got '%s'", devices.c_str());
        if (cfg.n_devices >= MUXGL_MAX_DEVICES) fatal("--devices names more than %d devices", MUXGL_MAX_DEVICES);
        cfg.device_ids[cfg.n_devices++] = atoi(tok.c_str());
        pos = comma + 1;
      }
      cfg.device_id = cfg.device_ids[0];
    }
    return cfg;
  }
  bool grouped() const { return devices.find(',') != std::string::npos; }
};

// The genotype flags of demuxlet's VCF, with their meanings; freemuxlet knows them only next to --match-vcf / --anchor-vcf
struct GenotypeFlags {
  std::vector<std::string> smIDs;
  std::string smList;
  void add(Args& a, LoadOptions& lo, VcfReader& vr) {
    a.add_string("field", &lo.field);
    a.add_double("geno-error-offset", &lo.genoErrorOffset);
    a.add_double("geno-error-coeff", &lo.genoErrorCoeffR2);
    a.add_string("r2-info", &lo.r2info);
    a.add_int("min-mac", &vr.vfilt.minMAC);
    a.add_double("min-callrate", &vr.vfilt.minCallRate);
    a.add_multi_string("sm", &smIDs);
    a.add_string("sm-list", &smList);
  }
  // the samples of --sm and --sm-list, then the reader is opened
  void init(VcfReader& vr) const {
    vr.wanted = smIDs;
    if (!smList.empty()) {
      TsvReader t(smList);
      while (t.read_line() > 0) vr.wanted.push_back(t.str_field_at(0));
    }
    vr.init();
  }
};

// The flags of the per-droplet tables, the same for demuxlet (<out>.X.gz) and freemuxlet (<out>.clust1.X.gz)
struct TableFlags {
  bool writeSinglets = false;   // .sing2.gz: every droplet against every column
  bool writeInclusion = false;  // .incl.gz: per-column marginals of the pair hypotheses
  bool writeUnknown = false;    // .unk.gz: every droplet against a donor that no column holds
  bool writeAmbient = false;    // .amb.gz: every droplet as one cell plus a share of ambient RNA
  bool fitAmbient = false;      // .ambfit.gz: the maximum-likelihood ambient share with its standard error
  double ambFitMax = 0.5;
  bool fitAlpha = false;        // .alphafit.gz: the maximum-likelihood mixing share of the best doublet and of the two best singlets
  double alphaFitMax = 1.0;
  std::vector<double> ambRho;
  std::string ambAfFile;
  int32_t ambMaxReads = 0;
  void add(Args& a) {
    a.add_bool("write-singlets", &writeSinglets);
    a.add_bool("write-inclusion", &writeInclusion);
    a.add_bool("write-unknown", &writeUnknown);
    a.add_bool("write-ambient", &writeAmbient);
    a.add_bool("fit-ambient", &fitAmbient);
    a.add_double("ambient-fit-max", &ambFitMax);
    a.add_bool("fit-alpha", &fitAlpha);
    a.add_double("alpha-fit-max", &alphaFitMax);
    a.add_multi_double("ambient-rho", &ambRho);
    a.add_string("ambient-af", &ambAfFile);
    a.add_int("ambient-max-reads", &ambMaxReads);
  }
  void validate() {
    if (ambRho.empty()) ambRho = {0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5};
    if ((int)ambRho.size() > MUXGL_MAX_ALPHA) fatal("at most %d --ambient-rho values are supported", MUXGL_MAX_ALPHA);
    if (ambMaxReads < 0) fatal("--ambient-max-reads must not be negative");
    if (!(std::isfinite(ambFitMax) && ambFitMax > 0.0 && ambFitMax <= 1.0)) fatal("--ambient-fit-max must lie in (0, 1]");
    if (!(std::isfinite(alphaFitMax) && alphaFitMax > 0.0 && alphaFitMax <= 1.0)) fatal("--alpha-fit-max must lie in (0, 1]");
  }
};

inline void upload(muxgl_handle* h, const Pileup& p) {
  check(h, muxgl_set_pileup(h, p.C(), p.S(), p.nnz(), (int64_t)p.reads.size(), p.cell_ptr.data(), p.entry_snp.data(),
                            p.entry_rptr.data(), p.reads.data()),
        "muxgl_set_pileup");
}

// The droplets the ambient profile is made from: those with at most --ambient-max-reads reads, or (empty) all of them
inline std::vector<uint8_t> ambient_mask(const Pileup& p, const TableFlags& tf, const int32_t* nReads) {
  std::vector<uint8_t> mask;
  if (tf.ambMaxReads > 0) {
    mask.resize((size_t)p.C());
    int64_t kept = 0;
    for (int64_t i = 0; i < p.C(); ++i) kept += mask[(size_t)i] = nReads[i] <= tf.ambMaxReads;
    notice("Ambient profile from the %lld of %lld droplets with at most %d reads", (long long)kept, (long long)p.C(), tf.ambMaxReads);
  }
  return mask;
}

// The ambient profile of --write-ambient and --fit-ambient: the caller's file, or the pileup's own reads with one
// pseudo-read at the population frequency.  Made once, into f: a second call returns it as it is.  nReads [C]: the
// droplets' read counts that --ambient-max-reads is held against; lap: the stage's name for the timer
inline const std::vector<double>& ambient_profile(std::vector<double>& f, muxgl_handle* h, const Pileup& p, const TableFlags& tf,
                                                  const int32_t* nReads, StageTimer& tm, const char* lap) {
  const size_t S = (size_t)p.S();
  if (!f.empty() || S == 0) return f;
  f.resize(S);
  if (!tf.ambAfFile.empty()) {
    TsvReader t(tf.ambAfFile);
    size_t n = 0;
    for (; t.read_line() > 0; ++n)
      if (n < S) f[n] = t.double_field_at(0);
    if (n != S) fatal("--ambient-af: %s holds %zu lines, the pileup has %zu markers", tf.ambAfFile.c_str(), n, S);
  } else {
    const std::vector<uint8_t> mask = ambient_mask(p, tf, nReads);
    std::vector<int64_t> n_ref(S), n_alt(S);
    check(h, muxgl_pileup_allele_counts(h, mask.empty() ? nullptr : mask.data(), n_ref.data(), n_alt.data()),
          "muxgl_pileup_allele_counts");
    for (size_t s = 0; s < S; ++s) f[s] = ((double)n_alt[s] + p.snps[s].af) / ((double)n_ref[s] + (double)n_alt[s] + 1.0);
    tm.lap(lap);
  }
  return f;
}

// The reference draws from the C library's rand().  Other code in this process (the HIP runtime) draws from and
// reseeds that shared generator, so the commands keep their own copy of it: glibc's rand() is random() on the default
// 128-byte additive-feedback state, which initstate_r / random_r reproduce value for value (srand(s) == seed s; a
// program that never calls srand() runs on seed 1).
struct RefRand {
  random_data rd;
  char state[128];
  explicit RefRand(unsigned seed) {
    memset(&rd, 0, sizeof(rd));
    memset(state, 0, sizeof(state));
    initstate_r(seed, state, sizeof(state), &rd);
  }
  int next() {
    int32_t r = 0;
    random_r(&rd, &r);
    return (int)r;
  }
};

inline const char* sid(const Pileup& p, int i) { return (i >= 0 && i < p.nv) ? p.sample_ids[(size_t)i].c_str() : "NA"; }

// ---- shared by freemuxlet and freemuxlet-old ----
// --init-cluster: barcode -> cluster (cmd_cram_freemux2.cpp:90-104, cmd_cram_freemuxlet.cpp:87-99)
inline std::map<std::string, int32_t> read_init_cluster(const std::string& path, int K) {
  std::map<std::string, int32_t> initCluster;
  if (path.empty()) return initCluster;
  TsvReader t(path);
  while (t.read_line() > 0) {
    if (t.nfields != 2) fatal("ERROR: Initial clustering file %s has to have 2 columnes", path.c_str());
    const int32_t ic = t.int_field_at(1);
    if (ic >= 0) {
      if (ic >= K)
        fatal("ERROR: --nsample %d parameter was set. The cluster ID must be between 0 to %d, or use negative values "
              "to not assign initial cluster (not implemented yet)", K, K - 1);
      initCluster[t.str_field_at(0)] = ic;
    }
  }
  return initCluster;
}

// the droplets' clusters from the file (cmd_cram_freemux2.cpp:198-216, cmd_cram_freemuxlet.cpp:227-243); ccounts: NULL, or
// [K] receiving the clusters' sizes
inline void assign_init_cluster(const std::map<std::string, int32_t>& initCluster, const std::vector<std::string>& bcs,
                                std::vector<int32_t>& clusts, int32_t* ccounts = nullptr) {
  int32_t nmiss = 0;
  for (size_t i = 0; i < bcs.size(); ++i) {
    auto it = initCluster.find(bcs[i]);
    if (it == initCluster.end()) {
      ++nmiss;
      continue;
    }
    clusts[i] = it->second;
    if (ccounts) ++ccounts[it->second];
  }
  if (nmiss > 0) notice("WARNING: %d of %d droplets do not have initial cluster assignment", nmiss, (int)bcs.size());
}

// What a run's droplets start from: the allele frequencies, the scores of muxgl_fmx_prepare and the row list of every table
struct FmxPrepared {
  std::vector<double> af, llk0, llk2;
  std::vector<int32_t> nSNPs, nReads;
  explicit FmxPrepared(const Pileup& p)
      : af((size_t)p.S()), llk0((size_t)p.C()), llk2((size_t)p.C()), nSNPs((size_t)p.C()), nReads((size_t)p.C()) {
    for (size_t s = 0; s < af.size(); ++s) af[s] = p.snps[s].af;
  }
  void run(muxgl_handle* h) {
    check(h, muxgl_fmx_prepare(h, af.data(), llk0.data(), llk2.data(), nSNPs.data(), nReads.data()), "muxgl_fmx_prepare");
  }
  std::vector<double> scores() const {  // the log Bayes factor of a singlet over a doublet
    std::vector<double> s(llk0.size());
    for (size_t i = 0; i < s.size(); ++i) s[i] = llk2[i] - llk0[i];
    return s;
  }
  Table table(const Pileup& p) const { return {p.bcs, all_droplets(p.C(), nSNPs.data(), nReads.data()), Label::clusters()}; }
};

// snps_observed[v] = 1 for every marker some droplet covers (cmd_cram_freemux2.cpp:279-288).  Threads over the entries;
// the flags are accessed with relaxed atomics (several threads may store the same 1), and a set flag is only read, so that
// its cache line stays shared between the threads.
inline void mark_observed_snps(const Pileup& p, std::vector<uint8_t>& snps_observed) {
  const int64_t nnz = p.nnz(), grain = 1 << 20;
  const int32_t* es = p.entry_snp.data();
  uint8_t* so = snps_observed.data();
  parallel_for((nnz + grain - 1) / grain, plp_threads(), [&](int64_t b) {
    for (int64_t e = b * grain, e1 = std::min(nnz, (b + 1) * grain); e < e1; ++e)
      if (!__atomic_load_n(so + es[e], __ATOMIC_RELAXED)) __atomic_store_n(so + es[e], (uint8_t)1, __ATOMIC_RELAXED);
  });
}

// The cluster VCFs of a run, .clust0.vcf.gz and .clust1.vcf.gz: the cluster pileups as the handle holds them at the
// time, over the markers some droplet covers, with the date the run began writing them
struct ClusterVcfs {
  const Pileup& p;
  int K;
  std::vector<uint8_t> snps_observed;
  tm date;
  BigVec<double> gls;   // (not zero-filled: 2.3 GB at configs[4]; muxgl_fmx_get_cluster_pileup writes all of it)
  BigVec<int32_t> cnt;
  ClusterVcfs(const Pileup& p_, int K_)
      : p(p_), K(K_), snps_observed((size_t)p_.S(), 0), gls((size_t)K_ * p_.S() * 9), cnt((size_t)K_ * p_.S() * 3) {
    mark_observed_snps(p, snps_observed);
    const time_t now = std::time(nullptr);
    date = *localtime(&now);
  }
  void write(muxgl_handle* h, const std::string& path, bool old_clust0 = false) {
    check(h, muxgl_fmx_get_cluster_pileup(h, gls.data(), cnt.data()), "muxgl_fmx_get_cluster_pileup");
    write_cluster_vcf(path, p, K, gls.data(), cnt.data(), snps_observed, &date, old_clust0);
  }
};

}  // namespace pa
