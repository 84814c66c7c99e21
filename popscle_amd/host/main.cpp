// popscle-amd -- popscle-compatible front end for the demuxlet / freemuxlet genotype-likelihood path, with the hot path
// running on an MI355X through the C-ABI of libmuxgl (include/muxgl.h).
//
//   popscle-amd demuxlet   --plp P --vcf V [--field GT|GP|PL] --out O [...]     mirrors cmdCramDemuxlet (cmd_cram_demuxlet.cpp)
//       --write-singlets: also <O>.sing2.gz (BGZF), the singlet log-likelihood of every printed droplet against every
//       sample -- the reference's disabled .sing2 writer (cmd_cram_demuxlet.cpp:580,839-848).  Columns BARCODE, SM_ID,
//       NUM.SNPS, NUM.READS (the droplet's columns of .best, in place of the reference's RD.TOTL / RD.PASS / RD.UNIQ: the
//       loader keeps no passed-read count), LLK1 (%.4lf), POSTPRB (%.3lg, equal priors over the samples); the reference's
//       LLK0 (llks00[0]) is left out: nothing computes llks00 and the reference reads it nowhere else
//       --write-inclusion: also <O>.incl.gz (BGZF), one row per printed droplet and sample: the evidence that the sample
//       is in the droplet, as a singlet or as either half of a doublet, and the doublet it pairs best in -- the row and
//       column marginals of the reference's disabled .pair writer (cmd_cram_demuxlet.cpp:852-877; muxgl_demux_inclusion).
//       Columns BARCODE, SM_ID, NUM.SNPS, NUM.READS, LLK.INCL (%.4lf), POSTPRB.INCL (%.3lg, exp(incl - tot)),
//       DBL.PARTNER (sample id), DBL.ALPHA (%.3lf: the share of the sample's OWN reads in that doublet, alpha if it
//       is the second, contaminating sample of the pair and 1 - alpha if it is the first, :694-695,734-736), DBL.LLK (%.4lf); the last three are NA where no doublet hypothesis
//       holds the sample (one sample, or a grid without a doublet alpha)
//       --write-unknown: also <O>.unk.gz (BGZF), one row per printed droplet: how well a donor that is NOT in the VCF
//       explains it -- the half-unspecified and unspecified doublet likelihoods the reference accumulates and never prints
//       (llksA0 / llks00, cmd_cram_demuxlet.cpp:749-773; muxgl_demux_unknown with the panel mean of :428-440 as the
//       unknown donor's genotype prior).  Columns BARCODE, NUM.SNPS, NUM.READS, BEST.LLK (of .best, %.4lf), UNK.SNG.LLK
//       (one unknown donor), UNK.DBL.ALPHA (%.2lf), UNK.DBL.LLK (two unknown donors, the best alpha), HALF.GUESS (SM,*,alpha:
//       the known donor has share 1 - alpha; *,SM,alpha: share alpha), HALF.LLK, DIFF.LLK.PANEL.UNK (BEST.LLK minus the
//       largest of the three); LLKs %.4lf; NA where a column has no hypothesis (a grid of one alpha)
//       --write-ambient: also <O>.amb.gz (BGZF), one row per printed droplet: the droplet as ONE cell of a sample plus a
//       share rho of ambient RNA (muxgl_demux_ambient) -- the reading the reference lacks, which calls a clean singlet
//       from a high-soup prep a doublet with a partner picked nearly at random.  --ambient-rho x (repeatable; default 0
//       0.05 0.1 0.15 0.2 0.3 0.4 0.5) is the grid of shares; the ALT fraction of the ambient RNA per marker is read from
//       --ambient-af FILE (one number per line, in .var.gz order) or else made from the pileup itself: the usable reads
//       of the loaded droplets by marker and allele (muxgl_pileup_allele_counts; --ambient-max-reads N: of the droplets
//       with at most N reads only, 0 = all) with one pseudo-read at the AF column of .var.gz, (n_alt + AF) / (n_ref + n_alt
//       + 1).  Columns BARCODE, NUM.SNPS, NUM.READS, DROPLET.TYPE, BEST.LLK, SNG.BEST.GUESS, SNG.BEST.LLK (those of .best,
//       LLKs %.4lf), AMB.GUESS (the sample), AMB.RHO (%.2lf: the best share ON THE GRID; --fit-ambient estimates it),
//       AMB.LLK (ties: the lower sample, then the lower rho index), DIFF.LLK.AMB.BEST = AMB.LLK - BEST.LLK.  The calls of
//       .best and every other file are unchanged
//       --fit-ambient: also <O>.ambfit.gz (BGZF), per printed droplet one row for SNG.BEST.GUESS and one for SNG.NEXT.GUESS
//       of .best: the maximum-likelihood share of ambient RNA on [0, --ambient-fit-max x] (default 0.5) under the model of
//       --write-ambient, with the profile of --ambient-af / --ambient-max-reads (muxgl_demux_ambient_fit).  Columns BARCODE,
//       NUM.SNPS, NUM.READS, SM_ID, SNG.LLK (the sample's singlet LLK), AMB.RHO.MLE, AMB.RHO.SE (the standard error from the
//       observed information; NA on a bound or where the information is not positive), AMB.LLK.MLE, AMB.LRT = 2 (AMB.LLK.MLE -
//       SNG.LLK), STATUS (0 interior, 1 lower bound, 2 upper bound, 3 step cap, 5 no scored marker); all %.4lf
//       --fit-alpha: also <O>.alphafit.gz (BGZF), per printed droplet one row DBL for the two samples of DBL.BEST.GUESS and
//       one row SNG for (SNG.BEST.GUESS, SNG.NEXT.GUESS) of .best: the maximum-likelihood share alpha of the second sample
//       on [0, --alpha-fit-max x] (default 1.0) under the reference's doublet model (muxgl_demux_alpha_fit).  Columns
//       BARCODE, NUM.SNPS, NUM.READS, PAIR, SM1_ID, SM2_ID, SNG1.LLK (the first sample alone), SNG2.LLK (the second alone; NA
//       when x < 1), ALPHA.MLE, ALPHA.SE (the standard error from the observed information; NA on a bound or where the
//       information is not positive), MIX.LLK.MLE, MIX.LRT = 2 (MIX.LLK.MLE - the better of SNG1.LLK and SNG2.LLK; SNG1.LLK
//       alone when x < 1), STATUS (0 interior, 1 lower bound, 2 upper bound, 3 step cap, 5 no scored marker); all %.4lf.
//       .best and every other file are unchanged
//   popscle-amd freemuxlet --plp P --nsample K --out O [...]                   mirrors cmdCramFreemux2 (cmd_cram_freemux2.cpp)
//       --write-singlets: also <O>.clust1.sing2.gz (BGZF), the singlet log-likelihood of every droplet against every
//       cluster as the last EM iteration formed it (llks[j(j+1)/2 + j], cmd_cram_freemux2.cpp:448-455; the reference
//       prints only the best and the next).  One row per droplet, in the order of .clust1.samples.gz, and cluster
//       0 .. K-1.  Columns BARCODE, CLUST, NUM.SNPS, NUM.READS (those of .clust1.samples.gz), LLK1 (%.4lf), POSTPRB
//       (%.3lg, equal priors over the clusters)
//       --write-inclusion: also <O>.clust1.incl.gz (BGZF), one row per droplet of .clust1.samples.gz and cluster 0 .. K-1:
//       the evidence that the cluster is in the droplet, as a singlet or as either half of a doublet, and the cluster it
//       pairs best with, from the last EM iteration (muxgl_fmx_inclusion; the reference keeps only the best and the next
//       doublet, cmd_cram_freemux2.cpp:469-513).  Columns BARCODE, CLUST, NUM.SNPS, NUM.READS, LLK.INCL (%.4lf),
//       POSTPRB.INCL (%.3lg, exp(incl - tot)), DBL.PARTNER (cluster), DBL.LLK (%.4lf); the last two are NA where no
//       doublet hypothesis holds the cluster (one cluster)
//       --write-unknown: also <O>.clust1.unk.gz (BGZF), one row per droplet of .clust1.samples.gz: how well a donor that NO
//       cluster holds explains it, from the last EM iteration -- a donor spread over other clusters because --nsample is
//       too small, or one the greedy start gave no cluster (muxgl_fmx_unknown with the Hardy-Weinberg triple of
//       cmd_cram_freemux2.cpp:388-390 as the unknown donor's genotype prior: the reference's own numbers for a cluster
//       without cells).  Columns BARCODE, NUM.SNPS, NUM.READS, BEST.LLK (of .clust1.samples.gz), UNK.SNG.LLK (one unknown
//       donor), UNK.DBL.LLK (two unknown donors), HALF.CLUST and HALF.LLK (the cluster that pairs best with an unknown
//       donor; ties to the lowest cluster), DIFF.LLK.CLUST.UNK (BEST.LLK minus the largest of the three); LLKs %.4lf
//       --write-ambient: also <O>.clust1.amb.gz (BGZF), one row per droplet of .clust1.samples.gz: the droplet as ONE cell of
//       a cluster plus a share rho of ambient RNA, from the last EM iteration (muxgl_fmx_ambient) -- the reading the
//       reference lacks, which calls a clean singlet from a high-soup prep a doublet of its own cluster with a partner
//       picked nearly at random.  --ambient-rho, --ambient-af and --ambient-max-reads mean what they mean for demuxlet
//       (the default grid too; the droplets of --ambient-max-reads are counted by NUM.READS).  Columns BARCODE, NUM.SNPS,
//       NUM.READS, DROPLET.TYPE, BEST.LLK, SNG.BEST.GUESS, SNG.BEST.LLK (those of .clust1.samples.gz, LLKs %.4lf), AMB.GUESS
//       (the cluster), AMB.RHO (%.2lf: the best share ON THE GRID), AMB.LLK (ties: the lower cluster, then the lower rho
//       index), DIFF.LLK.AMB.BEST = AMB.LLK - BEST.LLK.  The calls and every other file are unchanged
//       --fit-ambient: also <O>.clust1.ambfit.gz (BGZF), per droplet of .clust1.samples.gz one row for SNG.BEST.GUESS and one
//       for SNG.NEXT.GUESS: the maximum-likelihood share of ambient RNA on [0, --ambient-fit-max x] (default 0.5) under the
//       model of --write-ambient, from the last EM iteration, with the profile of --ambient-af / --ambient-max-reads
//       (muxgl_fmx_ambient_fit).  The columns of demuxlet's .ambfit.gz with CLUST in place of SM_ID: BARCODE, NUM.SNPS,
//       NUM.READS, CLUST, SNG.LLK (the cluster's singlet LLK), AMB.RHO.MLE, AMB.RHO.SE (NA on a bound or where the
//       information is not positive), AMB.LLK.MLE, AMB.LRT = 2 (AMB.LLK.MLE - SNG.LLK) (NA at status 6), STATUS (0 interior,
//       1 lower bound, 2 upper bound, 3 step cap, 5 no entries, 6 a posterior row of exactly 0); all %.4lf
//       --fit-alpha: also <O>.clust1.alphafit.gz (BGZF), per droplet of .clust1.samples.gz one row DBL for the two clusters of
//       DBL.BEST.GUESS and one row SNG for (SNG.BEST.GUESS, SNG.NEXT.GUESS) (none where the record has no such cluster): the
//       maximum-likelihood share of the second cluster on [0, --alpha-fit-max x] (default 1.0) under the reference's doublet
//       model with the share set free, from the last EM iteration (muxgl_fmx_alpha_fit; the reference fixes the share at
//       0.5).  The columns of demuxlet's .alphafit.gz with CLUST1 CLUST2 in place of SM1_ID SM2_ID: BARCODE, NUM.SNPS,
//       NUM.READS, PAIR, CLUST1, CLUST2, SNG1.LLK (the first cluster alone), SNG2.LLK (the second alone; NA where x < 1),
//       ALPHA.MLE, ALPHA.SE (NA on a bound or where the information is not positive), MIX.LLK.MLE, MIX.LRT = 2 (MIX.LLK.MLE
//       - the better of SNG1.LLK and SNG2.LLK; SNG1.LLK alone where x < 1; NA at status 6), STATUS; all %.4lf.  A notice
//       counts the droplets called SNG that the mix explains better by more than 2.  The calls and every other file are
//       unchanged
//       --write-cluster-pairs: did the run split one donor over two clusters.  After the EM every pair of final cluster
//       pileups is scored as one donor against two unrelated donors on the device (muxgl_fmx_cluster_pairs).  Writes
//       <O>.clust1.ldist.gz (BGZF), one row per pair a > b in ascending (a, b) order: ID1, ID2, NSNP (markers both have
//       reads at), LLK0, LLK2, LDIFF = LLK2 - LLK0 (%.2lf), DIFF.SNP (%.4lf): the reference's .ldist.gz row
//       (cmd_cram_freemuxlet.cpp:268) without its read-count columns.  One device only
//       --match-vcf FILE: which cluster is which donor.  FILE holds genotypes of some or all pooled donors; it is read with
//       demuxlet's genotype flags and their meanings (--field, --sm, --sm-list, --geno-error-offset, --geno-error-coeff,
//       --r2-info, --min-mac, --min-callrate; known to freemuxlet only next to --match-vcf) by the demuxlet loader, and after
//       the EM the final cluster pileups are scored against the donors on the device (muxgl_fmx_match_donors).  Writes
//       <O>.clust1.match.gz (BGZF), one row per cluster and donor: CLUST, SM_ID, NUM.SNPS (markers the cluster has reads at
//       and the donors have genotypes at), LLK, LLK0 (an unrelated individual at the allele frequencies), LLR = LLK - LLK0
//       (%.4lf), POSTPRB (%.3lg, equal priors over the donors); and <O>.clust1.match.best.gz, one row per cluster: CLUST,
//       NUM.SNPS, BEST.SM_ID, BEST.LLR, NEXT.SM_ID, NEXT.LLR, DIFF.LLR, RECIPROCAL (1: the cluster is also the best
//       cluster of its best donor), NA where there is none.  One device only: refused with --devices naming several
//       --anchor-vcf FILE: a pool of which only some donors are genotyped.  FILE is read as --match-vcf's (the same flags);
//       its n donors, in the VCF's sample order, become clusters 0 .. n-1, held to their genotypes for the whole EM
//       (muxgl_fmx_set_anchors), and the clusters n .. K-1 are learned from the droplets; --nsample K is the total, K >= n.
//       Start: the greedy clusters are matched to the donors (muxgl_fmx_match_donors, csrc/anchor_plan.hpp) and relabelled;
//       with --init-cluster the file's ids are taken as they are (required with --devices naming several).  Writes
//       <O>.clust1.anchors.gz (BGZF), one row per cluster: CLUST, SM_ID, START.CLUST and START.LLR (the greedy cluster the
//       donor started from and the log Bayes factor of that match), N.SNG (droplets called singlets of the cluster); NA for
//       a free cluster or where there was no start match; and, on one device, the two match tables above against the
//       anchor panel.  --match-vcf next to it is an error
//       --anchor-refine (with --anchor-vcf): every anchored donor's genotypes are the PRIOR of the posterior the droplets
//       form (MUXGL_ANCHOR_PRIOR, muxgl_fmx_set_anchors_mode), not the posterior itself: for low-pass or imputed panels,
//       RNA-derived calls, flat GP / PL rows.  --anchor-refine-list FILE: only the donors whose sample IDs FILE lists, one
//       per line; an ID that is no sample of the anchor VCF is an error.  Either flag adds a MODE column (HELD / PRIOR, NA
//       for a free cluster) to <O>.clust1.anchors.gz and writes <O>.clust1.refined.gz (BGZF), one row per PRIOR cluster:
//       CLUST, SM_ID, N.GENO (markers with genotypes), N.CHANGED (those whose most likely genotype moved), MEAN.MAXGP.PRIOR
//       and MEAN.MAXGP.POST (%.4lf: the means of the largest panel and of the largest posterior probability over them).
//       Without the two flags every output is what it is without them, byte for byte
//   popscle-amd freemuxlet-old --plp P --nsample K --out O [...]               mirrors cmdCramFreemuxlet (cmd_cram_freemuxlet.cpp)
//   popscle-amd dump-plp   --plp P [--vcf V --field F] --out FILE              loader only: packed pileup to a binary file
//   popscle-amd synth-plp  --cells C --snps S --samples V --out P              a synthetic data set in the real file formats
//
// Everything here is host plumbing: flag surface, loaders (plp.hpp, vcf.hpp), the sequential control flow of
// the reference commands, and the text writers with the reference's printf formats.  All arithmetic of the path is
// behind muxgl_* calls; there is no CPU implementation of it in this program.
#include <cmath>
#include <fstream>
#include <sstream>

#include "../csrc/anchor_plan.hpp"
#include "plp.hpp"
#include "synthplp.hpp"

using namespace pa;

namespace {

void check(muxgl_handle* h, int rc, const char* what) {
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

void upload(muxgl_handle* h, const Pileup& p) {
  check(h, muxgl_set_pileup(h, p.C(), p.S(), p.nnz(), (int64_t)p.reads.size(), p.cell_ptr.data(), p.entry_snp.data(),
                            p.entry_rptr.data(), p.reads.data()),
        "muxgl_set_pileup");
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

const char* sid(const Pileup& p, int i) { return (i >= 0 && i < p.nv) ? p.sample_ids[(size_t)i].c_str() : "NA"; }

// ---- what the four --fit-ambient / --fit-alpha writers share ----
struct FitField {  // a number of a fit's row as "%.4lf", or NA
  char s[32];
  FitField(bool have, double v) { have ? snprintf(s, sizeof(s), "%.4lf", v) : snprintf(s, sizeof(s), "NA"); }
};
// the standard error of an interior estimate (on a bound: none)
static FitField fit_se(int32_t status, double info) { return FitField(status == 0 && info > 0.0, 1.0 / sqrt(info)); }
// the likelihood ratio against `alone`; NA where it is not finite (freemuxlet: a posterior row of exactly 0 makes LL -inf.
// Demuxlet's LL is finite whatever the input, by the 1e-10 offset of every weight, so its writers never print NA here)
static FitField fit_lrt(double ll_hat, double alone) { return FitField(std::isfinite(2.0 * (ll_hat - alone)), 2.0 * (ll_hat - alone)); }
// what a mix is held against: the first column alone, or, where the fit's interval is the whole [0, 1] (only then is ll_top
// the second column alone), the better of the two
static double fit_alone(bool whole, double ll_zero, double ll_top) { return whole ? std::max(ll_zero, ll_top) : ll_zero; }
// a droplet's slots, -1 where the record has no such column among the n.  An ambient fit, q[2]: SNG.BEST and SNG.NEXT; a
// mixing-share fit, q[4]: DBL, the two columns of DBL.BEST, and SNG, (SNG.BEST, SNG.NEXT), both -1 where one is missing
static void fit_cands(int32_t* q, bool valid, int sBest, int sNext, int n) {
  q[0] = (valid && sBest >= 0 && sBest < n) ? sBest : -1;
  q[1] = (valid && sNext >= 0 && sNext < n) ? sNext : -1;
}
static void fit_pairs(int32_t* q, bool valid, int dBest1, int dBest2, int sBest, int sNext, int n) {
  auto ok = [&](int s) { return s >= 0 && s < n; };
  const bool dbl = valid && ok(dBest1) && ok(dBest2), sng = valid && ok(sBest) && ok(sNext);
  q[0] = dbl ? dBest1 : -1, q[1] = dbl ? dBest2 : -1;
  q[2] = sng ? sBest : -1, q[3] = sng ? sNext : -1;
}

// ------------------------------------------------------------------------------------------------ demuxlet
int cmd_demuxlet(int argc, char** argv) {
  CommonFlags cf;
  VcfReader vr;
  std::vector<std::string> smIDs;
  std::string smList;
  std::vector<double> gridAlpha;
  double doublet_prior = 0.5;  // cmd_cram_demuxlet.cpp:32
  std::string sam, tagGroup, tagUMI;
  int32_t dummy_i = 0;
  bool deviceCalls = false;  // (ours) skip the host pass that settles mirrored alpha = 0.5 pairs and near-tie calls as the reference does
  bool writeSinglets = false;  // (ours) <out>.sing2.gz: the reference's disabled .sing2 writer (:580,839-848)
  bool writeInclusion = false;  // (ours) <out>.incl.gz: per-sample marginals of the disabled .pair writer (:852-877)
  bool writeUnknown = false;  // (ours) <out>.unk.gz: the droplet against a donor missing from the VCF (llksA0 / llks00, :749-773)
  bool writeAmbient = false;  // (ours) <out>.amb.gz: the droplet as one cell plus a share of ambient RNA (muxgl_demux_ambient)
  bool fitAmbient = false;  // (ours) <out>.ambfit.gz: the maximum-likelihood ambient share with its standard error (muxgl_demux_ambient_fit)
  double ambFitMax = 0.5;
  bool fitAlpha = false;  // (ours) <out>.alphafit.gz: the maximum-likelihood mixing share of the best doublet and of the two best singlets (muxgl_demux_alpha_fit)
  double alphaFitMax = 1.0;
  std::vector<double> ambRho;
  std::string ambAfFile;
  int32_t ambMaxReads = 0;
  Args a;
  cf.add(a);
  a.add_bool("write-unknown", &writeUnknown);
  a.add_bool("write-ambient", &writeAmbient);
  a.add_bool("fit-ambient", &fitAmbient);
  a.add_double("ambient-fit-max", &ambFitMax);
  a.add_bool("fit-alpha", &fitAlpha);
  a.add_double("alpha-fit-max", &alphaFitMax);
  a.add_multi_double("ambient-rho", &ambRho);
  a.add_string("ambient-af", &ambAfFile);
  a.add_int("ambient-max-reads", &ambMaxReads);
  a.add_bool("device-calls", &deviceCalls);
  a.add_bool("write-singlets", &writeSinglets);
  a.add_bool("write-inclusion", &writeInclusion);
  a.add_string("vcf", &vr.path);
  a.add_string("field", &cf.lo.field);
  a.add_double("geno-error-offset", &cf.lo.genoErrorOffset);
  a.add_double("geno-error-coeff", &cf.lo.genoErrorCoeffR2);
  a.add_string("r2-info", &cf.lo.r2info);
  a.add_int("min-mac", &vr.vfilt.minMAC);
  a.add_double("min-callrate", &vr.vfilt.minCallRate);
  a.add_multi_string("sm", &smIDs);
  a.add_string("sm-list", &smList);
  a.add_multi_double("alpha", &gridAlpha);
  a.add_double("doublet-prior", &doublet_prior);
  a.add_string("sam", &sam);  // BAM-direct mode needs htslib: accepted and rejected
  a.add_string("tag-group", &tagGroup);
  a.add_string("tag-UMI", &tagUMI);
  a.add_int("sam-verbose", &dummy_i);
  a.add_int("vcf-verbose", &dummy_i);
  a.add_int("min-MQ", &dummy_i);
  a.add_int("min-TD", &dummy_i);
  a.add_int("excl-flag", &dummy_i);
  a.parse(argc, argv);
  if (!sam.empty()) fatal("--sam (BAM-direct mode) is not available in this build: run dsc-pileup first and pass --plp");
  if (cf.plpPrefix.empty() || vr.path.empty() || cf.outPrefix.empty()) fatal("Missing required option(s) : --plp, --vcf, --out");
  if (gridAlpha.empty()) {  // :85-89
    gridAlpha.push_back(0);
    gridAlpha.push_back(0.5);
  }
  if ((int)gridAlpha.size() > MUXGL_MAX_ALPHA) fatal("at most %d --alpha values are supported", MUXGL_MAX_ALPHA);
  if (ambRho.empty()) ambRho = {0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5};
  if ((int)ambRho.size() > MUXGL_MAX_ALPHA) fatal("at most %d --ambient-rho values are supported", MUXGL_MAX_ALPHA);
  if (ambMaxReads < 0) fatal("--ambient-max-reads must not be negative");
  if (!(std::isfinite(ambFitMax) && ambFitMax > 0.0 && ambFitMax <= 1.0)) fatal("--ambient-fit-max must lie in (0, 1]");
  if (!(std::isfinite(alphaFitMax) && alphaFitMax > 0.0 && alphaFitMax <= 1.0)) fatal("--alpha-fit-max must lie in (0, 1]");
  vr.wanted = smIDs;
  if (!smList.empty()) {
    TsvReader t(smList);
    while (t.read_line() > 0) vr.wanted.push_back(t.str_field_at(0));
  }
  vr.init();
  Pileup p;
  StageTimer tm;
  load_from_plp(cf.plpPrefix, cf.lo, &vr, p);
  tm.lap("demuxlet: load");

  muxgl_config cfg = cf.config(MUXGL_FLAG_DEMUX_ONLY);  // cells are independent: a group needs no column slabs
  muxgl_handle* h = nullptr;
  if (muxgl_create(&cfg, &h) != 0) fatal("%s", muxgl_last_error(nullptr));
  tm.lap("demuxlet: device init");
  upload(h, p);
  check(h, muxgl_demux_set_gp(h, p.nv, p.gp.data(), p.has_gp.data()), "muxgl_demux_set_gp");
  tm.lap("demuxlet: hand-over (H2D+plans)");
  muxgl_demux_params dp;
  memset(&dp, 0, sizeof(dp));
  dp.n_alpha = (int32_t)gridAlpha.size();
  for (size_t i = 0; i < gridAlpha.size(); ++i) dp.alpha[i] = gridAlpha[i];
  dp.doublet_prior = doublet_prior;
  notice("Starting to identify best matching individual IDs");
  std::vector<muxgl_demux_cell> cells((size_t)p.C());
  check(h, muxgl_demux_run(h, &dp, cells.data(), nullptr), "muxgl_demux_run");
  tm.lap("demuxlet: muxgl_demux_run");
  if (!deviceCalls) {
    // the calls rounding noise could decide -- the order of a mirrored alpha = 0.5 pair in DBL.BEST.GUESS / NEXT.GUESS
    // (cmd_cram_demuxlet.cpp:738-746,883-906) and near ties of the scans and thresholds (:827-837,925-988) -- settled in
    // the reference's own arithmetic (exact_calls.hpp)
    int64_t st[6];
    check(h, muxgl_demux_exact_calls(p.C(), p.nv, p.cell_ptr.data(), p.entry_snp.data(), p.entry_rptr.data(), p.reads.data(),
                                     p.gp.data(), p.has_gp.data(), &dp, cells.data(), compute_threads(), st),
          "muxgl_demux_exact_calls");
    notice("Exact-call pass: %lld droplets looked at (%lld near ties besides mirrored pairs, %lld needing every hypothesis, "
           "%lld calls changed)", (long long)st[0], (long long)st[3], (long long)st[4], (long long)st[5]);
    tm.lap("demuxlet: exact calls (host)");
  }

  // .best, cmd_cram_demuxlet.cpp:629,636-641,993-1013: rows in barcode-sorted order, INT_ID counts skipped cells too
  OutFile w(cf.outPrefix + ".best", false);
  w.printf("INT_ID\tBARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.GUESS\tBEST.LLK\tNEXT.GUESS\tNEXT.LLK\t"
           "DIFF.LLK.BEST.NEXT\tBEST.POSTERIOR\tSNG.POSTERIOR\tSNG.BEST.GUESS\tSNG.BEST.LLK\tSNG.NEXT.GUESS\t"
           "SNG.NEXT.LLK\tSNG.ONLY.POSTERIOR\tDBL.BEST.GUESS\tDBL.BEST.LLK\tDIFF.LLK.SNG.DBL\n");
  std::map<std::string, int32_t> bc_map;
  for (int64_t i = 0; i < p.C(); ++i) bc_map[p.bcs[(size_t)i]] = (int32_t)i;
  static const char* tname[3] = {"SNG", "DBL", "AMB"};
  int ncells = 0;
  for (auto it = bc_map.begin(); it != bc_map.end(); ++it, ++ncells) {
    const int32_t i = it->second;
    const muxgl_demux_cell& c = cells[(size_t)i];
    if (p.cell_totl_reads[(size_t)i] < cf.lo.minRead || p.cell_uniq_reads[(size_t)i] < cf.lo.minUMI ||
        c.nsnps < cf.lo.minSNP)
      continue;  // :641
    if (!c.valid) continue;  // :653
    auto al = [&](int n) { return (n >= 0 && n < dp.n_alpha) ? dp.alpha[n] : NAN; };
    w.printf("%d\t%s\t%u\t%d\t%s\t%s,%s,%.2lf\t%.2lf\t%s,%s,%.2lf\t%.2lf\t%.2lf\t%.2lg\t%.2lg\t%s\t%.2lf\t%s\t%.2lf\t"
             "%.5lf\t%s,%s,%.2lf\t%.2lf\t%.2lf\n",
             ncells, it->first.c_str(), (unsigned)c.nsnps, p.cell_uniq_reads[(size_t)i], tname[c.type],
             sid(p, c.jBest), sid(p, c.kBest), al(c.aBest), c.bestLLK, sid(p, c.jNext), sid(p, c.kNext), al(c.aNext),
             c.nextLLK, c.bestLLK - c.nextLLK, c.bestPP, c.sngPP, sid(p, c.sBest), c.sngBestLLK, sid(p, c.sNext),
             c.sngNextLLK, c.sngOnlyPP, sid(p, c.dBest1), sid(p, c.dBest2), al(c.dBestA), c.dblBestLLK,
             c.sngBestLLK - c.dblBestLLK);
  }
  w.close();
  tm.lap("demuxlet: write .best");
  if (writeSinglets) {
    // .sing2.gz: one row per printed droplet (the order and the filters of .best) and sample, in VCF column order.
    // POSTPRB is the writer's posterior with equal priors over the samples: a softmax over the droplet's row
    const size_t V = (size_t)p.nv;
    std::vector<double> sng((size_t)p.C() * V);
    check(h, muxgl_demux_singlets(h, &dp, sng.data()), "muxgl_demux_singlets");
    tm.lap("demuxlet: muxgl_demux_singlets");
    OutFile ws(cf.outPrefix + ".sing2.gz", true);
    ws.printf("BARCODE\tSM_ID\tNUM.SNPS\tNUM.READS\tLLK1\tPOSTPRB\n");
    for (auto it = bc_map.begin(); it != bc_map.end(); ++it) {
      const int32_t i = it->second;
      const muxgl_demux_cell& c = cells[(size_t)i];
      if (p.cell_totl_reads[(size_t)i] < cf.lo.minRead || p.cell_uniq_reads[(size_t)i] < cf.lo.minUMI ||
          c.nsnps < cf.lo.minSNP || !c.valid)
        continue;
      const double* row = sng.data() + (size_t)i * V;
      double mx = row[0], sum = 0.0;
      for (size_t j = 1; j < V; ++j) mx = std::max(mx, row[j]);
      for (size_t j = 0; j < V; ++j) sum += exp(row[j] - mx);
      for (size_t j = 0; j < V; ++j)
        ws.printf("%s\t%s\t%u\t%d\t%.4lf\t%.3lg\n", it->first.c_str(), sid(p, (int)j), (unsigned)c.nsnps,
                  p.cell_uniq_reads[(size_t)i], row[j], exp(row[j] - mx) / sum);
    }
    ws.close();
    tm.lap("demuxlet: write .sing2.gz");
  }
  if (writeInclusion) {
    // .incl.gz: one row per printed droplet (the order and the filters of .best) and sample, in VCF column order
    const size_t V = (size_t)p.nv, n = (size_t)p.C() * V;
    std::vector<double> incl(n), tot((size_t)p.C()), dbl(n);
    std::vector<int32_t> partner(n), aidx(n), first(n);
    check(h, muxgl_demux_inclusion(h, &dp, incl.data(), tot.data(), dbl.data(), partner.data(), aidx.data(), first.data()),
          "muxgl_demux_inclusion");
    tm.lap("demuxlet: muxgl_demux_inclusion");
    OutFile wi(cf.outPrefix + ".incl.gz", true);
    wi.printf("BARCODE\tSM_ID\tNUM.SNPS\tNUM.READS\tLLK.INCL\tPOSTPRB.INCL\tDBL.PARTNER\tDBL.ALPHA\tDBL.LLK\n");
    for (auto it = bc_map.begin(); it != bc_map.end(); ++it) {
      const int32_t i = it->second;
      const muxgl_demux_cell& c = cells[(size_t)i];
      if (p.cell_totl_reads[(size_t)i] < cf.lo.minRead || p.cell_uniq_reads[(size_t)i] < cf.lo.minUMI ||
          c.nsnps < cf.lo.minSNP || !c.valid)
        continue;
      for (size_t j = 0; j < V; ++j) {
        const size_t x = (size_t)i * V + j;
        wi.printf("%s\t%s\t%u\t%d\t%.4lf\t%.3lg\t", it->first.c_str(), sid(p, (int)j), (unsigned)c.nsnps,
                  p.cell_uniq_reads[(size_t)i], incl[x], exp(incl[x] - tot[(size_t)i]));
        if (partner[x] < 0) {
          wi.printf("NA\tNA\tNA\n");
        } else {
          const double a = dp.alpha[aidx[x]];
          wi.printf("%s\t%.3lf\t%.4lf\n", sid(p, partner[x]), first[x] ? 1.0 - a : a, dbl[x]);
        }
      }
    }
    wi.close();
    tm.lap("demuxlet: write .incl.gz");
  }
  if (writeUnknown) {
    // .unk.gz: one row per printed droplet (the order and the filters of .best).  The best hypothesis with one panel
    // sample: (j, n >= 1, known donor first) and, where alpha[n] != 0.5, (k, n >= 1, known donor second) -- at 0.5 the
    // two are one hypothesis, the reference's k < j rule for mirrored pairs (:812-815); ties by value, then (sample, n,
    // known donor first) ascending
    const size_t V = (size_t)p.nv, A = (size_t)dp.n_alpha;
    std::vector<double> ju((size_t)p.C() * V * A), uj((size_t)p.C() * V * A), uu((size_t)p.C() * A);
    check(h, muxgl_demux_unknown(h, &dp, nullptr, ju.data(), uj.data(), uu.data(), nullptr), "muxgl_demux_unknown");
    tm.lap("demuxlet: muxgl_demux_unknown");
    OutFile wu(cf.outPrefix + ".unk.gz", true);
    wu.printf("BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.ALPHA\tUNK.DBL.LLK\tHALF.GUESS\tHALF.LLK\t"
              "DIFF.LLK.PANEL.UNK\n");
    for (auto it = bc_map.begin(); it != bc_map.end(); ++it) {
      const int32_t i = it->second;
      const muxgl_demux_cell& c = cells[(size_t)i];
      if (p.cell_totl_reads[(size_t)i] < cf.lo.minRead || p.cell_uniq_reads[(size_t)i] < cf.lo.minUMI ||
          c.nsnps < cf.lo.minSNP || !c.valid)
        continue;
      const double* r2 = uu.data() + (size_t)i * A;
      double top = r2[0], dblv = -1e300, halfv = -1e300;
      int dn = -1, hj = -1, hn = -1, hmajor = -1;
      for (size_t n = 1; n < A; ++n)
        if (r2[n] > dblv) dblv = r2[n], dn = (int)n;
      for (size_t j = 0; j < V; ++j)
        for (size_t n = 1; n < A; ++n) {
          const size_t x = ((size_t)i * V + j) * A + n;
          if (ju[x] > halfv) halfv = ju[x], hj = (int)j, hn = (int)n, hmajor = 1;
          if (dp.alpha[n] != 0.5 && uj[x] > halfv) halfv = uj[x], hj = (int)j, hn = (int)n, hmajor = 0;
        }
      wu.printf("%s\t%u\t%d\t%.4lf\t%.4lf\t", it->first.c_str(), (unsigned)c.nsnps, p.cell_uniq_reads[(size_t)i], c.bestLLK, r2[0]);
      if (dn < 0) {
        wu.printf("NA\tNA\t");
      } else {
        wu.printf("%.2lf\t%.4lf\t", dp.alpha[dn], dblv);
        top = std::max(top, dblv);
      }
      if (hj < 0) {
        wu.printf("NA\tNA\t");
      } else {
        wu.printf("%s,%s,%.2lf\t%.4lf\t", hmajor ? sid(p, hj) : "*", hmajor ? "*" : sid(p, hj), dp.alpha[hn], halfv);
        top = std::max(top, halfv);
      }
      wu.printf("%.4lf\n", c.bestLLK - top);
    }
    wu.close();
    tm.lap("demuxlet: write .unk.gz");
  }
  // The ambient profile of --write-ambient and --fit-ambient: the caller's file, or the pileup's own reads with one
  // pseudo-read at the population frequency; made once
  std::vector<double> ambProfile;
  auto ambient_profile = [&]() -> const std::vector<double>& {
    const size_t S = (size_t)p.S();
    std::vector<double>& f = ambProfile;
    if (!f.empty() || S == 0) return f;
    f.resize(S);
    if (!ambAfFile.empty()) {
      TsvReader t(ambAfFile);
      size_t n = 0;
      for (; t.read_line() > 0; ++n)
        if (n < S) f[n] = t.double_field_at(0);
      if (n != S) fatal("--ambient-af: %s holds %zu lines, the pileup has %zu markers", ambAfFile.c_str(), n, S);
    } else {
      std::vector<uint8_t> mask;
      if (ambMaxReads > 0) {
        mask.resize((size_t)p.C());
        int64_t kept = 0;
        for (int64_t i = 0; i < p.C(); ++i) kept += mask[(size_t)i] = p.cell_uniq_reads[(size_t)i] <= ambMaxReads;
        notice("Ambient profile from the %lld of %lld droplets with at most %d reads", (long long)kept, (long long)p.C(), ambMaxReads);
      }
      std::vector<int64_t> n_ref(S), n_alt(S);
      check(h, muxgl_pileup_allele_counts(h, mask.empty() ? nullptr : mask.data(), n_ref.data(), n_alt.data()),
            "muxgl_pileup_allele_counts");
      for (size_t s = 0; s < S; ++s)
        f[s] = ((double)n_alt[s] + p.snps[s].af) / ((double)n_ref[s] + (double)n_alt[s] + 1.0);
      tm.lap("demuxlet: muxgl_pileup_allele_counts");
    }
    return f;
  };
  if (writeAmbient) {
    // .amb.gz: one row per printed droplet (the order and the filters of .best)
    const size_t V = (size_t)p.nv, NR = ambRho.size();
    const std::vector<double>& f = ambient_profile();
    std::vector<double> amb((size_t)p.C() * V * NR);
    check(h, muxgl_demux_ambient(h, &dp, f.data(), (int32_t)NR, ambRho.data(), amb.data(), nullptr), "muxgl_demux_ambient");
    tm.lap("demuxlet: muxgl_demux_ambient");
    OutFile wa(cf.outPrefix + ".amb.gz", true);
    wa.printf("BARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.LLK\tSNG.BEST.GUESS\tSNG.BEST.LLK\tAMB.GUESS\tAMB.RHO\tAMB.LLK\t"
              "DIFF.LLK.AMB.BEST\n");
    int64_t rescued = 0;
    for (auto it = bc_map.begin(); it != bc_map.end(); ++it) {
      const int32_t i = it->second;
      const muxgl_demux_cell& c = cells[(size_t)i];
      if (p.cell_totl_reads[(size_t)i] < cf.lo.minRead || p.cell_uniq_reads[(size_t)i] < cf.lo.minUMI ||
          c.nsnps < cf.lo.minSNP || !c.valid)
        continue;
      const double* row = amb.data() + (size_t)i * V * NR;
      size_t at = 0;  // the best (sample, rho): by value, then (sample, rho index) ascending
      for (size_t x = 1; x < V * NR; ++x)
        if (row[x] > row[at]) at = x;
      if (c.type == 1 && row[at] > c.dblBestLLK + 2.0) ++rescued;
      wa.printf("%s\t%u\t%d\t%s\t%.4lf\t%s\t%.4lf\t%s\t%.2lf\t%.4lf\t%.4lf\n", it->first.c_str(), (unsigned)c.nsnps,
                p.cell_uniq_reads[(size_t)i], tname[c.type], c.bestLLK, sid(p, c.sBest), c.sngBestLLK, sid(p, (int)(at / NR)),
                ambRho[at % NR], row[at], row[at] - c.bestLLK);
    }
    wa.close();
    notice("Ambient RNA: %lld droplets called DBL are explained better, by more than 2 in log-likelihood, as one cell plus "
           "ambient RNA than as their best doublet", (long long)rescued);
    tm.lap("demuxlet: write .amb.gz");
  }
  if (fitAmbient) {
    // .ambfit.gz: per printed droplet (the order and the filters of .best) one row for SNG.BEST.GUESS and one for
    // SNG.NEXT.GUESS (none where .best has NA there)
    const std::vector<double>& f = ambient_profile();
    const size_t n = (size_t)p.C() * 2;
    std::vector<int32_t> cand(n), status(n);
    for (int64_t i = 0; i < p.C(); ++i) {
      const muxgl_demux_cell& c = cells[(size_t)i];
      fit_cands(&cand[(size_t)i * 2], c.valid, c.sBest, c.sNext, p.nv);
    }
    std::vector<double> rho(n), llh(n), ll0(n), info(n);
    check(h, muxgl_demux_ambient_fit(h, &dp, f.data(), 2, cand.data(), ambFitMax, rho.data(), llh.data(), ll0.data(), info.data(),
                                     status.data(), nullptr, nullptr),
          "muxgl_demux_ambient_fit");
    tm.lap("demuxlet: muxgl_demux_ambient_fit");
    OutFile wf(cf.outPrefix + ".ambfit.gz", true);
    wf.printf("BARCODE\tNUM.SNPS\tNUM.READS\tSM_ID\tSNG.LLK\tAMB.RHO.MLE\tAMB.RHO.SE\tAMB.LLK.MLE\tAMB.LRT\tSTATUS\n");
    for (auto it = bc_map.begin(); it != bc_map.end(); ++it) {
      const int32_t i = it->second;
      const muxgl_demux_cell& c = cells[(size_t)i];
      if (p.cell_totl_reads[(size_t)i] < cf.lo.minRead || p.cell_uniq_reads[(size_t)i] < cf.lo.minUMI ||
          c.nsnps < cf.lo.minSNP || !c.valid)
        continue;
      for (size_t k = 0; k < 2; ++k) {
        const size_t x = (size_t)i * 2 + k;
        if (cand[x] < 0) continue;
        wf.printf("%s\t%u\t%d\t%s\t%.4lf\t%.4lf\t%s\t%.4lf\t%s\t%d\n", it->first.c_str(), (unsigned)c.nsnps,
                  p.cell_uniq_reads[(size_t)i], sid(p, cand[x]), ll0[x], rho[x], fit_se(status[x], info[x]).s, llh[x],
                  fit_lrt(llh[x], ll0[x]).s, (int)status[x]);
      }
    }
    wf.close();
    tm.lap("demuxlet: write .ambfit.gz");
  }
  if (fitAlpha) {
    // .alphafit.gz: per printed droplet (the order and the filters of .best) one row DBL for the two samples of DBL.BEST
    // and one row SNG for (SNG.BEST, SNG.NEXT) (none where .best has NA there)
    const size_t n = (size_t)p.C() * 2;
    std::vector<int32_t> pair(n * 2), status(n);
    for (int64_t i = 0; i < p.C(); ++i) {
      const muxgl_demux_cell& c = cells[(size_t)i];
      fit_pairs(&pair[(size_t)i * 4], c.valid, c.dBest1, c.dBest2, c.sBest, c.sNext, p.nv);
    }
    std::vector<double> ah(n), llh(n), ll0(n), llt(n), info(n);
    check(h, muxgl_demux_alpha_fit(h, &dp, 2, pair.data(), alphaFitMax, ah.data(), llh.data(), ll0.data(), llt.data(), info.data(),
                                   status.data(), nullptr, nullptr),
          "muxgl_demux_alpha_fit");
    tm.lap("demuxlet: muxgl_demux_alpha_fit");
    OutFile wf(cf.outPrefix + ".alphafit.gz", true);
    wf.printf("BARCODE\tNUM.SNPS\tNUM.READS\tPAIR\tSM1_ID\tSM2_ID\tSNG1.LLK\tSNG2.LLK\tALPHA.MLE\tALPHA.SE\tMIX.LLK.MLE\tMIX.LRT\t"
              "STATUS\n");
    const bool whole = alphaFitMax == 1.0;
    int64_t mixed = 0;
    for (auto it = bc_map.begin(); it != bc_map.end(); ++it) {
      const int32_t i = it->second;
      const muxgl_demux_cell& c = cells[(size_t)i];
      if (p.cell_totl_reads[(size_t)i] < cf.lo.minRead || p.cell_uniq_reads[(size_t)i] < cf.lo.minUMI ||
          c.nsnps < cf.lo.minSNP || !c.valid)
        continue;
      for (size_t k = 0; k < 2; ++k) {
        const size_t x = (size_t)i * 2 + k;
        if (pair[x * 2] < 0) continue;
        const double one = fit_alone(whole, ll0[x], llt[x]);
        wf.printf("%s\t%u\t%d\t%s\t%s\t%s\t%.4lf\t%s\t%.4lf\t%s\t%.4lf\t%s\t%d\n", it->first.c_str(), (unsigned)c.nsnps,
                  p.cell_uniq_reads[(size_t)i], k == 0 ? "DBL" : "SNG", sid(p, pair[x * 2]), sid(p, pair[x * 2 + 1]), ll0[x],
                  FitField(whole, llt[x]).s, ah[x], fit_se(status[x], info[x]).s, llh[x], fit_lrt(llh[x], one).s,
                  (int)status[x]);
        if (k == 1 && c.type == 0 && llh[x] > one + 2.0) ++mixed;
      }
    }
    wf.close();
    notice("Mixing share: %lld droplets called SNG are explained better, by more than 2 in log-likelihood, as a mix of their "
           "best and next singlet at the fitted share than as the better of the two alone", (long long)mixed);
    tm.lap("demuxlet: write .alphafit.gz");
  }
  notice("Finished writing output files");
  muxgl_destroy(h);
  return 0;
}

// ------------------------------------------------------------------------------------------------ freemuxlet
// rows [0, n) of a table, formatted by the worker pool in batches and written in order
template <class F>
void write_rows_parallel(OutFile& w, int64_t n, F format_row) {
  constexpr int64_t GRAIN = 1024, BATCH = 64;  // rows per work item, work items per batch
  std::vector<std::string> parts((size_t)BATCH);
  for (int64_t r0 = 0; r0 < n; r0 += GRAIN * BATCH) {
    const int64_t nparts = std::min<int64_t>(BATCH, (n - r0 + GRAIN - 1) / GRAIN);
    parallel_for(nparts, plp_threads(), [&](int64_t i) {
      std::string& o = parts[(size_t)i];
      o.clear();
      for (int64_t r = r0 + i * GRAIN, re = std::min(n, r + GRAIN); r < re; ++r) format_row(r, o);
    });
    for (int64_t i = 0; i < nparts; ++i) w.write(parts[(size_t)i].data(), parts[(size_t)i].size());
  }
}

// old_clust0: the .clust0.vcf.gz of freemuxlet-old (cmd_cram_freemuxlet.cpp:377-431) differs from every other cluster
// VCF in two expressions: pps = gps * gls / maxGL (:409-411) and gq = (int)(-0.1*log10(..)) (:421)
void write_cluster_vcf(const std::string& path, const Pileup& p, int K, const double* gls /* [K][S][9] */,
                       const int32_t* cnt /* [K][S][3] */, const std::vector<uint8_t>& snps_observed, const tm* ltm,
                       bool old_clust0 = false) {
  // cmd_cram_freemux2.cpp:608-658 == cmd_cram_freemuxlet.cpp:655-707
  OutFile vc(path, true);
  vc.printf("##fileformat=VCFv4.2\n");
  vc.printf("##fileDate=%04d%02d%02d\n", 1970 + ltm->tm_year, 1 + ltm->tm_mon, ltm->tm_mday);  // sic: 1970+
  vc.printf("##source=cramore-freemuxlet\n");
  for (size_t i = 0; i < p.rid2chr.size(); ++i) vc.printf("##contig=<ID=%s>\n", p.rid2chr[i].c_str());
  vc.printf("##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele Frequency\">\n");
  vc.printf("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n");
  vc.printf("##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Phred-scale Genotype Quality\">\n");
  vc.printf("##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Read Depth\">\n");
  vc.printf("##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Allelic Read Depth\">\n");
  vc.printf("##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scale genotype likelihood\">\n");
  vc.printf("##FORMAT=<ID=GP,Number=G,Type=Float,Description=\"Posterior probability using pooled allele frequencies\">\n");
  vc.printf("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT");
  for (int i = 0; i < K; ++i) vc.printf("\tCLUST%d", i);
  vc.printf("\n");
  const int64_t S = p.S();
  // rows are formatted by the worker pool in batches of SNPs and written in order
  auto appendf = [](std::string& o, const char* fmt, auto... args) {
    char buf[512];
    const int n = snprintf(buf, sizeof(buf), fmt, args...);
    o.append(buf, (size_t)(n < (int)sizeof(buf) ? n : (int)sizeof(buf) - 1));
  };
  std::atomic<int> checked(0);
  static const bool check_all = getenv("POPSCLE_AMD_CHECK_FORMAT") != nullptr;
  auto format_snp = [&](int64_t v, std::string& o) {
    const SnpInfo& s = p.snps[(size_t)v];
    appendf(o, "%s\t%d\t.\t%c\t%c\t.\tPASS\tAF=%.5lf\tGT:GQ:DP:AD:PL:GP", p.rid2chr[(size_t)s.rid].c_str(), s.pos,
            s.ref, s.alt, s.af);
    const double gps[3] = {(1. - s.af) * (1. - s.af), 2. * s.af * (1. - s.af), s.af * s.af};
    for (int i = 0; i < K; ++i) {
      const double* g = &gls[((size_t)i * S + v) * 9];
      const int32_t* c = &cnt[((size_t)i * S + v) * 3];
      double maxGL = g[0];
      if (maxGL < g[4]) maxGL = g[4];
      if (maxGL < g[8]) maxGL = g[8];
      int32_t pls[3];
      pls[0] = (int32_t)(-10.0 * log10(g[0] / maxGL));
      pls[1] = (int32_t)(-10.0 * log10(g[4] / maxGL));
      pls[2] = (int32_t)(-10.0 * log10(g[8] / maxGL));
      double pps[3];
      if (old_clust0) {
        pps[0] = gps[0] * g[0] / maxGL + 1e-100;
        pps[1] = gps[1] * g[4] / maxGL + 1e-100;
        pps[2] = gps[2] * g[8] / maxGL + 1e-100;
      } else {
        pps[0] = gps[0] * (g[0] / maxGL) + 1e-100;
        pps[1] = gps[1] * (g[4] / maxGL) + 1e-100;
        pps[2] = gps[2] * (g[8] / maxGL) + 1e-100;
      }
      const double sumPP = pps[0] + pps[1] + pps[2];
      pps[0] /= sumPP;
      pps[1] /= sumPP;
      pps[2] /= sumPP;
      const int bestG = (pps[0] > pps[1]) ? (pps[0] > pps[2] ? 0 : 2) : (pps[1] > pps[2] ? 1 : 2);
      int32_t gq = old_clust0 ? (int32_t)(-0.1 * log10(1 - pps[bestG] + 1e-100))
                              : (int32_t)(-10 * log10(1.0 - pps[bestG] + 1e-100));
      if (gq > 255) gq = 255;
      // "\t%d/%d:%d:%d:%d,%d:%d,%d,%d:%.3lg,%.3lg,%.3lg" (cmd_cram_freemux2.cpp:650-652), digit for digit (util.hpp:
      // fmt_int, fmt_g3_or_printf -- the latter hands any value it is not sure of to printf itself)
      char fb[192];
      int k = 0;
      fb[k++] = '\t';
      fb[k++] = bestG == 2 ? '1' : '0';
      fb[k++] = '/';
      fb[k++] = bestG > 0 ? '1' : '0';
      fb[k++] = ':';
      k += fmt_int(gq, fb + k);
      fb[k++] = ':';
      k += fmt_int(c[0], fb + k);
      fb[k++] = ':';
      k += fmt_int(c[1], fb + k);
      fb[k++] = ',';
      k += fmt_int(c[2], fb + k);
      fb[k++] = ':';
      k += fmt_int(pls[0], fb + k);
      fb[k++] = ',';
      k += fmt_int(pls[1], fb + k);
      fb[k++] = ',';
      k += fmt_int(pls[2], fb + k);
      fb[k++] = ':';
      k += fmt_g3_or_printf(pps[0], fb + k);
      fb[k++] = ',';
      k += fmt_g3_or_printf(pps[1], fb + k);
      fb[k++] = ',';
      k += fmt_g3_or_printf(pps[2], fb + k);
      // the reference's own conversion specification stays the authority: the first fields of every file (and every
      // field with POPSCLE_AMD_CHECK_FORMAT=1) are also printed with it and compared
      if (check_all || checked.load(std::memory_order_relaxed) < 4096) {
        checked.fetch_add(1, std::memory_order_relaxed);
        char ref[192];
        const int n = snprintf(ref, sizeof(ref), "\t%d/%d:%d:%d:%d,%d:%d,%d,%d:%.3lg,%.3lg,%.3lg", bestG == 2 ? 1 : 0,
                               bestG > 0 ? 1 : 0, gq, c[0], c[1], c[2], pls[0], pls[1], pls[2], pps[0], pps[1], pps[2]);
        if (n != k || memcmp(ref, fb, (size_t)k) != 0) {
          fb[k] = 0;
          fatal("cluster VCF: the fast number formatting wrote '%s' where printf writes '%s'", fb + 1, ref + 1);
        }
      }
      o.append(fb, (size_t)k);
    }
    o.push_back('\n');
  };
  constexpr int64_t GRAIN = 256, BATCH = 64;  // SNPs per work item, work items per batch
  std::vector<std::string> parts((size_t)BATCH);
  for (int64_t v0 = 0; v0 < S; v0 += GRAIN * BATCH) {
    const int64_t nparts = std::min<int64_t>(BATCH, (S - v0 + GRAIN - 1) / GRAIN);
    parallel_for(nparts, plp_threads(), [&](int64_t i) {
      std::string& o = parts[(size_t)i];
      o.clear();
      const int64_t vb = v0 + i * GRAIN, ve = std::min(S, vb + GRAIN);
      for (int64_t v = vb; v < ve; ++v)
        if (snps_observed[(size_t)v]) format_snp(v, o);
    });
    for (int64_t i = 0; i < nparts; ++i) vc.write(parts[(size_t)i].data(), parts[(size_t)i].size());
  }
  vc.close();
}

// snps_observed[v] = 1 for every marker some droplet covers (cmd_cram_freemux2.cpp:279-288).  Threads over the entries;
// the flags are accessed with relaxed atomics (several threads may store the same 1), and a set flag is only read, so that
// its cache line stays shared between the threads.
static void mark_observed_snps(const Pileup& p, std::vector<uint8_t>& snps_observed) {
  const int64_t nnz = p.nnz(), grain = 1 << 20;
  const int32_t* es = p.entry_snp.data();
  uint8_t* so = snps_observed.data();
  parallel_for((nnz + grain - 1) / grain, plp_threads(), [&](int64_t b) {
    for (int64_t e = b * grain, e1 = std::min(nnz, (b + 1) * grain); e < e1; ++e)
      if (!__atomic_load_n(so + es[e], __ATOMIC_RELAXED)) __atomic_store_n(so + es[e], (uint8_t)1, __ATOMIC_RELAXED);
  });
}

int cmd_freemuxlet(int argc, char** argv) {
  CommonFlags cf;
  std::string initClusterFile;
  double doublet_prior = 0.5, geno_error = 0.1, bfThres = 5.41, fracInitClust = 1.0;  // cmd_cram_freemux2.cpp:19-28
  double singletScoreThres = -1e300;
  int32_t nSamples = 0, initIteration = 10, randomSeed = 0, verbose = 0, maxIter = 10;
  bool auxFiles = false, keepInitMissing = false, randomizeSingletScore = false, noEarlyStop = false;
  bool writeSinglets = false;  // (ours) <out>.clust1.sing2.gz: every droplet against every cluster
  bool writeInclusion = false;  // (ours) <out>.clust1.incl.gz: per-cluster marginals of the last E-step's pair triangle
  bool writeUnknown = false;    // (ours) <out>.clust1.unk.gz: every droplet against a donor no cluster holds
  bool writeAmbient = false;    // (ours) <out>.clust1.amb.gz: every droplet as one cell plus a share of ambient RNA
  bool fitAmbient = false;      // (ours) <out>.clust1.ambfit.gz: the maximum-likelihood ambient share with its standard error
  double ambFitMax = 0.5;
  bool fitAlpha = false;        // (ours) <out>.clust1.alphafit.gz: the maximum-likelihood mixing share of the best doublet and of the two best singlets (muxgl_fmx_alpha_fit)
  double alphaFitMax = 1.0;
  std::vector<double> ambRho;
  std::string ambAfFile;
  int32_t ambMaxReads = 0;
  bool writeClusterPairs = false;  // (ours) <out>.clust1.ldist.gz: every pair of final clusters as one donor or two
  VcfReader vr;  // (ours) --match-vcf: genotypes of pooled donors the final clusters are scored against
  std::vector<std::string> smIDs;
  std::string smList;
  Args a;
  cf.add(a);
  std::string anchorVcf;  // (ours) --anchor-vcf: genotypes of SOME pooled donors; clusters 0 .. n-1 are held to them
  a.add_string("match-vcf", &vr.path);
  a.add_string("anchor-vcf", &anchorVcf);
  bool anchorRefine = false;      // (ours) --anchor-refine: every anchored donor in PRIOR mode
  std::string anchorRefineList;   // (ours) --anchor-refine-list: the listed sample IDs in PRIOR mode
  a.add_bool("anchor-refine", &anchorRefine);
  a.add_string("anchor-refine-list", &anchorRefineList);
  bool wantMatch = false, wantAnchor = false;
  for (int i = 0; i < argc; ++i) wantMatch = wantMatch || !strcmp(argv[i], "--match-vcf");
  for (int i = 0; i < argc; ++i) wantAnchor = wantAnchor || !strcmp(argv[i], "--anchor-vcf");
  if (wantMatch || wantAnchor) {  // demuxlet's genotype flags, with their meanings; unknown to freemuxlet otherwise, as in the reference
    a.add_string("field", &cf.lo.field);
    a.add_double("geno-error-offset", &cf.lo.genoErrorOffset);
    a.add_double("geno-error-coeff", &cf.lo.genoErrorCoeffR2);
    a.add_string("r2-info", &cf.lo.r2info);
    a.add_int("min-mac", &vr.vfilt.minMAC);
    a.add_double("min-callrate", &vr.vfilt.minCallRate);
    a.add_multi_string("sm", &smIDs);
    a.add_string("sm-list", &smList);
  }
  a.add_string("init-cluster", &initClusterFile);
  a.add_int("nsample", &nSamples);
  a.add_bool("aux-files", &auxFiles);
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
  a.add_bool("write-cluster-pairs", &writeClusterPairs);
  a.add_int("verbose", &verbose);
  a.add_double("doublet-prior", &doublet_prior);
  a.add_double("geno-error", &geno_error);
  a.add_double("bf-thres", &bfThres);              // accepted, unused (as in the reference)
  a.add_double("frac-init-clust", &fracInitClust);
  a.add_int("iter-init", &initIteration);          // accepted, unused
  a.add_bool("keep-init-missing", &keepInitMissing);  // accepted, unused
  a.add_bool("randomize-singlet-score", &randomizeSingletScore);
  a.add_int("seed", &randomSeed);
  a.add_int("max-iter", &maxIter);                 // extension: the reference hard-codes 10 (:372)
  a.add_bool("no-early-stop", &noEarlyStop);       // extension for benchmarking fixed iteration counts
  a.parse(argc, argv);
  if (cf.plpPrefix.empty() || cf.outPrefix.empty() || nSamples == 0) fatal("Missing required option(s) : --plp, --out, --nsample");
  if (nSamples < 0 || nSamples > MUXGL_MAX_CLUSTERS)
    fatal("freemuxlet: --nsample %d outside [1, %d], the clusters the library supports (MUXGL_MAX_CLUSTERS)", nSamples,
          MUXGL_MAX_CLUSTERS);
  if (ambRho.empty()) ambRho = {0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5};
  if ((int)ambRho.size() > MUXGL_MAX_ALPHA) fatal("at most %d --ambient-rho values are supported", MUXGL_MAX_ALPHA);
  if (ambMaxReads < 0) fatal("--ambient-max-reads must not be negative");
  if (!(std::isfinite(ambFitMax) && ambFitMax > 0.0 && ambFitMax <= 1.0)) fatal("--ambient-fit-max must lie in (0, 1]");
  if (!(std::isfinite(alphaFitMax) && alphaFitMax > 0.0 && alphaFitMax <= 1.0)) fatal("--alpha-fit-max must lie in (0, 1]");
  if (wantMatch && wantAnchor)
    fatal("freemuxlet: --match-vcf cannot be combined with --anchor-vcf: an anchored run's match tables (.clust1.match.gz, "
          ".clust1.match.best.gz) are written against the anchor panel");
  if (wantMatch && vr.path.empty()) fatal("freemuxlet: --match-vcf needs a file name");
  if (wantAnchor && anchorVcf.empty()) fatal("freemuxlet: --anchor-vcf needs a file name");
  const bool wantRefine = anchorRefine || !anchorRefineList.empty();
  if (wantRefine && !wantAnchor) fatal("freemuxlet: --anchor-refine and --anchor-refine-list need --anchor-vcf");
  if (wantAnchor && cf.grouped() && initClusterFile.empty())
    fatal("freemuxlet: --anchor-vcf with --devices naming more than one device needs --init-cluster: the default start of an "
          "anchored run matches the greedy clusters to the donors (muxgl_fmx_match_donors), which is not available on a "
          "device group");
  if (wantAnchor) vr.path = anchorVcf;
  if (wantMatch && cf.grouped())
    fatal("freemuxlet: --match-vcf is not available with --devices naming more than one device: a group's cluster pileups "
          "are cut by SNP range (muxgl_fmx_match_donors scores the whole pileup on one device); run it on one device");
  if (writeClusterPairs && cf.grouped())
    fatal("freemuxlet: --write-cluster-pairs is not available with --devices naming more than one device: "
          "muxgl_fmx_cluster_pairs: not available on a device group (use a one-device handle)");

  Pileup p;
  StageTimer tmr;
  if (wantMatch || wantAnchor) {  // the demuxlet loader: its merge-join with the markers and its GP construction (the pileup is the same)
    vr.wanted = smIDs;
    if (!smList.empty()) {
      TsvReader t(smList);
      while (t.read_line() > 0) vr.wanted.push_back(t.str_field_at(0));
    }
    vr.init();
    load_from_plp(cf.plpPrefix, cf.lo, &vr, p);
  } else {
    load_from_plp(cf.plpPrefix, cf.lo, nullptr, p);
  }
  tmr.lap("freemuxlet: load");
  const int64_t C = p.C(), S = p.S();
  const int K = nSamples;
  const int nAnchor = wantAnchor ? p.nv : 0;  // donors are anchored in the VCF's sample order: cluster i is sample i
  if (wantAnchor && (nAnchor < 1 || nAnchor > K))
    fatal("freemuxlet: --anchor-vcf holds %d donors; --nsample %d is the total number of clusters and must be at least that",
          nAnchor, K);
  std::vector<uint8_t> anchorMode((size_t)nAnchor, anchorRefine ? MUXGL_ANCHOR_PRIOR : MUXGL_ANCHOR_HELD);
  if (!anchorRefineList.empty()) {  // (with --anchor-refine next to it all donors are PRIOR; the list is still checked)
    std::ifstream lf(anchorRefineList);
    if (!lf) fatal("freemuxlet: cannot open --anchor-refine-list %s", anchorRefineList.c_str());
    std::stringstream text;
    text << lf.rdbuf();
    std::vector<std::string> ids;
    for (int i = 0; i < nAnchor; ++i) ids.push_back(sid(p, i));
    std::vector<uint8_t> listed;
    std::string unknown;
    if (!anchor_plan::refine_modes(ids, text.str(), &listed, &unknown))
      fatal("freemuxlet: --anchor-refine-list: '%s' is not a sample of the anchor VCF", unknown.c_str());
    if (!anchorRefine) anchorMode = listed;
  }

  std::map<std::string, int32_t> initCluster;  // :90-104
  if (!initClusterFile.empty()) {
    TsvReader t(initClusterFile);
    while (t.read_line() > 0) {
      if (t.nfields != 2) fatal("ERROR: Initial clustering file %s has to have 2 columnes", initClusterFile.c_str());
      const int32_t ic = t.int_field_at(1);
      if (ic >= 0) {
        if (ic >= K)
          fatal("ERROR: --nsample %d parameter was set. The cluster ID must be between 0 to %d, or use negative values "
                "to not assign initial cluster (not implemented yet)", K, K - 1);
        initCluster[t.str_field_at(0)] = ic;
      }
    }
  }

  muxgl_config cfg = cf.config(0);
  muxgl_handle* h = nullptr;
  std::vector<double> af((size_t)S), llk0((size_t)C), llk2((size_t)C);
  std::vector<int32_t> nSNPs((size_t)C), nReads((size_t)C);
  for (int64_t s = 0; s < S; ++s) af[(size_t)s] = p.snps[(size_t)s].af;
  // A device group with a greedy start: the greedy procedure is sequential over all cells, each step scoring one cell
  // against the cluster pileups of all earlier ones, so it runs on ONE device holding the whole pileup (the group's
  // first) -- BEFORE the group exists, so that this device never holds the whole pileup next to its slabs.  The scores
  // it starts from (muxgl_fmx_prepare) are the same numbers on either kind of handle.
  const bool greedy_first = cf.grouped() && initClusterFile.empty();
  muxgl_handle* g = nullptr;
  if (greedy_first) {
    muxgl_config one = MUXGL_CONFIG_INIT;
    one.device_id = cfg.device_ids[0];
    if (muxgl_create(&one, &g) != 0) fatal("%s", muxgl_last_error(nullptr));
    upload(g, p);
    tmr.lap("freemuxlet: device init+hand-over (one device, for the greedy start)");
    check(g, muxgl_fmx_prepare(g, af.data(), llk0.data(), llk2.data(), nSNPs.data(), nReads.data()), "muxgl_fmx_prepare");
  } else {
    if (muxgl_create(&cfg, &h) != 0) fatal("%s", muxgl_last_error(nullptr));
    upload(h, p);
    tmr.lap("freemuxlet: device init+hand-over");
    check(h, muxgl_fmx_prepare(h, af.data(), llk0.data(), llk2.data(), nSNPs.data(), nReads.data()), "muxgl_fmx_prepare");
  }
  tmr.lap("freemuxlet: muxgl_fmx_prepare");

  std::vector<double> scores((size_t)C);
  {  // .lmix, :111-163
    OutFile wmix(cf.outPrefix + ".lmix", false);
    wmix.printf("INT_ID\tBARCODE\tNSNPs\tNREADs\tDBL.LLK\tSNG.LLK\tBF.SINGLET\tBF.SINGLET.PER.SNP\n");
    for (int64_t i = 0; i < C; ++i) {
      scores[(size_t)i] = llk2[(size_t)i] - llk0[(size_t)i];
      wmix.printf("%d\t%s\t%d\t%d\t%.2lf\t%.2lf\t%.2lf\t%.4lf\n", (int)i, p.bcs[(size_t)i].c_str(), nSNPs[(size_t)i],
                  nReads[(size_t)i], llk0[(size_t)i], llk2[(size_t)i], llk2[(size_t)i] - llk0[(size_t)i],
                  (llk2[(size_t)i] - llk0[(size_t)i]) / nSNPs[(size_t)i]);
    }
  }
  RefRand rng(randomSeed == 0 ? (unsigned)std::time(0) : (unsigned)randomSeed);  // srand(), :165-168
  if (randomizeSingletScore) {  // :171-181
    for (int64_t i = 0; i < C - 1; ++i) {
      const int64_t j = i + rng.next() % (C - i);
      if (i < j) std::swap(scores[(size_t)i], scores[(size_t)j]);
    }
  }

  std::vector<int32_t> clusts((size_t)C, -1);
  if (!initClusterFile.empty()) {  // :198-216
    int32_t nmiss = 0;
    for (int64_t i = 0; i < C; ++i) {
      auto it = initCluster.find(p.bcs[(size_t)i]);
      if (it == initCluster.end()) ++nmiss;
      else clusts[(size_t)i] = it->second;
    }
    if (nmiss > 0) notice("WARNING: %d of %d droplets do not have initial cluster assignment", nmiss, (int)C);
  } else if (!greedy_first) {  // greedy clustering, :217-261
    check(h, muxgl_fmx_greedy_init(h, K, scores.data(), fracInitClust, singletScoreThres, clusts.data()),
          "muxgl_fmx_greedy_init");
  } else {  // on the one-device handle; then the group is made and takes over
    check(g, muxgl_fmx_greedy_init(g, K, scores.data(), fracInitClust, singletScoreThres, clusts.data()),
          "muxgl_fmx_greedy_init");
    muxgl_destroy(g);
    g = nullptr;
    if (muxgl_create(&cfg, &h) != 0) fatal("%s", muxgl_last_error(nullptr));
    upload(h, p);
    check(h, muxgl_fmx_prepare(h, af.data(), nullptr, nullptr, nullptr, nullptr), "muxgl_fmx_prepare");
    tmr.lap("freemuxlet: device group init+hand-over");
  }
  // Where an anchored run starts (csrc/anchor_plan.hpp): the greedy clusters matched to the donors, one to one while the
  // Bayes factor favours the donor, take the donors' ids; the others fill the free ids, the largest first
  std::vector<int32_t> anchorStart((size_t)nAnchor, -1);
  std::vector<double> anchorStartLlr((size_t)nAnchor, NAN);
  if (wantAnchor && initClusterFile.empty()) {
    const size_t V = (size_t)p.nv, Kz = (size_t)K;
    check(h, muxgl_fmx_set_clusters(h, K, clusts.data()), "muxgl_fmx_set_clusters");
    check(h, muxgl_demux_set_gp(h, p.nv, p.gp.data(), p.has_gp.data()), "muxgl_demux_set_gp");
    std::vector<double> mll(Kz * V), mll0(Kz);
    std::vector<int32_t> mns(Kz), donor((size_t)nAnchor);
    check(h, muxgl_fmx_match_donors(h, mll.data(), mll0.data(), mns.data(), nullptr), "muxgl_fmx_match_donors");
    for (size_t k = 0; k < Kz; ++k)
      for (size_t v = 0; v < V; ++v) mll[k * V + v] -= mll0[k];
    std::vector<int64_t> ncells(Kz, 0);
    for (int64_t i = 0; i < C; ++i)
      if (clusts[(size_t)i] >= 0) ++ncells[(size_t)clusts[(size_t)i]];
    for (int i = 0; i < nAnchor; ++i) donor[(size_t)i] = i;
    const anchor_plan::start st = anchor_plan::plan(K, p.nv, mll.data(), mns.data(), ncells.data(), nAnchor, donor.data());
    for (int64_t i = 0; i < C; ++i)
      if (clusts[(size_t)i] >= 0) clusts[(size_t)i] = st.new_id[(size_t)clusts[(size_t)i]];
    anchorStart = st.match;
    anchorStartLlr = st.match_llr;
    int matched = 0;
    for (int i = 0; i < nAnchor; ++i) matched += st.match[(size_t)i] >= 0;
    notice("Anchored start: %d of %d donors matched to a greedy cluster", matched, nAnchor);
  }
  tmr.lap("freemuxlet: .lmix + initial clusters");
  notice("Finished assigning initial identity of the cluster..");
  if (auxFiles) {  // :265-274
    OutFile wc0(cf.outPrefix + ".clust0.samples.gz", true);
    wc0.printf("INT_ID\tBARCODE\tCLUST0\n");
    for (int64_t i = 0; i < C; ++i) wc0.printf("%d\t%s\t%d\n", (int)i, p.bcs[(size_t)i].c_str(), clusts[(size_t)i]);
  }
  std::vector<uint8_t> snps_observed((size_t)S, 0);  // :279-288
  mark_observed_snps(p, snps_observed);
  check(h, muxgl_fmx_set_clusters(h, K, clusts.data()), "muxgl_fmx_set_clusters");
  if (wantAnchor) {  // clusters 0 .. nAnchor-1 read the donors' genotypes from here on; the others are learned
    std::vector<int32_t> donor((size_t)nAnchor);
    for (int i = 0; i < nAnchor; ++i) donor[(size_t)i] = i;
    if (!initClusterFile.empty())  // (the default start has handed the panel over already)
      check(h, muxgl_demux_set_gp(h, p.nv, p.gp.data(), p.has_gp.data()), "muxgl_demux_set_gp");
    if (wantRefine) check(h, muxgl_fmx_set_anchors_mode(h, nAnchor, donor.data(), anchorMode.data()), "muxgl_fmx_set_anchors_mode");
    else check(h, muxgl_fmx_set_anchors(h, nAnchor, donor.data()), "muxgl_fmx_set_anchors");
  }
  time_t now = std::time(nullptr);
  tm* ltm = localtime(&now);
  BigVec<double> cgls((size_t)K * S * 9);  // (not zero-filled: 2.3 GB at configs[4]; muxgl_fmx_get_cluster_pileup writes all of it)
  BigVec<int32_t> ccnt((size_t)K * S * 3);
  if (auxFiles) {
    check(h, muxgl_fmx_get_cluster_pileup(h, cgls.data(), ccnt.data()), "muxgl_fmx_get_cluster_pileup");
    write_cluster_vcf(cf.outPrefix + ".clust0.vcf.gz", p, K, cgls.data(), ccnt.data(), snps_observed, ltm);
  }

  std::vector<muxgl_fmx_cell> cells((size_t)C);
  muxgl_fmx_params fp{doublet_prior, geno_error};
  tmr.lap("freemuxlet: set_clusters");
  for (int32_t iter = 0; iter < maxIter; ++iter) {  // :373-605
    notice("Inferring doublets and refining clusters.., iter = %d", iter + 1);
    int32_t nsingle = 0, namb = 0, nchanged = 0;
    check(h, muxgl_fmx_iterate(h, &fp, cells.data(), &nsingle, &namb, &nchanged, nullptr), "muxgl_fmx_iterate");
    notice("Refining per-cluster genotype likelihoods.... %d singlets, %d doublets, %d ambiguous, and %d changed", nsingle,
           (int)C - nsingle - namb, namb, nchanged);
    if (nchanged == 0 && !noEarlyStop) {
      notice("No more changes in cluster assginment and singlet identities. Finishing iterations early");
      break;
    }
  }
  tmr.lap("freemuxlet: EM iterations");
  check(h, muxgl_fmx_get_cluster_pileup(h, cgls.data(), ccnt.data()), "muxgl_fmx_get_cluster_pileup");
  write_cluster_vcf(cf.outPrefix + ".clust1.vcf.gz", p, K, cgls.data(), ccnt.data(), snps_observed, ltm);
  tmr.lap("freemuxlet: write .clust1.vcf.gz");

  OutFile wc1(cf.outPrefix + ".clust1.samples.gz", true);  // :660-665
  wc1.printf("INT_ID\tBARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.GUESS\tBEST.LLK\tNEXT.GUESS\tNEXT.LLK\t"
             "DIFF.LLK.BEST.NEXT\tBEST.POSTERIOR\tSNG.POSTERIOR\tSNG.BEST.GUESS\tSNG.BEST.LLK\tSNG.NEXT.GUESS\t"
             "SNG.NEXT.LLK\tSNG.ONLY.POSTERIOR\tDBL.BEST.GUESS\tDBL.BEST.LLK\tDIFF.LLK.SNG.DBL\n");
  write_rows_parallel(wc1, C, [&](int64_t i, std::string& o) {  // rows formatted by the worker pool, written in order
    const muxgl_fmx_cell& c = cells[(size_t)i];
    char buf[1024];
    const int n = snprintf(buf, sizeof(buf),
               "%d\t%s\t%d\t%d\t%s\t%d,%d\t%.2lf\t%d,%d\t%.2lf\t%.2lf\t%.5lf\t%.2lg\t%d\t%.2lf\t%d\t%.2lf\t%.5lf\t%d,%d\t"
               "%.2lf\t%.2lf\n",
               (int)i, p.bcs[(size_t)i].c_str(), nSNPs[(size_t)i], nReads[(size_t)i],
               (c.type == 2) ? "AMB" : ((c.type == 0) ? "SNG" : "DBL"), c.jBest, c.kBest, c.bestLLK, c.jNext, c.kNext,
               c.nextLLK, c.bestLLK - c.nextLLK, c.bestPP, c.sngPP, c.sBest, c.sngBestLLK, c.sNext, c.sngNextLLK,
               c.sngOnlyPP, c.dBest1, c.dBest2, c.dblBestLLK, c.sngBestLLK - c.dblBestLLK);
    if (n < (int)sizeof(buf)) {
      o.append(buf, (size_t)n);
    } else {  // (a barcode of a kilobyte)
      std::vector<char> big((size_t)n + 1);
      snprintf(big.data(), big.size(),
               "%d\t%s\t%d\t%d\t%s\t%d,%d\t%.2lf\t%d,%d\t%.2lf\t%.2lf\t%.5lf\t%.2lg\t%d\t%.2lf\t%d\t%.2lf\t%.5lf\t%d,%d\t"
               "%.2lf\t%.2lf\n",
               (int)i, p.bcs[(size_t)i].c_str(), nSNPs[(size_t)i], nReads[(size_t)i],
               (c.type == 2) ? "AMB" : ((c.type == 0) ? "SNG" : "DBL"), c.jBest, c.kBest, c.bestLLK, c.jNext, c.kNext,
               c.nextLLK, c.bestLLK - c.nextLLK, c.bestPP, c.sngPP, c.sBest, c.sngBestLLK, c.sNext, c.sngNextLLK,
               c.sngOnlyPP, c.dBest1, c.dBest2, c.dblBestLLK, c.sngBestLLK - c.dblBestLLK);
      o.append(big.data(), (size_t)n);
    }
  });
  wc1.close();
  tmr.lap("freemuxlet: write .clust1.samples.gz");
  if (writeSinglets) {
    // .clust1.sing2.gz: one row per droplet (the order of .clust1.samples.gz) and cluster 0 .. K-1, from the posteriors
    // of the last E-step (the M-step behind it left them alone).  POSTPRB: equal priors over the clusters, a softmax over
    // the droplet's row with its maximum subtracted
    const size_t Kz = (size_t)K;
    BigVec<double> sng((size_t)C * Kz);
    check(h, muxgl_fmx_singlets(h, sng.data()), "muxgl_fmx_singlets");
    tmr.lap("freemuxlet: muxgl_fmx_singlets");
    std::vector<double> rmax((size_t)C), rsum((size_t)C);
    parallel_for(C, plp_threads(), [&](int64_t i) {
      const double* row = sng.data() + (size_t)i * Kz;
      double mx = row[0], sum = 0.0;
      for (size_t j = 1; j < Kz; ++j) mx = std::max(mx, row[j]);
      for (size_t j = 0; j < Kz; ++j) sum += exp(row[j] - mx);
      rmax[(size_t)i] = mx;
      rsum[(size_t)i] = sum;
    });
    OutFile ws(cf.outPrefix + ".clust1.sing2.gz", true);
    ws.printf("BARCODE\tCLUST\tNUM.SNPS\tNUM.READS\tLLK1\tPOSTPRB\n");
    write_rows_parallel(ws, C * (int64_t)K, [&](int64_t r, std::string& o) {
      const int64_t i = r / K;
      const int j = (int)(r - i * K);
      const double v = sng.data()[(size_t)r];
      const std::string& bc = p.bcs[(size_t)i];
      char num[160];
      const int n = snprintf(num, sizeof(num), "\t%d\t%d\t%d\t%.4lf\t%.3lg\n", j, nSNPs[(size_t)i], nReads[(size_t)i], v,
                             exp(v - rmax[(size_t)i]) / rsum[(size_t)i]);
      o.append(bc);
      o.append(num, (size_t)std::min<int>(n, (int)sizeof(num) - 1));
    });
    ws.close();
    tmr.lap("freemuxlet: write .clust1.sing2.gz");
  }
  if (writeInclusion) {
    // .clust1.incl.gz: one row per droplet (the order of .clust1.samples.gz) and cluster 0 .. K-1, from the posteriors of
    // the last E-step, like .clust1.sing2.gz
    const size_t n = (size_t)C * (size_t)K;
    BigVec<double> incl(n), dbl(n);
    BigVec<int32_t> partner(n);
    std::vector<double> tot((size_t)C);
    check(h, muxgl_fmx_inclusion(h, &fp, incl.data(), tot.data(), dbl.data(), partner.data()), "muxgl_fmx_inclusion");
    tmr.lap("freemuxlet: muxgl_fmx_inclusion");
    OutFile wi(cf.outPrefix + ".clust1.incl.gz", true);
    wi.printf("BARCODE\tCLUST\tNUM.SNPS\tNUM.READS\tLLK.INCL\tPOSTPRB.INCL\tDBL.PARTNER\tDBL.LLK\n");
    write_rows_parallel(wi, C * (int64_t)K, [&](int64_t r, std::string& o) {
      const int64_t i = r / K;
      const int j = (int)(r - i * K);
      const double v = incl.data()[(size_t)r];
      char num[240];
      int m = snprintf(num, sizeof(num), "\t%d\t%d\t%d\t%.4lf\t%.3lg\t", j, nSNPs[(size_t)i], nReads[(size_t)i], v,
                       exp(v - tot[(size_t)i]));
      m = std::min<int>(m, (int)sizeof(num) - 1);
      if (partner.data()[(size_t)r] < 0)
        m += snprintf(num + m, sizeof(num) - (size_t)m, "NA\tNA\n");
      else
        m += snprintf(num + m, sizeof(num) - (size_t)m, "%d\t%.4lf\n", (int)partner.data()[(size_t)r], dbl.data()[(size_t)r]);
      o.append(p.bcs[(size_t)i]);
      o.append(num, (size_t)std::min<int>(m, (int)sizeof(num) - 1));
    });
    wi.close();
    tmr.lap("freemuxlet: write .clust1.incl.gz");
  }
  if (writeUnknown) {
    // .clust1.unk.gz: one row per droplet (the order of .clust1.samples.gz), from the posteriors of the last E-step, like
    // .clust1.sing2.gz.  The cluster that pairs best with the unknown donor: the largest ll_ju, ties to the lowest cluster
    const size_t Kz = (size_t)K;
    BigVec<double> ju((size_t)C * Kz);
    std::vector<double> lu((size_t)C), uu((size_t)C);
    check(h, muxgl_fmx_unknown(h, nullptr, ju.data(), lu.data(), uu.data(), nullptr), "muxgl_fmx_unknown");
    tmr.lap("freemuxlet: muxgl_fmx_unknown");
    std::vector<int32_t> hclust((size_t)C);
    std::vector<double> hllk((size_t)C), diff((size_t)C);
    parallel_for(C, plp_threads(), [&](int64_t i) {
      const double* row = ju.data() + (size_t)i * Kz;
      auto val = [](double v) { return std::isnan(v) ? -INFINITY : v; };
      size_t b = 0;
      for (size_t j = 1; j < Kz; ++j)
        if (val(row[j]) > val(row[b])) b = j;
      hclust[(size_t)i] = (int32_t)b;
      hllk[(size_t)i] = val(row[b]);
      const double top = std::max(std::max(val(lu[(size_t)i]), val(uu[(size_t)i])), val(row[b]));
      const double d = cells[(size_t)i].bestLLK - top;
      diff[(size_t)i] = std::isnan(d) ? 0.0 : d;  // (-inf against -inf: neither explains the droplet)
    });
    int64_t nbetter = 0;
    for (int64_t i = 0; i < C; ++i) nbetter += diff[(size_t)i] < -2.0;
    OutFile wu(cf.outPrefix + ".clust1.unk.gz", true);
    wu.printf("BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.LLK\tHALF.CLUST\tHALF.LLK\tDIFF.LLK.CLUST.UNK\n");
    write_rows_parallel(wu, C, [&](int64_t i, std::string& o) {
      char num[320];
      const int n = snprintf(num, sizeof(num), "\t%d\t%d\t%.4lf\t%.4lf\t%.4lf\t%d\t%.4lf\t%.4lf\n", nSNPs[(size_t)i],
                             nReads[(size_t)i], cells[(size_t)i].bestLLK, lu[(size_t)i], uu[(size_t)i], (int)hclust[(size_t)i],
                             hllk[(size_t)i], diff[(size_t)i]);
      o.append(p.bcs[(size_t)i]);
      o.append(num, (size_t)std::min<int>(n, (int)sizeof(num) - 1));
    });
    wu.close();
    notice("%lld of %lld droplets are explained better by more than 2 by a donor that no cluster holds (DIFF.LLK.CLUST.UNK < "
           "-2 in .clust1.unk.gz): a larger --nsample may be meant",
           (long long)nbetter, (long long)C);
    tmr.lap("freemuxlet: write .clust1.unk.gz");
  }
  // The ambient profile of --write-ambient and --fit-ambient: the caller's file, or the pileup's own reads with one
  // pseudo-read at the population frequency; made once
  std::vector<double> ambProfile;
  auto ambient_profile = [&]() -> const std::vector<double>& {
    std::vector<double>& f = ambProfile;
    if (!f.empty() || S == 0) return f;
    f.resize((size_t)S);
    if (!ambAfFile.empty()) {
      TsvReader t(ambAfFile);
      size_t n = 0;
      for (; t.read_line() > 0; ++n)
        if (n < (size_t)S) f[n] = t.double_field_at(0);
      if (n != (size_t)S) fatal("--ambient-af: %s holds %zu lines, the pileup has %zu markers", ambAfFile.c_str(), n, (size_t)S);
    } else {
      std::vector<uint8_t> mask;
      if (ambMaxReads > 0) {
        mask.resize((size_t)C);
        int64_t kept = 0;
        for (int64_t i = 0; i < C; ++i) kept += mask[(size_t)i] = nReads[(size_t)i] <= ambMaxReads;
        notice("Ambient profile from the %lld of %lld droplets with at most %d reads", (long long)kept, (long long)C, ambMaxReads);
      }
      std::vector<int64_t> n_ref((size_t)S), n_alt((size_t)S);
      check(h, muxgl_pileup_allele_counts(h, mask.empty() ? nullptr : mask.data(), n_ref.data(), n_alt.data()),
            "muxgl_pileup_allele_counts");
      for (size_t s = 0; s < (size_t)S; ++s) f[s] = ((double)n_alt[s] + af[s]) / ((double)n_ref[s] + (double)n_alt[s] + 1.0);
      tmr.lap("freemuxlet: muxgl_pileup_allele_counts");
    }
    return f;
  };
  if (writeAmbient) {
    // .clust1.amb.gz: one row per droplet (the order of .clust1.samples.gz), from the posteriors of the last E-step, like
    // .clust1.sing2.gz
    const size_t Kz = (size_t)K, NR = ambRho.size();
    const std::vector<double>& f = ambient_profile();
    BigVec<double> amb((size_t)C * Kz * NR);
    check(h, muxgl_fmx_ambient(h, f.data(), (int32_t)NR, ambRho.data(), amb.data(), nullptr), "muxgl_fmx_ambient");
    tmr.lap("freemuxlet: muxgl_fmx_ambient");
    std::vector<size_t> best((size_t)C);
    parallel_for(C, plp_threads(), [&](int64_t i) {
      const double* row = amb.data() + (size_t)i * Kz * NR;
      auto val = [](double v) { return std::isnan(v) ? -INFINITY : v; };
      size_t at = 0;  // the best (cluster, rho): by value, then (cluster, rho index) ascending
      for (size_t x = 1; x < Kz * NR; ++x)
        if (val(row[x]) > val(row[at])) at = x;
      best[(size_t)i] = at;
    });
    int64_t rescued = 0;
    for (int64_t i = 0; i < C; ++i) {
      const double v = amb.data()[(size_t)i * Kz * NR + best[(size_t)i]];
      rescued += cells[(size_t)i].type == 1 && v > cells[(size_t)i].dblBestLLK + 2.0;
    }
    OutFile wa(cf.outPrefix + ".clust1.amb.gz", true);
    wa.printf("BARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.LLK\tSNG.BEST.GUESS\tSNG.BEST.LLK\tAMB.GUESS\tAMB.RHO\tAMB.LLK\t"
              "DIFF.LLK.AMB.BEST\n");
    write_rows_parallel(wa, C, [&](int64_t i, std::string& o) {
      const muxgl_fmx_cell& c = cells[(size_t)i];
      const size_t at = best[(size_t)i];
      const double v = amb.data()[(size_t)i * Kz * NR + at];
      char num[320];
      const int n = snprintf(num, sizeof(num), "\t%d\t%d\t%s\t%.4lf\t%d\t%.4lf\t%d\t%.2lf\t%.4lf\t%.4lf\n", nSNPs[(size_t)i],
                             nReads[(size_t)i], (c.type == 2) ? "AMB" : ((c.type == 0) ? "SNG" : "DBL"), c.bestLLK, c.sBest,
                             c.sngBestLLK, (int)(at / NR), ambRho[at % NR], v, v - c.bestLLK);
      o.append(p.bcs[(size_t)i]);
      o.append(num, (size_t)std::min<int>(n, (int)sizeof(num) - 1));
    });
    wa.close();
    notice("Ambient RNA: %lld droplets called DBL are explained better, by more than 2 in log-likelihood, as one cell plus "
           "ambient RNA than as their best doublet", (long long)rescued);
    tmr.lap("freemuxlet: write .clust1.amb.gz");
  }
  if (fitAmbient) {
    // .clust1.ambfit.gz: per droplet (the order of .clust1.samples.gz) one row for SNG.BEST.GUESS and one for SNG.NEXT.GUESS
    // (none where the record has no such cluster), from the posteriors of the last E-step
    const std::vector<double>& f = ambient_profile();
    const size_t n = (size_t)C * 2;
    std::vector<int32_t> cand(n), status(n);
    for (int64_t i = 0; i < C; ++i) {
      const muxgl_fmx_cell& c = cells[(size_t)i];
      fit_cands(&cand[(size_t)i * 2], true, c.sBest, c.sNext, K);
    }
    std::vector<double> rho(n), llh(n), ll0(n), info(n);
    check(h, muxgl_fmx_ambient_fit(h, f.data(), 2, cand.data(), ambFitMax, rho.data(), llh.data(), ll0.data(), info.data(),
                                   status.data(), nullptr, nullptr),
          "muxgl_fmx_ambient_fit");
    tmr.lap("freemuxlet: muxgl_fmx_ambient_fit");
    OutFile wf(cf.outPrefix + ".clust1.ambfit.gz", true);
    wf.printf("BARCODE\tNUM.SNPS\tNUM.READS\tCLUST\tSNG.LLK\tAMB.RHO.MLE\tAMB.RHO.SE\tAMB.LLK.MLE\tAMB.LRT\tSTATUS\n");
    write_rows_parallel(wf, C, [&](int64_t i, std::string& o) {
      for (size_t k = 0; k < 2; ++k) {
        const size_t x = (size_t)i * 2 + k;
        if (cand[x] < 0) continue;
        char num[320];
        const int m = snprintf(num, sizeof(num), "\t%d\t%d\t%d\t%.4lf\t%.4lf\t%s\t%.4lf\t%s\t%d\n", nSNPs[(size_t)i],
                               nReads[(size_t)i], cand[x], ll0[x], rho[x], fit_se(status[x], info[x]).s, llh[x],
                               fit_lrt(llh[x], ll0[x]).s, (int)status[x]);
        o.append(p.bcs[(size_t)i]);
        o.append(num, (size_t)std::min<int>(m, (int)sizeof(num) - 1));
      }
    });
    wf.close();
    tmr.lap("freemuxlet: write .clust1.ambfit.gz");
  }
  if (fitAlpha) {
    // .clust1.alphafit.gz: per droplet (the order of .clust1.samples.gz) one row DBL for the two clusters of DBL.BEST.GUESS
    // and one row SNG for (SNG.BEST.GUESS, SNG.NEXT.GUESS) (none where the record has no such cluster), from the posteriors of
    // the last E-step
    const size_t n = (size_t)C * 2;
    std::vector<int32_t> pair(n * 2), status(n);
    for (int64_t i = 0; i < C; ++i) {
      const muxgl_fmx_cell& c = cells[(size_t)i];
      fit_pairs(&pair[(size_t)i * 4], true, c.dBest1, c.dBest2, c.sBest, c.sNext, K);
    }
    std::vector<double> ah(n), llh(n), ll0(n), llt(n), info(n);
    check(h, muxgl_fmx_alpha_fit(h, 2, pair.data(), alphaFitMax, ah.data(), llh.data(), ll0.data(), llt.data(), info.data(),
                                 status.data(), nullptr, nullptr),
          "muxgl_fmx_alpha_fit");
    tmr.lap("freemuxlet: muxgl_fmx_alpha_fit");
    const bool whole = alphaFitMax == 1.0;
    auto one_of = [&](size_t x) { return fit_alone(whole, ll0[x], llt[x]); };
    int64_t mixed = 0;
    for (int64_t i = 0; i < C; ++i) {
      const size_t x = (size_t)i * 2 + 1;
      if (pair[x * 2] < 0) continue;
      mixed += cells[(size_t)i].type == 0 && llh[x] > one_of(x) + 2.0;
    }
    OutFile wf(cf.outPrefix + ".clust1.alphafit.gz", true);
    wf.printf("BARCODE\tNUM.SNPS\tNUM.READS\tPAIR\tCLUST1\tCLUST2\tSNG1.LLK\tSNG2.LLK\tALPHA.MLE\tALPHA.SE\tMIX.LLK.MLE\tMIX.LRT\t"
              "STATUS\n");
    write_rows_parallel(wf, C, [&](int64_t i, std::string& o) {
      for (size_t k = 0; k < 2; ++k) {
        const size_t x = (size_t)i * 2 + k;
        if (pair[x * 2] < 0) continue;
        char num[400];
        const int m = snprintf(num, sizeof(num), "\t%d\t%d\t%s\t%d\t%d\t%.4lf\t%s\t%.4lf\t%s\t%.4lf\t%s\t%d\n", nSNPs[(size_t)i],
                               nReads[(size_t)i], k == 0 ? "DBL" : "SNG", pair[x * 2], pair[x * 2 + 1], ll0[x],
                               FitField(whole, llt[x]).s, ah[x], fit_se(status[x], info[x]).s, llh[x],
                               fit_lrt(llh[x], one_of(x)).s, (int)status[x]);
        o.append(p.bcs[(size_t)i]);
        o.append(num, (size_t)std::min<int>(m, (int)sizeof(num) - 1));
      }
    });
    wf.close();
    notice("Mixing share: %lld droplets called SNG are explained better, by more than 2 in log-likelihood, as a mix of their "
           "best and next singlet cluster at the fitted share than as the better of the two alone", (long long)mixed);
    tmr.lap("freemuxlet: write .clust1.alphafit.gz");
  }
  if (wantAnchor) {
    // .clust1.anchors.gz: one row per cluster -- the donor it is held to, the greedy cluster it started from with the log
    // Bayes factor of that match, and the droplets called singlets of it
    std::vector<int64_t> nsng((size_t)K, 0);
    for (int64_t i = 0; i < C; ++i)
      if (cells[(size_t)i].clust >= 0 && cells[(size_t)i].clust < K) ++nsng[(size_t)cells[(size_t)i].clust];
    OutFile wa(cf.outPrefix + ".clust1.anchors.gz", true);
    wa.printf("CLUST\tSM_ID\tSTART.CLUST\tSTART.LLR\tN.SNG%s\n", wantRefine ? "\tMODE" : "");
    for (int k = 0; k < K; ++k) {
      wa.printf("%d\t%s\t", k, k < nAnchor ? sid(p, k) : "NA");
      if (k < nAnchor && anchorStart[(size_t)k] >= 0) wa.printf("%d\t%.4lf\t", (int)anchorStart[(size_t)k], anchorStartLlr[(size_t)k]);
      else wa.printf("NA\tNA\t");
      wa.printf("%lld", (long long)nsng[(size_t)k]);
      if (wantRefine) wa.printf("\t%s", k >= nAnchor ? "NA" : anchorMode[(size_t)k] == MUXGL_ANCHOR_PRIOR ? "PRIOR" : "HELD");
      wa.printf("\n");
    }
    wa.close();
    tmr.lap("freemuxlet: write .clust1.anchors.gz");
  }
  if (wantRefine) {
    // .clust1.refined.gz: what the droplets made of the PRIOR donors' genotypes (freemuxlet.refine_summary is the same
    // summary in numpy) -- the posterior rows the last E-step read against the panel rows, over the markers with genotypes
    const size_t V = (size_t)p.nv, n = (size_t)nAnchor;
    std::vector<double> rows((size_t)S * n * 3);
    check(h, muxgl_fmx_get_cluster_gp(h, 0, nAnchor, rows.data()), "muxgl_fmx_get_cluster_gp");
    auto argmax3 = [](const double* r) { return r[1] > r[0] ? (r[2] > r[1] ? 2 : 1) : (r[2] > r[0] ? 2 : 0); };  // (the first maximum)
    OutFile wr(cf.outPrefix + ".clust1.refined.gz", true);
    wr.printf("CLUST\tSM_ID\tN.GENO\tN.CHANGED\tMEAN.MAXGP.PRIOR\tMEAN.MAXGP.POST\n");
    for (size_t k = 0; k < n; ++k) {
      if (anchorMode[k] != MUXGL_ANCHOR_PRIOR) continue;
      int64_t ng = 0, nc = 0;
      double sw = 0, sq = 0;
      for (int64_t s = 0; s < S; ++s) {
        if (!p.has_gp[(size_t)s]) continue;
        const double* w = &p.gp[((size_t)s * V + k) * 3];
        const double* q = &rows[((size_t)s * n + k) * 3];
        ++ng;
        nc += argmax3(w) != argmax3(q);
        sw += std::max(w[0], std::max(w[1], w[2]));
        sq += std::max(q[0], std::max(q[1], q[2]));
      }
      if (ng) wr.printf("%d\t%s\t%lld\t%lld\t%.4lf\t%.4lf\n", (int)k, sid(p, (int)k), (long long)ng, (long long)nc, sw / ng, sq / ng);
      else wr.printf("%d\t%s\t0\t0\tNA\tNA\n", (int)k, sid(p, (int)k));
    }
    wr.close();
    tmr.lap("freemuxlet: write .clust1.refined.gz");
  }
  if (wantMatch || (wantAnchor && !cf.grouped())) {
    // .clust1.match.gz / .clust1.match.best.gz: the final cluster pileups (what .clust1.vcf.gz printed) against the donors
    // (an anchored run: against the anchor panel, which the handle holds already -- a check of the droplets assigned to an
    // anchored cluster against the genotypes the cluster was held to)
    const size_t V = (size_t)p.nv, Kz = (size_t)K;
    if (!wantAnchor) check(h, muxgl_demux_set_gp(h, p.nv, p.gp.data(), p.has_gp.data()), "muxgl_demux_set_gp");
    std::vector<double> mll(Kz * V), mll0(Kz);
    std::vector<int32_t> mns(Kz);
    float kms = 0.f;
    check(h, muxgl_fmx_match_donors(h, mll.data(), mll0.data(), mns.data(), &kms), "muxgl_fmx_match_donors");
    tmr.lap("freemuxlet: muxgl_demux_set_gp + muxgl_fmx_match_donors");
    auto llr = [&](size_t k, size_t v) {
      const double d = mll[k * V + v] - mll0[k];
      return std::isnan(d) ? -INFINITY : d;  // (-inf against -inf: no evidence for that donor either)
    };
    // best and next donor of every cluster (ties: lower donor index), best cluster of every donor (ties: lower cluster)
    std::vector<int> best(Kz, -1), next(Kz, -1), bestClust(V, -1);
    for (size_t k = 0; k < Kz; ++k) {
      if (mns[k] == 0) continue;
      for (size_t v = 0; v < V; ++v) {
        if (best[k] < 0 || llr(k, v) > llr(k, (size_t)best[k])) {
          next[k] = best[k];
          best[k] = (int)v;
        } else if (next[k] < 0 || llr(k, v) > llr(k, (size_t)next[k])) {
          next[k] = (int)v;
        }
      }
      for (size_t v = 0; v < V; ++v)
        if (bestClust[v] < 0 || llr(k, v) > llr((size_t)bestClust[v], v)) bestClust[v] = (int)k;
    }
    OutFile wm(cf.outPrefix + ".clust1.match.gz", true);
    wm.printf("CLUST\tSM_ID\tNUM.SNPS\tLLK\tLLK0\tLLR\tPOSTPRB\n");
    for (size_t k = 0; k < Kz; ++k) {
      const double* row = mll.data() + k * V;
      double mx = row[0], sum = 0.0;
      for (size_t v = 1; v < V; ++v) mx = std::max(mx, row[v]);
      if (std::isinf(mx)) mx = 0.0;  // (every donor at -inf)
      for (size_t v = 0; v < V; ++v) sum += exp(row[v] - mx);
      for (size_t v = 0; v < V; ++v)
        wm.printf("%d\t%s\t%d\t%.4lf\t%.4lf\t%.4lf\t%.3lg\n", (int)k, sid(p, (int)v), mns[k], row[v], mll0[k], llr(k, v),
                  sum > 0.0 ? exp(row[v] - mx) / sum : 1.0 / (double)V);
    }
    wm.close();
    OutFile wb(cf.outPrefix + ".clust1.match.best.gz", true);
    wb.printf("CLUST\tNUM.SNPS\tBEST.SM_ID\tBEST.LLR\tNEXT.SM_ID\tNEXT.LLR\tDIFF.LLR\tRECIPROCAL\n");
    for (size_t k = 0; k < Kz; ++k) {
      wb.printf("%d\t%d\t", (int)k, mns[k]);
      if (best[k] < 0) {
        wb.printf("NA\tNA\tNA\tNA\tNA\tNA\n");
        continue;
      }
      wb.printf("%s\t%.4lf\t", sid(p, best[k]), llr(k, (size_t)best[k]));
      if (next[k] < 0) wb.printf("NA\tNA\tNA\t");
      else
        wb.printf("%s\t%.4lf\t%.4lf\t", sid(p, next[k]), llr(k, (size_t)next[k]),
                  llr(k, (size_t)best[k]) - llr(k, (size_t)next[k]));
      wb.printf("%d\n", bestClust[(size_t)best[k]] == (int)k ? 1 : 0);
    }
    wb.close();
    tmr.lap("freemuxlet: write .clust1.match.gz + .clust1.match.best.gz");
  }
  if (writeClusterPairs) {
    // .clust1.ldist.gz: the final cluster pileups against each other, the row of the reference's .ldist.gz
    // (cmd_cram_freemuxlet.cpp:268) without its read-count columns, one row per pair a > b in ascending (a, b) order
    const size_t Kz = (size_t)K, np = Kz * (Kz - 1) / 2;
    std::vector<double> l2(np), l0(np);
    std::vector<int32_t> ns(np);
    float kms = 0.f;
    check(h, muxgl_fmx_cluster_pairs(h, l2.data(), l0.data(), ns.data(), &kms), "muxgl_fmx_cluster_pairs");
    tmr.lap("freemuxlet: muxgl_fmx_cluster_pairs");
    OutFile wp(cf.outPrefix + ".clust1.ldist.gz", true);
    wp.printf("ID1\tID2\tNSNP\tLLK0\tLLK2\tLDIFF\tDIFF.SNP\n");
    for (size_t a = 1, i = 0; a < Kz; ++a)
      for (size_t b = 0; b < a; ++b, ++i)
        wp.printf("%d\t%d\t%d\t%.2lf\t%.2lf\t%.2lf\t%.4lf\n", (int)a, (int)b, ns[i], l0[i], l2[i], l2[i] - l0[i],
                  (l2[i] - l0[i]) / (ns[i] + 1e-6));
    wp.close();
    tmr.lap("freemuxlet: write .clust1.ldist.gz");
  }
  muxgl_destroy(h);
  return 0;
}

// ------------------------------------------------------------------------------------------------ freemuxlet-old
// mirrors cmdCramFreemuxlet (cmd_cram_freemuxlet.cpp), registered as "freemuxlet-old" (cramore.cpp:44).  Differences
// from freemux2 that are reproduced as written:
//   * the read/cell filter flags are parsed and then never handed to the loader (:55-62 vs :83), so the pileup is loaded
//     with sc_dropseq_lib_t's own defaults minBQ = 1, capBQ = 60 and no droplet filters (sc_drop_seq.h:181);
//   * no srand(): rand() runs from the C library's default seed, so the command is deterministic (RefRand(1));
//   * initial clusters from votes over a pairwise distance matrix (:176-343) instead of the greedy pass;
//   * ten EM iterations without early stop; --geno-error only enters the last one (:485,500).
int cmd_freemuxlet_old(int argc, char** argv) {
  CommonFlags cf;
  std::string initClusterFile;
  double doublet_prior = 0.5, geno_error = 0.0, bfThres = 5.41, fracInitClust = 1.0;  // :19-28
  int32_t nSamples = 0, initIteration = 10, verbose = 0, minUniq = 0;
  bool auxFiles = false, keepInitMissing = false;
  Args a;
  cf.add(a);
  cf.lo.capBQ = 40;  // the flag's default (:16); see above: it never reaches the loader
  a.add_int("min-uniq", &minUniq);
  a.add_string("init-cluster", &initClusterFile);
  a.add_int("nsample", &nSamples);
  a.add_bool("aux-files", &auxFiles);
  a.add_int("verbose", &verbose);
  a.add_double("doublet-prior", &doublet_prior);
  a.add_double("geno-error", &geno_error);
  a.add_double("bf-thres", &bfThres);
  a.add_double("frac-init-clust", &fracInitClust);
  a.add_int("iter-init", &initIteration);
  a.add_bool("keep-init-missing", &keepInitMissing);
  a.parse(argc, argv);
  if (cf.plpPrefix.empty() || cf.outPrefix.empty() || nSamples == 0) fatal("Missing required option(s) : --plp, --out, --nsample");
  if (nSamples > 64) fatal("freemuxlet-old: --nsample %d exceeds the 64 clusters the vote kernel supports", nSamples);

  Pileup p;
  StageTimer tmr;
  LoadOptions lo;  // sc_drop_seq.h:181
  lo.minBQ = 1;
  lo.capBQ = 60;
  load_from_plp(cf.plpPrefix, lo, nullptr, p);
  tmr.lap("freemuxlet-old: load");
  const int64_t C = p.C(), S = p.S();
  const int K = nSamples;

  std::map<std::string, int32_t> initCluster;  // :87-99
  if (!initClusterFile.empty()) {
    TsvReader t(initClusterFile);
    while (t.read_line() > 0) {
      if (t.nfields != 2) fatal("ERROR: Initial clustering file %s has to have 2 columnes", initClusterFile.c_str());
      const int32_t ic = t.int_field_at(1);
      if (ic >= 0) {
        if (ic >= K)
          fatal("ERROR: --nsample %d parameter was set. The cluster ID must be between 0 to %d, or use negative values "
                "to not assign initial cluster (not implemented yet)", K, K - 1);
        initCluster[t.str_field_at(0)] = ic;
      }
    }
  }

  if (cf.grouped()) fatal("freemuxlet-old: --devices is not supported (its pairwise matrix and votes run on one device)");
  muxgl_config cfg = cf.config(0);
  muxgl_handle* h = nullptr;
  if (muxgl_create(&cfg, &h) != 0) fatal("%s", muxgl_last_error(nullptr));
  upload(h, p);
  std::vector<double> af((size_t)S), llk0((size_t)C), llk2((size_t)C);
  std::vector<int32_t> nSNPs((size_t)C), nReads((size_t)C);
  for (int64_t s = 0; s < S; ++s) af[(size_t)s] = p.snps[(size_t)s].af;
  check(h, muxgl_fmx_prepare(h, af.data(), llk0.data(), llk2.data(), nSNPs.data(), nReads.data()), "muxgl_fmx_prepare");
  tmr.lap("freemuxlet-old: hand-over + muxgl_fmx_prepare");

  std::vector<double> scores((size_t)C);
  {  // .lmix, :110-165
    OutFile wmix(cf.outPrefix + ".lmix", false);
    wmix.printf("INT_ID\tBARCODE\tNSNPs\tNREADs\tDBL.LLK\tSNG.LLK\tLOG.BF\tBFpSNP\n");
    for (int64_t i = 0; i < C; ++i) {
      scores[(size_t)i] = llk2[(size_t)i] - llk0[(size_t)i];
      wmix.printf("%d\t%s\t%d\t%d\t%.2lf\t%.2lf\t%.2lf\t%.4lf\n", (int)i, p.bcs[(size_t)i].c_str(), nSNPs[(size_t)i],
                  nReads[(size_t)i], llk0[(size_t)i], llk2[(size_t)i], llk0[(size_t)i] - llk2[(size_t)i],
                  (llk0[(size_t)i] - llk2[(size_t)i]) / nSNPs[(size_t)i]);
    }
  }
  std::vector<int32_t> drops_srted((size_t)C);  // :167-173, comparator sc_drop_seq.h:190-198
  for (int64_t i = 0; i < C; ++i) drops_srted[(size_t)i] = (int32_t)i;
  std::sort(drops_srted.begin(), drops_srted.end(), [&](int32_t lhs, int32_t rhs) {
    const double cmp = scores[(size_t)lhs] - scores[(size_t)rhs];
    if (cmp != 0) return cmp > 0;
    return lhs > rhs;
  });

  notice("Calculate pairwise genetic distance matrix..");
  const bool wantDist = auxFiles && initClusterFile.empty();  // .ldist.gz rows are printed by the voting loop only (:262-265)
  std::vector<muxgl_dropd> dropDs(wantDist ? (size_t)(C * (C - 1) / 2) : 0);
  check(h, muxgl_fmxold_pair_dist(h, bfThres, wantDist ? dropDs.data() : nullptr), "muxgl_fmxold_pair_dist");
  tmr.lap("freemuxlet-old: pairwise distance matrix");

  std::vector<int32_t> clusts((size_t)C, -1), ccounts((size_t)K, 0);
  std::vector<double> jitter;
  RefRand rng(1);
  auto draw_jitter = [&](int64_t rows) {  // `votes[j] = rand()/(RAND_MAX+1.)/1000.` per visited cell (:257-259,304-306)
    jitter.resize((size_t)rows * K);
    for (size_t x = 0; x < jitter.size(); ++x) jitter[x] = rng.next() / (RAND_MAX + 1.) / 1000.;
  };
  auto counts_str = [&]() {
    std::string buf;
    for (int j = 0; j < K; ++j) buf += " " + std::to_string(ccounts[(size_t)j]);
    return buf;
  };
  {
    OutFile* wdist = nullptr;
    if (auxFiles) {  // :178-182
      wdist = new OutFile(cf.outPrefix + ".ldist.gz", true);
      wdist->printf("ID1\tID2\tNSNP\tREAD1\tREAD2\tREADMIN\tLLK0\tLLK2\tLDIFF\tDIFF.SNP\n");
    }
    if (!initClusterFile.empty()) {  // :227-243
      int32_t nmiss = 0;
      for (int64_t i = 0; i < C; ++i) {
        auto it = initCluster.find(p.bcs[(size_t)i]);
        if (it == initCluster.end()) ++nmiss;
        else {
          clusts[(size_t)i] = it->second;
          ++ccounts[(size_t)it->second];
        }
      }
      if (nmiss > 0) notice("WARNING: %d of %d droplets do not have initial cluster assignment", nmiss, (int)C);
    } else {  // :245-291
      int64_t nvis = 0;
      for (int64_t i = 0; i < C; ++i)
        if (!((double)i > (double)C * fracInitClust)) ++nvis;
      draw_jitter(nvis);
      check(h, muxgl_fmxold_vote_init(h, K, drops_srted.data(), jitter.data(), fracInitClust, clusts.data(), ccounts.data()),
            "muxgl_fmxold_vote_init");
      if (wdist) {  // :262-265
        for (int64_t i = 0; i < nvis; ++i) {
          const int32_t si = drops_srted[(size_t)i];
          for (int64_t j = 0; j < i; ++j) {
            const int32_t sj = drops_srted[(size_t)j];
            const int64_t hi = si > sj ? si : sj, lo2 = si > sj ? sj : si;
            const muxgl_dropd& dd = dropDs[(size_t)(hi * (hi - 1) / 2 + lo2)];
            wdist->printf("%d\t%d\t%d\t%d\t%d\t%d\t%.2lf\t%.2lf\t%.2lf\t%.4lf\n", si, sj, dd.nsnps, dd.nread1, dd.nread2,
                          dd.nread1 > dd.nread2 ? dd.nread2 : dd.nread1, dd.llk0, dd.llk2, dd.llk2 - dd.llk0,
                          (dd.llk2 - dd.llk0) / (dd.nsnps + 1e-6));
          }
        }
      }
    }
    if (wdist) {
      wdist->close();
      delete wdist;
    }
  }
  notice("Finished calculating pairwise distance between the droplets..");
  tmr.lap("freemuxlet-old: first voting pass");

  if (initIteration > 0) {  // :295-351: ten passes whatever the value
    std::vector<int32_t> orand((size_t)C);
    for (int32_t iter = 0; iter < 10; ++iter) {
      for (int64_t i = 0; i < C; ++i) orand[(size_t)i] = (int32_t)i;
      // std::random_shuffle(orand.begin(), orand.end()) as libstdc++ implements it (bits/stl_algo.h): the reference
      // binary's behaviour; spelled out because the function is gone from C++17
      for (int64_t i = 1; i < C; ++i) {
        const int64_t j = rng.next() % (i + 1);
        if (i != j) std::swap(orand[(size_t)i], orand[(size_t)j]);
      }
      draw_jitter(C);
      int32_t changed = 0;
      check(h, muxgl_fmxold_vote_refine(h, K, orand.data(), jitter.data(), keepInitMissing ? 1 : 0, clusts.data(), &changed,
                                        ccounts.data()),
            "muxgl_fmxold_vote_refine");
      notice("Iteration %d, # changed = %d, cluster counts:%s", iter, changed, counts_str().c_str());
    }
  }
  tmr.lap("freemuxlet-old: refinement passes");

  if (auxFiles) {  // :353-363
    OutFile wc0(cf.outPrefix + ".clust0.samples.gz", true);
    wc0.printf("INT_ID\tBARCODE\tCLUST0\n");
    for (int64_t i = 0; i < C; ++i) wc0.printf("%d\t%s\t%d\n", (int)i, p.bcs[(size_t)i].c_str(), clusts[(size_t)i]);
  }
  std::vector<uint8_t> snps_observed((size_t)S, 0);  // :367-376
  mark_observed_snps(p, snps_observed);
  check(h, muxgl_fmx_set_clusters(h, K, clusts.data()), "muxgl_fmx_set_clusters");
  time_t now = std::time(nullptr);
  tm* ltm = localtime(&now);
  BigVec<double> cgls((size_t)K * S * 9);  // (not zero-filled: 2.3 GB at configs[4]; muxgl_fmx_get_cluster_pileup writes all of it)
  BigVec<int32_t> ccnt((size_t)K * S * 3);
  if (auxFiles) {
    check(h, muxgl_fmx_get_cluster_pileup(h, cgls.data(), ccnt.data()), "muxgl_fmx_get_cluster_pileup");
    write_cluster_vcf(cf.outPrefix + ".clust0.vcf.gz", p, K, cgls.data(), ccnt.data(), snps_observed, ltm, true);
  }

  std::vector<muxgl_fmx_cell> cells((size_t)C);
  const int32_t max_iter = 10;  // :457
  for (int32_t iter = 0; iter < max_iter; ++iter) {
    notice("Inferring doublets and refining clusters.., iter = %d", iter + 1);
    muxgl_fmx_params fp{doublet_prior, (geno_error > 0 && iter + 1 == max_iter) ? geno_error : 0.0};  // :485,500
    int32_t nsingle = 0, namb = 0, nchanged = 0;
    check(h, muxgl_fmx_iterate(h, &fp, cells.data(), &nsingle, &namb, &nchanged, nullptr), "muxgl_fmx_iterate");
    notice("Refining per-cluster genotype likelihoods.... %d singlets, %d doublets, and %d ambiguous", nsingle,
           (int)C - nsingle - namb, namb);
  }
  tmr.lap("freemuxlet-old: EM iterations");
  check(h, muxgl_fmx_get_cluster_pileup(h, cgls.data(), ccnt.data()), "muxgl_fmx_get_cluster_pileup");
  write_cluster_vcf(cf.outPrefix + ".clust1.vcf.gz", p, K, cgls.data(), ccnt.data(), snps_observed, ltm);

  OutFile wc1(cf.outPrefix + ".clust1.samples.gz", true);  // :709-714
  wc1.printf("INT_ID\tBARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.GUESS\tBEST.LLK\tNEXT.GUESS\tNEXT.LLK\t"
             "DIFF.LLK.BEST.NEXT\tBEST.POSTERIOR\tSNG.POSTERIOR\tSNG.BEST.GUESS\tSNG.BEST.LLK\tSNG.NEXT.GUESS\t"
             "SNG.NEXT.LLK\tSNG.ONLY.POSTERIOR\tDBL.BEST.GUESS\tDBL.BEST.LLK\tDIFF.LLK.SNG.DBL\n");
  write_rows_parallel(wc1, C, [&](int64_t i, std::string& o) {  // rows formatted by the worker pool, written in order
    const muxgl_fmx_cell& c = cells[(size_t)i];
    char buf[1024];
    const int n = snprintf(buf, sizeof(buf),
               "%d\t%s\t%d\t%d\t%s\t%d,%d\t%.2lf\t%d,%d\t%.2lf\t%.2lf\t%.5lf\t%.2lg\t%d\t%.2lf\t%d\t%.2lf\t%.5lf\t%d,%d\t"
               "%.2lf\t%.2lf\n",
               (int)i, p.bcs[(size_t)i].c_str(), nSNPs[(size_t)i], nReads[(size_t)i],
               (c.type == 2) ? "AMB" : ((c.type == 0) ? "SNG" : "DBL"), c.jBest, c.kBest, c.bestLLK, c.jNext, c.kNext,
               c.nextLLK, c.bestLLK - c.nextLLK, c.bestPP, c.sngPP, c.sBest, c.sngBestLLK, c.sNext, c.sngNextLLK,
               c.sngOnlyPP, c.dBest1, c.dBest2, c.dblBestLLK, c.sngBestLLK - c.dblBestLLK);
    if (n < (int)sizeof(buf)) {
      o.append(buf, (size_t)n);
    } else {  // (a barcode of a kilobyte)
      std::vector<char> big((size_t)n + 1);
      snprintf(big.data(), big.size(),
               "%d\t%s\t%d\t%d\t%s\t%d,%d\t%.2lf\t%d,%d\t%.2lf\t%.2lf\t%.5lf\t%.2lg\t%d\t%.2lf\t%d\t%.2lf\t%.5lf\t%d,%d\t"
               "%.2lf\t%.2lf\n",
               (int)i, p.bcs[(size_t)i].c_str(), nSNPs[(size_t)i], nReads[(size_t)i],
               (c.type == 2) ? "AMB" : ((c.type == 0) ? "SNG" : "DBL"), c.jBest, c.kBest, c.bestLLK, c.jNext, c.kNext,
               c.nextLLK, c.bestLLK - c.nextLLK, c.bestPP, c.sngPP, c.sBest, c.sngBestLLK, c.sNext, c.sngNextLLK,
               c.sngOnlyPP, c.dBest1, c.dBest2, c.dblBestLLK, c.sngBestLLK - c.dblBestLLK);
      o.append(big.data(), (size_t)n);
    }
  });
  wc1.close();
  tmr.lap("freemuxlet-old: writers");
  muxgl_destroy(h);
  return 0;
}

// ------------------------------------------------------------------------------------------------ dump-plp
// loader-only command for the CPU tests: writes the packed pileup as a flat little-endian file
//   magic "MUXGLPLP", int64 C,S,nnz,R,nv, then cell_ptr, entry_snp, entry_rptr, reads, af[S], has_gp[S], gp[S*nv*3],
//   cell_totl_reads[C], cell_uniq_reads[C], then C barcodes and nv sample ids as NUL-terminated strings
int cmd_dump_plp(int argc, char** argv) {
  CommonFlags cf;
  VcfReader vr;
  std::vector<std::string> smIDs;
  std::string smList;
  Args a;
  cf.add(a);
  a.add_string("vcf", &vr.path);
  a.add_string("field", &cf.lo.field);
  a.add_double("geno-error-offset", &cf.lo.genoErrorOffset);
  a.add_double("geno-error-coeff", &cf.lo.genoErrorCoeffR2);
  a.add_string("r2-info", &cf.lo.r2info);
  a.add_int("min-mac", &vr.vfilt.minMAC);
  a.add_double("min-callrate", &vr.vfilt.minCallRate);
  a.add_multi_string("sm", &smIDs);
  a.add_string("sm-list", &smList);
  a.add_int("rank", &cf.lo.rank);    // one rank's two slabs of a sharded run (LoadOptions): the file then holds the row
  a.add_int("world", &cf.lo.world);  // slab in place of the pileup and the column slab behind it
  a.parse(argc, argv);
  if (cf.plpPrefix.empty() || cf.outPrefix.empty()) fatal("Missing required option(s) : --plp, --out");
  Pileup p;
  if (!vr.path.empty()) {
    vr.wanted = smIDs;
    if (!smList.empty()) {
      TsvReader t(smList);
      while (t.read_line() > 0) vr.wanted.push_back(t.str_field_at(0));
    }
    vr.init();
    load_from_plp(cf.plpPrefix, cf.lo, &vr, p);
  } else {
    load_from_plp(cf.plpPrefix, cf.lo, nullptr, p);
  }
  FILE* f = fopen(cf.outPrefix.c_str(), "wb");
  if (!f) fatal("Cannot open %s for writing", cf.outPrefix.c_str());
  if (p.slabbed) {  // --rank / --world: magic "MUXGLSLB", int64 C, S, c0, c1, s0, s1, nnz_r, R_r, nnz_c, R_c; the row slab's
                    // cell_ptr[c1-c0+1], entry_snp, entry_rptr, reads; the column slab's cell_ptr[C+1], ...; af[S]; the
                    // two read counts [C]
    const int64_t hdr[10] = {p.C(), p.S(), p.slab_c0, p.slab_c1, p.slab_s0, p.slab_s1, p.nnz(), (int64_t)p.reads.size(),
                             (int64_t)p.col_entry_snp.size(), (int64_t)p.col_reads.size()};
    fwrite("MUXGLSLB", 1, 8, f);
    fwrite(hdr, sizeof(int64_t), 10, f);
    fwrite(p.cell_ptr.data(), sizeof(int64_t), p.cell_ptr.size(), f);
    fwrite(p.entry_snp.data(), sizeof(int32_t), p.entry_snp.size(), f);
    fwrite(p.entry_rptr.data(), sizeof(int64_t), p.entry_rptr.size(), f);
    fwrite(p.reads.data(), 1, p.reads.size(), f);
    fwrite(p.col_cell_ptr.data(), sizeof(int64_t), p.col_cell_ptr.size(), f);
    fwrite(p.col_entry_snp.data(), sizeof(int32_t), p.col_entry_snp.size(), f);
    fwrite(p.col_entry_rptr.data(), sizeof(int64_t), p.col_entry_rptr.size(), f);
    fwrite(p.col_reads.data(), 1, p.col_reads.size(), f);
    std::vector<double> af((size_t)p.S());
    for (int64_t s = 0; s < p.S(); ++s) af[(size_t)s] = p.snps[(size_t)s].af;
    fwrite(af.data(), sizeof(double), af.size(), f);
    fwrite(p.cell_totl_reads.data(), sizeof(int32_t), p.cell_totl_reads.size(), f);
    fwrite(p.cell_uniq_reads.data(), sizeof(int32_t), p.cell_uniq_reads.size(), f);
    fclose(f);
    return 0;
  }
  const int64_t hdr[5] = {p.C(), p.S(), p.nnz(), (int64_t)p.reads.size(), p.nv};
  fwrite("MUXGLPLP", 1, 8, f);
  fwrite(hdr, sizeof(int64_t), 5, f);
  fwrite(p.cell_ptr.data(), sizeof(int64_t), p.cell_ptr.size(), f);
  fwrite(p.entry_snp.data(), sizeof(int32_t), p.entry_snp.size(), f);
  fwrite(p.entry_rptr.data(), sizeof(int64_t), p.entry_rptr.size(), f);
  fwrite(p.reads.data(), 1, p.reads.size(), f);
  std::vector<double> af((size_t)p.S());
  for (int64_t s = 0; s < p.S(); ++s) af[(size_t)s] = p.snps[(size_t)s].af;
  fwrite(af.data(), sizeof(double), af.size(), f);
  std::vector<uint8_t> hg = p.has_gp;
  hg.resize((size_t)p.S(), 0);
  fwrite(hg.data(), 1, hg.size(), f);
  fwrite(p.gp.data(), sizeof(double), p.gp.size(), f);
  fwrite(p.cell_totl_reads.data(), sizeof(int32_t), p.cell_totl_reads.size(), f);
  fwrite(p.cell_uniq_reads.data(), sizeof(int32_t), p.cell_uniq_reads.size(), f);
  for (const std::string& s : p.bcs) fwrite(s.c_str(), 1, s.size() + 1, f);
  for (const std::string& s : p.sample_ids) fwrite(s.c_str(), 1, s.size() + 1, f);
  fclose(f);
  return 0;
}

// ------------------------------------------------------------------------------------------------ selftest-fmt
// fmt_g3 / fmt_int against printf on N random values plus the hard ones (exact ties of the third digit and their
// neighbours, powers of ten, both ends of the "%e" / "%f" switch); prints the counts, exit status 1 on any difference
int cmd_selftest_fmt(int argc, char** argv) {
  const long N = argc > 0 ? atol(argv[0]) : 1000000;
  uint64_t st = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() {  // xorshift64*
    st ^= st >> 12, st ^= st << 25, st ^= st >> 27;
    return st * 2685821657736338717ull;
  };
  auto unif = [&]() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); };
  long n = 0, declined = 0, bad = 0;
  char a[64], b[64];
  auto check = [&](double x) {
    ++n;
    const int k = fmt_g3(x, a);
    if (k < 0) {
      ++declined;
      return;
    }
    a[k] = 0;
    snprintf(b, sizeof(b), "%.3lg", x);
    if (strcmp(a, b)) {
      if (bad++ < 20) fprintf(stderr, "fmt_g3 %.17g: %s, printf: %s\n", x, a, b);
    }
  };
  for (long i = 0; i < N; ++i) {
    const double u = unif();
    check(u);
    check(u * pow(10.0, -(double)(rnd() % 20)));
    check(pow(10.0, -100.0 * unif()) * (1 + u));
    const int D = 100 + (int)(rnd() % 900), E = -(int)(rnd() % 12);
    const double t = (D + 0.5) * pow(10.0, E - 2), r = D * pow(10.0, E - 2);
    check(t), check(nextafter(t, 0)), check(nextafter(t, 1e9));
    check(r), check(nextafter(r, 0)), check(nextafter(r, 1e9));
    const int32_t v = (int32_t)rnd();
    const int k = fmt_int(v, a);
    a[k] = 0;
    snprintf(b, sizeof(b), "%d", v);
    if (strcmp(a, b)) ++bad;
  }
  for (double x : {1.0, 0.9995, 0.99949999999999994, 0.9996, 1e-5, 9.995e-5, 9.9949999e-5, 1e-4, 0.0001235, 0.5, 0.125, 1e-100,
                   1e-99, 9.99e-100, 2.5e-7, 999.4, 999.5, 12.35, 100.0, 1e-290, 0.0, -1.0, 1e3, 1e-300})
    check(x);
  for (int32_t v : {0, 1, -1, 9, 10, 255, INT32_MAX, INT32_MIN}) {
    const int k = fmt_int(v, a);
    a[k] = 0;
    snprintf(b, sizeof(b), "%d", v);
    if (strcmp(a, b)) ++bad;
  }
  printf("%ld values, %ld left to printf, %ld differences\n", n, declined, bad);
  return bad != 0;
}

// ------------------------------------------------------------------------------------------------ bgzf
// writer-only command for the CPU tests: copies a file through the BGZF writer of util.hpp (line by line, as the
// commands' printf calls do)
int cmd_bgzf(int argc, char** argv) {
  std::string in, outp;
  Args a;
  a.add_string("in", &in);
  a.add_string("out", &outp);
  a.parse(argc, argv);
  if (in.empty() || outp.empty()) fatal("Missing required option(s) : --in, --out");
  FILE* f = fopen(in.c_str(), "rb");
  if (!f) fatal("Cannot open %s for reading", in.c_str());
  OutFile w(outp, true);
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, 777, f)) > 0) w.write(buf, n);  // odd-sized pieces across block borders
  fclose(f);
  w.close();
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: popscle-amd <demuxlet|freemuxlet|freemuxlet-old|dump-plp> [options]\n"
                    "  demuxlet --write-singlets: also <out>.sing2.gz, the singlet log-likelihood of every printed droplet\n"
                    "    against every sample (BARCODE SM_ID NUM.SNPS NUM.READS LLK1 POSTPRB; the reference's RD.* columns\n"
                    "    give way to the two counts of .best, its LLK0 is left out)\n"
                    "  demuxlet --write-inclusion: also <out>.incl.gz, per printed droplet and sample the evidence that the sample\n"
                    "    is in the droplet and the doublet it pairs best in (BARCODE SM_ID NUM.SNPS NUM.READS LLK.INCL\n"
                    "    POSTPRB.INCL DBL.PARTNER DBL.ALPHA DBL.LLK)\n"
                    "  demuxlet --write-ambient [--ambient-rho x ...] [--ambient-af FILE] [--ambient-max-reads N]: also <out>.amb.gz,\n"
                    "      per printed droplet the best reading as one cell of a sample plus a share rho of ambient RNA\n"
                    "  demuxlet --write-unknown: also <out>.unk.gz, per printed droplet how well a donor missing from the VCF\n"
                    "    explains it (BARCODE NUM.SNPS NUM.READS BEST.LLK UNK.SNG.LLK UNK.DBL.ALPHA UNK.DBL.LLK HALF.GUESS\n"
                    "    HALF.LLK DIFF.LLK.PANEL.UNK)\n"
                    "  freemuxlet --write-singlets: also <out>.clust1.sing2.gz, the singlet log-likelihood of every droplet\n"
                    "    against every cluster in the last iteration (BARCODE CLUST NUM.SNPS NUM.READS LLK1 POSTPRB)\n"
                    "  freemuxlet --match-vcf FILE [demuxlet's genotype flags]: also <out>.clust1.match.gz and .clust1.match.best.gz,\n"
                    "      the final clusters scored against the donors' genotypes in FILE (one device)\n"
                    "  freemuxlet --anchor-vcf FILE [demuxlet's genotype flags]: clusters 0 .. n-1 are held to the n donors of FILE\n"
                    "      (sample order), the others up to --nsample are learned; also <out>.clust1.anchors.gz (CLUST SM_ID\n"
                    "      START.CLUST START.LLR N.SNG) and, on one device, the match tables against FILE; several devices need\n"
                    "      --init-cluster; not together with --match-vcf\n"
                    "  freemuxlet --anchor-vcf FILE --anchor-refine: the donors' genotypes are the prior of the genotypes the\n"
                    "      droplets form, not held (--anchor-refine-list FILE: only the sample IDs listed there); adds a MODE\n"
                    "      column to <out>.clust1.anchors.gz and writes <out>.clust1.refined.gz (CLUST SM_ID N.GENO N.CHANGED\n"
                    "      MEAN.MAXGP.PRIOR MEAN.MAXGP.POST)\n"
                    "  freemuxlet --write-cluster-pairs: also <out>.clust1.ldist.gz, every pair of final clusters as one donor\n"
                    "    against two unrelated donors (ID1 ID2 NSNP LLK0 LLK2 LDIFF DIFF.SNP; one device)\n"
                    "  freemuxlet --write-inclusion: also <out>.clust1.incl.gz, per droplet and cluster the evidence that the\n"
                    "    cluster is in the droplet and the cluster it pairs best with, in the last iteration (BARCODE CLUST\n"
                    "    NUM.SNPS NUM.READS LLK.INCL POSTPRB.INCL DBL.PARTNER DBL.LLK)\n"
                    "  demuxlet --fit-ambient [--ambient-fit-max x] [--ambient-af FILE] [--ambient-max-reads N]: also <out>.ambfit.gz,\n"
                    "      per printed droplet and for its best and next singlet sample the maximum-likelihood ambient share on\n"
                    "      [0, x] (default 0.5) with its standard error and the likelihood ratio against no ambient RNA\n"
                    "  demuxlet --fit-alpha [--alpha-fit-max x]: also <out>.alphafit.gz, per printed droplet the maximum-likelihood\n"
                    "      mixing share on [0, x] (default 1.0) of its best doublet's two samples (row DBL) and of its best and next\n"
                    "      singlet sample (row SNG), with its standard error and the likelihood ratio against the better singlet\n"
                    "  freemuxlet --write-ambient [--ambient-rho x ...] [--ambient-af FILE] [--ambient-max-reads N]: also\n"
                    "    <out>.clust1.amb.gz, per droplet the best reading as one cell of a cluster plus a share rho of ambient RNA\n"
                    "  freemuxlet --fit-ambient [--ambient-fit-max x] [--ambient-af FILE] [--ambient-max-reads N]: also\n"
                    "    <out>.clust1.ambfit.gz, per droplet and for its best and next singlet cluster the maximum-likelihood ambient\n"
                    "    share on [0, x] (default 0.5) with its standard error and the likelihood ratio against no ambient RNA\n"
                    "  freemuxlet --fit-alpha [--alpha-fit-max x]: also <out>.clust1.alphafit.gz, per droplet the maximum-likelihood\n"
                    "    mixing share on [0, x] (default 1.0) of its best doublet's two clusters (row DBL) and of its best and next\n"
                    "    singlet cluster (row SNG), with its standard error and the likelihood ratio against the better singlet\n"
                    "  freemuxlet --write-unknown: also <out>.clust1.unk.gz, per droplet how well a donor that no cluster holds\n"
                    "    explains it in the last iteration (BARCODE NUM.SNPS NUM.READS BEST.LLK UNK.SNG.LLK UNK.DBL.LLK HALF.CLUST\n"
                    "    HALF.LLK DIFF.LLK.CLUST.UNK); a notice counts the droplets it explains better by more than 2\n");
    return 1;
  }
  try {
    const std::string cmd = argv[1];
    if (cmd == "demuxlet") return cmd_demuxlet(argc - 2, argv + 2);
    if (cmd == "freemuxlet") return cmd_freemuxlet(argc - 2, argv + 2);
    if (cmd == "freemuxlet-old") return cmd_freemuxlet_old(argc - 2, argv + 2);
    if (cmd == "dump-plp") return cmd_dump_plp(argc - 2, argv + 2);
    if (cmd == "bgzf") return cmd_bgzf(argc - 2, argv + 2);
    if (cmd == "selftest-fmt") return cmd_selftest_fmt(argc - 2, argv + 2);
    if (cmd == "synth-plp") return cmd_synth_plp(argc - 2, argv + 2);
    fprintf(stderr, "Cannot recognize the command %s\n", argv[1]);
    return 1;
  } catch (const std::exception&) {
    return 1;
  }
}
