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
//       --ambient-mix: the ALT fraction of the ambient RNA per marker fitted as a mixture of the donors of the VCF
//       (muxgl_demux_soup_mix) instead of counted per marker: the soup is free RNA of the pooled donors, so its ALT fraction
//       is a weighted mean of their genotype dosages with the same shares at every marker -- V unknowns where the count
//       route estimates one per marker from 0-3 reads.  The reads are those of the droplets of --ambient-max-reads (0 =
//       all), as for the count profile; --ambient-mix-iter N (default 500) caps the EM steps, --ambient-mix-tol x (default
//       1e-8) is the largest change of a share at which it stops; --ambient-mix-unknown adds one component for a donor
//       missing from the VCF, with the Hardy-Weinberg genotype frequencies of the AF column of .var.gz as its genotype
//       prior (the panel mean, the library's default, is the mean of the other components: its share would not be
//       identified).  Fatal together with --ambient-af.  Writes <O>.soupmix.gz (BGZF), one row per component: SM_ID
//       (UNKNOWN for the extra component), SHARE, GRAD (%.6lf; GRAD is 1 at the maximum where SHARE > 0 and at most 1
//       where it is 0), and <O>.soupmix.af.gz (BGZF): the fitted profile, one value (%.17g) per line in .var.gz order, the
//       format --ambient-af reads, so a freemuxlet run can take it.  A notice gives the reads used, the steps, the status
//       (0 converged, 1 step cap, 2 no read took part) and the log-likelihood at the start and at the end.  With it
//       --write-ambient and --fit-ambient use the fitted profile; without it every output file is what it was
//   popscle-amd freemuxlet --plp P --nsample K --out O [...]                  mirrors cmdCramFreemux2 (cmd_cram_freemux2.cpp)
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
//
// The commands are cmd_demuxlet.hpp, cmd_freemuxlet.hpp and cmd_freemuxlet_old.hpp; what they share, cli_common.hpp; every
// text writer, table_writers.hpp.  This file keeps the tool commands and main().
#include "cmd_demuxlet.hpp"
#include "cmd_freemuxlet.hpp"
#include "cmd_freemuxlet_old.hpp"
#include "synthplp.hpp"

using namespace pa;

namespace {

// ------------------------------------------------------------------------------------------------ dump-plp
// loader-only command for the CPU tests: writes the packed pileup as a flat little-endian file
//   magic "MUXGLPLP", int64 C,S,nnz,R,nv, then cell_ptr, entry_snp, entry_rptr, reads, af[S], has_gp[S], gp[S*nv*3],
//   cell_totl_reads[C], cell_uniq_reads[C], then C barcodes and nv sample ids as NUL-terminated strings
int cmd_dump_plp(int argc, char** argv) {
  CommonFlags cf;
  GenotypeFlags gf;
  VcfReader vr;
  Args a;
  cf.add(a);
  gf.add(a, cf.lo, vr);
  a.add_string("vcf", &vr.path);
  a.add_int("rank", &cf.lo.rank);    // one rank's two slabs of a sharded run (LoadOptions): the file then holds the row
  a.add_int("world", &cf.lo.world);  // slab in place of the pileup and the column slab behind it
  a.parse(argc, argv);
  if (cf.plpPrefix.empty() || cf.outPrefix.empty()) fatal("Missing required option(s) : --plp, --out");
  Pileup p;
  if (!vr.path.empty()) {
    gf.init(vr);
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
