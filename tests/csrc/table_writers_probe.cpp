// table_writers_probe.cpp -- drives every table writer of popscle_amd/host/table_writers.hpp without the library or a device
// (tests/test_table_writers.py).  usage: table_writers_probe INPUT OUTDIR.  INPUT holds the arrays, one per line, `name value
// value ...`, as the test wrote them; the writers' files are left in OUTDIR uncompressed, with rows.txt (the two row lists)
// and counts.txt (what the writers returned).
#include <fstream>
#include <sstream>

#include "../../popscle_amd/host/table_writers.hpp"

using namespace pa;

static std::map<std::string, std::vector<std::string>> g_in;

static const std::vector<std::string>& S(const char* name) {
  if (!g_in.count(name)) fatal("no array %s", name);
  return g_in[name];
}
static std::vector<double> D(const char* name) {
  std::vector<double> v;
  for (const std::string& s : S(name)) v.push_back(strtod(s.c_str(), nullptr));  // (reads nan and -inf too)
  return v;
}
static std::vector<int32_t> I(const char* name) {
  std::vector<int32_t> v;
  for (const std::string& s : S(name)) v.push_back((int32_t)atoi(s.c_str()));
  return v;
}
static std::vector<uint8_t> B(const char* name) {
  std::vector<uint8_t> v;
  for (int32_t x : I(name)) v.push_back((uint8_t)x);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  for (std::string line; std::getline(in, line);) {
    std::istringstream ls(line);
    std::string name, tok;
    ls >> name;
    while (ls >> tok) g_in[name].push_back(tok);
  }
  const std::string out = std::string(argv[2]) + "/";
  try {
    const std::vector<std::string>& bcs = S("bcs");
    const size_t C = bcs.size(), n = 3;
    // the records of both commands, from one set of arrays
    const std::vector<int32_t> valid = I("valid"), nsnps = I("nsnps"), type = I("type"), clust = I("clust"), jBest = I("jBest"),
                               kBest = I("kBest"), jNext = I("jNext"), kNext = I("kNext"), sBest = I("sBest"), sNext = I("sNext"),
                               dBest1 = I("dBest1"), dBest2 = I("dBest2");
    const std::vector<double> bestLLK = D("bestLLK"), nextLLK = D("nextLLK"), sngBestLLK = D("sngBestLLK"),
                              sngNextLLK = D("sngNextLLK"), dblBestLLK = D("dblBestLLK"), bestPP = D("bestPP"), sngPP = D("sngPP"),
                              sngOnlyPP = D("sngOnlyPP");
    std::vector<muxgl_demux_cell> dc(C);
    std::vector<muxgl_fmx_cell> fc(C);
    memset(dc.data(), 0, C * sizeof(dc[0]));
    memset(fc.data(), 0, C * sizeof(fc[0]));
    for (size_t i = 0; i < C; ++i) {
      muxgl_demux_cell& d = dc[i];
      muxgl_fmx_cell& f = fc[i];
      d.valid = valid[i], d.nsnps = nsnps[i], f.clust = clust[i];
      d.type = f.type = type[i];
      d.jBest = f.jBest = jBest[i], d.kBest = f.kBest = kBest[i], d.jNext = f.jNext = jNext[i], d.kNext = f.kNext = kNext[i];
      d.sBest = f.sBest = sBest[i], d.sNext = f.sNext = sNext[i], d.dBest1 = f.dBest1 = dBest1[i], d.dBest2 = f.dBest2 = dBest2[i];
      d.bestLLK = f.bestLLK = bestLLK[i], d.nextLLK = f.nextLLK = nextLLK[i];
      d.sngBestLLK = f.sngBestLLK = sngBestLLK[i], d.sngNextLLK = f.sngNextLLK = sngNextLLK[i];
      d.dblBestLLK = f.dblBestLLK = dblBestLLK[i];
      d.bestPP = f.bestPP = bestPP[i], d.sngPP = f.sngPP = sngPP[i], d.sngOnlyPP = f.sngOnlyPP = sngOnlyPP[i];
    }
    // the two row lists
    const std::vector<int32_t> totl = I("totl_reads"), uniq = I("uniq_reads"), lim = I("min_read_umi_snp"), fSNPs = I("f_nsnps"),
                               fReads = I("f_nreads");
    const Table td{bcs, printed_droplets(bcs, totl.data(), uniq.data(), dc.data(), lim[0], lim[1], lim[2]), Label::samples(S("ids"))};
    const Table tf{bcs, all_droplets((int64_t)C, fSNPs.data(), fReads.data()), Label::clusters()};
    {
      OutFile w(out + "rows.txt", false);
      for (const Table* t : {&td, &tf})
        for (const TableRow& r : t->rows) w.printf("%s\t%d\t%d\t%d\t%d\n", t == &td ? "d" : "f", r.cell, r.nsnps, r.nreads, r.pos);
    }
    OutFile counts(out + "counts.txt", false);

    // the shared per-droplet tables, once per row list and label
    const std::vector<double> sng = D("sng"), incl = D("incl"), tot = D("tot"), dbl = D("dbl"), alpha = D("alpha"), rhos = D("rhos"),
                              amb = D("amb");
    const std::vector<int32_t> partner = I("partner"), aidx = I("aidx"), first = I("first");
    write_singlets(OutFile(out + "d.sing2", false), td, n, sng.data());
    write_singlets(OutFile(out + "f.sing2", false), tf, n, sng.data());
    write_inclusion(OutFile(out + "d.incl", false), td, n, incl.data(), tot.data(), dbl.data(), partner.data(), alpha.data(),
                    aidx.data(), first.data());
    write_inclusion(OutFile(out + "f.incl", false), tf, n, incl.data(), tot.data(), dbl.data(), partner.data());
    counts.printf("d.amb\t%lld\n", (long long)write_ambient(OutFile(out + "d.amb", false), td, dc.data(), n, rhos, amb.data(), false));
    counts.printf("f.amb\t%lld\n", (long long)write_ambient(OutFile(out + "f.amb", false), tf, fc.data(), n, rhos, amb.data(), true));

    const std::vector<int32_t> dcand = all_fit_cands(dc.data(), C, (int)n), fcand = all_fit_cands(fc.data(), C, (int)n),
                               dpair = all_fit_pairs(dc.data(), C, (int)n), fpair = all_fit_pairs(fc.data(), C, (int)n),
                               status = I("status");
    const std::vector<double> est = D("est"), llh = D("ll_hat"), ll0 = D("ll_zero"), llt = D("ll_top"), info = D("info");
    {
      OutFile w(out + "slots.txt", false);  // the candidates and pairs of every droplet, as handed to the library
      for (size_t i = 0; i < C; ++i)
        w.printf("%d %d\t%d %d %d %d\t%d %d\t%d %d %d %d\n", dcand[i * 2], dcand[i * 2 + 1], dpair[i * 4], dpair[i * 4 + 1],
                 dpair[i * 4 + 2], dpair[i * 4 + 3], fcand[i * 2], fcand[i * 2 + 1], fpair[i * 4], fpair[i * 4 + 1], fpair[i * 4 + 2],
                 fpair[i * 4 + 3]);
    }
    write_ambient_fit(OutFile(out + "d.ambfit", false), td, dcand.data(), status.data(), est.data(), llh.data(), ll0.data(), info.data());
    write_ambient_fit(OutFile(out + "f.ambfit", false), tf, fcand.data(), status.data(), est.data(), llh.data(), ll0.data(), info.data());
    for (int whole = 1; whole >= 0; --whole) {
      const std::string sfx = whole ? ".alphafit" : ".alphafit_capped";
      counts.printf("d%s\t%lld\n", sfx.c_str(),
                    (long long)write_alpha_fit(OutFile(out + "d" + sfx, false), td, dc.data(), whole, dpair.data(), status.data(),
                                               est.data(), llh.data(), ll0.data(), llt.data(), info.data()));
      counts.printf("f%s\t%lld\n", sfx.c_str(),
                    (long long)write_alpha_fit(OutFile(out + "f" + sfx, false), tf, fc.data(), whole, fpair.data(), status.data(),
                                               est.data(), llh.data(), ll0.data(), llt.data(), info.data()));
    }

    // .unk.gz: one writer per command
    const std::vector<double> d_ju = D("d_ju"), d_uj = D("d_uj"), d_uu = D("d_uu"), f_ju = D("f_ju"), f_lu = D("f_lu"), f_uu = D("f_uu");
    write_unknown_demux(OutFile(out + "d.unk", false), td, dc.data(), n, alpha.size(), alpha.data(), d_ju.data(), d_uj.data(), d_uu.data());
    counts.printf("f.unk\t%lld\n",
                  (long long)write_unknown_fmx(OutFile(out + "f.unk", false), tf, fc.data(), n, f_ju.data(), f_lu.data(), f_uu.data()));

    // the files of the two freemuxlet commands
    const std::vector<double> llk0 = D("llk0"), llk2 = D("llk2");
    write_lmix(OutFile(out + "f.lmix", false), tf, kLmixHeader, true, llk0.data(), llk2.data());
    write_lmix(OutFile(out + "f.lmix_old", false), tf, kLmixHeaderOld, false, llk0.data(), llk2.data());
    write_clust0_samples(OutFile(out + "f.clust0", false), tf, clust.data());
    write_clust1_samples(OutFile(out + "f.clust1", false), tf, fc.data());
    const std::vector<int32_t> srted = I("drops_srted"), dd_n = I("dd_nsnps"), dd_r1 = I("dd_nread1"), dd_r2 = I("dd_nread2");
    const std::vector<double> dd_l0 = D("dd_llk0"), dd_l2 = D("dd_llk2");
    std::vector<muxgl_dropd> dds(dd_n.size());
    memset(dds.data(), 0, dds.size() * sizeof(dds[0]));
    for (size_t i = 0; i < dds.size(); ++i)
      dds[i].nsnps = dd_n[i], dds[i].nread1 = dd_r1[i], dds[i].nread2 = dd_r2[i], dds[i].llk0 = dd_l0[i], dds[i].llk2 = dd_l2[i];
    write_droplet_ldist(OutFile(out + "old.ldist", false), I("nvis")[0], srted.data(), dds.data());
    write_droplet_ldist(OutFile(out + "old.ldist_header", false), I("nvis")[0], srted.data(), nullptr);

    // the cluster-level tables: K = 3 clusters, the first two anchored to two of the three donors
    const Label donors = Label::samples(S("ids"));
    const std::vector<int32_t> start = I("anchor_start");
    const std::vector<double> start_llr = D("anchor_start_llr");
    const std::vector<uint8_t> mode = B("anchor_mode");
    const int nAnchor = (int)mode.size();
    write_anchors(OutFile(out + "anchors", false), (int)n, nAnchor, donors, start.data(), start_llr.data(), nullptr, (int64_t)C, fc.data());
    write_anchors(OutFile(out + "anchors_mode", false), (int)n, nAnchor, donors, start.data(), start_llr.data(), mode.data(), (int64_t)C,
                  fc.data());
    const std::vector<uint8_t> has_gp = B("has_gp");
    const std::vector<double> gp = D("gp"), post = D("post");
    write_refined(OutFile(out + "refined", false), (int64_t)has_gp.size(), n, (size_t)nAnchor, donors, mode.data(), has_gp.data(), gp.data(),
                  post.data());
    const std::vector<double> mll = D("match_ll"), mll0 = D("match_ll0");
    const std::vector<int32_t> mns = I("match_nsnps");
    const DonorMatch m{mns.size(), mll.size() / mns.size(), mll.data(), mll0.data(), mns.data()};
    write_match(OutFile(out + "match", false), m, donors);
    write_match_best(OutFile(out + "match.best", false), m, donors);
    const std::vector<double> pl2 = D("pairs_l2"), pl0 = D("pairs_l0");
    const std::vector<int32_t> pns = I("pairs_nsnps");
    write_cluster_ldist(OutFile(out + "clust.ldist", false), n, pl2.data(), pl0.data(), pns.data());
  } catch (const std::exception&) {
    return 1;
  }
  return 0;
}
