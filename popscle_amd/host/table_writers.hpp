// table_writers.hpp -- the text writers of the front end: one function per output file, over arrays the C-ABI has filled.
// Plain host code: nothing here calls the library (muxgl.h is included for the record structs only), so every writer runs
// without a device (tests/csrc/table_writers_probe.cpp).  The columns are described in the comment at the top of main.cpp.
//
// A per-droplet writer is given two things besides its arrays, both in a Table:
//   * the row list: {droplet index, NUM.SNPS, NUM.READS} of the droplets it prints, in the order it prints them --
//     demuxlet: the droplets of .best, in barcode order (printed_droplets); freemuxlet: every droplet (all_droplets);
//   * the label of a column: a sample id, or the cluster's number (Label).
// Arrays are indexed by the droplet index, [C][...], whatever the row list leaves out.
#pragma once

#include <cmath>

#include "plp.hpp"

namespace pa {

// appends printf(fmt, ...) to o, whatever its length
__attribute__((format(printf, 2, 3))) inline void appendf(std::string& o, const char* fmt, ...) {
  char buf[512];
  va_list ap, ap2;
  va_start(ap, fmt);
  va_copy(ap2, ap);
  const int n = vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (n < (int)sizeof(buf)) {
    o.append(buf, (size_t)n);
  } else {  // (a barcode of a kilobyte): the buffer grows to what snprintf reported
    const size_t at = o.size();
    o.resize(at + (size_t)n + 1);
    vsnprintf(&o[at], (size_t)n + 1, fmt, ap2);
    o.resize(at + (size_t)n);
  }
  va_end(ap2);
}

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

// ---- the row list and the label ----
struct TableRow {
  int32_t cell, nsnps, nreads;  // the droplet's index, NUM.SNPS and NUM.READS
  int32_t pos;                  // its position among ALL droplets in the table's order (INT_ID of .best counts skipped droplets too)
};

// the label of column j: the sample id (NA outside the panel), or the cluster's number
struct Label {
  const std::vector<std::string>* ids;  // NULL: clusters
  const char *head, *head12;            // the header's word for one column and for a pair
  static Label samples(const std::vector<std::string>& ids) { return {&ids, "SM_ID", "SM1_ID\tSM2_ID"}; }
  static Label clusters() { return {nullptr, "CLUST", "CLUST1\tCLUST2"}; }
  std::string operator()(int j) const {
    if (!ids) return std::to_string(j);
    return (j >= 0 && j < (int)ids->size()) ? (*ids)[(size_t)j] : "NA";
  }
};

struct Table {
  const std::vector<std::string>& bcs;  // [C]
  std::vector<TableRow> rows;
  Label label;
  int64_t n() const { return (int64_t)rows.size(); }
  const char* bc(const TableRow& r) const { return bcs[(size_t)r.cell].c_str(); }
};

// The droplets .best prints (cmd_cram_demuxlet.cpp:636-641,653), in barcode-sorted order: those with enough reads, UMIs
// and markers that have an entry at all
inline std::vector<TableRow> printed_droplets(const std::vector<std::string>& bcs, const int32_t* totl_reads,
                                              const int32_t* uniq_reads, const muxgl_demux_cell* cells, int32_t minRead,
                                              int32_t minUMI, int32_t minSNP) {
  std::map<std::string, int32_t> bc_map;
  for (size_t i = 0; i < bcs.size(); ++i) bc_map[bcs[i]] = (int32_t)i;
  std::vector<TableRow> rows;
  int32_t pos = 0;
  for (auto it = bc_map.begin(); it != bc_map.end(); ++it, ++pos) {
    const int32_t i = it->second;
    const muxgl_demux_cell& c = cells[i];
    if (totl_reads[i] < minRead || uniq_reads[i] < minUMI || c.nsnps < minSNP) continue;  // :641
    if (!c.valid) continue;                                                              // :653
    rows.push_back({i, c.nsnps, uniq_reads[i], pos});
  }
  return rows;
}

// every droplet in index order, with the counts of muxgl_fmx_prepare: the rows of .clust1.samples.gz
inline std::vector<TableRow> all_droplets(int64_t C, const int32_t* nSNPs, const int32_t* nReads) {
  std::vector<TableRow> rows((size_t)C);
  for (int64_t i = 0; i < C; ++i) rows[(size_t)i] = {(int32_t)i, nSNPs[i], nReads[i], (int32_t)i};
  return rows;
}

inline const char* type_name(int32_t type) { return (type == 2) ? "AMB" : ((type == 0) ? "SNG" : "DBL"); }

// ---- .sing2.gz: one row per droplet and column.  POSTPRB: equal priors over the columns, a softmax over the droplet's
// row with its maximum subtracted ----
inline void write_singlets(OutFile&& w, const Table& t, size_t n, const double* sng /* [C][n] */) {
  std::vector<double> rmax((size_t)t.n()), rsum((size_t)t.n());
  parallel_for(t.n(), plp_threads(), [&](int64_t i) {
    const double* row = sng + (size_t)t.rows[(size_t)i].cell * n;
    double mx = row[0], sum = 0.0;
    for (size_t j = 1; j < n; ++j) mx = std::max(mx, row[j]);
    for (size_t j = 0; j < n; ++j) sum += exp(row[j] - mx);
    rmax[(size_t)i] = mx;
    rsum[(size_t)i] = sum;
  });
  w.printf("BARCODE\t%s\tNUM.SNPS\tNUM.READS\tLLK1\tPOSTPRB\n", t.label.head);
  write_rows_parallel(w, t.n() * (int64_t)n, [&](int64_t r, std::string& o) {
    const size_t i = (size_t)r / n, j = (size_t)r % n;
    const TableRow& d = t.rows[i];
    const double v = sng[(size_t)d.cell * n + j];
    appendf(o, "%s\t%s\t%d\t%d\t%.4lf\t%.3lg\n", t.bc(d), t.label((int)j).c_str(), d.nsnps, d.nreads, v,
            exp(v - rmax[i]) / rsum[i]);
  });
  w.close();
}

// ---- .incl.gz: one row per droplet and column.  alpha: the grid, for demuxlet's DBL.ALPHA column (the share of the
// column's OWN reads in its best doublet), or NULL for a table without it ----
inline void write_inclusion(OutFile&& w, const Table& t, size_t n, const double* incl /* [C][n] */, const double* tot /* [C] */,
                            const double* dbl, const int32_t* partner /* [C][n] */, const double* alpha = nullptr,
                            const int32_t* aidx = nullptr, const int32_t* first = nullptr /* [C][n] */) {
  w.printf("BARCODE\t%s\tNUM.SNPS\tNUM.READS\tLLK.INCL\tPOSTPRB.INCL\tDBL.PARTNER\t%sDBL.LLK\n", t.label.head,
           alpha ? "DBL.ALPHA\t" : "");
  write_rows_parallel(w, t.n() * (int64_t)n, [&](int64_t r, std::string& o) {
    const size_t j = (size_t)r % n;
    const TableRow& d = t.rows[(size_t)r / n];
    const size_t x = (size_t)d.cell * n + j;
    appendf(o, "%s\t%s\t%d\t%d\t%.4lf\t%.3lg\t", t.bc(d), t.label((int)j).c_str(), d.nsnps, d.nreads, incl[x],
            exp(incl[x] - tot[d.cell]));
    if (partner[x] < 0) {
      o += alpha ? "NA\tNA\tNA\n" : "NA\tNA\n";
      return;
    }
    appendf(o, "%s\t", t.label(partner[x]).c_str());
    if (alpha) appendf(o, "%.3lf\t", first[x] ? 1.0 - alpha[aidx[x]] : alpha[aidx[x]]);
    appendf(o, "%.4lf\n", dbl[x]);
  });
  w.close();
}

// ---- .unk.gz of demuxlet: one row per droplet.  The best hypothesis with one panel sample: (j, n >= 1, known donor first)
// and, where alpha[n] != 0.5, (k, n >= 1, known donor second) -- at 0.5 the two are one hypothesis, the reference's k < j
// rule for mirrored pairs (:812-815); ties by value, then (sample, n, known donor first) ascending.  The values are
// compared as they are ----
inline void write_unknown_demux(OutFile&& w, const Table& t, const muxgl_demux_cell* cells, size_t V, size_t A,
                                const double* alpha /* [A] */, const double* ju, const double* uj /* [C][V][A] */,
                                const double* uu /* [C][A] */) {
  w.printf("BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.ALPHA\tUNK.DBL.LLK\tHALF.GUESS\tHALF.LLK\t"
           "DIFF.LLK.PANEL.UNK\n");
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    const muxgl_demux_cell& c = cells[d.cell];
    const double* r2 = uu + (size_t)d.cell * A;
    double top = r2[0], dblv = -1e300, halfv = -1e300;
    int dn = -1, hj = -1, hn = -1, hmajor = -1;
    for (size_t n = 1; n < A; ++n)
      if (r2[n] > dblv) dblv = r2[n], dn = (int)n;
    for (size_t j = 0; j < V; ++j)
      for (size_t n = 1; n < A; ++n) {
        const size_t x = ((size_t)d.cell * V + j) * A + n;
        if (ju[x] > halfv) halfv = ju[x], hj = (int)j, hn = (int)n, hmajor = 1;
        if (alpha[n] != 0.5 && uj[x] > halfv) halfv = uj[x], hj = (int)j, hn = (int)n, hmajor = 0;
      }
    appendf(o, "%s\t%d\t%d\t%.4lf\t%.4lf\t", t.bc(d), d.nsnps, d.nreads, c.bestLLK, r2[0]);
    if (dn < 0) {
      o += "NA\tNA\t";
    } else {
      appendf(o, "%.2lf\t%.4lf\t", alpha[dn], dblv);
      top = std::max(top, dblv);
    }
    if (hj < 0) {
      o += "NA\tNA\t";
    } else {
      const std::string sm = t.label(hj);
      appendf(o, "%s,%s,%.2lf\t%.4lf\t", hmajor ? sm.c_str() : "*", hmajor ? "*" : sm.c_str(), alpha[hn], halfv);
      top = std::max(top, halfv);
    }
    appendf(o, "%.4lf\n", c.bestLLK - top);
  });
  w.close();
}

// ---- .clust1.unk.gz of freemuxlet: one row per droplet.  The cluster that pairs best with the unknown donor: the largest
// ll_ju, ties to the lowest cluster; a NaN ranks as -inf.  Returns the droplets with DIFF.LLK.CLUST.UNK < -2 ----
inline int64_t write_unknown_fmx(OutFile&& w, const Table& t, const muxgl_fmx_cell* cells, size_t K, const double* ju /* [C][K] */,
                                 const double* lu, const double* uu /* [C] */) {
  std::vector<int32_t> hclust((size_t)t.n());
  std::vector<double> hllk((size_t)t.n()), diff((size_t)t.n());
  parallel_for(t.n(), plp_threads(), [&](int64_t r) {
    const int32_t i = t.rows[(size_t)r].cell;
    const double* row = ju + (size_t)i * K;
    auto val = [](double v) { return std::isnan(v) ? -INFINITY : v; };
    size_t b = 0;
    for (size_t j = 1; j < K; ++j)
      if (val(row[j]) > val(row[b])) b = j;
    hclust[(size_t)r] = (int32_t)b;
    hllk[(size_t)r] = val(row[b]);
    const double top = std::max(std::max(val(lu[i]), val(uu[i])), val(row[b]));
    const double d = cells[i].bestLLK - top;
    diff[(size_t)r] = std::isnan(d) ? 0.0 : d;  // (-inf against -inf: neither explains the droplet)
  });
  int64_t nbetter = 0;
  for (double d : diff) nbetter += d < -2.0;
  w.printf("BARCODE\tNUM.SNPS\tNUM.READS\tBEST.LLK\tUNK.SNG.LLK\tUNK.DBL.LLK\tHALF.CLUST\tHALF.LLK\tDIFF.LLK.CLUST.UNK\n");
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    appendf(o, "%s\t%d\t%d\t%.4lf\t%.4lf\t%.4lf\t%d\t%.4lf\t%.4lf\n", t.bc(d), d.nsnps, d.nreads, cells[d.cell].bestLLK,
            lu[d.cell], uu[d.cell], (int)hclust[(size_t)r], hllk[(size_t)r], diff[(size_t)r]);
  });
  w.close();
  return nbetter;
}

// ---- .amb.gz: one row per droplet, the best (column, rho): by value, then (column, rho index) ascending.  nan_low: a
// NaN ranks as -inf (freemuxlet, whose table holds one where a posterior row is exactly 0); demuxlet compares the values
// as they are.  Returns the droplets called DBL that the best reading beats their best doublet by more than 2 ----
template <class Cell>
int64_t write_ambient(OutFile&& w, const Table& t, const Cell* cells, size_t n, const std::vector<double>& rhos,
                      const double* amb /* [C][n][NR] */, bool nan_low) {
  const size_t NR = rhos.size();
  std::vector<size_t> best((size_t)t.n());
  parallel_for(t.n(), plp_threads(), [&](int64_t r) {
    const double* row = amb + (size_t)t.rows[(size_t)r].cell * n * NR;
    auto val = [nan_low](double v) { return nan_low && std::isnan(v) ? -INFINITY : v; };
    size_t at = 0;
    for (size_t x = 1; x < n * NR; ++x)
      if (val(row[x]) > val(row[at])) at = x;
    best[(size_t)r] = at;
  });
  int64_t rescued = 0;
  for (int64_t r = 0; r < t.n(); ++r) {
    const int32_t i = t.rows[(size_t)r].cell;
    rescued += cells[i].type == 1 && amb[(size_t)i * n * NR + best[(size_t)r]] > cells[i].dblBestLLK + 2.0;
  }
  w.printf("BARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.LLK\tSNG.BEST.GUESS\tSNG.BEST.LLK\tAMB.GUESS\tAMB.RHO\tAMB.LLK\t"
           "DIFF.LLK.AMB.BEST\n");
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    const Cell& c = cells[d.cell];
    const size_t at = best[(size_t)r];
    const double v = amb[(size_t)d.cell * n * NR + at];
    appendf(o, "%s\t%d\t%d\t%s\t%.4lf\t%s\t%.4lf\t%s\t%.2lf\t%.4lf\t%.4lf\n", t.bc(d), d.nsnps, d.nreads, type_name(c.type),
            c.bestLLK, t.label(c.sBest).c_str(), c.sngBestLLK, t.label((int)(at / NR)).c_str(), rhos[at % NR], v, v - c.bestLLK);
  });
  w.close();
  return rescued;
}

// ---- what the --fit-ambient / --fit-alpha writers share ----
struct FitField {  // a number of a fit's row as "%.4lf", or NA
  char s[32];
  FitField(bool have, double v) { have ? snprintf(s, sizeof(s), "%.4lf", v) : snprintf(s, sizeof(s), "NA"); }
};
// the standard error of an interior estimate (on a bound: none)
inline FitField fit_se(int32_t status, double info) { return FitField(status == 0 && info > 0.0, 1.0 / sqrt(info)); }
// the likelihood ratio against `alone`; NA where it is not finite (freemuxlet: a posterior row of exactly 0 makes LL -inf.
// Demuxlet's LL is finite whatever the input, by the 1e-10 offset of every weight, so its tables never print NA here)
inline FitField fit_lrt(double ll_hat, double alone) { return FitField(std::isfinite(2.0 * (ll_hat - alone)), 2.0 * (ll_hat - alone)); }
// what a mix is held against: the first column alone, or, where the fit's interval is the whole [0, 1] (only then is ll_top
// the second column alone), the better of the two
inline double fit_alone(bool whole, double ll_zero, double ll_top) { return whole ? std::max(ll_zero, ll_top) : ll_zero; }
// a droplet's slots, -1 where the record has no such column among the n.  An ambient fit, q[2]: SNG.BEST and SNG.NEXT; a
// mixing-share fit, q[4]: DBL, the two columns of DBL.BEST, and SNG, (SNG.BEST, SNG.NEXT), both -1 where one is missing
inline void fit_cands(int32_t* q, bool valid, int sBest, int sNext, int n) {
  q[0] = (valid && sBest >= 0 && sBest < n) ? sBest : -1;
  q[1] = (valid && sNext >= 0 && sNext < n) ? sNext : -1;
}
inline void fit_pairs(int32_t* q, bool valid, int dBest1, int dBest2, int sBest, int sNext, int n) {
  auto ok = [&](int s) { return s >= 0 && s < n; };
  const bool dbl = valid && ok(dBest1) && ok(dBest2), sng = valid && ok(sBest) && ok(sNext);
  q[0] = dbl ? dBest1 : -1, q[1] = dbl ? dBest2 : -1;
  q[2] = sng ? sBest : -1, q[3] = sng ? sNext : -1;
}
// the slots of all C droplets among n columns.  A demuxlet record without entries (valid = 0) has none
inline bool has_calls(const muxgl_demux_cell& c) { return c.valid; }
inline bool has_calls(const muxgl_fmx_cell&) { return true; }
template <class Cell>
std::vector<int32_t> all_fit_cands(const Cell* cells, size_t C, int n) {  // [C][2]
  std::vector<int32_t> q(C * 2);
  for (size_t i = 0; i < C; ++i) fit_cands(&q[i * 2], has_calls(cells[i]), cells[i].sBest, cells[i].sNext, n);
  return q;
}
template <class Cell>
std::vector<int32_t> all_fit_pairs(const Cell* cells, size_t C, int n) {  // [C][2][2]
  std::vector<int32_t> q(C * 4);
  for (size_t i = 0; i < C; ++i)
    fit_pairs(&q[i * 4], has_calls(cells[i]), cells[i].dBest1, cells[i].dBest2, cells[i].sBest, cells[i].sNext, n);
  return q;
}

// ---- .ambfit.gz: per droplet one row for SNG.BEST.GUESS and one for SNG.NEXT.GUESS (none where cand is -1) ----
inline void write_ambient_fit(OutFile&& w, const Table& t, const int32_t* cand, const int32_t* status, const double* rho,
                              const double* llh, const double* ll0, const double* info /* each [C][2] */) {
  w.printf("BARCODE\tNUM.SNPS\tNUM.READS\t%s\tSNG.LLK\tAMB.RHO.MLE\tAMB.RHO.SE\tAMB.LLK.MLE\tAMB.LRT\tSTATUS\n", t.label.head);
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    for (size_t k = 0; k < 2; ++k) {
      const size_t x = (size_t)d.cell * 2 + k;
      if (cand[x] < 0) continue;
      appendf(o, "%s\t%d\t%d\t%s\t%.4lf\t%.4lf\t%s\t%.4lf\t%s\t%d\n", t.bc(d), d.nsnps, d.nreads, t.label(cand[x]).c_str(), ll0[x],
              rho[x], fit_se(status[x], info[x]).s, llh[x], fit_lrt(llh[x], ll0[x]).s, (int)status[x]);
    }
  });
  w.close();
}

// ---- .alphafit.gz: per droplet one row DBL for the two columns of DBL.BEST.GUESS and one row SNG for (SNG.BEST.GUESS,
// SNG.NEXT.GUESS) (none where the pair is -1).  whole: the fit's interval is [0, 1].  Returns the droplets called SNG whose
// SNG row beats what it is held against by more than 2 ----
template <class Cell>
int64_t write_alpha_fit(OutFile&& w, const Table& t, const Cell* cells, bool whole, const int32_t* pair /* [C][2][2] */,
                        const int32_t* status, const double* ah, const double* llh, const double* ll0, const double* llt,
                        const double* info /* each [C][2] */) {
  auto one_of = [&](size_t x) { return fit_alone(whole, ll0[x], llt[x]); };
  int64_t mixed = 0;
  for (const TableRow& d : t.rows) {
    const size_t x = (size_t)d.cell * 2 + 1;
    mixed += pair[x * 2] >= 0 && cells[d.cell].type == 0 && llh[x] > one_of(x) + 2.0;
  }
  w.printf("BARCODE\tNUM.SNPS\tNUM.READS\tPAIR\t%s\tSNG1.LLK\tSNG2.LLK\tALPHA.MLE\tALPHA.SE\tMIX.LLK.MLE\tMIX.LRT\tSTATUS\n",
           t.label.head12);
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    for (size_t k = 0; k < 2; ++k) {
      const size_t x = (size_t)d.cell * 2 + k;
      if (pair[x * 2] < 0) continue;
      appendf(o, "%s\t%d\t%d\t%s\t%s\t%s\t%.4lf\t%s\t%.4lf\t%s\t%.4lf\t%s\t%d\n", t.bc(d), d.nsnps, d.nreads, k == 0 ? "DBL" : "SNG",
              t.label(pair[x * 2]).c_str(), t.label(pair[x * 2 + 1]).c_str(), ll0[x], FitField(whole, llt[x]).s, ah[x],
              fit_se(status[x], info[x]).s, llh[x], fit_lrt(llh[x], one_of(x)).s, (int)status[x]);
    }
  });
  w.close();
  return mixed;
}

// ---- the files of the two freemuxlet commands ----
// .lmix (cmd_cram_freemux2.cpp:111-163, cmd_cram_freemuxlet.cpp:110-165): the two commands differ in the header's last two
// words and in the sign of the Bayes factor they print there
constexpr const char* kLmixHeader = "INT_ID\tBARCODE\tNSNPs\tNREADs\tDBL.LLK\tSNG.LLK\tBF.SINGLET\tBF.SINGLET.PER.SNP\n";
constexpr const char* kLmixHeaderOld = "INT_ID\tBARCODE\tNSNPs\tNREADs\tDBL.LLK\tSNG.LLK\tLOG.BF\tBFpSNP\n";
inline void write_lmix(OutFile&& w, const Table& t, const char* header, bool singlet_over_doublet, const double* llk0,
                       const double* llk2 /* [C] */) {
  w.write(header, strlen(header));
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    const double bf = singlet_over_doublet ? llk2[d.cell] - llk0[d.cell] : llk0[d.cell] - llk2[d.cell];
    appendf(o, "%d\t%s\t%d\t%d\t%.2lf\t%.2lf\t%.2lf\t%.4lf\n", d.pos, t.bc(d), d.nsnps, d.nreads, llk0[d.cell], llk2[d.cell], bf,
            bf / d.nsnps);
  });
  w.close();
}

// .clust0.samples.gz (cmd_cram_freemux2.cpp:265-274, cmd_cram_freemuxlet.cpp:353-363)
inline void write_clust0_samples(OutFile&& w, const Table& t, const int32_t* clusts /* [C] */) {
  w.printf("INT_ID\tBARCODE\tCLUST0\n");
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    appendf(o, "%d\t%s\t%d\n", d.pos, t.bc(d), clusts[d.cell]);
  });
  w.close();
}

// .clust1.samples.gz (cmd_cram_freemux2.cpp:660-665, cmd_cram_freemuxlet.cpp:709-714)
inline void write_clust1_samples(OutFile&& w, const Table& t, const muxgl_fmx_cell* cells) {
  w.printf("INT_ID\tBARCODE\tNUM.SNPS\tNUM.READS\tDROPLET.TYPE\tBEST.GUESS\tBEST.LLK\tNEXT.GUESS\tNEXT.LLK\t"
           "DIFF.LLK.BEST.NEXT\tBEST.POSTERIOR\tSNG.POSTERIOR\tSNG.BEST.GUESS\tSNG.BEST.LLK\tSNG.NEXT.GUESS\t"
           "SNG.NEXT.LLK\tSNG.ONLY.POSTERIOR\tDBL.BEST.GUESS\tDBL.BEST.LLK\tDIFF.LLK.SNG.DBL\n");
  write_rows_parallel(w, t.n(), [&](int64_t r, std::string& o) {
    const TableRow& d = t.rows[(size_t)r];
    const muxgl_fmx_cell& c = cells[d.cell];
    appendf(o,
            "%d\t%s\t%d\t%d\t%s\t%d,%d\t%.2lf\t%d,%d\t%.2lf\t%.2lf\t%.5lf\t%.2lg\t%d\t%.2lf\t%d\t%.2lf\t%.5lf\t%d,%d\t"
            "%.2lf\t%.2lf\n",
            d.pos, t.bc(d), d.nsnps, d.nreads, type_name(c.type), c.jBest, c.kBest, c.bestLLK, c.jNext, c.kNext, c.nextLLK,
            c.bestLLK - c.nextLLK, c.bestPP, c.sngPP, c.sBest, c.sngBestLLK, c.sNext, c.sngNextLLK, c.sngOnlyPP, c.dBest1,
            c.dBest2, c.dblBestLLK, c.sngBestLLK - c.dblBestLLK);
  });
  w.close();
}

// .ldist.gz of freemuxlet-old (cmd_cram_freemuxlet.cpp:178-182,262-265): the pairs of the first `nvis` droplets of the
// sorted order, as the voting loop visits them; dropDs: the lower triangle [hi (hi - 1) / 2 + lo], or NULL for the header alone
inline void write_droplet_ldist(OutFile&& w, int64_t nvis, const int32_t* drops_srted, const muxgl_dropd* dropDs) {
  w.printf("ID1\tID2\tNSNP\tREAD1\tREAD2\tREADMIN\tLLK0\tLLK2\tLDIFF\tDIFF.SNP\n");
  for (int64_t i = 0; dropDs && i < nvis; ++i) {
    const int32_t si = drops_srted[i];
    for (int64_t j = 0; j < i; ++j) {
      const int32_t sj = drops_srted[j];
      const int64_t hi = si > sj ? si : sj, lo = si > sj ? sj : si;
      const muxgl_dropd& dd = dropDs[hi * (hi - 1) / 2 + lo];
      w.printf("%d\t%d\t%d\t%d\t%d\t%d\t%.2lf\t%.2lf\t%.2lf\t%.4lf\n", si, sj, dd.nsnps, dd.nread1, dd.nread2,
               dd.nread1 > dd.nread2 ? dd.nread2 : dd.nread1, dd.llk0, dd.llk2, dd.llk2 - dd.llk0,
               (dd.llk2 - dd.llk0) / (dd.nsnps + 1e-6));
    }
  }
  w.close();
}

// ---- the soup mixture of demuxlet (--ambient-mix) ----
// .soupmix.gz: one row per component of muxgl_demux_soup_mix -- the V samples of the panel in VCF column order and, where
// M == V + 1, the donor missing from the VCF as UNKNOWN -- with its share of the soup and its gradient (1 at a maximum of
// the likelihood where the share is above 0, at most 1 where it is 0); and .soupmix.af.gz: the fitted ALT fraction of the
// soup, one value per line in .var.gz order, written so that --ambient-af reads back the same doubles
inline void write_soup_mix(OutFile&& w, OutFile&& wf, const Label& donor, size_t V, size_t M, const double* pi /* [M] */,
                           const double* grad /* [M] */, size_t S, const double* amb_af /* [S] */) {
  w.printf("SM_ID\tSHARE\tGRAD\n");
  for (size_t v = 0; v < M; ++v) w.printf("%s\t%.6lf\t%.6lf\n", v < V ? donor((int)v).c_str() : "UNKNOWN", pi[v], grad[v]);
  w.close();
  for (size_t s = 0; s < S; ++s) wf.printf("%.17g\n", amb_af[s]);
  wf.close();
}

// ---- the cluster-level tables of freemuxlet ----
// .clust1.anchors.gz: one row per cluster -- the donor it is held to, the greedy cluster it started from with the log Bayes
// factor of that match, and the droplets called singlets of it.  mode: [nAnchor] MUXGL_ANCHOR_*, or NULL for no MODE column
inline void write_anchors(OutFile&& w, int K, int nAnchor, const Label& donor, const int32_t* start, const double* start_llr,
                          const uint8_t* mode /* each [nAnchor] */, int64_t C, const muxgl_fmx_cell* cells) {
  std::vector<int64_t> nsng((size_t)K, 0);
  for (int64_t i = 0; i < C; ++i)
    if (cells[i].clust >= 0 && cells[i].clust < K) ++nsng[(size_t)cells[i].clust];
  w.printf("CLUST\tSM_ID\tSTART.CLUST\tSTART.LLR\tN.SNG%s\n", mode ? "\tMODE" : "");
  for (int k = 0; k < K; ++k) {
    w.printf("%d\t%s\t", k, k < nAnchor ? donor(k).c_str() : "NA");
    if (k < nAnchor && start[k] >= 0) w.printf("%d\t%.4lf\t", (int)start[k], start_llr[k]);
    else w.printf("NA\tNA\t");
    w.printf("%lld", (long long)nsng[(size_t)k]);
    if (mode) w.printf("\t%s", k >= nAnchor ? "NA" : mode[k] == MUXGL_ANCHOR_PRIOR ? "PRIOR" : "HELD");
    w.printf("\n");
  }
  w.close();
}

// .clust1.refined.gz: what the droplets made of the PRIOR donors' genotypes (freemuxlet.refine_summary is the same summary
// in numpy) -- the posterior rows the last E-step read against the panel rows, over the markers with genotypes
inline void write_refined(OutFile&& w, int64_t S, size_t V, size_t nAnchor, const Label& donor, const uint8_t* mode /* [nAnchor] */,
                          const uint8_t* has_gp /* [S] */, const double* gp /* [S][V][3] */, const double* post /* [S][nAnchor][3] */) {
  auto argmax3 = [](const double* r) { return r[1] > r[0] ? (r[2] > r[1] ? 2 : 1) : (r[2] > r[0] ? 2 : 0); };  // (the first maximum)
  w.printf("CLUST\tSM_ID\tN.GENO\tN.CHANGED\tMEAN.MAXGP.PRIOR\tMEAN.MAXGP.POST\n");
  for (size_t k = 0; k < nAnchor; ++k) {
    if (mode[k] != MUXGL_ANCHOR_PRIOR) continue;
    int64_t ng = 0, nc = 0;
    double sw = 0, sq = 0;
    for (int64_t s = 0; s < S; ++s) {
      if (!has_gp[s]) continue;
      const double* pr = &gp[((size_t)s * V + k) * 3];
      const double* q = &post[((size_t)s * nAnchor + k) * 3];
      ++ng;
      nc += argmax3(pr) != argmax3(q);
      sw += std::max(pr[0], std::max(pr[1], pr[2]));
      sq += std::max(q[0], std::max(q[1], q[2]));
    }
    if (ng) w.printf("%d\t%s\t%lld\t%lld\t%.4lf\t%.4lf\n", (int)k, donor((int)k).c_str(), (long long)ng, (long long)nc, sw / ng, sq / ng);
    else w.printf("%d\t%s\t0\t0\tNA\tNA\n", (int)k, donor((int)k).c_str());
  }
  w.close();
}

// The final cluster pileups against the donors (muxgl_fmx_match_donors): ll [K][V], ll0 and nsnps [K]
struct DonorMatch {
  size_t K, V;
  const double *ll, *ll0;
  const int32_t* nsnps;
  double llr(size_t k, size_t v) const {
    const double d = ll[k * V + v] - ll0[k];
    return std::isnan(d) ? -INFINITY : d;  // (-inf against -inf: no evidence for that donor either)
  }
};

// .clust1.match.gz: one row per cluster and donor
inline void write_match(OutFile&& w, const DonorMatch& m, const Label& donor) {
  w.printf("CLUST\tSM_ID\tNUM.SNPS\tLLK\tLLK0\tLLR\tPOSTPRB\n");
  for (size_t k = 0; k < m.K; ++k) {
    const double* row = m.ll + k * m.V;
    double mx = row[0], sum = 0.0;
    for (size_t v = 1; v < m.V; ++v) mx = std::max(mx, row[v]);
    if (std::isinf(mx)) mx = 0.0;  // (every donor at -inf)
    for (size_t v = 0; v < m.V; ++v) sum += exp(row[v] - mx);
    for (size_t v = 0; v < m.V; ++v)
      w.printf("%d\t%s\t%d\t%.4lf\t%.4lf\t%.4lf\t%.3lg\n", (int)k, donor((int)v).c_str(), m.nsnps[k], row[v], m.ll0[k], m.llr(k, v),
               sum > 0.0 ? exp(row[v] - mx) / sum : 1.0 / (double)m.V);
  }
  w.close();
}

// .clust1.match.best.gz: one row per cluster -- its best and next donor (ties: the lower donor), and whether it is the
// best cluster of its best donor (ties: the lower cluster)
inline void write_match_best(OutFile&& w, const DonorMatch& m, const Label& donor) {
  std::vector<int> best(m.K, -1), next(m.K, -1), bestClust(m.V, -1);
  for (size_t k = 0; k < m.K; ++k) {
    if (m.nsnps[k] == 0) continue;
    for (size_t v = 0; v < m.V; ++v) {
      if (best[k] < 0 || m.llr(k, v) > m.llr(k, (size_t)best[k])) {
        next[k] = best[k];
        best[k] = (int)v;
      } else if (next[k] < 0 || m.llr(k, v) > m.llr(k, (size_t)next[k])) {
        next[k] = (int)v;
      }
    }
    for (size_t v = 0; v < m.V; ++v)
      if (bestClust[v] < 0 || m.llr(k, v) > m.llr((size_t)bestClust[v], v)) bestClust[v] = (int)k;
  }
  w.printf("CLUST\tNUM.SNPS\tBEST.SM_ID\tBEST.LLR\tNEXT.SM_ID\tNEXT.LLR\tDIFF.LLR\tRECIPROCAL\n");
  for (size_t k = 0; k < m.K; ++k) {
    w.printf("%d\t%d\t", (int)k, m.nsnps[k]);
    if (best[k] < 0) {
      w.printf("NA\tNA\tNA\tNA\tNA\tNA\n");
      continue;
    }
    w.printf("%s\t%.4lf\t", donor(best[k]).c_str(), m.llr(k, (size_t)best[k]));
    if (next[k] < 0) w.printf("NA\tNA\tNA\t");
    else
      w.printf("%s\t%.4lf\t%.4lf\t", donor(next[k]).c_str(), m.llr(k, (size_t)next[k]),
               m.llr(k, (size_t)best[k]) - m.llr(k, (size_t)next[k]));
    w.printf("%d\n", bestClust[(size_t)best[k]] == (int)k ? 1 : 0);
  }
  w.close();
}

// .clust1.ldist.gz: the final cluster pileups against each other (muxgl_fmx_cluster_pairs), the row of the reference's
// .ldist.gz (cmd_cram_freemuxlet.cpp:268) without its read-count columns, one row per pair a > b in ascending (a, b) order
inline void write_cluster_ldist(OutFile&& w, size_t K, const double* l2, const double* l0, const int32_t* ns /* each [K (K - 1) / 2] */) {
  w.printf("ID1\tID2\tNSNP\tLLK0\tLLK2\tLDIFF\tDIFF.SNP\n");
  for (size_t a = 1, i = 0; a < K; ++a)
    for (size_t b = 0; b < a; ++b, ++i)
      w.printf("%d\t%d\t%d\t%.2lf\t%.2lf\t%.2lf\t%.4lf\n", (int)a, (int)b, ns[i], l0[i], l2[i], l2[i] - l0[i],
               (l2[i] - l0[i]) / (ns[i] + 1e-6));
  w.close();
}

// ---- the cluster VCFs ----
// old_clust0: the .clust0.vcf.gz of freemuxlet-old (cmd_cram_freemuxlet.cpp:377-431) differs from every other cluster
// VCF in two expressions: pps = gps * gls / maxGL (:409-411) and gq = (int)(-0.1*log10(..)) (:421)
inline void write_cluster_vcf(const std::string& path, const Pileup& p, int K, const double* gls /* [K][S][9] */,
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

}  // namespace pa
