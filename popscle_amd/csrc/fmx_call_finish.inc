// fmx_call_finish.inc -- the freemuxlet re-assignment after the scans (cmd_cram_freemux2.cpp:515-584), included as the
// tail of both freemuxlet call kernels: fmx_call_kernel (fmx_kernels.hip), which scans the [C][K(K+1)/2] table, and the
// streamed E-step's call (fmx_stream.hip), which keeps only the scan results per cell.  A fragment, not a function: the
// kernel of fmx_kernels.hip must keep its machine code (its family is fingerprinted in profiles/traffic.json), and an
// inlined call is optimised in another order.  In scope at the include: i (the cell), log_single_prior,
// log_double_prior, the scan results sBest, sNext, dBest1, dBest2, dNext1, dNext2, sngBestLLK, sngNextLLK, dblBestLLK,
// dblNextLLK, sngThird, dblThird (a settled cell's table entry overwrites some of them), the sums sumLLK, sngLLK, the
// kernel arguments cells, clust, stat, prev_state, flagged, xc_epoch, xc, epoch, and the constant FMX_WIDE_PREV (the
// packing of prev_state: fmx_pack_prev, fmx_call_body.hpp).
  // (round 6) A decision whose margin is within rounding reach of the kernels' numbers -- best / next of a scan, next /
  // third, one of the four +2 thresholds -- is not this kernel's to make: the cell goes on the list fmx_exact.hip settles
  // in the reference's own arithmetic.  What that needs of the state BEFORE this iteration is kept aside (the previous
  // (type, jBest, kBest) of the nchanged rules below; the assignments the cluster pileups were built from: the launcher).
  // A cell settled in an earlier iteration whose inputs have not changed since (no assignment changed anywhere: same
  // `epoch`) takes the exact scan results from the table instead of being listed again: a converged job pays nothing.
  bool listed = false;
  double sngBestDev = -1e300;  // the kernels' own value where the table overrides it (sngOnlyPP stays what a listed cell keeps)
  bool from_table = false;
  if (prev_state) {
    double mag = 1.0;
    if (sngBestLLK > -1e299) mag = fmax(mag, fabs(sngBestLLK));
    if (dblBestLLK > -1e299) mag = fmax(mag, fabs(dblBestLLK));
    if (sngNextLLK > -1e299) mag = fmax(mag, fabs(sngNextLLK));
    if (dblNextLLK > -1e299) mag = fmax(mag, fabs(dblNextLLK));
    const double eps = 1e-9 * mag;
    auto near = [eps](double a, double b) { return a > -1e299 && b > -1e299 && fabs(a - b) <= eps; };
    if (near(sngBestLLK, sngNextLLK) || near(sngNextLLK, sngThird) || near(dblBestLLK, dblNextLLK) ||
        near(dblNextLLK, dblThird) || near(dblBestLLK, sngBestLLK + 2) || near(dblNextLLK, sngBestLLK + 2) ||
        near(sngBestLLK, sngNextLLK + 2) || near(dblBestLLK, sngNextLLK + 2)) {
      if (xc_epoch && xc_epoch[i] == epoch) {
        const fmx_xc e = xc[i];
        sngBestDev = sngBestLLK;
        from_table = true;
        sBest = e.sBest, sNext = e.sNext, dBest1 = e.dBest1, dBest2 = e.dBest2, dNext1 = e.dNext1, dNext2 = e.dNext2;
        sngBestLLK = e.sngBestLLK, sngNextLLK = e.sngNextLLK, dblBestLLK = e.dblBestLLK, dblNextLLK = e.dblNextLLK;
      } else {
        listed = true;
      }
    }
  }
  muxgl_fmx_cell c = cells[i];
  const int32_t prev_type = c.type, prev_j = c.jBest, prev_k = c.kBest;
  c.sBest = sBest;
  c.sngBestLLK = sngBestLLK;
  c.sNext = sNext;
  c.sngNextLLK = sngNextLLK;
  c.dBest1 = dBest1;
  c.dBest2 = dBest2;
  c.dblBestLLK = dblBestLLK;
  c.dNext1 = dNext1;
  c.dNext2 = dNext2;
  c.dblNextLLK = dblNextLLK;
  c.sngPP = exp(sngLLK - sumLLK);
  c.sngOnlyPP = exp((from_table ? sngBestDev : sngBestLLK) + log_single_prior - sngLLK);
  c.sumLLK = sumLLK;
  c.sngThirdLLK = sngThird;
  c.dblThirdLLK = dblThird;

  int32_t dsingle = 0, damb = 0, dchanged = 0;
  c.clust = -1;                           // :520
  if (dblBestLLK > sngBestLLK + 2) {      // :521
    if (c.type != 1) dchanged = 1;
    c.type = 1;
    c.bestPP = (dblBestLLK + log_double_prior - sumLLK);
    c.jBest = dBest1;
    c.kBest = dBest2;
    c.bestLLK = dblBestLLK;
    if (dblNextLLK > sngBestLLK + 2) {
      c.jNext = dNext1;
      c.kNext = dNext2;
      c.nextLLK = dblNextLLK;
    } else {
      c.jNext = c.kNext = sBest;
      c.nextLLK = sngBestLLK;
    }
  } else if (sngBestLLK > sngNextLLK + 2) {  // :542
    if ((c.type != 0) || (c.jBest != sBest) || (c.kBest != sBest)) dchanged = 1;
    c.type = 0;
    dsingle = 1;
    c.bestPP = (sngBestLLK + log_single_prior - sumLLK);
    c.jBest = c.kBest = sBest;
    c.bestLLK = sngBestLLK;
    c.clust = sBest;
    if (dblBestLLK > sngNextLLK + 2) {
      c.jNext = dBest1;
      c.kNext = dBest2;
      c.nextLLK = dblBestLLK;
    } else {
      c.jNext = c.kNext = sNext;
      c.nextLLK = sngNextLLK;
    }
  } else {  // :565
    if (c.type != 2) dchanged = 1;
    c.type = 2;
    damb = 1;
    c.bestPP = (sngBestLLK + log_single_prior - sumLLK);
    c.jBest = c.kBest = sBest;
    c.bestLLK = sngBestLLK;
    if (dblBestLLK > sngNextLLK + 2) {
      c.jNext = dBest1;
      c.kNext = dBest2;
      c.nextLLK = dblNextLLK;  // sic, :577
    } else {
      c.jNext = c.kNext = sNext;
      c.nextLLK = sngNextLLK;
    }
  }
  if (prev_state) prev_state[i] = fmx_pack_prev<FMX_WIDE_PREV>(prev_type, prev_j, prev_k);
  if (listed) flagged[atomicAdd(&stat[3], 1)] = (int32_t)i;
  cells[i] = c;
  clust[i] = c.clust;
  if (dsingle) atomicAdd(&stat[0], 1);
  if (damb) atomicAdd(&stat[1], 1);
  if (dchanged) atomicAdd(&stat[2], 1);
