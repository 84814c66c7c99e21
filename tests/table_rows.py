"""The rows of the front end's per-droplet fit tables, restated from the column rules in the comment at the top of
popscle_amd/host/main.cpp: what the *_cli_gpu.py tests hold a run's files to, and what test_table_writers.py holds the
writers of popscle_amd/host/table_writers.hpp to without a device.

`printed` is the row list: (droplet index, [BARCODE, NUM.SNPS, NUM.READS] as printed) in the order of the file; `label`
turns a column index into its text (a sample id, or the cluster's number).  `fit` holds [C][2] arrays under the names of
the Engine's dicts; `sm` the se and lrt of muxgl.ambient_fit_summary / muxgl.alpha_fit_summary."""
import math


def number(v, have=True):
    """%.4lf, or NA"""
    return "%.4f" % v if have else "NA"


def ambient_fit_rows(printed, label, cand, fit, sm):
    """.ambfit.gz: a row per candidate that is not -1; AMB.RHO.SE is NA where se is NaN, AMB.LRT where lrt is not finite"""
    rows = []
    for i, head in printed:
        for k in range(2):
            if cand[i][k] < 0:
                continue
            se, lrt = float(sm["se"][i][k]), float(sm["lrt"][i][k])
            rows.append("\t".join(list(head) + [label(int(cand[i][k])), number(fit["ll_zero"][i][k]), number(fit["rho_hat"][i][k]),
                                                number(se, not math.isnan(se)), number(fit["ll_hat"][i][k]),
                                                number(lrt, math.isfinite(lrt)), "%d" % fit["status"][i][k]]))
    return rows


def alpha_fit_rows(printed, label, fit, sm):
    """.alphafit.gz: a row DBL and a row SNG per droplet, none where the pair is (-1, -1); SNG2.LLK is NA where the fit's
    interval is not the whole [0, 1]"""
    whole = fit["alpha_max"] == 1.0
    rows = []
    for i, head in printed:
        for k in range(2):
            j1, j2 = (int(v) for v in fit["pair"][i][k])
            if j1 < 0:
                continue
            se, lrt = float(sm["se"][i][k]), float(sm["lrt"][i][k])
            rows.append("\t".join(list(head) + [("DBL", "SNG")[k], label(j1), label(j2), number(fit["ll_zero"][i][k]),
                                                number(fit["ll_top"][i][k], whole), number(fit["alpha_hat"][i][k]),
                                                number(se, not math.isnan(se)), number(fit["ll_hat"][i][k]),
                                                number(lrt, math.isfinite(lrt)), "%d" % fit["status"][i][k]]))
    return rows
