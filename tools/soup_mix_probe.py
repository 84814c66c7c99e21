"""Time of muxgl_demux_soup_mix and muxgl_pileup_read_hist (soup_mix.hip) at the panels of the benchmark's shapes.

    python tools/soup_mix_probe.py [--cases a,b,...] [--repeats N] [--out profiles/soup_mix_probe.jsonl]

One JSON line per shape, appended to --out.  Every shape runs in a child process of its own under `timeout`, one after
the other, and the probe stops at the first child that fails: nothing is started on a device another step has just left in
doubt.

The shapes are the panels (S markers x V samples) of configs[1], configs[2] and of 2 000 x 255 / 512 and 1 000 x 1024 of
tools/ambient_probe.py.  The soup is read from nearly empty droplets only, so the pileup of a shape holds nothing else:
min(C, 20 000) droplets of about 25 entries, of which those with at most 40 reads are taken (the mask of
--ambient-max-reads 40).  Per shape:
  hist_wall_ms      muxgl_pileup_read_hist under that mask, host clock, median (the call has no event time of its own)
  records, n_reads, active   the histogram's records, the reads that take part and the active markers
  iter_kernel_ms    the event time of a call with tol = 0 and 50 steps over its 51 evaluations (three kernels each and the
                    16-byte read-back behind them), median over the repeats
  roof_frac         the panel bytes of an evaluation, 2 x 24 x active x M, over iter_kernel_ms, as a fraction of 8 TB/s
  steps_to_tol, status, fit_wall_ms   a fit from uniform shares to tol = 1e-8 (at most 5 000 steps), and its wall time
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (config or None, droplets, S, V, time limit of the child in seconds)
CASES = {
    "configs1": (1, None, None, None, 300),
    "configs2": (2, None, None, None, 600),
    "c2000_V255": (None, 2000, 20000, 255, 300),
    "c2000_V512": (None, 2000, 20000, 512, 300),
    "c1000_V1024": (None, 1000, 20000, 1024, 300),
}
MAX_READS, EVAL_STEPS, MAX_DROPLETS, ROOF = 40, 50, 20000, 8e12


def run_case(name, repeats):
    from popscle_amd import muxgl, synth

    cfg, C, S, V, _ = CASES[name]
    if cfg is not None:
        c = synth.CONFIGS[cfg]
        C, S, V = c["C"], c["S"], c["V"]
    C = min(C, MAX_DROPLETS)
    p = synth.make_pileup(C, S, V, seed=11, mean_entries=25, min_entries=5, max_entries=40, doublet_frac=0.0)
    mask = np.diff(p.entry_rptr[p.cell_ptr]) <= MAX_READS
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        e.pileup_read_hist(mask)
        hw = []
        for _ in range(repeats):
            t = time.perf_counter()
            hist = e.pileup_read_hist(mask)
            hw.append((time.perf_counter() - t) * 1e3)
        e.demux_soup_mix(hist=hist, n_iter_max=EVAL_STEPS, tol=0.0, want=("pi",))
        km = []
        for _ in range(repeats):
            r = e.demux_soup_mix(hist=hist, n_iter_max=EVAL_STEPS, tol=0.0, want=("pi",))
            km.append(r["kernel_ms"] / (EVAL_STEPS + 1))
        t = time.perf_counter()
        fit = e.demux_soup_mix(hist=hist, n_iter_max=5000, tol=1e-8, want=("pi", "grad"))
        fit_wall = (time.perf_counter() - t) * 1e3
    active = int(np.count_nonzero(p.has_gp[np.unique(hist[0] >> 8)]))
    it = float(np.median(km))
    out = dict(case=name, droplets=int(p.C), masked=int(mask.sum()), S=int(p.S), V=int(V), M=int(V), repeats=repeats,
               hist_wall_ms=round(float(np.median(hw)), 3), records=int(hist[0].size), n_reads=int(r["n_reads"]), active=active,
               iter_kernel_ms=round(it, 5), iter_kernel_ms_min=round(min(km), 5), iter_kernel_ms_max=round(max(km), 5),
               panel_mb=round(24.0 * p.S * V / 1e6, 1), roof_frac=round(2 * 24.0 * active * V / (it * 1e-3) / ROOF, 4),
               steps_to_tol=int(fit["n_iter"]), status=int(fit["status"]), fit_wall_ms=round(fit_wall, 2),
               max_grad_dev=float(muxgl.soup_mix_summary(dict(fit, ll=np.zeros(1)))["max_grad_dev"]))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soup_mix_probe.jsonl"))
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.repeats)
        return 0
    done = 0
    for name in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][4]), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--repeats", str(a.repeats)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        done += 1
    return 0 if done == len(a.cases.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
