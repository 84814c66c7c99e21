#!/usr/bin/env python3
"""Times muxgl_demux_inclusion (demux_incl.hip) on one device: kernel ms (MUXGL_T_DEMUX_INCLUSION), wall ms including
the copies to the host, the kernel ms of muxgl_demux_run on the same handle, and the device memory high-water -- the
median of seven calls after one untimed call.  Up to 255 samples it also times the only other route to these tables,
muxgl_demux_run(full_ll) with the [C][V][V][A] tensor fetched to the host (--full-ll; the host reduction of that tensor
would come on top, so the figure is a lower bound of that route).  One JSON line per shape is appended to
profiles/inclusion_probe.jsonl.

  tools/inclusion_probe.py --shape 2000x255x2 --shape 2000x255x6 --shape 2000x512x2 --shape 1000x1024x2 --full-ll
  tools/inclusion_probe.py --config 1 --config 2
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from popscle_amd import muxgl, synth  # noqa: E402

G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)


def median_ms(f, n=7):
    f()  # untimed
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def probe(name, p, alphas, full_ll):
    import torch

    V = p.gp.shape[1]
    rec = {"shape": name, "C": int(p.C), "V": int(V), "n_alpha": len(alphas), "nnz": int(p.nnz)}
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        free0, total = torch.cuda.mem_get_info()
        kern = []

        def incl():
            e.demux_inclusion(alphas)
            kern.append(float(e.timing()[muxgl.T_DEMUX_INCLUSION]))

        rec["inclusion_wall_ms"] = median_ms(incl)
        rec["inclusion_kernel_ms"] = statistics.median(kern[1:])
        free1, _ = torch.cuda.mem_get_info()   # the handle's cache keeps the call's blocks: the high-water of the call
        rec["device_bytes_call"] = int(free0 - free1)
        rec["device_bytes_inputs"] = int(total - free0)
        runk = []

        def run():
            e.demux_run(alphas, 0.5)
            t = e.timing()
            runk.append(float(t[muxgl.T_DEMUX_SWEEP] + t[muxgl.T_DEMUX_CALL]))

        rec["run_wall_ms"] = median_ms(run)
        rec["run_kernel_ms"] = statistics.median(runk[1:])
        if full_ll and V <= 255 and p.C * V * V * len(alphas) * 8 <= 8 << 30:
            rec["full_ll_route_wall_ms"] = median_ms(lambda: e.demux_run(alphas, 0.5, want_full_ll=True), n=3)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", action="append", default=[], help="CxVxA (A = 2: {0, 0.5}; 6: {0, 0.1 .. 0.5})")
    ap.add_argument("--config", action="append", type=int, default=[], help="BASELINE.json configs[i] (1 or 2)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the cell count of --config")
    ap.add_argument("--mean-entries", type=float, default=150.0)
    ap.add_argument("--full-ll", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inclusion_probe.jsonl"))
    a = ap.parse_args()
    jobs = []
    for i in a.config:
        cfg = synth.CONFIGS[i]
        jobs.append((f"configs[{i}]" + (f" x {a.scale}" if a.scale != 1.0 else ""), synth.make_config(i, a.scale),
                     tuple(cfg.get("alphas", G2))))
    for sh in a.shape:
        Cn, V, A = (int(x) for x in sh.split("x"))
        jobs.append((sh, synth.make_pileup(Cn, 20000, V, seed=11, mean_entries=a.mean_entries, min_entries=20,
                                           missing_gp_frac=0.03), G2 if A == 2 else G6))
    for name, p, alphas in jobs:
        rec = probe(name, p, alphas, a.full_ll)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
