#!/usr/bin/env python3
"""Times muxgl_fmx_inclusion (fmx_incl.hip) on one device, after two EM iterations from a greedy start (spread clusters
beyond 64): kernel ms (MUXGL_T_FMX_INCLUSION) and wall ms including the copies to the host -- the median of seven calls
after one untimed call -- the MUXGL_T_FMX_ESTEP of the same iteration, and the device memory high-water of the call.  Where
full_ll exists (K <= 255) it also times the only other route to these tables: muxgl_fmx_iterate(full_ll) minus the same
iteration without it (the host reduction of that table would come on top, so the figure is a lower bound of that route).
Each shape runs in a child process under a time limit of its own; one JSON line per shape goes to
profiles/fmx_inclusion_probe.jsonl (the lines of the shapes run now replace those of the same shapes).

  tools/fmx_inclusion_probe.py
  tools/fmx_inclusion_probe.py --cases c2000_K255,configs3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (config index | None, scale, C, S, K, mean_entries, child timeout in seconds)
CASES = {
    "configs3": (3, 1.0, None, None, None, None, 600),          # 50 k cells, K = 16
    "c2000_K255": (None, None, 2000, 20000, 255, 150, 300),     # the widest job that still has full_ll
    "c2000_K256": (None, None, 2000, 20000, 256, 150, 300),
    "c2000_K512": (None, None, 2000, 20000, 512, 150, 300),
    "c1000_K1024": (None, None, 1000, 20000, 1024, 150, 300),
}


def run_case(name, repeats, full_ll_max_gb):
    import torch

    from popscle_amd import muxgl, synth

    cfg, scale, C, S, K, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg, scale, with_gp=False)
        K = synth.CONFIGS[cfg]["V"]
    else:
        p = synth.make_pileup(C, S, 16, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment,
                              with_gp=False)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        init = e.fmx_greedy_init(K, llk2 - llk0) if K <= 64 else ((np.arange(p.C) * 7) % K).astype(np.int32)
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        t0 = time.perf_counter()
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        iterate_wall = (time.perf_counter() - t0) * 1e3
        estep = float(e.timing()[muxgl.T_FMX_ESTEP])
        torch.cuda.synchronize()
        free0, total = torch.cuda.mem_get_info()
        e.fmx_inclusion(0.5)  # untimed
        kern, wall = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            e.fmx_inclusion(0.5)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(float(e.timing()[muxgl.T_FMX_INCLUSION]))
        free1, _ = torch.cuda.mem_get_info()   # the handle's cache keeps the call's blocks: the high-water of the call
        npairs = K * (K + 1) // 2
        tensor_gb = p.C * npairs * 8 / 1e9
        route = None
        if K <= 255 and tensor_gb <= full_ll_max_gb:
            with_full, without = [], []
            for _ in range(3):   # the same iteration (same clusters, second E-step) with and without the table
                for want, acc in ((False, without), (True, with_full)):
                    e.fmx_set_clusters(K, init)
                    e.fmx_iterate(0.5, 0.1, want_cells=False)
                    t0 = time.perf_counter()
                    e.fmx_iterate(0.5, 0.1, want_cells=False, want_full_ll=want)
                    acc.append((time.perf_counter() - t0) * 1e3)
            route = statistics.median(with_full) - statistics.median(without)
    r = dict(case=name, C=int(p.C), S=int(p.S), K=int(K), nnz=int(p.nnz), repeats=repeats,
             kernel_ms=round(statistics.median(kern), 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4),
             wall_ms=round(statistics.median(wall), 3), estep_ms=round(estep, 4), iterate_wall_ms=round(iterate_wall, 3),
             device_bytes_call=int(free0 - free1), device_bytes_inputs=int(total - free0),
             tables_gb=round(p.C * K * 20 / 1e9, 4), tensor_gb=round(tensor_gb, 2),
             full_ll_route_wall_ms=None if route is None else round(route, 1))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--full-ll-max-gb", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_inclusion_probe.jsonl"))
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.repeats, a.full_ll_max_gb)
        return 0
    lines = []
    for name in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][6]), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--repeats", str(a.repeats), "--full-ll-max-gb", str(a.full_ll_max_gb)],
                           capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if lines:  # the lines of the shapes run now replace those of the same shapes in an existing file
        done = {json.loads(ln)["case"] for ln in lines}
        kept = []
        if os.path.exists(a.out):
            kept = [ln for ln in open(a.out).read().splitlines() if ln.strip() and json.loads(ln)["case"] not in done]
        rank = {name: i for i, name in enumerate(CASES)}
        allc = sorted(kept + lines, key=lambda ln: rank.get(json.loads(ln)["case"], len(rank)))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(allc) + "\n")
    return 0 if len(lines) == len(a.cases.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
