"""Time and device memory of muxgl_fmx_unknown (fmx_unknown.hip), beside muxgl_fmx_singlets and the E-step of the same
handle and, where it is accepted, the only earlier route to the same numbers.

    python tools/fmx_unknown_probe.py [--cases a,b,...] [--repeats N] [--full-ll-max-gb G] [--out profiles/fmx_unknown_probe.jsonl]

One JSON line per shape (the shapes of tools/fmx_singlets_probe.py).  Every shape runs in a child process of its own
under `timeout`, one after the other, and the probe stops at the first child that fails: nothing is started on a device
another step has just left in doubt.

Per shape, after two EM iterations from a greedy start (spread clusters beyond 64): kernel_ms = the call's own event time
(prior + weights + both sweeps + join + split of every batch) of `repeats` calls after one untimed call, as median / min
/ max; wall_ms = host clock around the whole call, its copies of the three tables to the host included, median;
singlets_kernel_ms / singlets_wall_ms = muxgl_fmx_singlets on the same handle (MUXGL_T_FMX_SINGLETS), median;
singlet_calls = kernel_ms / singlets_kernel_ms, to hold against the expectation of one singlet sweep plus one pass over
the entry likelihoods (1.2 to 1.7); estep_ms = MUXGL_T_FMX_ESTEP of the iteration before; mem_gb = device memory in use
after the calls minus before the handle (the handle's cache keeps every block, so this is the high-water mark);
bytes: egl_gb = nnz x 72 (the entry likelihoods, read once), weights_gb = nnz x 40 (written once, read by both sweeps),
row_bytes_gb = nnz x K x 24 (every posterior row once per entry).  Where K + 2 <= 255 and the [C][(K + 2)(K + 3) / 2]
tensor is at most --full-ll-max-gb, old_route_wall_ms = a second handle with K + 2 clusters, two of them empty, started
from the assignments the second iteration's posteriors were made of: muxgl_fmx_set_clusters and one muxgl_fmx_iterate
with full_ll and its copy to the host, and max_abs_diff_vs_old_route the largest difference of the three tables to its
slots.
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

# name: (config index | None, scale, C, S, K, mean_entries, child timeout in seconds)
CASES = {
    "configs3": (3, 1.0, None, None, None, None, 600),          # 50 k cells, K = 16
    "configs4_tenth": (4, 0.1, None, None, None, None, 600),    # configs[4]'s S, K = 64 and density, a tenth of its cells
    "c2000_K256": (None, None, 2000, 20000, 256, 150, 300),
    "c2000_K512": (None, None, 2000, 20000, 512, 150, 300),
    "c1000_K1024": (None, None, 1000, 20000, 1024, 150, 300),
}


def used_bytes():
    import torch

    fr, tot = torch.cuda.mem_get_info(0)
    return tot - fr


def run_case(name, repeats, full_ll_max_gb):
    from popscle_amd import muxgl, synth

    cfg, scale, C, S, K, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg, scale, with_gp=False)
        K = synth.CONFIGS[cfg]["V"]
    else:
        p = synth.make_pileup(C, S, 16, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment,
                              with_gp=False)
    base = used_bytes()
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        init = e.fmx_greedy_init(K, llk2 - llk0) if K <= 64 else ((np.arange(p.C) * 7) % K).astype(np.int32)
        e.fmx_set_clusters(K, init)
        cells1, _ = e.fmx_iterate(0.5, 0.1)
        clust1 = cells1["clust"].copy()   # what the second iteration's posteriors are made of
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        estep = float(e.timing()[muxgl.T_FMX_ESTEP])
        e.fmx_unknown()
        kern, wall = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            unk = e.fmx_unknown()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(unk["kernel_ms"])
        peak = used_bytes() - base
        e.fmx_singlets()
        sk, sw = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            e.fmx_singlets()
            sw.append((time.perf_counter() - t0) * 1e3)
            sk.append(float(e.timing()[muxgl.T_FMX_SINGLETS]))
    K2 = K + 2
    tensor_gb = p.C * (K2 * (K2 + 1) // 2) * 8 / 1e9
    old_ms, old_dev = None, None
    if K2 <= 255 and tensor_gb <= full_ll_max_gb:
        with muxgl.Engine(0) as e:
            e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
            e.fmx_prepare(p.af)
            e.fmx_set_clusters(K2, clust1)
            e.fmx_iterate(0.5, 0.1, want_cells=False)   # (untimed: first launches)
            t0 = time.perf_counter()
            e.fmx_set_clusters(K2, clust1)
            _, _, full = e.fmx_iterate(0.5, 0.1, want_cells=False, want_full_ll=True)
            old_ms = (time.perf_counter() - t0) * 1e3
        rk, rk1 = K * (K + 1) // 2, (K + 1) * (K + 2) // 2
        with np.errstate(invalid="ignore"):
            d = [np.abs(full[:, rk:rk + K] - unk["ll_ju"]), np.abs(full[:, rk + K] - unk["ll_u"]),
                 np.abs(full[:, rk1 + K] - unk["ll_uu"])]
        old_dev = float(max(np.nanmax(x) for x in d))
        del full
    med, smed = float(np.median(kern)), float(np.median(sk))
    r = dict(case=name, C=int(p.C), S=int(p.S), K=int(K), nnz=int(p.nnz), repeats=repeats,
             kernel_ms=round(med, 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4),
             wall_ms=round(float(np.median(wall)), 3), singlets_kernel_ms=round(smed, 4),
             singlets_wall_ms=round(float(np.median(sw)), 3), singlet_calls=round(med / smed, 3) if smed > 0 else None,
             estep_ms=round(estep, 4), mem_gb=round(peak / 1e9, 3), tables_gb=round(p.C * (K + 2) * 8 / 1e9, 4),
             egl_gb=round(p.nnz * 72 / 1e9, 3), weights_gb=round(p.nnz * 40 / 1e9, 3),
             row_bytes_gb=round(p.nnz * K * 24 / 1e9, 3), old_route_tensor_gb=round(tensor_gb, 2),
             old_route_wall_ms=None if old_ms is None else round(old_ms, 1), max_abs_diff_vs_old_route=old_dev)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--full-ll-max-gb", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_unknown_probe.jsonl"))
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
        with open(a.out, "w") as f:
            f.write("\n".join(sorted(kept + lines, key=lambda ln: rank.get(json.loads(ln)["case"], 99))) + "\n")
    return 0 if len(lines) == len(a.cases.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
