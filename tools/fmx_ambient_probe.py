"""Time and device memory of muxgl_fmx_ambient (fmx_ambient.hip), beside muxgl_fmx_singlets and muxgl_fmx_unknown on the
same handle.

    python tools/fmx_ambient_probe.py [--cases a,b,...] [--repeats N] [--rhos x,y,...] [--out profiles/fmx_ambient_probe.jsonl]

One JSON line per shape (the shapes of tools/fmx_unknown_probe.py).  Every shape runs in a child process of its own
under `timeout`, one after the other, and the probe stops at the first child that fails: nothing is started on a device
another step has just left in doubt.

Per shape, after two EM iterations from a greedy start (spread clusters beyond 64), with the ambient profile made of the
pileup's own read counts (Engine.pileup_allele_counts, muxgl.ambient_profile) and the front end's default grid of eight
rhos: kernel_ms = the call's own event time (weights + sweep + emit of every batch) of `repeats` calls after one untimed
call, as median / min / max; wall_ms = host clock around the whole call, its copy of the table to the host included,
median; batches = the batches of whole cells the call's plan makes at the device's budget (table_plan.hpp restated:
fmx_ambient_bytes per cell, cells taken while they fit); mem_gb = device memory in use after the calls minus before the
handle (the handle's cache keeps every block, so this is the high-water mark); singlets_kernel_ms = muxgl_fmx_singlets
(MUXGL_T_FMX_SINGLETS) and unknown_kernel_ms = muxgl_fmx_unknown (its own event time) on the same handle, medians, with
singlet_calls = kernel_ms / singlets_kernel_ms and unknown_calls = kernel_ms / unknown_kernel_ms; bytes: weights_gb = nnz x
n_rho x 24 (written once, read once per 64-cluster block), reads_gb = the read bytes (walked once per pass of the weight
kernel), row_bytes_gb = nnz x K x 24 x ceil(n_rho / 4) (every posterior row once per entry and chunk of rhos), table_gb =
C x K x n_rho x 8.
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

DEFAULT_RHOS = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)
PART = 2048
# name: (config index | None, scale, C, S, K, mean_entries, child timeout in seconds)
CASES = {
    "configs3": (3, 1.0, None, None, None, None, 600),          # 50 k cells, K = 16
    "configs4_tenth": (4, 0.1, None, None, None, None, 600),    # configs[4]'s S, K = 64 and density, a tenth of its cells
    "c2000_K256": (None, None, 2000, 20000, 256, 150, 300),
    "c2000_K512": (None, None, 2000, 20000, 512, 150, 300),
    "c1000_K1024": (None, None, 1000, 20000, 1024, 150, 300),
}


def mem_info():
    import torch

    fr, tot = torch.cuda.mem_get_info(0)
    return tot - fr, tot


def batches_of(cell_ptr, n_rho, K, budget):
    """table_plan::plan with table_plan::fmx_ambient_bytes: the number of batches of whole cells"""
    lens = np.diff(cell_ptr)
    parts = np.maximum(1, -(-lens // PART))
    row = 8 * n_rho * K
    cost = lens * n_rho * 24 + parts * (row + 24) + row + 16
    n, used = 0, None
    for w in cost.tolist():
        if used is None or used + w > budget:
            n, used = n + 1, 0
        used += w
    return n


def run_case(name, repeats, rhos):
    from popscle_amd import muxgl, synth

    cfg, scale, C, S, K, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg, scale, with_gp=False)
        K = synth.CONFIGS[cfg]["V"]
    else:
        p = synth.make_pileup(C, S, 16, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment,
                              with_gp=False)
    base, total = mem_info()
    env_mb = int(os.environ.get("MUXGL_FMX_SLAB_MB", "0") or 0)
    budget = env_mb << 20 if env_mb > 0 else min(4 << 30, total // 3)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        f = muxgl.ambient_profile(*e.pileup_allele_counts(), p.af)
        init = e.fmx_greedy_init(K, llk2 - llk0) if K <= 64 else ((np.arange(p.C) * 7) % K).astype(np.int32)
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        e.fmx_ambient(f, rhos)
        kern, wall = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            amb = e.fmx_ambient(f, rhos)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(amb["kernel_ms"])
        peak = mem_info()[0] - base
        e.fmx_singlets()
        sk = []
        for _ in range(repeats):
            e.fmx_singlets()
            sk.append(float(e.timing()[muxgl.T_FMX_SINGLETS]))
        e.fmx_unknown()
        uk = [e.fmx_unknown()["kernel_ms"] for _ in range(repeats)]
    NR = len(rhos)
    med, smed, umed = float(np.median(kern)), float(np.median(sk)), float(np.median(uk))
    r = dict(case=name, C=int(p.C), S=int(p.S), K=int(K), nnz=int(p.nnz), n_rho=NR, repeats=repeats,
             kernel_ms=round(med, 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4),
             wall_ms=round(float(np.median(wall)), 3), batches=batches_of(p.cell_ptr, NR, K, budget),
             mem_gb=round(peak / 1e9, 3), singlets_kernel_ms=round(smed, 4), unknown_kernel_ms=round(umed, 4),
             singlet_calls=round(med / smed, 3) if smed > 0 else None, unknown_calls=round(med / umed, 3) if umed > 0 else None,
             weights_gb=round(p.nnz * NR * 24 / 1e9, 3), reads_gb=round(p.reads.size / 1e9, 3),
             row_bytes_gb=round(p.nnz * K * 24 * (-(-NR // 4)) / 1e9, 3), table_gb=round(p.C * K * NR * 8 / 1e9, 4))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rhos", default=",".join(repr(x) for x in DEFAULT_RHOS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_ambient_probe.jsonl"))
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.repeats, tuple(float(x) for x in a.rhos.split(",")))
        return 0
    lines = []
    for name in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][6]), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--repeats", str(a.repeats), "--rhos", a.rhos], capture_output=True, text=True)
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
