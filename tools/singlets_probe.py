"""Time and device memory of muxgl_demux_singlets (demux_singlets.hip), beside muxgl_demux_run of the same job.

    python tools/singlets_probe.py [--cases a,b,...] [--repeats N] [--full-ll-max-gb G] [--out profiles/singlets_probe.jsonl]

One JSON line per shape.  Every shape runs in a child process of its own under `timeout`, one after the other, and the
probe stops at the first child that fails: nothing is started on a device another step has just left in doubt.

Per shape: kernel_ms = MUXGL_T_DEMUX_SINGLETS (hipEvents around weights + sweep) of `repeats` calls after one untimed call,
as median / min / max; wall_ms = host clock around the whole call (its copy of the table to the host included), median;
run_kernel_ms / run_wall_ms = muxgl_demux_run on the same handle (sweep + call slots; wall), median; mem_gb = device
memory in use after the calls minus before the handle (the handle's cache keeps every block, so this is the high-water
mark); roof_frac = nnz x V x 24 bytes (every genotype row once per entry) / kernel time / 8 TB/s, the HBM roof of
DESIGN.md 4.1.  Where the [C][V][V][A] tensor is at most --full-ll-max-gb, full_ll_wall_ms = muxgl_demux_run with full_ll
and its copy to the host: the only way to get these numbers without the call.
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

G2 = (0.0, 0.5)
G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
HBM_ROOF = 8e12  # bytes / s

# name: (config index | None, C, S, V, alphas, mean_entries, child timeout in seconds)
CASES = {
    "configs1": (1, None, None, None, None, None, 300),
    "configs2": (2, None, None, None, None, None, 900),
    "c2000_V255": (None, 2000, 20000, 255, G2, 150, 300),
    "c2000_V512": (None, 2000, 20000, 512, G2, 150, 300),
    "c1000_V1024": (None, 1000, 20000, 1024, G2, 150, 300),
    "c10000_V8": (None, 10000, 50000, 8, G2, 800, 300),
}


def used_bytes():
    import torch

    fr, tot = torch.cuda.mem_get_info(0)
    return tot - fr


def run_case(name, repeats, full_ll_max_gb):
    from popscle_amd import muxgl, synth

    cfg, C, S, V, alphas, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg)
        alphas = synth.CONFIGS[cfg].get("alphas", G2)
        V = p.gp.shape[1]
    else:
        p = synth.make_pileup(C, S, V, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment)
    base = used_bytes()
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        e.demux_singlets(alphas)
        kern, wall = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            sng = e.demux_singlets(alphas)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(float(e.timing()[muxgl.T_DEMUX_SINGLETS]))
        peak_singlets = used_bytes() - base
        e.demux_run(alphas, 0.5, want_cells=False)
        rk, rw = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            e.demux_run(alphas, 0.5, want_cells=False)
            rw.append((time.perf_counter() - t0) * 1e3)
            ms = e.timing()
            rk.append(float(ms[muxgl.T_DEMUX_REDUCE] + ms[muxgl.T_DEMUX_SWEEP] + ms[muxgl.T_DEMUX_CALL]))
        tensor_gb = p.C * V * V * len(alphas) * 8 / 1e9
        full_ms, full_dev = None, None
        if V <= 255 and tensor_gb <= full_ll_max_gb:
            t0 = time.perf_counter()
            _, full = e.demux_run(alphas, 0.5, want_cells=False, want_full_ll=True)
            full_ms = (time.perf_counter() - t0) * 1e3
            full_dev = float(np.max(np.abs(full[:, :, 0, 0] - sng)))
            del full
    k = float(np.median(kern))
    r = dict(case=name, C=int(p.C), S=int(p.S), V=int(V), alphas=list(alphas), nnz=int(p.nnz), repeats=repeats,
             kernel_ms=round(k, 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4),
             wall_ms=round(float(np.median(wall)), 3), run_kernel_ms=round(float(np.median(rk)), 4),
             run_wall_ms=round(float(np.median(rw)), 3), mem_gb=round(peak_singlets / 1e9, 3),
             table_gb=round(p.C * V * 8 / 1e9, 4), tensor_gb=round(tensor_gb, 2),
             row_bytes_gb=round(p.nnz * V * 24 / 1e9, 3), roof_frac=round(p.nnz * V * 24.0 / (k * 1e-3) / HBM_ROOF, 4),
             full_ll_wall_ms=None if full_ms is None else round(full_ms, 1),
             max_abs_diff_vs_full_ll=full_dev)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--full-ll-max-gb", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "singlets_probe.jsonl"))
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
