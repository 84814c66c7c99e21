"""Time of muxgl_fmx_singlets (fmx_singlets.hip), beside the E-step of the same iteration and the full_ll route.

    python tools/fmx_singlets_probe.py [--cases a,b,...] [--repeats N] [--full-ll-max-gb G] [--out profiles/fmx_singlets_probe.jsonl]

One JSON line per shape.  Every shape runs in a child process of its own under `timeout`, one after the other, and the
probe stops at the first child that fails: nothing is started on a device another step has just left in doubt.

Per shape, after two EM iterations from a greedy start (spread clusters beyond 64): kernel_ms = MUXGL_T_FMX_SINGLETS of
`repeats` calls after one untimed call, as median / min / max; wall_ms = host clock around the whole call, its copy of
the table to the host included, median;
estep_ms / iter_ms = MUXGL_T_FMX_ESTEP and the sum of the GP, E-step, call and M-step slots of the iteration before;
roof_frac = nnz x K x 24 bytes (every posterior row once per entry) / kernel time / 8 TB/s.  Where full_ll exists
(K <= 255, table at most --full-ll-max-gb) full_ll_wall_ms = muxgl_fmx_iterate(..., full_ll) with its copy to the host,
iterate_wall_ms the same call without it: their difference is what the same numbers cost without muxgl_fmx_singlets.
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

HBM_ROOF = 8e12  # bytes / s

# name: (config index | None, scale, C, S, K, mean_entries, child timeout in seconds)
CASES = {
    "configs3": (3, 1.0, None, None, None, None, 600),          # 50 k cells, K = 16
    "configs4_tenth": (4, 0.1, None, None, None, None, 600),    # configs[4]'s S, K = 64 and density, a tenth of its cells
    "c2000_K256": (None, None, 2000, 20000, 256, 150, 300),
    "c2000_K512": (None, None, 2000, 20000, 512, 150, 300),
    "c1000_K1024": (None, None, 1000, 20000, 1024, 150, 300),
}


def run_case(name, repeats, full_ll_max_gb):
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
        ms = e.timing()
        estep = float(ms[muxgl.T_FMX_ESTEP])
        it_ms = float(ms[muxgl.T_FMX_GP] + ms[muxgl.T_FMX_ESTEP] + ms[muxgl.T_FMX_CALL] + ms[muxgl.T_FMX_MSTEP])
        e.fmx_singlets()
        kern, wall = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            sng = e.fmx_singlets()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(float(e.timing()[muxgl.T_FMX_SINGLETS]))
        npairs = K * (K + 1) // 2
        tensor_gb = p.C * npairs * 8 / 1e9
        full_ms, full_dev = None, None
        if K <= 255 and tensor_gb <= full_ll_max_gb:
            e.fmx_set_clusters(K, init)
            e.fmx_iterate(0.5, 0.1, want_cells=False)
            t0 = time.perf_counter()
            _, _, full = e.fmx_iterate(0.5, 0.1, want_cells=False, want_full_ll=True)
            full_ms = (time.perf_counter() - t0) * 1e3
            j = np.arange(K)
            full_dev = float(np.max(np.abs(full[:, j * (j + 1) // 2 + j] - sng)))
            del full
    med = float(np.median(kern))
    r = dict(case=name, C=int(p.C), S=int(p.S), K=int(K), nnz=int(p.nnz), repeats=repeats,
             kernel_ms=round(med, 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4),
             wall_ms=round(float(np.median(wall)), 3), estep_ms=round(estep, 4), iter_ms=round(it_ms, 4),
             iterate_wall_ms=round(iterate_wall, 3), table_gb=round(p.C * K * 8 / 1e9, 4), tensor_gb=round(tensor_gb, 2),
             row_bytes_gb=round(p.nnz * K * 24 / 1e9, 3), roof_frac=round(p.nnz * K * 24.0 / (med * 1e-3) / HBM_ROOF, 4),
             full_ll_wall_ms=None if full_ms is None else round(full_ms, 1), max_abs_diff_vs_full_ll=full_dev)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--full-ll-max-gb", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_singlets_probe.jsonl"))
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
