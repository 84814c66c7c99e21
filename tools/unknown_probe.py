"""Time and device memory of muxgl_demux_unknown (demux_unknown.hip), beside muxgl_demux_run and muxgl_demux_singlets of the
same handle and, where it is accepted, the only earlier route to the same numbers.

    python tools/unknown_probe.py [--cases a,b,...] [--repeats N] [--full-ll-max-gb G] [--out profiles/unknown_probe.jsonl]

One JSON line per shape (the shapes of tools/singlets_probe.py).  Every shape runs in a child process of its own under
`timeout`, one after the other, and the probe stops at the first child that fails: nothing is started on a device another
step has just left in doubt.

Per shape: kernel_ms = the call's own event time (weights + sweep + emit of every batch) of `repeats` calls after one untimed
call, as median / min / max; wall_ms = host clock around the whole call (its copies of the three tables to the host
included), median; batches = how many batches of cells the budget cut the job into; singlets_kernel_ms / singlets_wall_ms =
muxgl_demux_singlets on the same handle; run_kernel_ms / run_wall_ms = muxgl_demux_run (sweep + call slots; wall), median;
sweeps = kernel_ms / singlets_kernel_ms, to hold against the expectation of ceil(A / 3) singlet sweeps plus one pass over
the reads; mem_gb = device memory in use after the calls minus before the handle (the handle's cache keeps every block, so
this is the high-water mark).  Where V + 1 <= 255 and the [C][V + 1][V + 1][A] tensor is at most --full-ll-max-gb,
old_route_wall_ms = the panel with the mean row appended as sample V handed over, muxgl_demux_run with full_ll and its copy
to the host -- once, after one untimed run -- and max_abs_diff_vs_old_route the largest difference of the three tables to
its slices.
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
UNK_PART = 2048

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


def batches_of(p, A, budget):
    """the cut of demux_unknown.hip, restated: whole cells while their weights, slab rows and table rows fit"""
    lens = np.diff(p.cell_ptr)
    parts = np.maximum(1, -(-lens // UNK_PART))
    row = 8 * A * 2 * (p.gp.shape[1] + 1)
    need = lens * A * 48 + parts * (row + 24) + row + 16
    n, acc = 0, 0
    for b in need:
        if acc == 0 or acc + b > budget:
            n, acc = n + 1, 0
        acc += int(b)
    return n


def panel_mean(gp, has_gp):
    u = np.zeros((gp.shape[0], 3))
    for j in range(gp.shape[1]):
        u += gp[:, j, :]
    u /= gp.shape[1]
    u[np.asarray(has_gp) == 0] = 0.0
    return u


def run_case(name, repeats, full_ll_max_gb):
    import torch

    from popscle_amd import muxgl, synth

    cfg, C, S, V, alphas, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg)
        alphas = synth.CONFIGS[cfg].get("alphas", G2)
        V = p.gp.shape[1]
    else:
        p = synth.make_pileup(C, S, V, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment)
    A = len(alphas)
    mb = os.environ.get("MUXGL_DEMUX_SLAB_MB")
    budget = int(mb) << 20 if mb and int(mb) > 0 else min(4 << 30, torch.cuda.mem_get_info(0)[1] // 3)
    base = used_bytes()
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        e.demux_unknown(alphas)
        kern, wall = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            unk = e.demux_unknown(alphas)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(unk["kernel_ms"])
        peak = used_bytes() - base
        e.demux_singlets(alphas)
        sk, sw = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            e.demux_singlets(alphas)
            sw.append((time.perf_counter() - t0) * 1e3)
            sk.append(float(e.timing()[muxgl.T_DEMUX_SINGLETS]))
        e.demux_run(alphas, 0.5, want_cells=False)
        rk, rw = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            e.demux_run(alphas, 0.5, want_cells=False)
            rw.append((time.perf_counter() - t0) * 1e3)
            ms = e.timing()
            rk.append(float(ms[muxgl.T_DEMUX_REDUCE] + ms[muxgl.T_DEMUX_SWEEP] + ms[muxgl.T_DEMUX_CALL]))
    tensor_gb = p.C * (V + 1) * (V + 1) * A * 8 / 1e9
    old_ms, old_dev = None, None
    if V + 1 <= 255 and tensor_gb <= full_ll_max_gb:
        aug = np.ascontiguousarray(np.concatenate([p.gp, panel_mean(p.gp, p.has_gp)[:, None, :]], axis=1))
        with muxgl.Engine(0) as e:
            e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
            e.demux_set_gp(aug, p.has_gp)
            e.demux_run(alphas, 0.5, want_cells=False)
            t0 = time.perf_counter()
            e.demux_set_gp(aug, p.has_gp)
            _, full = e.demux_run(alphas, 0.5, want_cells=False, want_full_ll=True)
            old_ms = (time.perf_counter() - t0) * 1e3
        # full_ll holds the slots the reference reads, (j, 0, 0) and (j, k != j, n >= 1): compare those
        old_dev = 0.0
        if A > 1:
            old_dev = max(float(np.max(np.abs(full[:, :V, V, 1:] - unk["ju"][:, :, 1:]))),
                          float(np.max(np.abs(full[:, V, :V, 1:] - unk["uj"][:, :, 1:]))))
        del full
    k, s = float(np.median(kern)), float(np.median(sk))
    r = dict(case=name, C=int(p.C), S=int(p.S), V=int(V), alphas=list(alphas), nnz=int(p.nnz), repeats=repeats,
             kernel_ms=round(k, 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4),
             wall_ms=round(float(np.median(wall)), 3), batches=batches_of(p, A, budget),
             singlets_kernel_ms=round(s, 4), singlets_wall_ms=round(float(np.median(sw)), 3),
             sweeps=round(k / s, 2) if s > 0 else None, chunks=(A + 2) // 3,
             run_kernel_ms=round(float(np.median(rk)), 4), run_wall_ms=round(float(np.median(rw)), 3),
             mem_gb=round(peak / 1e9, 3), tables_gb=round(p.C * (2 * V + 1) * A * 8 / 1e9, 4),
             weights_gb_if_held=round(p.nnz * A * 48 / 1e9, 3), old_route_tensor_gb=round(tensor_gb, 2),
             old_route_wall_ms=None if old_ms is None else round(old_ms, 1), max_abs_diff_vs_old_route=old_dev)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--full-ll-max-gb", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unknown_probe.jsonl"))
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
