"""Time and device memory of muxgl_demux_ambient (demux_ambient.hip), beside muxgl_demux_singlets and muxgl_demux_unknown
of the same handle.

    python tools/ambient_probe.py [--cases a,b,...] [--repeats N] [--out profiles/ambient_probe.jsonl]

One JSON line per shape (shapes of tools/unknown_probe.py), appended to --out.  Every shape runs in a child process of
its own under `timeout`, one after the other, and the probe stops at the first child that fails: nothing is started on a
device another step has just left in doubt.

Per shape, with the front end's default grid of eight rhos and the ambient profile made from the pileup's own reads
(muxgl_pileup_allele_counts + muxgl.ambient_profile): kernel_ms = the call's own event time (weights + sweep + emit of
every batch) of `repeats` calls after one untimed call, as median / min / max; wall_ms = host clock around the whole call
(its copy of the table to the host included), median; counts_wall_ms = muxgl_pileup_allele_counts, wall; batches = how many
batches of cells the budget cut the job into; singlets_kernel_ms / singlets_wall_ms = muxgl_demux_singlets on the same
handle; unknown_kernel_ms / unknown_wall_ms = muxgl_demux_unknown (panel mean) on the same handle; per_singlets and
per_unknown = kernel_ms over the two; mem_gb = device memory in use after the calls minus before the handle (the handle's
cache keeps every block, so this is the high-water mark).
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
RHOS = (0.0, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)
AMB_PART = 2048

# name: (config index | None, C, S, V, alphas, mean_entries, child timeout in seconds)
CASES = {
    "configs1": (1, None, None, None, None, None, 300),
    "configs2": (2, None, None, None, None, None, 900),
    "c2000_V255": (None, 2000, 20000, 255, G2, 150, 300),
    "c2000_V512": (None, 2000, 20000, 512, G2, 150, 300),
    "c1000_V1024": (None, 1000, 20000, 1024, G2, 150, 300),
}


def used_bytes():
    import torch

    fr, tot = torch.cuda.mem_get_info(0)
    return tot - fr


def batches_of(p, NR, budget):
    """the cut of demux_ambient.hip, restated: whole cells while their weights, slab rows and table rows fit"""
    lens = np.diff(p.cell_ptr)
    parts = np.maximum(1, -(-lens // AMB_PART))
    row = 8 * NR * p.gp.shape[1]
    need = lens * NR * 24 + parts * (row + 24) + row + 16
    n, acc = 0, 0
    for b in need:
        if acc == 0 or acc + b > budget:
            n, acc = n + 1, 0
        acc += int(b)
    return n


def timed(repeats, call, kernel):
    call()
    kern, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(kernel(r))
    return kern, float(np.median(wall))


def run_case(name, repeats):
    import torch

    from popscle_amd import muxgl, synth

    cfg, C, S, V, alphas, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg)
        alphas = synth.CONFIGS[cfg].get("alphas", G2)
        V = p.gp.shape[1]
    else:
        p = synth.make_pileup(C, S, V, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment)
    mb = os.environ.get("MUXGL_DEMUX_SLAB_MB")
    budget = int(mb) << 20 if mb and int(mb) > 0 else min(4 << 30, torch.cuda.mem_get_info(0)[1] // 3)
    base = used_bytes()
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        e.pileup_allele_counts()
        t0 = time.perf_counter()
        n_ref, n_alt = e.pileup_allele_counts()
        counts_ms = (time.perf_counter() - t0) * 1e3
        f = muxgl.ambient_profile(n_ref, n_alt, p.af)
        kern, wall = timed(repeats, lambda: e.demux_ambient(alphas, f, RHOS), lambda r: r["kernel_ms"])
        peak = used_bytes() - base
        sk, sw = timed(repeats, lambda: e.demux_singlets(alphas), lambda r: float(e.timing()[muxgl.T_DEMUX_SINGLETS]))
        uk, uw = timed(repeats, lambda: e.demux_unknown(alphas), lambda r: r["kernel_ms"])
    k, s, u = float(np.median(kern)), float(np.median(sk)), float(np.median(uk))
    r = dict(case=name, C=int(p.C), S=int(p.S), V=int(V), alphas=list(alphas), rhos=list(RHOS), nnz=int(p.nnz), repeats=repeats,
             kernel_ms=round(k, 4), kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4), wall_ms=round(wall, 3),
             counts_wall_ms=round(counts_ms, 3), batches=batches_of(p, len(RHOS), budget),
             singlets_kernel_ms=round(s, 4), singlets_wall_ms=round(sw, 3), unknown_kernel_ms=round(u, 4),
             unknown_wall_ms=round(uw, 3), per_singlets=round(k / s, 2) if s > 0 else None,
             per_unknown=round(k / u, 2) if u > 0 else None, mem_gb=round(peak / 1e9, 3),
             table_gb=round(p.C * V * len(RHOS) * 8 / 1e9, 4), weights_gb_if_held=round(p.nnz * len(RHOS) * 24 / 1e9, 3))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ambient_probe.jsonl"))
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.repeats)
        return 0
    done = 0
    for name in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][6]), sys.executable, os.path.abspath(__file__), "--case", name,
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
