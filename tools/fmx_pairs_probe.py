"""Time of muxgl_fmx_cluster_pairs (fmx_pairs.hip), beside the fetch of the cluster pileups it replaces and one EM iteration.

    python tools/fmx_pairs_probe.py [--cases a,b,...] [--repeats N] [--out profiles/fmx_pairs_probe.jsonl]

One JSON line per shape (K clusters, S markers).  Every shape runs in a child process of its own under `timeout`, one
after the other, and the probe stops at the first child that fails: nothing is started on a device another step has just
left in doubt.

Per shape, after one EM iteration from spread clusters: kernel_ms = the call's own event time over `repeats` calls after
one untimed call, as median / min / max; wall_ms = host clock around the whole call, its copy of the triangle to the host
included; fetch_wall_ms = host clock around muxgl_fmx_get_cluster_pileup alone into buffers that exist and have been
touched (the first step of the only route there was: 96 K S bytes to the host, the scoring still to come); iter_ms /
iterate_wall_ms = the kernel slots and the wall time of one muxgl_fmx_iterate; pair_snps_per_ns = K (K - 1) / 2 x S /
kernel time; dev_used_mb_before / _after = device memory in use (hipMemGetInfo) before the first call and after the last
(the call's temporaries go back to the handle's cache, so the second figure is the high-water).  For the shapes that name
them, kernel_ms once per candidate tile (MUXGL_FMX_PAIRS_TILE = row clusters per wave; the outputs are the same bits).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (K, S, cells, mean entries per cell, candidate tiles, child timeout in seconds): the shapes of fmx_match_probe.py
CASES = {
    "K16_S100k": (16, 100_000, 4000, 400, (), 300),
    "K64_S500k": (64, 500_000, 4000, 800, (), 400),
    "K256_S200k": (256, 200_000, 2048, 400, (4, 8), 500),
    "K1024_S100k": (1024, 100_000, 2048, 400, (4, 8), 900),
}
FIELDS = ("llk2", "llk0", "nsnps")


def dev_used_mb():
    import torch

    free, total = torch.cuda.mem_get_info(0)
    return round((total - free) / 2 ** 20, 1)


def run_case(name, repeats):
    from popscle_amd import muxgl, synth

    K, S, C, ment, tiles, _ = CASES[name]
    p = synth.make_pileup(C, S, 16, seed=23, mean_entries=ment, min_entries=ment // 4, max_entries=4 * ment, with_gp=False)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.fmx_prepare(p.af)
        e.fmx_set_clusters(K, ((np.arange(p.C) * 7) % K).astype(np.int32))
        t0 = time.perf_counter()
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        iterate_wall = (time.perf_counter() - t0) * 1e3
        ms = e.timing()
        it_ms = float(ms[muxgl.T_FMX_GP] + ms[muxgl.T_FMX_ESTEP] + ms[muxgl.T_FMX_CALL] + ms[muxgl.T_FMX_MSTEP])
        used0 = dev_used_mb()

        def calls(n):
            ks, ws, last = [], [], None
            e.fmx_cluster_pairs()
            for _ in range(n):
                t0 = time.perf_counter()
                last = e.fmx_cluster_pairs()
                ws.append((time.perf_counter() - t0) * 1e3)
                ks.append(last["kernel_ms"])
            return ks, ws, last

        kern, wall, ref = calls(repeats)
        by_tile = {}
        for t in tiles:
            os.environ["MUXGL_FMX_PAIRS_TILE"] = str(t)
            ks, _, r = calls(repeats)
            assert all(r[n].tobytes() == ref[n].tobytes() for n in FIELDS)
            by_tile[str(t)] = round(float(np.median(ks)), 4)
        os.environ.pop("MUXGL_FMX_PAIRS_TILE", None)
        used1 = dev_used_mb()
        # the fetch, into buffers that exist and are resident
        gls = np.ones((K, S, 9))
        cnt = np.ones((K, S, 3), dtype=np.int32)
        vp = ctypes.c_void_p
        fetch = []
        for i in range(1 + min(repeats, 3)):
            t0 = time.perf_counter()
            rc = e.lib.muxgl_fmx_get_cluster_pileup(e.h, gls.ctypes.data_as(vp), cnt.ctypes.data_as(vp))
            assert rc == 0
            if i:
                fetch.append((time.perf_counter() - t0) * 1e3)
    km = float(np.median(kern))
    r = dict(case=name, K=K, S=S, C=int(p.C), nnz=int(p.nnz), repeats=repeats, kernel_ms=round(km, 4),
             kernel_ms_min=round(min(kern), 4), kernel_ms_max=round(max(kern), 4), wall_ms=round(float(np.median(wall)), 3),
             fetch_wall_ms=round(float(np.median(fetch)), 3), fetch_gb=round(96.0 * K * S / 1e9, 3),
             iter_ms=round(it_ms, 4), iterate_wall_ms=round(iterate_wall, 3),
             pair_snps_per_ns=round(K * (K - 1) / 2.0 * S / (km * 1e6), 2), kernel_ms_by_tile=by_tile,
             dev_used_mb_before=used0, dev_used_mb_after=used1,
             nsnps_min=int(ref["nsnps"].min()), nsnps_max=int(ref["nsnps"].max()))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_pairs_probe.jsonl"))
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.repeats)
        return 0
    lines = []
    for name in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][5]), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--repeats", str(a.repeats)], capture_output=True, text=True)
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
