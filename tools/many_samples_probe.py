"""Rate and device memory of the demuxlet call at many samples: the existing paths against the streamed call
(demux_stream.hip), beyond 255 samples, and one job whose [C][V][V][A] tensor does not fit the device (the memory wall).

    python tools/many_samples_probe.py [--quick] [--cli] [--out FILE.jsonl]

Rate = hypothesis-entries per second: sum over cells of entries_c x hypotheses per entry (V singlets + V (V - 1) pairs
for every doublet alpha, counted once per unordered pair at alpha = 0.5, as the call reads them) / kernel time (sweep +
call, hipEvents; warm run, after one untimed run).  Memory: device memory in use after the run minus before the handle
(the handle's cache keeps every block the run allocated, so this is its high-water mark).  --cli: one cohort-sized
`popscle-amd demuxlet` end to end (10 k cells x 1000 samples, GT VCF), wall time.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from popscle_amd import muxgl, plpio, synth  # noqa: E402


def used_bytes():
    import torch

    fr, tot = torch.cuda.mem_get_info(0)
    return tot - fr


def hyp_per_entry(V, alphas):
    n = V
    for a in alphas[1:]:
        n += V * (V - 1) // (2 if a == 0.5 else 1)
    return n


def case(name, C, S, V, alphas, flags, mean_entries, seed=11):
    p = synth.make_pileup(C, S, V, seed=seed, mean_entries=mean_entries, min_entries=max(1, mean_entries // 4),
                          max_entries=4 * mean_entries)
    base = used_bytes()
    with muxgl.Engine(0, flags) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        e.demux_run(alphas, 0.5, want_cells=False)
        t0 = time.perf_counter()
        e.demux_run(alphas, 0.5, want_cells=False)
        wall = time.perf_counter() - t0
        ms = e.timing()
        kern = float(ms[muxgl.T_DEMUX_SWEEP] + ms[muxgl.T_DEMUX_CALL])
        peak = used_bytes() - base
    work = float(p.nnz) * hyp_per_entry(V, alphas)
    r = dict(case=name, C=C, V=V, alphas=list(alphas), nnz=int(p.nnz),
             path="streamed" if (V > 255 or flags & muxgl.FLAG_FORCE_STREAMED_CALL or name.startswith("wall")) else "existing",
             kernel_ms=round(kern, 3), wall_s=round(wall, 3), hyp_entries_per_s=work / (kern * 1e-3),
             mem_gb=round(peak / 1e9, 3), tensor_gb=round(C * V * V * len(alphas) * 8 / 1e9, 1))
    print(json.dumps(r), flush=True)
    return r


def cli_case(C=10000, V=1000, S=20000, mean_entries=120):
    p = synth.make_pileup(C, S, V, seed=21, mean_entries=mean_entries)
    with tempfile.TemporaryDirectory() as td:
        prefix, vcf, out = os.path.join(td, "plp"), os.path.join(td, "g.vcf.gz"), os.path.join(td, "out")
        t0 = time.perf_counter()
        plpio.write_plp(prefix, p, seed=21)
        plpio.write_vcf(vcf, p, p.truth["G"].astype(np.int64), field="GT")
        t1 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "popscle_amd", "bin", "popscle-amd"), "demuxlet", "--plp", prefix, "--vcf",
                            vcf, "--field", "GT", "--out", out], capture_output=True, text=True)
        wall = time.perf_counter() - t1
        rows = sum(1 for _ in open(out + ".best")) - 1 if r.returncode == 0 else 0
        res = dict(case="cli_cohort", C=C, V=V, S=S, nnz=int(p.nnz), rc=r.returncode, rows=rows, write_inputs_s=round(t1 - t0, 1),
                   cli_wall_s=round(wall, 1), stderr_tail=r.stderr[-600:])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes (a check that the tool runs)")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-only", action="store_true", help="only the cohort-sized CLI run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G6 = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
    G2 = (0.0, 0.5)
    F = muxgl.FLAG_FORCE_STREAMED_CALL
    q = a.quick
    C = 200 if q else 2000
    runs = []
    if a.cli_only:
        runs.append(cli_case() if not q else cli_case(C=300, V=300, S=2000, mean_entries=60))
    for V in (64, 255) if not a.cli_only else ():
        for al in (G2, G6):
            runs.append(case(f"V{V}_existing", C, 20000, V, al, 0, 150))
            runs.append(case(f"V{V}_streamed", C, 20000, V, al, F, 150))
    for V in (512, 1024) if not a.cli_only else ():
        runs.append(case(f"V{V}_streamed", C // 2 if V > 512 else C, 20000, V, G2, 0, 150))
    if not a.cli_only:
        runs.append(case("V1024_streamed", C // 4, 20000, 1024, G6, 0, 150))
    # the memory wall: 100 k cells x 255 samples x 6 alphas = 312 GB of tensor (an MI355X holds 288 GB)
    if not q and not a.cli_only:
        runs.append(case("wall_V255_A6", 100000, 20000, 255, G6, 0, 20))
    if a.cli and not a.cli_only:
        runs.append(cli_case() if not q else cli_case(C=300, V=300, S=2000, mean_entries=60))
    if a.out:
        with open(a.out, "w") as f:
            for r in runs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
