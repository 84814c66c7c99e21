"""Time of muxgl_fmx_ambient_fit (fmx_ambient_fit.hip) beside one muxgl_fmx_ambient call with the front end's default grid of
eight rhos and one muxgl_fmx_singlets call, on the same handle.

    python tools/fmx_ambient_fit_probe.py [--cases a,b,...] [--repeats N] [--out profiles/fmx_ambient_fit_probe.jsonl]

One JSON line per shape (the shapes of tools/fmx_ambient_probe.py).  Every shape runs in a child process of its own under
`timeout`, one after the other, and the probe stops at the first child that fails: nothing is started on a device another
step has just left in doubt.

Per shape, after two EM iterations from a greedy start (spread clusters beyond 64), with the ambient profile made of the
pileup's own read counts, rho_max = 0.5 and n_cand = 2 (the two best clusters of every droplet's row of the singlet table):
kernel_ms = the call's own event time (its one kernel) of `repeats` calls after one untimed call, as median / min / max;
wall_ms = host clock around the whole call, median; table_kernel_ms / table_wall_ms = muxgl_fmx_ambient with eight rhos;
singlets_kernel_ms = muxgl_fmx_singlets (MUXGL_T_FMX_SINGLETS); per_table = kernel_ms over table_kernel_ms, per_singlets
likewise; mean_steps / max_steps = n_steps over the interior fits; status = how many (droplet, candidate) pairs ended in
each status 0..6; mem_gb = device memory in use after the fit minus before it (the call allocates
the profile, cand and the outputs).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fmx_ambient_probe import CASES, DEFAULT_RHOS, mem_info  # noqa: E402

RHO_MAX, N_CAND = 0.5, 2


def timed(repeats, call, kernel_of):
    """(kernel times of `repeats` calls after one untimed call, median wall time in ms)"""
    call()
    kern, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(kernel_of(r))
    return kern, float(np.median(wall))


def run_case(name, repeats):
    from popscle_amd import freemuxlet, muxgl, synth

    cfg, scale, C, S, K, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg, scale, with_gp=False)
        K = synth.CONFIGS[cfg]["V"]
    else:
        p = synth.make_pileup(C, S, 16, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment,
                              with_gp=False)
    mem_info()  # (torch opens the device before the library does, as in tools/fmx_ambient_probe.py)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        f = muxgl.ambient_profile(*e.pileup_allele_counts(), p.af)
        init = e.fmx_greedy_init(K, llk2 - llk0) if K <= 64 else ((np.arange(p.C) * 7) % K).astype(np.int32)
        e.fmx_set_clusters(K, init)
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        cand = freemuxlet.top_clusters(e.fmx_singlets(), min(N_CAND, K))
        base = mem_info()[0]
        kern, wall = timed(repeats, lambda: e.fmx_ambient_fit(f, cand, RHO_MAX), lambda r: r["kernel_ms"])
        peak = mem_info()[0] - base
        fit = e.fmx_ambient_fit(f, cand, RHO_MAX)
        tk, tw = timed(repeats, lambda: e.fmx_ambient(f, DEFAULT_RHOS), lambda r: r["kernel_ms"])
        sk, _ = timed(repeats, e.fmx_singlets, lambda _r: float(e.timing()[muxgl.T_FMX_SINGLETS]))
    k, t, s = float(np.median(kern)), float(np.median(tk)), float(np.median(sk))
    inner = fit["status"] == 0
    r = dict(case=name, C=int(p.C), S=int(p.S), K=int(K), rho_max=RHO_MAX, n_cand=int(cand.shape[1]), nnz=int(p.nnz),
             reads=int(p.reads.size), repeats=repeats, kernel_ms=round(k, 4), kernel_ms_min=round(min(kern), 4),
             kernel_ms_max=round(max(kern), 4), wall_ms=round(wall, 3), table_kernel_ms=round(t, 4), table_wall_ms=round(tw, 3),
             singlets_kernel_ms=round(s, 4), per_table=round(k / t, 2) if t > 0 else None,
             per_singlets=round(k / s, 2) if s > 0 else None,
             mean_steps=round(float(fit["n_steps"][inner].mean()), 2) if inner.any() else None,
             max_steps=int(fit["n_steps"].max()),
             status=np.bincount(fit["status"].ravel(), minlength=7).tolist(), mem_gb=round(peak / 1e9, 4))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_ambient_fit_probe.jsonl"))
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
