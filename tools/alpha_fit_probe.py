"""Time of muxgl_demux_alpha_fit (demux_alpha_fit.hip) beside its nearest sibling, muxgl_demux_ambient_fit with two
candidates, and beside one muxgl_demux_run, on the same handle.

    python tools/alpha_fit_probe.py [--cases a,b,...] [--repeats N] [--out profiles/alpha_fit_probe.jsonl]

One JSON line per shape (shapes of tools/ambient_probe.py), appended to --out.  Every shape runs in a child process of
its own under `timeout`, one after the other, and the probe stops at the first child that fails: nothing is started on a
device another step has just left in doubt.

Per shape, with the pairs of demuxlet.call_pairs on the records of one muxgl_demux_run (two per droplet: the best doublet's
two samples, and the best and next singlet) and alpha_max = 1: kernel_ms = the call's own event time (its one kernel) of
`repeats` calls after one untimed call, as median / min / max; wall_ms = host clock around the whole call, median;
mean_steps / max_steps = n_steps over the interior fits; status = how many (droplet, slot) pairs ended in each status
0..5; sibling_kernel_ms / sibling_wall_ms = muxgl_demux_ambient_fit with the two best singlet samples as candidates, the
pileup's own profile and rho_max = 0.5, with sibling_mean_steps; per_sibling = kernel_ms over sibling_kernel_ms;
run_kernel_ms / run_wall_ms = one muxgl_demux_run with the shape's grid (the sum of its timing slots, and the host clock),
run_per_alpha = run_kernel_ms over the grid's size: about what one more grid point costs, which the fit replaces;
mem_gb = device memory in use after the fit minus before it (the call allocates the pairs and the outputs).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ambient_probe import CASES, G2, timed, used_bytes  # noqa: E402

ALPHA_MAX, RHO_MAX = 1.0, 0.5


def run_case(name, repeats):
    from popscle_amd import demuxlet, muxgl, synth

    cfg, C, S, V, alphas, ment, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg)
        alphas = synth.CONFIGS[cfg].get("alphas", G2)
        V = p.gp.shape[1]
    else:
        p = synth.make_pileup(C, S, V, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment)
    used_bytes()  # (torch opens the device before the library does, as in tools/ambient_probe.py)
    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        e.demux_set_gp(p.gp, p.has_gp)
        rk, rw = timed(repeats, lambda: e.demux_run(alphas, 0.5), lambda r: float(np.sum(e.timing())))
        pairs = demuxlet.call_pairs(e.demux_run(alphas, 0.5))
        base = used_bytes()
        kern, wall = timed(repeats, lambda: e.demux_alpha_fit(alphas, pairs, ALPHA_MAX), lambda r: r["kernel_ms"])
        peak = used_bytes() - base
        fit = e.demux_alpha_fit(alphas, pairs, ALPHA_MAX)
        f = muxgl.ambient_profile(*e.pileup_allele_counts(), p.af)
        cand = demuxlet.top_samples(e.demux_singlets(alphas), min(2, V))
        sk, sw = timed(repeats, lambda: e.demux_ambient_fit(alphas, f, cand, RHO_MAX), lambda r: r["kernel_ms"])
        sib = e.demux_ambient_fit(alphas, f, cand, RHO_MAX)
    k, s, run = float(np.median(kern)), float(np.median(sk)), float(np.median(rk))
    inner, sinner = fit["status"] == 0, sib["status"] == 0
    r = dict(case=name, C=int(p.C), S=int(p.S), V=int(V), alphas=list(alphas), alpha_max=ALPHA_MAX, n_cand=int(pairs.shape[1]),
             nnz=int(p.nnz), repeats=repeats, kernel_ms=round(k, 4), kernel_ms_min=round(min(kern), 4),
             kernel_ms_max=round(max(kern), 4), wall_ms=round(wall, 3),
             mean_steps=round(float(fit["n_steps"][inner].mean()), 2) if inner.any() else None,
             max_steps=int(fit["n_steps"].max()), status=np.bincount(fit["status"].ravel(), minlength=6).tolist(),
             sibling_kernel_ms=round(s, 4), sibling_wall_ms=round(sw, 3),
             sibling_mean_steps=round(float(sib["n_steps"][sinner].mean()), 2) if sinner.any() else None,
             per_sibling=round(k / s, 2) if s > 0 else None, run_kernel_ms=round(run, 4), run_wall_ms=round(rw, 3),
             run_per_alpha=round(run / len(alphas), 4), mem_gb=round(peak / 1e9, 4))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_fit_probe.jsonl"))
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
