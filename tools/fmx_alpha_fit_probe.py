"""Time of muxgl_fmx_alpha_fit (fmx_alpha_fit.hip) beside its nearest sibling, muxgl_fmx_ambient_fit with two candidates, one
muxgl_fmx_singlets call and one E-step, on the same handle.

    python tools/fmx_alpha_fit_probe.py [--cases a,b,...] [--repeats N] [--out profiles/fmx_alpha_fit_probe.jsonl]

One JSON line per shape (the shapes of tools/fmx_ambient_probe.py).  Every shape runs in a child process of its own under
`timeout`, one after the other, and the probe stops at the first child that fails: nothing is started on a device another
step has just left in doubt.

Per shape, after two EM iterations from a greedy start (spread clusters beyond 64), with alpha_max = 1 and the two pairs of
freemuxlet.call_pairs() of every droplet ((dBest1, dBest2) and (sBest, sNext)): kernel_ms = the call's own event time (its
one kernel) of `repeats` calls after one untimed call, as median / min / max; wall_ms = host clock around the whole call,
median; sibling_kernel_ms = muxgl_fmx_ambient_fit with the droplet's two best singlet clusters, rho_max = 0.5 and the
profile of the pileup's own read counts; singlets_kernel_ms = muxgl_fmx_singlets (MUXGL_T_FMX_SINGLETS); estep_ms = the
E-step of the second iteration (MUXGL_T_FMX_ESTEP); per_sibling = kernel_ms over sibling_kernel_ms, per_singlets and
per_estep likewise; mean_steps / max_steps = n_steps over the interior fits; status = how many (droplet, slot) pairs ended in
each status 0..6; scan_share = the share of `scan_sample` drawn fitted pairs whose bracket the 65-point scan ran on, by the
search rule restated on the host (tests/fmx_alpha_fit_ref.search: the kernel does not report it); mem_gb = device memory in
use after the fit minus before it (the call allocates the pairs and the outputs).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fmx_ambient_probe import CASES, mem_info  # noqa: E402

ALPHA_MAX, RHO_MAX, SCAN_SAMPLE = 1.0, 0.5, 48


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


def scan_share(p, q, pair, status, n):
    """of n drawn pairs the device fitted (status 0, 1 or 2): how many the 65-point scan ran on, restated on the host"""
    import fmx_alpha_fit_ref as far

    r = np.random.default_rng(7)
    cs, ts = np.nonzero(status <= 2)
    if cs.size == 0:
        return None, 0
    pick = r.permutation(cs.size)[:n]
    hit = sum(bool(far.search(far.Cell(p, q, int(c), int(pair[c, t, 0]), int(pair[c, t, 1])), ALPHA_MAX)["scanned"])
              for c, t in zip(cs[pick], ts[pick]))
    return hit / pick.size, int(pick.size)


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
        cells, _st = e.fmx_iterate(0.5, 0.1)
        estep = float(e.timing()[muxgl.T_FMX_ESTEP])
        pair = freemuxlet.call_pairs(cells)
        cand = freemuxlet.top_clusters(e.fmx_singlets(), min(2, K))
        base = mem_info()[0]
        kern, wall = timed(repeats, lambda: e.fmx_alpha_fit(pair, ALPHA_MAX), lambda r: r["kernel_ms"])
        peak = mem_info()[0] - base
        fit = e.fmx_alpha_fit(pair, ALPHA_MAX)
        ak, _ = timed(repeats, lambda: e.fmx_ambient_fit(f, cand, RHO_MAX), lambda r: r["kernel_ms"])
        sk, _ = timed(repeats, e.fmx_singlets, lambda _r: float(e.timing()[muxgl.T_FMX_SINGLETS]))
        q = e.fmx_cluster_gp()
    share, n_share = scan_share(p, q, pair, fit["status"], SCAN_SAMPLE)
    k, a, s = float(np.median(kern)), float(np.median(ak)), float(np.median(sk))
    inner = fit["status"] == 0
    ratio = lambda x: round(k / x, 2) if x > 0 else None
    r = dict(case=name, C=int(p.C), S=int(p.S), K=int(K), alpha_max=ALPHA_MAX, n_cand=int(pair.shape[1]), nnz=int(p.nnz),
             reads=int(p.reads.size), repeats=repeats, kernel_ms=round(k, 4), kernel_ms_min=round(min(kern), 4),
             kernel_ms_max=round(max(kern), 4), wall_ms=round(wall, 3), sibling_kernel_ms=round(a, 4),
             singlets_kernel_ms=round(s, 4), estep_ms=round(estep, 4), per_sibling=ratio(a), per_singlets=ratio(s),
             per_estep=ratio(estep), mean_steps=round(float(fit["n_steps"][inner].mean()), 2) if inner.any() else None,
             max_steps=int(fit["n_steps"][inner].max()) if inner.any() else None,
             status=np.bincount(fit["status"].ravel(), minlength=7).tolist(),
             scan_share=None if share is None else round(share, 3), scan_sample=n_share, mem_gb=round(peak / 1e9, 4))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_alpha_fit_probe.jsonl"))
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
