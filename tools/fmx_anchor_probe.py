"""What anchoring costs an EM iteration (muxgl_fmx_set_anchors, fmx_anchor.hip): the posterior phase and a whole
iteration, with and without anchors, on the same handle.

    python tools/fmx_anchor_probe.py [--cases a,b] [--repeats N] [--mode held|prior]
                                     [--out profiles/fmx_anchor_probe.jsonl]

One JSON line per shape.  Every shape runs in a child process of its own under `timeout`, one after the other, and the
probe stops at the first child that fails: nothing is started on a device another step has just left in doubt.

Per shape, after two EM iterations from a greedy start (spread clusters beyond 64), three rounds on the one handle --
plain, anchored (n of the K clusters held to a panel of the true donors' genotypes, unrelated ones beyond them), plain
again -- each one untimed iteration and then `repeats` timed ones (default seven): gp_ms = MUXGL_T_FMX_GP, the bracket
around fmx_cgp_kernel and, when anchored, fmx_anchor_kernel; iter_ms = the sum of the iteration's four timing slots (GP,
E-step, call, M-step); wall_ms = host clock around
muxgl_fmx_iterate without records.  Medians, with min and max of iter_ms.  The E-step's machine code is the same in all
three rounds and the anchor kernel moves S x n x 24 bytes once per iteration (anchor_mb), so the expectation is "within the
spread between the two plain rounds"; the EM moves on between the rounds (other assignments, other cluster pileups), which
is part of that spread.  Nothing is asserted.

--mode prior (muxgl_fmx_set_anchors_mode): four rounds -- plain, HELD, PRIOR (the same n clusters with the panel as the
prior of the posterior the droplets form: fmx_prior_kernel behind fmx_anchor_kernel, the cluster pileups' three diagonal
doubles at a 72-byte stride plus 24 bytes of panel per lane), plain again; the line carries "mode": "prior".  A line
replaces the line of the same shape and mode; lines carrying "build" (figures of another commit's build, taken with that
commit's probe and added by hand) are kept.
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

# name: (config index | None, scale, C, S, K, mean_entries, anchored clusters, child timeout in seconds)
CASES = {
    "configs3_8of16": (3, 1.0, None, None, None, None, 8, 600),       # 50 k cells, K = 16
    "c2000_K256_128": (None, None, 2000, 20000, 256, 150, 128, 300),
}


def run_case(name, repeats, mode="held"):
    from popscle_amd import muxgl, synth

    cfg, scale, C, S, K, ment, n, _ = CASES[name]
    if cfg is not None:
        p = synth.make_config(cfg, scale, with_gp=False)
        K = synth.CONFIGS[cfg]["V"]
    else:
        p = synth.make_pileup(C, S, 16, seed=11, mean_entries=ment, min_entries=max(1, ment // 4), max_entries=4 * ment,
                              with_gp=False)
    G = np.asarray(p.truth["G"], dtype=np.int64)
    if G.shape[1] < n:  # unrelated donors beyond the true ones
        extra = np.random.default_rng(5).binomial(2, np.asarray(p.af)[:, None], size=(p.S, n - G.shape[1]))
        G = np.concatenate([G, extra], axis=1)
    gp = synth.gt_to_gp(G[:, :n], 0.1)
    has_gp = np.ones(p.S, dtype=np.uint8)
    slots = [muxgl.T_FMX_GP, muxgl.T_FMX_ESTEP, muxgl.T_FMX_CALL, muxgl.T_FMX_MSTEP]

    def round_of(e):
        e.fmx_iterate(0.5, 0.1, want_cells=False)
        gpm, itm, wall = [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            e.fmx_iterate(0.5, 0.1, want_cells=False)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = e.timing()
            gpm.append(float(ms[muxgl.T_FMX_GP]))
            itm.append(float(sum(ms[s] for s in slots)))
        return dict(gp_ms=round(float(np.median(gpm)), 4), iter_ms=round(float(np.median(itm)), 4),
                    iter_ms_min=round(min(itm), 4), iter_ms_max=round(max(itm), 4), wall_ms=round(float(np.median(wall)), 3))

    with muxgl.Engine(0) as e:
        e.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
        llk0, llk2, _, _ = e.fmx_prepare(p.af)
        init = e.fmx_greedy_init(K, llk2 - llk0) if K <= 64 else ((np.arange(p.C) * 7) % K).astype(np.int32)
        e.demux_set_gp(gp, has_gp)
        e.fmx_set_clusters(K, init)
        for _ in range(2):
            e.fmx_iterate(0.5, 0.1, want_cells=False)
        plain = round_of(e)
        e.fmx_set_anchors(list(range(n)))
        anchored = round_of(e)
        if mode == "prior":
            e.fmx_set_anchors(list(range(n)), [muxgl.ANCHOR_PRIOR] * n)
            prior = round_of(e)
        e.fmx_set_anchors([])
        again = round_of(e)
    r = dict(case=name, C=int(p.C), S=int(p.S), K=int(K), n_anchor=int(n), nnz=int(p.nnz), repeats=repeats,
             anchor_mb=round(p.S * n * 24 / 1e6, 3), plain=plain, anchored=anchored, plain_again=again)
    if mode == "prior":
        r = dict(r, mode="prior", prior=prior)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--case", default=None, help="(child) run one shape in this process")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--mode", choices=["held", "prior"], default="held")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmx_anchor_probe.jsonl"))
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.repeats, a.mode)
        return 0
    lines = []
    for name in a.cases.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(CASES[name][7]), sys.executable, os.path.abspath(__file__), "--case", name,
                            "--repeats", str(a.repeats), "--mode", a.mode], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    if lines:  # the lines of the shapes run now replace those of the same shapes (and mode) in an existing file
        def key(ln):
            j = json.loads(ln)
            return (j["case"], j.get("mode", "held"), j.get("build"))

        done = {key(ln) for ln in lines}
        kept = []
        if os.path.exists(a.out):
            kept = [ln for ln in open(a.out).read().splitlines() if ln.strip() and key(ln) not in done]
        rank = {name: i for i, name in enumerate(CASES)}
        with open(a.out, "w") as f:   # (stable: by mode and build first, then by shape)
            f.write("\n".join(sorted(kept + lines, key=lambda ln: (key(ln)[1], key(ln)[2] or "", rank.get(key(ln)[0], 99)))) + "\n")
    return 0 if len(lines) == len(a.cases.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
