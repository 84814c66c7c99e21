#!/usr/bin/env python
"""demuxlet pass time for a given number of samples (which sweep kernel a shape gets: popscle_amd/csrc/path_choice.hpp,
choose_demux_path -- oct/row up to 16, oct/row2/wave up to 32, wave up to 255 but tile at 65..72, streamed call beyond):
python tools/v_probe.py V cells [snps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from popscle_amd import muxgl, synth  # noqa: E402

V, C = int(sys.argv[1]), int(sys.argv[2])
S = int(sys.argv[3]) if len(sys.argv) > 3 else 200000
alphas = (0.0, 0.5) if os.environ.get("VPROBE_DEFAULT_GRID") else (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
p = synth.make_pileup(C, S, V, seed=5)
eng = muxgl.Engine(0)
eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
eng.demux_set_gp(p.gp, p.has_gp)
eng.demux_run(alphas, 0.5, want_cells=False)
dt = 1e9
for _ in range(5):  # best of five passes (the first ones still allocate)
    t0 = time.time()
    eng.demux_run(alphas, 0.5, want_cells=False)
    dt = min(dt, time.time() - t0)
ms = eng.timing()
cells = eng.demux_results_view()
sng = ~p.truth["is_doublet"]
print(json.dumps({"V": V, "cells": C, "entries": p.nnz, "pass_s": dt, "sweep_ms": float(ms[muxgl.T_DEMUX_SWEEP]), "reduce_ms": float(ms[muxgl.T_DEMUX_REDUCE]),
                  "call_ms": float(ms[muxgl.T_DEMUX_CALL]), "ns_per_entry_hypothesis":
                  dt * 1e9 / (p.nnz * (V + V * (V - 1) * (len(alphas) - 1))), "singlet_acc": float((cells["sBest"][sng] == p.truth["s1"][sng]).mean())}))
