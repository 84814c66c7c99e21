"""CPU test of the argument rules of the four per-droplet fits (popscle_amd/csrc/fit_args.hpp): muxgl_demux_ambient_fit,
muxgl_demux_alpha_fit, muxgl_fmx_ambient_fit and muxgl_fmx_alpha_fit, in the manner of test_fmx_refusal.py.

Each call once carried its rule, or its half of one, in its own unit (demux_ambient_fit.hip, demux_alpha_fit.hip,
fmx_ambient_fit.hip, fmx_alpha_fit.hip; the head in ambient_fit_search.hpp).  The texts are written out below as those
units formed them, and the shared rules are held to them byte for byte, with the order in which the rules are asked.

tests/csrc/fit_args_probe.cpp is compiled into a stand-alone host program with hipcc (plain C++: no device code, no
device is touched); it runs every case through the four calls' rules with 2 droplets, n_cand = 2, 5 samples or clusters
and 3 markers, and prints one line per (call, case)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CALLS = ["demux_ambient_fit", "demux_alpha_fit", "fmx_ambient_fit", "fmx_alpha_fit"]

# case -> what the four calls say, in the order of CALLS (None: the arguments pass)
WANT = {
    "ok": [None, None, None, None],
    # every output NULL: asked first, before n_cand = 0 and a NULL cand / pair
    "no_output": [
        "muxgl_demux_ambient_fit: every output is NULL",
        "muxgl_demux_alpha_fit: every output is NULL",
        "muxgl_fmx_ambient_fit: every output is NULL",
        "muxgl_fmx_alpha_fit: every output is NULL",
    ],
    "n_cand_0": [
        "muxgl_demux_ambient_fit: n_cand=0 outside [1,16]",
        "muxgl_demux_alpha_fit: n_cand=0 outside [1,16]",
        "muxgl_fmx_ambient_fit: n_cand=0 outside [1,16]",
        "muxgl_fmx_alpha_fit: n_cand=0 outside [1,16]",
    ],
    "n_cand_over": [  # MUXGL_MAX_FIT_CAND + 1
        "muxgl_demux_ambient_fit: n_cand=17 outside [1,16]",
        "muxgl_demux_alpha_fit: n_cand=17 outside [1,16]",
        "muxgl_fmx_ambient_fit: n_cand=17 outside [1,16]",
        "muxgl_fmx_alpha_fit: n_cand=17 outside [1,16]",
    ],
    # cand / pair and amb_af NULL, and the bound 0: cand before amb_af, both before the bound
    "null_slot": [
        "muxgl_demux_ambient_fit: cand is NULL",
        "muxgl_demux_alpha_fit: pair is NULL",
        "muxgl_fmx_ambient_fit: cand is NULL",
        "muxgl_fmx_alpha_fit: pair is NULL",
    ],
    # amb_af NULL and the bound 0 (the mixing-share fits have no amb_af)
    "null_af": [
        "muxgl_demux_ambient_fit: amb_af is NULL",
        "muxgl_demux_alpha_fit: alpha_max (0) is not a finite number in (0, 1]",
        "muxgl_fmx_ambient_fit: amb_af is NULL",
        "muxgl_fmx_alpha_fit: alpha_max (0) is not a finite number in (0, 1]",
    ],
    # the bound 0 and an index of -2: the bound before the indices
    "bound_0": [
        "muxgl_demux_ambient_fit: rho_max (0) is not a finite number in (0, 1]",
        "muxgl_demux_alpha_fit: alpha_max (0) is not a finite number in (0, 1]",
        "muxgl_fmx_ambient_fit: rho_max (0) is not a finite number in (0, 1]",
        "muxgl_fmx_alpha_fit: alpha_max (0) is not a finite number in (0, 1]",
    ],
    "bound_1.5": [
        "muxgl_demux_ambient_fit: rho_max (1.5) is not a finite number in (0, 1]",
        "muxgl_demux_alpha_fit: alpha_max (1.5) is not a finite number in (0, 1]",
        "muxgl_fmx_ambient_fit: rho_max (1.5) is not a finite number in (0, 1]",
        "muxgl_fmx_alpha_fit: alpha_max (1.5) is not a finite number in (0, 1]",
    ],
    "bound_nan": [
        "muxgl_demux_ambient_fit: rho_max (nan) is not a finite number in (0, 1]",
        "muxgl_demux_alpha_fit: alpha_max (nan) is not a finite number in (0, 1]",
        "muxgl_fmx_ambient_fit: rho_max (nan) is not a finite number in (0, 1]",
        "muxgl_fmx_alpha_fit: alpha_max (nan) is not a finite number in (0, 1]",
    ],
    "bound_1": [None, None, None, None],
    # the fourth index is -2: candidate [1][1], or the second of pair [0][1]
    "index_-2": [
        "muxgl_demux_ambient_fit: cand[1][1] (-2) is neither -1 nor a sample in [0,5)",
        "muxgl_demux_alpha_fit: pair[0][1][1] (-2) is neither -1 nor a sample in [0,5)",
        "muxgl_fmx_ambient_fit: cand[1][1] (-2) is neither -1 nor a cluster in [0,5)",
        "muxgl_fmx_alpha_fit: pair[0][1][1] (-2) is neither -1 nor a cluster in [0,5)",
    ],
    # the third and fourth index are n_what: the first that is met is named
    "index_n": [
        "muxgl_demux_ambient_fit: cand[1][0] (5) is neither -1 nor a sample in [0,5)",
        "muxgl_demux_alpha_fit: pair[0][1][0] (5) is neither -1 nor a sample in [0,5)",
        "muxgl_fmx_ambient_fit: cand[1][0] (5) is neither -1 nor a cluster in [0,5)",
        "muxgl_fmx_alpha_fit: pair[0][1][0] (5) is neither -1 nor a cluster in [0,5)",
    ],
    # pair [1][1] is (-1, 0) (the candidates end before it)
    "one_negative": [
        None,
        "muxgl_demux_alpha_fit: pair[1][1] (-1, 0) has exactly one negative index",
        None,
        "muxgl_fmx_alpha_fit: pair[1][1] (-1, 0) has exactly one negative index",
    ],
    # an index of -2 and an amb_af of -0.5: the indices before freemuxlet's amb_af
    "index_before_af": [
        "muxgl_demux_ambient_fit: cand[1][1] (-2) is neither -1 nor a sample in [0,5)",
        "muxgl_demux_alpha_fit: pair[0][1][1] (-2) is neither -1 nor a sample in [0,5)",
        "muxgl_fmx_ambient_fit: cand[1][1] (-2) is neither -1 nor a cluster in [0,5)",
        "muxgl_fmx_alpha_fit: pair[0][1][1] (-2) is neither -1 nor a cluster in [0,5)",
    ],
    # freemuxlet's amb_af outside [0, 1] (demuxlet's is held against has_gp on the handle, not here)
    "af_1.5": [None, None, "muxgl_fmx_ambient_fit: amb_af of marker 1 (1.5) is not a finite number in [0, 1]", None],
    "af_nan": [None, None, "muxgl_fmx_ambient_fit: amb_af of marker 2 (nan) is not a finite number in [0, 1]", None],
    "af_negative": [None, None, "muxgl_fmx_ambient_fit: amb_af of marker 0 (-0.25) is not a finite number in [0, 1]", None],
}


@pytest.fixture(scope="module")
def said(tmp_path_factory):
    """(call, case) -> (return code, text) as the probe printed them"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("probe") / "fit_args_probe")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "fit_args_probe.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        call, case, rc, text = line.split("\t")
        assert (call, case) not in out
        out[(call, case)] = (int(rc), text)
    return out


def test_the_probe_ran_every_case_and_no_other(said):
    assert set(said) == {(call, case) for call in CALLS for case in WANT}


@pytest.mark.parametrize("case", list(WANT))
def test_every_call_says_what_it_said(said, case):
    for call, want in zip(CALLS, WANT[case]):
        # (arguments that pass leave the buffer alone: the probe zeroes it first)
        assert said[(call, case)] == ((0, "") if want is None else (1, want)), (call, case)


def test_every_text_fits_the_callers_buffer():
    assert max(len(t) for ts in WANT.values() for t in ts if t) < 256
