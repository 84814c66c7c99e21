"""CPU test of the one refusal rule of the freemuxlet calls that read the last E-step's posteriors
(popscle_amd/csrc/fmx_refusal.hpp): muxgl_fmx_singlets, _inclusion, _unknown, _ambient and _ambient_fit.

Each call once carried the rule as a function of its own that returned string literals.  Those literals are written out
below as they stood in the five units (fmx_singlets.hip, fmx_incl.hip, fmx_unknown.hip, fmx_ambient.hip,
fmx_ambient_fit.hip) and the shared rule is held to them byte for byte, in the order the five functions asked.

The header is compiled into a small shared object with hipcc (plain C++: no device code, no device is touched)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (call, the subject of its last rule)
CALLS = [("muxgl_fmx_singlets", "the table belongs"), ("muxgl_fmx_inclusion", "the tables belong"),
         ("muxgl_fmx_unknown", "the tables belong"), ("muxgl_fmx_ambient", "the table belongs"),
         ("muxgl_fmx_ambient_fit", "the fit belongs")]

# the literals of the five functions, rule by rule
OLD = {
    "muxgl_fmx_singlets": [
        "muxgl_fmx_singlets: no pileup set (muxgl_set_pileup)",
        "muxgl_fmx_singlets: call muxgl_fmx_prepare first",
        "muxgl_fmx_singlets: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)",
        "muxgl_fmx_singlets: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep first)",
        "muxgl_fmx_singlets: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; the table "
        "belongs to an E-step's own posteriors: call it before the next iteration's posterior phase",
    ],
    "muxgl_fmx_inclusion": [
        "muxgl_fmx_inclusion: no pileup set (muxgl_set_pileup)",
        "muxgl_fmx_inclusion: call muxgl_fmx_prepare first",
        "muxgl_fmx_inclusion: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)",
        "muxgl_fmx_inclusion: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep first)",
        "muxgl_fmx_inclusion: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; the tables "
        "belong to an E-step's own posteriors: call it before the next iteration's posterior phase",
    ],
    "muxgl_fmx_unknown": [
        "muxgl_fmx_unknown: no pileup set (muxgl_set_pileup)",
        "muxgl_fmx_unknown: call muxgl_fmx_prepare first",
        "muxgl_fmx_unknown: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)",
        "muxgl_fmx_unknown: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep first)",
        "muxgl_fmx_unknown: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; the tables "
        "belong to an E-step's own posteriors: call it before the next iteration's posterior phase",
    ],
    "muxgl_fmx_ambient": [
        "muxgl_fmx_ambient: no pileup set (muxgl_set_pileup)",
        "muxgl_fmx_ambient: call muxgl_fmx_prepare first",
        "muxgl_fmx_ambient: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)",
        "muxgl_fmx_ambient: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep first)",
        "muxgl_fmx_ambient: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; the table "
        "belongs to an E-step's own posteriors: call it before the next iteration's posterior phase",
    ],
    "muxgl_fmx_ambient_fit": [
        "muxgl_fmx_ambient_fit: no pileup set (muxgl_set_pileup)",
        "muxgl_fmx_ambient_fit: call muxgl_fmx_prepare first",
        "muxgl_fmx_ambient_fit: no clusters set and no E-step run (muxgl_fmx_set_clusters, then muxgl_fmx_iterate)",
        "muxgl_fmx_ambient_fit: no E-step since muxgl_fmx_set_clusters (run muxgl_fmx_iterate or muxgl_fmx_iter_estep "
        "first)",
        "muxgl_fmx_ambient_fit: the cluster posteriors were rewritten (muxgl_fmx_iter_gp) since the last E-step; the fit "
        "belongs to an E-step's own posteriors: call it before the next iteration's posterior phase",
    ],
}
NONE, READY, STALE = 0, 1, 2  # FMX_SNG_*, checked against the header below


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "fmx_refusal_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "fmx_refusal_probe.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.probe_fmx_refusal.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint64]
    return lib


def rule(lib, who, what, have_pileup, prepared, K, state, n=256):
    """(return code, message) of the shared rule; the buffer is 256 bytes, as the callers'"""
    buf = C.create_string_buffer(b"\xff" * n, n)
    rc = lib.probe_fmx_refusal(who.encode(), what.encode(), have_pileup, prepared, K, state, buf, n)
    return rc, buf.value.decode() if rc else None  # (a call that may run leaves the buffer alone)


def old_rule(who, have_pileup, prepared, K, state):
    """the five functions' order of questions"""
    if not have_pileup:
        return OLD[who][0]
    if not prepared:
        return OLD[who][1]
    if K < 1:
        return OLD[who][2]
    if state == NONE:
        return OLD[who][3]
    if state != READY:
        return OLD[who][4]
    return None


def test_states_are_the_handles(probe):
    assert [probe.probe_fmx_sng_state(i) for i in range(3)] == [NONE, READY, STALE]


@pytest.mark.parametrize("who,what", CALLS)
def test_every_state_gives_the_old_text(probe, who, what):
    seen = set()
    for have_pileup in (0, 1):
        for prepared in (0, 1):
            for K in (0, 1, 300):
                for state in (NONE, READY, STALE):
                    rc, msg = rule(probe, who, what, have_pileup, prepared, K, state)
                    want = old_rule(who, have_pileup, prepared, K, state)
                    assert (rc, msg) == (0 if want is None else 1, want), (have_pileup, prepared, K, state)
                    seen.add(want)
    assert seen == set(OLD[who]) | {None}  # each of the five texts was met, and the call that may run


@pytest.mark.parametrize("who,what", CALLS)
def test_every_text_fits_the_callers_buffer(probe, who, what):
    assert max(len(t) for t in OLD[who]) < 256
    # a shorter buffer is cut, not overrun
    rc, msg = rule(probe, who, what, 1, 1, 2, STALE, n=40)
    assert rc == 1 and msg == OLD[who][4][:39]
