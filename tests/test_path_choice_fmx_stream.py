"""CPU test of the streamed freemuxlet E-step's routing (popscle_amd/csrc/path_choice.hpp, choose_fmx_estep): beyond 255
clusters, under MUXGL_FLAG_FORCE_STREAMED_ESTEP beyond 32, and where the [C][K(K+1)/2] table does not fit the device.
With the two new facts at zero every answer is the one tests/test_path_choice.py pins.

The header is compiled into a small shared object with hipcc (plain C++: no device code, no device is touched)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from test_path_choice import ESTEP_BY_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

T, R, W, X, XE = 1, 2, 4, 2048, 4096  # FORCE_TILE_SWEEP, _ROW_KERNEL, _WAVE_KERNEL, _STREAMED_CALL, _STREAMED_ESTEP
ESTEP = ["oct", "row2", "wave", "pair", "stream"]
ALL_FMX = 1 | 2 | 4  # fqrow, qrow, row
DEV = 288e9


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "path_choice_fmx_stream_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "csrc", "path_choice_fmx_stream_probe.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.probe_fmx_estep2.argtypes = [C.c_int, C.c_int32, C.c_int64, C.c_int, C.c_double, C.c_int64, C.c_double,
                                     C.c_double]
    lib.probe_fll_bytes.argtypes = [C.c_int64, C.c_int]
    lib.probe_fll_bytes.restype = C.c_double
    return lib


def estep(lib, K, flags=0, S=200000, states=ALL_FMX, row2=1e6, items=2000, fll=0.0, dev=0.0):
    return ESTEP[lib.probe_fmx_estep2(K, flags, S, states, row2, items, fll, dev)]


@pytest.mark.parametrize("K", [256, 300, 512, 1024])
def test_beyond_255_clusters_always_streams(probe, K):
    for flags in (0, T, R, W, X, XE, T | R | W | X | XE):
        for states, items in ((ALL_FMX, 2000), (0, 0)):
            assert estep(probe, K, flags, states=states, items=items) == "stream", (K, flags, states)
            assert estep(probe, K, flags, states=states, items=items, fll=1e9, dev=DEV) == "stream"


def test_flag_streams_above_32_only(probe):
    for K in (33, 48, 64, 65, 128, 200, 255):
        for extra in (0, T, R, W):
            assert estep(probe, K, XE | extra) == "stream", (K, extra)
    for K in sorted(ESTEP_BY_K):
        if K <= 32:  # the old answer under every other flag
            assert tuple(estep(probe, K, f | XE) for f in (0, T, R, W)) == ESTEP_BY_K[K], K
    assert estep(probe, 64, X) == "wave"  # demuxlet's flag is not freemuxlet's


def test_fit_rule_at_its_boundary(probe):
    for K in (8, 24, 64, 255):
        edge = 0.9 * DEV
        assert estep(probe, K, fll=edge, dev=DEV) != "stream", K
        assert estep(probe, K, fll=edge * (1 + 1e-12), dev=DEV) == "stream", K
        assert estep(probe, K, fll=1e15, dev=0.0) != "stream", K  # device memory unknown: the old answer
        assert estep(probe, K, fll=0.0, dev=DEV) != "stream", K
    # the table's bytes: a row of K(K+1)/2 doubles per cell and extra part
    assert probe.probe_fll_bytes(1000, 255) == 1000 * 255 * 256 / 2 * 8
    assert probe.probe_fll_bytes(500_000, 255) > 130e9


@pytest.mark.parametrize("K", sorted(ESTEP_BY_K))
def test_old_table_unchanged_with_zero_facts(probe, K):
    assert tuple(estep(probe, K, f) for f in (0, T, R, W)) == ESTEP_BY_K[K]
    assert tuple(estep(probe, K, f, fll=1e9, dev=DEV) for f in (0, T, R, W)) == ESTEP_BY_K[K]
