"""CPU test of the host side of the streamed paths (popscle_amd/csrc/stream_plan.hpp): the slab budget, the cut of
(cells x blocks) into groups whose slab fits it, and the block lists of the streamed demuxlet call and of the streamed
freemuxlet E-step.  The cut decides launch shapes; on a device only a budget of 1 MB reaches its second branch.

The header is compiled into a small shared object with hipcc (plain C++: no device code, no device is touched)."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VAR = "MUXGL_TEST_SLAB_MB"
GIB = 1 << 30


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "stream_plan_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "stream_plan_probe.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.probe_budget.argtypes = [C.c_char_p, C.c_uint64]
    lib.probe_budget.restype = C.c_uint64
    lib.probe_cut.argtypes = [C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.probe_cut.restype = None
    lib.probe_blocks.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int, C.POINTER(C.c_int32)]
    return lib


def cut(lib, cells, blocks, per, budget):
    gc, gb = C.c_int64(), C.c_int64()
    lib.probe_cut(cells, blocks, per, budget, C.byref(gc), C.byref(gb))
    return gc.value, gb.value


def budget(lib, total):
    return lib.probe_budget(VAR.encode(), total)


def blocks(lib, nblk, lower_only, stride):
    out = (C.c_int32 * (nblk * nblk))()
    n = lib.probe_blocks(nblk, int(lower_only), stride, nblk * nblk, out)
    assert n <= nblk * nblk
    return list(out[:n])


# ---- cut_groups
PER = 6 * 4096 * 8  # one (cell, block) of the streamed demuxlet call at six alphas


def test_everything_fits(probe):
    assert cut(probe, 1000, 25, PER, 8 * GIB) == (1000, 25)
    assert cut(probe, 1000, 25, PER, 1000 * 25 * PER) == (1000, 25)  # exactly
    assert cut(probe, 1, 1, PER, PER) == (1, 1)


def test_cells_fit_but_not_all_blocks(probe):
    assert cut(probe, 1000, 25, PER, 1000 * 25 * PER - 1) == (1000, 24)
    assert cut(probe, 1000, 25, PER, 7 * 1000 * PER + 5) == (1000, 7)
    assert cut(probe, 1000, 25, PER, 2 * 1000 * PER - 1) == (1000, 1)
    assert cut(probe, 1000, 25, PER, 1000 * PER) == (1000, 1)  # one block of every cell fits exactly


def test_one_block_of_every_cell_does_not_fit(probe):
    assert cut(probe, 1000, 25, PER, 1000 * PER - 1) == (999, 1)
    assert cut(probe, 2000, 15, PER, 1 << 20) == ((1 << 20) // PER, 1)  # the GPU tests' budget of 1 MB
    assert cut(probe, 1000, 25, PER, PER) == (1, 1)


def test_budget_below_one_cell_block(probe):
    for b in (0, 1, PER - 1):
        assert cut(probe, 1000, 25, PER, b) == (1, 1)
        assert cut(probe, 1, 1, PER, b) == (1, 1)


def test_caps(probe):
    assert cut(probe, 1, 100000, 8, 1 << 40) == (1, 65535)
    assert cut(probe, 1, 65535, 8, 1 << 40) == (1, 65535)
    assert cut(probe, 1, 65534, 8, 1 << 40) == (1, 65534)
    assert cut(probe, 1 << 41, 3, 1, 1 << 40) == (1 << 30, 1)
    assert cut(probe, 1 << 31, 3, 1, 1 << 40) == (1 << 30, 3)  # the cap holds on the first branch too
    assert cut(probe, 1 << 30, 3, 1, 1 << 40) == (1 << 30, 3)


def test_random_sweep_never_exceeds_the_budget(probe):
    rng = random.Random(20240)
    for _ in range(20000):
        cells = rng.choice([1, rng.randint(1, 100), rng.randint(1, 10 ** 6), rng.randint(1, 1 << 33)])
        nblk = rng.choice([1, rng.randint(1, 300), rng.randint(1, 200000)])
        per = rng.choice([1, 8, 32768, rng.randint(1, 1 << 22)])
        bud = rng.choice([0, rng.randint(0, 2 * per), rng.randint(0, 1 << 24), rng.randint(0, 1 << 36)])
        gc, gb = cut(probe, cells, nblk, per, bud)
        assert gc >= 1 and gb >= 1, (cells, nblk, per, bud)
        assert gc <= min(cells, 1 << 30) and gb <= min(nblk, 65535), (cells, nblk, per, bud)
        assert gc * gb * per <= max(bud, per), (cells, nblk, per, bud)
        assert gc == min(cells, 1 << 30) or gb == 1, (cells, nblk, per, bud)  # several blocks only with every cell


# ---- slab_budget_bytes
def test_budget_from_the_variable(probe, monkeypatch):
    monkeypatch.setenv(VAR, "1")
    assert budget(probe, 288 * GIB) == 1 << 20
    assert budget(probe, 0) == 1 << 20
    monkeypatch.setenv(VAR, "5000")
    assert budget(probe, 3 * GIB) == 5000 << 20  # the variable wins over the bound
    monkeypatch.setenv(VAR, "7")  # read at each call
    assert budget(probe, 288 * GIB) == 7 << 20


@pytest.mark.parametrize("value", [None, "0", "-3", "", "abc", "MB"])
def test_budget_default(probe, monkeypatch, value):
    if value is None:
        monkeypatch.delenv(VAR, raising=False)
    else:
        monkeypatch.setenv(VAR, value)
    assert budget(probe, 288 * GIB) == 4 * GIB
    assert budget(probe, 12 * GIB) == 4 * GIB  # a third of the device, exactly
    assert budget(probe, 12 * GIB - 3) == 4 * GIB - 1
    assert budget(probe, 6 * GIB) == 2 * GIB
    assert budget(probe, 0) == 4 * GIB  # device memory unknown


def test_budget_variables_are_separate(probe, monkeypatch):
    monkeypatch.setenv("MUXGL_DEMUX_SLAB_MB", "1")
    monkeypatch.delenv("MUXGL_FMX_SLAB_MB", raising=False)
    assert probe.probe_budget(b"MUXGL_DEMUX_SLAB_MB", 288 * GIB) == 1 << 20
    assert probe.probe_budget(b"MUXGL_FMX_SLAB_MB", 288 * GIB) == 4 * GIB


# ---- block lists
@pytest.mark.parametrize("nblk", [1, 2, 5, 16])
def test_block_lists(probe, nblk):
    full = [(X, Y) for X in range(nblk) for Y in range(nblk)]  # row by row
    lower = [(X, Y) for X in range(nblk) for Y in range(X + 1)]
    assert lower == [b for b in full if b[0] >= b[1]] and len(lower) == nblk * (nblk + 1) // 2
    # the streamed demuxlet call (codes X * nblk + Y): every block, or X >= Y when every doublet alpha is 0.5
    assert blocks(probe, nblk, False, nblk) == [X * nblk + Y for X, Y in full] == list(range(nblk * nblk))
    assert blocks(probe, nblk, True, nblk) == [X * nblk + Y for X, Y in lower]
    # the streamed freemuxlet E-step (codes X << 16 | Y): always X >= Y
    assert blocks(probe, nblk, True, 1 << 16) == [X << 16 | Y for X, Y in lower]
    assert blocks(probe, nblk, False, 1 << 16) == [X << 16 | Y for X, Y in full]
