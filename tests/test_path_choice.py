"""CPU test of the routing table (popscle_amd/csrc/path_choice.hpp): which kernel path each demuxlet and freemuxlet
decision picks, case by case, on both sides of every boundary.  The choosers are the only place the launchers ask, so
this table is the routing the library runs.

The header is compiled into a small shared object with hipcc (plain C++: no device code, no device is touched)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

T, R, W, X = 1, 2, 4, 2048  # MUXGL_FLAG_FORCE_TILE_SWEEP, _ROW_KERNEL, _WAVE_KERNEL, _STREAMED_CALL
DEMUX = ["stream", "oct8", "oct16", "row", "row2", "wave", "tile"]
ESTEP = ["oct", "row2", "wave", "pair"]

DEFAULT = (0.0, 0.5)
SIX = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5)
FIVE_PLAIN = (0.0, 0.1, 0.2, 0.3, 0.4, 0.6, 0.5)   # five values other than 0.5 beside alpha[0]: still the row kernel
SEVEN_PLAIN = (0.0, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7)  # six beside alpha[0]
SINGLETS = (0.0,)
ROW2_LIMIT, WAVE_LIMIT = 64e9, 230e9
ALL_DEMUX = 1 | 2 | 4 | 8 | 16  # row, qrow, d_gpq, d_qent, wave
ALL_FMX = 1 | 2 | 4  # fqrow, qrow, row


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "path_choice_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "csrc", "path_choice_probe.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.probe_demux.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int32, C.c_int64, C.c_int64, C.c_int,
                                C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int)]
    lib.probe_wave_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int]
    lib.probe_wave_bytes.restype = C.c_double
    lib.probe_fmx_estep.argtypes = [C.c_int, C.c_int32, C.c_int64, C.c_int, C.c_double, C.c_int64]
    lib.probe_fmx_call.argtypes = [C.c_int, C.c_int32]
    lib.probe_fmx_mstep.argtypes = [C.c_int, C.c_int32, C.c_int64, C.c_int64, C.c_int64]
    lib.probe_greedy.argtypes = [C.c_int, C.c_int32, C.c_int64, C.c_int, C.c_int]
    return lib


def demux(lib, V, alpha=DEFAULT, flags=0, states=ALL_DEMUX, C_=2000, S=200000, full_ll=False, row2=1e6, wave=1e9,
          dev=288e9):
    a = (C.c_double * len(alpha))(*alpha)
    ll = C.c_int()
    p = lib.probe_demux(V, len(alpha), a, flags, C_, S, states, int(full_ll), row2, wave, dev, C.byref(ll))
    return DEMUX[p], bool(ll.value)


# V: (default grid, six alphas, {0.1, 0.5}, {0.5, 0.5}, {0.0, 0.5, 0.5}, five non-0.5, seven non-0.5, singlets only)
BY_V = {
    1: ("oct8", "row", "row", "row", "tile", "row", "tile", "row"),
    16: ("oct8", "row", "row", "row", "tile", "row", "tile", "row"),
    17: ("oct16", "wave", "row2", "wave", "wave", "wave", "wave", "tile"),
    32: ("oct16", "wave", "row2", "wave", "wave", "wave", "wave", "tile"),
    33: ("wave",) * 7 + ("tile",),
    64: ("wave",) * 7 + ("tile",),
    65: ("tile",) * 8,
    72: ("tile",) * 8,
    73: ("wave",) * 7 + ("tile",),
    127: ("wave",) * 7 + ("tile",),
    128: ("wave",) * 7 + ("tile",),
    255: ("wave",) * 7 + ("tile",),
    256: ("stream",) * 8,
}
GRIDS = (DEFAULT, SIX, (0.1, 0.5), (0.5, 0.5), (0.0, 0.5, 0.5), FIVE_PLAIN, SEVEN_PLAIN, SINGLETS)


@pytest.mark.parametrize("V", sorted(BY_V))
def test_demux_by_samples_and_grid(probe, V):
    got = tuple(demux(probe, V, g)[0] for g in GRIDS)
    assert got == BY_V[V]


# (V, grid, flags, expected)
FLAGS = [
    (8, DEFAULT, T, "tile"), (24, DEFAULT, T, "tile"), (64, DEFAULT, T, "tile"), (300, DEFAULT, T, "stream"),
    (64, DEFAULT, T | X, "stream"),
    (8, DEFAULT, R, "row"), (24, DEFAULT, R, "row2"), (24, SIX, R, "wave"), (64, DEFAULT, R, "wave"),
    (8, DEFAULT, W, "wave"), (8, SIX, W, "wave"), (8, SINGLETS, W, "tile"), (24, DEFAULT, W, "wave"),
    (24, (0.1, 0.5), W, "wave"), (64, DEFAULT, W, "wave"), (65, DEFAULT, W, "tile"),
    (8, DEFAULT, X, "oct8"), (32, DEFAULT, X, "oct16"), (33, DEFAULT, X, "stream"), (65, SIX, X, "stream"),
    (33, SINGLETS, X, "stream"),
]


@pytest.mark.parametrize("V,grid,flags,want", FLAGS)
def test_demux_flags(probe, V, grid, flags, want):
    assert demux(probe, V, grid, flags)[0] == want


# (V, grid, states, expected)
STATES = [
    (8, DEFAULT, ALL_DEMUX & ~2, "row"), (8, DEFAULT, ALL_DEMUX & ~4, "row"), (8, DEFAULT, ALL_DEMUX & ~8, "row"),
    (24, DEFAULT, ALL_DEMUX & ~2, "row2"), (24, DEFAULT, ALL_DEMUX & ~8, "row2"),
    (24, DEFAULT, ALL_DEMUX & ~(2 | 1), "wave"), (8, SIX, ALL_DEMUX & ~1, "tile"), (24, (0.1, 0.5), ALL_DEMUX & ~1, "wave"),
    (24, SIX, ALL_DEMUX & ~16, "tile"), (64, DEFAULT, ALL_DEMUX & ~16, "tile"), (8, DEFAULT, 2 | 4 | 8, "oct8"),
]


@pytest.mark.parametrize("V,grid,states,want", STATES)
def test_demux_missing_states(probe, V, grid, states, want):
    assert demux(probe, V, grid, states=states)[0] == want


def test_demux_oct_offset_limit(probe):
    # (S + 1) * 32 * P < 2^32: P = 8 up to 16 samples, 16 beyond
    assert demux(probe, 8, S=2**24 - 2)[0] == "oct8"
    assert demux(probe, 8, S=2**24 - 1)[0] == "row"
    assert demux(probe, 24, S=2**23 - 2)[0] == "oct16"
    assert demux(probe, 24, S=2**23 - 1)[0] == "row2"


def test_demux_row2_partials(probe):
    g = (0.1, 0.5)
    assert demux(probe, 24, g, row2=ROW2_LIMIT)[0] == "row2"
    assert demux(probe, 24, g, row2=ROW2_LIMIT * (1 + 1e-15))[0] == "wave"
    assert demux(probe, 24, g, row2=ROW2_LIMIT * (1 + 1e-15), wave=WAVE_LIMIT * 2)[0] == "tile"


def test_demux_wave_bytes_and_device_memory(probe):
    V, A, C_ = 64, 2, 1000
    tile = C_ * V * V * A * 8.0
    fits, over = WAVE_LIMIT, WAVE_LIMIT * (1 + 1e-15)
    assert demux(probe, V, C_=C_, wave=fits, dev=tile)[0] == "wave"
    # beyond 230 GB: the tile sweep if its tensor takes at most 0.9 of the device, else the streamed call
    assert demux(probe, V, C_=C_, wave=over, dev=tile / 0.9 * (1 + 1e-12))[0] == "tile"
    assert demux(probe, V, C_=C_, wave=over, dev=tile / 0.9 * (1 - 1e-12))[0] == "stream"
    assert demux(probe, V, C_=C_, wave=over, dev=0.0)[0] == "tile"  # device memory unknown
    assert demux(probe, V, SINGLETS, C_=C_, wave=over, dev=1.0)[0] == "tile"  # singlets only: never streamed here
    # up to 32 samples the fit rule does not apply
    assert demux(probe, 24, SIX, C_=C_, wave=over, dev=1.0)[0] == "tile"
    assert demux(probe, 8, SIX, flags=W, C_=C_, wave=over, dev=1.0)[0] == "tile"


def test_demux_wave_bytes_formula(probe):
    for nnz, C_, n_over, V, A in [(0, 1, 0, 17, 2), (10**9, 2000, 37, 64, 6), (5 * 10**8, 1000, 0, 65, 2),
                                  (123456789, 4321, 99, 255, 16)]:
        nblk = (V + 63) // 64
        want = (nnz * A * 9 + (C_ + n_over) * nblk * nblk * A * 4096 + (C_ * V * V * A if nblk > 1 else 0)) * 8.0
        assert probe.probe_wave_bytes(nnz, C_, n_over, V, A) == want


# (V, grid, flags, full_ll, ll_first)
LL_FIRST = [
    (8, DEFAULT, 0, False, True), (8, SIX, 0, False, True), (8, DEFAULT, W, False, True), (8, DEFAULT, T, False, True),
    (24, DEFAULT, 0, False, False), (24, DEFAULT, 0, True, True), (24, (0.1, 0.5), 0, False, False),
    (24, (0.1, 0.5), 0, True, True), (24, SIX, 0, True, True), (24, SIX, 0, False, False), (24, DEFAULT, W, True, False),
    (24, DEFAULT, T, False, True), (64, DEFAULT, 0, True, False), (65, DEFAULT, 0, False, True),
    (300, DEFAULT, 0, False, False),
]


@pytest.mark.parametrize("V,grid,flags,full_ll,want", LL_FIRST)
def test_demux_ll_tensor_before_the_sweep(probe, V, grid, flags, full_ll, want):
    assert demux(probe, V, grid, flags, full_ll=full_ll)[1] == want


def estep(lib, K, flags=0, S=200000, states=ALL_FMX, row2=1e6, items=2000):
    return ESTEP[lib.probe_fmx_estep(K, flags, S, states, row2, items)]


# K: (no flags, T, R, W)
ESTEP_BY_K = {
    1: ("oct", "pair", "pair", "oct"),
    16: ("oct", "pair", "pair", "oct"),
    17: ("row2", "pair", "row2", "pair"),
    24: ("row2", "pair", "row2", "pair"),
    25: ("row2", "pair", "row2", "pair"),
    32: ("row2", "pair", "row2", "pair"),
    33: ("wave", "pair", "wave", "wave"),
    64: ("wave", "pair", "wave", "wave"),
    65: ("wave", "pair", "wave", "wave"),
    255: ("wave", "pair", "wave", "wave"),
}


@pytest.mark.parametrize("K", sorted(ESTEP_BY_K))
def test_fmx_estep_by_clusters_and_flags(probe, K):
    assert tuple(estep(probe, K, f) for f in (0, T, R, W)) == ESTEP_BY_K[K]


def test_fmx_estep_states_and_limits(probe):
    assert estep(probe, 8, states=2 | 4) == "oct"  # the oct tables are cut from qrow on first use
    assert estep(probe, 8, states=1 | 4) == "oct"  # a shard's own tables
    assert estep(probe, 8, states=4) == "pair"
    assert estep(probe, 8, S=2**23 - 2) == "oct"
    assert estep(probe, 8, S=2**23 - 1) == "pair"
    assert estep(probe, 24, states=1 | 2) == "pair"  # no row tables
    assert estep(probe, 24, row2=ROW2_LIMIT) == "row2"
    assert estep(probe, 24, row2=ROW2_LIMIT * (1 + 1e-15)) == "pair"
    assert estep(probe, 48, items=0) == "pair"
    assert estep(probe, 48, states=0) == "wave"


def test_fmx_call(probe):
    for K, flags, want in [(2, 0, 0), (16, 0, 0), (24, 0, 0), (25, 0, 1), (64, 0, 1), (255, 0, 1), (48, T, 0),
                           (48, R | W, 1)]:
        assert probe.probe_fmx_call(K, flags) == want, (K, flags)  # 0 lane per cell, 1 wave per cell


def test_fmx_mstep(probe):
    for K, flags, ns, nnz, C_, want in [(2, 0, 10, 10, 10, 0), (64, 0, 10, 10, 10, 0), (65, 0, 10, 10, 10, 1),
                                        (16, T, 10, 10, 10, 1), (16, R | W, 10, 10, 10, 0), (16, 0, 0, 10, 10, 1),
                                        (16, 0, 10, 0, 10, 1), (16, 0, 10, 10, 0, 1)]:
        assert probe.probe_fmx_mstep(K, flags, ns, nnz, C_) == want, (K, flags, ns, nnz, C_)  # 0 stream, 1 chain


def test_greedy(probe):
    gb = 128
    for K, flags, P, cus, want in [(16, 0, 10**6, 256, 0), (64, 0, 10**6, 256, 0), (65, 0, 10**6, 256, 1),
                                   (16, 0, 0, 256, 1), (16, 0, 2**31 - 1, 256, 0), (16, 0, 2**31, 256, 1),
                                   (16, T, 10**6, 256, 1), (16, R | W, 10**6, 256, 0), (16, 0, 10**6, 255, 1)]:
        assert probe.probe_greedy(K, flags, P, cus, gb) == want, (K, flags, P, cus)  # 0 batched, 1 serial
