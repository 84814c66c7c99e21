"""CPU test of the call sequences a long-lived handle is put through (tests/handle_sequences.py): the generator, the
lifecycle model and the routing table of popscle_amd/csrc/path_choice.hpp (through tests/csrc/path_choice_probe.cpp,
as tests/test_path_choice.py compiles it) must, over the seed list that tests/test_handle_sequences_gpu.py runs, reach
every transition listed in handle_sequences.required_coverage().  Nothing here touches a device."""
import ctypes as C
import os
import shutil
import subprocess
from collections import Counter

import pytest

import handle_sequences as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# The sequences of the suite: twelve random seeds, chosen (by a search over seeds 0..40000 with this file's own
# coverage function) so that together with the eight constructed sequences they reach every required item; three of
# them are multiples of four and run on a device group.
RANDOM_SEEDS = (4329, 6072, 7080, 15387, 15605, 16264, 20640, 21330, 21331, 27829, 31590, 36493)
SEEDS = RANDOM_SEEDS + hs.CONSTRUCTED_SEEDS
DEVICE_BYTES = 288e9   # what the fit rules compare with; the sequences' jobs are far below every limit


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
    return lib


def _parts_over(longest):
    """extra parts of the cells beyond 2048 entries (the wave plan's n_over): every pileup here has at most one"""
    return (longest + 2047) // 2048 - 1 if longest > 2048 else 0


def demux_path(lib):
    """the path of a demux_run as demux_launch gathers its facts (demux_kernels.hip) for a pileup (C, S, nnz, longest cell)"""
    def f(V, grid, flags, facts, full_ll):
        Cn, S, nnz, longest = facts
        # after muxgl_set_pileup the row, quad and wave plans exist; the packed quad records when there are entries;
        # the oct layout of the panel up to 32 samples
        states = 1 | 2 | (4 if V <= 32 and S > 0 else 0) | (8 if nnz > 0 else 0) | 16
        a = (C.c_double * len(grid))(*grid)
        ll = C.c_int()
        wave = lib.probe_wave_bytes(nnz, Cn, _parts_over(longest), V, len(grid))
        got = lib.probe_demux(V, len(grid), a, flags, Cn, S, states, int(full_ll), 1e6, wave, DEVICE_BYTES, C.byref(ll))
        return ["stream", "oct8", "oct16", "row", "row2", "wave", "tile"][got]   # enum class demux_path
    return f


def estep_path(lib):
    """the path of an E-step as fmx_phase_estep gathers its facts (fmx_kernels.hip); beyond 255 clusters
    muxgl_fmx_set_clusters has chosen the streamed one"""
    def f(K, flags, facts):
        Cn, S, nnz, longest = facts
        return ["oct", "row2", "wave", "pair", "stream"][lib.probe_fmx_estep(K, flags, S, 2 | 4, 1e6, Cn + _parts_over(longest))]
    return f


@pytest.fixture(scope="module")
def reached(probe):
    dp, ep = demux_path(probe), estep_path(probe)
    return {seed: hs.coverage(seed, dp, ep) for seed in SEEDS}


def test_seed_list_shape():
    assert len(SEEDS) == len(set(SEEDS)) <= 20
    assert sum(hs.is_group(s) for s in SEEDS) >= 3 and not any(hs.is_group(s) for s in hs.CONSTRUCTED_SEEDS)
    for seed in SEEDS:
        seq = hs.sequence(seed)
        assert 1 <= len(seq) <= hs.MAX_STEPS, seed
        assert seq == hs.sequence(seed), "a sequence is a function of its seed"


def test_every_required_transition_is_reached(reached):
    req = hs.required_coverage()
    counts = Counter(item for got in reached.values() for item in got if item in req)
    missing = sorted(req - set(counts))
    print(f"{len(req)} required items, reached {len(counts)}; fewest visits: {sorted(counts.values())[:5]}")
    assert not missing, missing
    # the groups of the list, by name, so that a failure says what kind of thing went missing
    assert sum(1 for k in counts if k[0] == "demux") == 49 and sum(1 for k in counts if k[0] == "estep") == 25
    assert sum(1 for k in counts if k[0] == "refusal") == len(hs.REFUSALS)
    assert sum(1 for k in counts if k[0] == "budget") == len(hs.TABLES) == 7


def test_hints_are_the_routing_table(probe):
    """the generator aims at paths with a restatement of the choosers for small jobs: it must agree with path_choice.hpp
    on everything the vocabulary can ask"""
    dp, ep = demux_path(probe), estep_path(probe)
    facts = (40, 3000, 4000, 2500)
    for flags in (0, hs.FLAG_R, hs.FLAG_W):
        for V in hs.PANEL_V:
            for g in hs.GRIDS.values():
                for full in (False, True):
                    assert dp(V, g, flags, facts, full) == hs.hint_demux_path(V, g, flags), (V, g, flags)
        for K in hs.CLUSTER_K:
            assert ep(K, flags, facts) == hs.hint_estep_path(K, flags), (K, flags)


def test_model_refuses_demuxlet_after_a_new_pileup_without_a_panel():
    """set_pileup -> demux_* without a panel: refused, for every demuxlet call and the donor match, on one device and on
    a group; and so is muxgl_demux_get_entry_pg, whose grid went with the panel"""
    pl = hs.pl_facts(1)
    for group in (False, True):
        m = hs.Lifecycle(pl, 0, group)
        for st in (dict(op="load", i=0), dict(op="panel", V=8, mode="hard"), dict(op="demux_run", grid="default", full_ll=False),
                   dict(op="fmx_prepare"), dict(op="set_clusters", K=3), dict(op="iterate", full_ll=False)):
            assert m.apply(st) is None
        assert m.refusal(dict(op="demux_entry_pg")) is None and m.refusal(dict(op="demux_singlets", grid="default")) is None
        assert m.apply(dict(op="load", i=2)) is None   # fewer SNPs than pileup 0
        assert pl[2][1] < pl[0][1]
        want = {"demux_run": "group_run_no_pileup_or_panel" if group else "demux_no_panel", "demux_singlets": "demux_no_panel",
                "demux_inclusion": "demux_no_panel", "demux_unknown": "demux_no_panel", "demux_entry_pg": "entry_pg_no_run"}
        for op, why in want.items():
            st = dict(op=op, grid="default", full_ll=False)
            assert m.refusal(st) == why, (op, group)
            assert m.apply(st) == why and m.panel is None   # a refused call changes nothing
        assert "no GP tensor set (muxgl_demux_set_gp)" in hs.REFUSALS["demux_no_panel"]
        # the freemuxlet job went too; the match asks for it first
        assert m.refusal(dict(op="fmx_match_donors")) == ("group_match" if group else "match_not_prepared")
        assert m.refusal(dict(op="iterate", full_ll=False)) == "iterate_no_clusters"


def test_refused_steps_are_about_one_in_eight():
    n = r = 0
    for seed in range(200):
        seq = hs.sequence(seed)
        n += len(seq)
        r += sum(st["expect"] is not None for st in seq)
    assert 0.06 < r / n < 0.25, r / n


def test_stale_state_steps_go_from_the_larger_problem_to_the_smaller():
    """wherever a call that reads the panel is made without one on a handle that had one before, the pileup in force has
    fewer SNPs than the one that panel was made for: even a library that kept the panel would stay inside it"""
    seen = 0
    for seed in SEEDS + tuple(range(300)):
        flags, seq = hs.sequence_and_flags(seed)
        pl = hs.pl_facts(seed)
        cur, paneled, panel_S = None, False, None
        for st in seq:
            if st["op"] == "load":
                cur, paneled = st["i"], False
            elif st["op"] == "panel":
                paneled, panel_S = True, pl[cur][1]
            elif st["op"] in hs.PANEL_READERS and not paneled and panel_S is not None:
                assert st["expect"] is not None, (seed, st)
                assert pl[cur][1] < panel_S, (seed, st)
                seen += 1
    assert seen > 0
