"""The randomised differential test of tests/test_fuzz_gpu.py on the two streamed paths: demuxlet's streamed call
(demux_stream.hip: stream_sweep_kernel, the top2 fold of stream_fold.hpp, stream_call_kernel) and freemuxlet's streamed
E-step (fmx_stream.hip: sweep, fold, call, and fmx_stream_rows for the exact pass), forced by flag from 33 to 255 samples /
clusters and as the product's own choice from 256 on.  The generator (stream_demux_case, stream_fmx_case) and what every
case asserts (run_stream_demux, run_stream_fmx) are in tests/test_fuzz_gpu.py, next to the cases they are made like; a
campaign is `python tests/test_fuzz_gpu.py --kind stream-demux|stream-fmx --seeds a:b`.

Every case: full_ll is refused (the documented sign of the streamed path) and the same handle then gives records that
equal the reference library's in every integer field (demuxlet: after the exact-call pass) with log-likelihoods within
1e-7; below 256 the records also equal those of the path the job takes without the flag; a run under a slab budget of
1 MB gives the bytes of the default budget; the singlet (and, below 256 samples, inclusion) tables of the same handle.

The seeds are chosen so that together they hold the checklist of test_seed_list_covers_the_streamed_paths, which needs
no GPU: a later edit of the generator cannot lose a structural case without that test saying so.
"""
import pytest

import ref_binding as rb
import test_fuzz_gpu as fz
from popscle_amd import muxgl

STREAM_SEEDS = {"stream-demux": [3, 10, 18, 31, 77, 102, 161, 180], "stream-fmx": [0, 19, 24, 78, 83, 113, 151, 195]}

needs_ref = pytest.mark.skipif(not rb.available(), reason="oracle/_ref/libscdrop_ref.so not built")


def test_seed_list_covers_the_streamed_paths():
    d = [fz.stream_demux_case(s)[0] for s in STREAM_SEEDS["stream-demux"]]
    X = muxgl.FLAG_FORCE_STREAMED_CALL
    for i in d:
        assert i["V"] in (fz.STREAM_DEMUX_V if i["flags"] & X else fz.STREAM_DEMUX_V_NATURAL) and (i["V"] > 255) == (not i["flags"] & X)
    assert any(i["V"] > 255 for i in d) and any(i["V"] <= 64 for i in d)           # natural; forced, a single block
    assert any(i["V"] % 64 == 1 for i in d) and any(i["V"] % 64 == 0 for i in d)
    assert any(0.5 not in i["alphas"] for i in d)
    assert any(len(i["alphas"]) == 1 and i["V"] > 255 for i in d)                  # singlets only, the product's path
    assert any(i["alphas"] == (0.0, 0.3) and i["V"] > 255 for i in d)              # no symmetric alpha, the product's path
    assert any(0.5 in i["alphas"] and i["alphas"][-1] != 0.5 for i in d)
    assert any(i["mode"] in ("all_same", "dup") for i in d)
    assert any(i["missing_gp"] >= 0.5 for i in d)
    assert any(i["empty_cells"] > 0 for i in d)
    assert any(i["ment"] == 1.5 for i in d)
    assert any(i["dp"] != 0.5 for i in d)
    assert any(i["how"] == "group" for i in d)
    assert any(i["flags"] & muxgl.FLAG_NO_LINEAR_ENTRIES for i in d)
    assert {i["run_slab"] for i in d} == {"1", None}

    f = [fz.stream_fmx_case(s)[0] for s in STREAM_SEEDS["stream-fmx"]]
    XE = muxgl.FLAG_FORCE_STREAMED_ESTEP
    for i in f:
        assert i["K"] in (fz.STREAM_FMX_K if i["flags"] & XE else fz.STREAM_FMX_K_NATURAL) and (i["K"] > 255) == (not i["flags"] & XE)
        assert i["K"] <= 255 or (i["C"] == i["K"] + 20 and i["ment"] <= 8)
    assert any(i["K"] > 255 for i in f) and any(i["K"] <= 64 for i in f)
    assert any(i["K"] % 64 == 1 for i in f) and any(i["K"] % 64 == 0 for i in f)
    assert {i["how"] for i in f} == {"one", "group", "shard"}
    assert any(i["K"] > 255 and i["how"] == "shard" for i in f)                    # fmx_stream_rows from several ranks, 12-bit prev
    assert any(i["start"] == "given" and (i["init"] < 0).any() for i in f)
    assert any(i["start"] == "partial" for i in f)
    assert any(i["flags"] & muxgl.FLAG_NO_PIVOT_SUMS for i in f) and any(i["flags"] & muxgl.FLAG_NO_LINEAR_ENTRIES for i in f)
    assert any(i["ment"] <= 3 for i in f)
    assert any(i["ment"] >= 120 and i["K"] <= 100 for i in f)
    assert {i["run_slab"] for i in f} == {"1", None}


@pytest.fixture(scope="module")
def eng():
    e = muxgl.Engine(0)
    yield e
    e.close()


_DONE = {}


def _case(eng, kind, seed):
    """the case's record, run once (the two tests across the seeds read what the per-seed tests left; a case that
    failed is not run again)"""
    if (kind, seed) not in _DONE:
        try:
            _DONE[kind, seed] = fz.run_case(eng, kind, seed)
        except BaseException as ex:
            _DONE[kind, seed] = ex
            raise
    if isinstance(_DONE[kind, seed], BaseException):
        raise _DONE[kind, seed]
    return _DONE[kind, seed]


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("seed", STREAM_SEEDS["stream-demux"])
def test_streamed_demuxlet_fuzz(eng, seed):
    _case(eng, "stream-demux", seed)


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("seed", STREAM_SEEDS["stream-fmx"])
def test_streamed_freemuxlet_fuzz(eng, seed):
    _case(eng, "stream-fmx", seed)


@pytest.mark.gpu
@needs_ref
def test_demuxlet_exact_pass_looked_at_streamed_records(eng):
    """across the seeds, the exact-call pass had work on records of the streamed call (near ties, DEEP bits from its
    third value): the cases are not all decided by a wide margin"""
    recs = [_case(eng, "stream-demux", s) for s in STREAM_SEEDS["stream-demux"]]
    assert sum(r["deep"] for r in recs) > 0 or sum(r["near"] for r in recs) > 0, [(r["seed"], r["deep"], r["near"]) for r in recs]


@pytest.mark.gpu
@needs_ref
def test_freemuxlet_exact_path_ran_on_streamed_handles(eng):
    """across the seeds, near-tie cells were settled on a streamed handle, whose rows come from fmx_stream_rows, and the
    records the reference agreed with show near-tie cells (parity.fmx_near_tie_mask, the count the fuzz reports)"""
    recs = [_case(eng, "stream-fmx", s) for s in STREAM_SEEDS["stream-fmx"]]
    seen = [(r["seed"], r["exact"], r["near"]) for r in recs]
    assert sum(r["exact"][0] for r in recs) > 0 and sum(r["near"] for r in recs) > 0, seen

