"""The finish of the default-grid demuxlet path (demux_oct.hip) against the CPU oracle: eight-byte chunk partials with
their escape, the slot table, the trips over a cell's chunks in the fused finish kernel (four chunks a trip) and in the
reduce kernel behind the LL tensor (eight), at eight and at sixteen lanes per entry.

Bar, as tests/test_demux_gpu.py: calls exact, log-likelihoods within 1e-7 (the bar of tests/parity.py is 1e-5); the
records made in LDS equal, bit for bit, those made behind the tensor.
"""
import numpy as np
import pytest

import oracle_binding as ob
import parity
from popscle_amd import muxgl, synth

pytestmark = pytest.mark.gpu

ALPHAS = (0.0, 0.5)
CHUNK = 192  # entries of a chunk of the oct sweep


@pytest.fixture(scope="module")
def eng():
    e = muxgl.Engine(0)
    yield e
    e.close()


def check(eng, p, V):
    """records and LL tensor against the oracle, with and without the tensor requested; returns the oracle's tensor"""
    want, wfull = ob.demux(p, alphas=ALPHAS, full_ll=True, nthreads=4)
    eng.set_pileup(p.S, p.cell_ptr, p.entry_snp, p.entry_rptr, p.reads)
    eng.demux_set_gp(p.gp, p.has_gp)
    without = eng.demux_run(ALPHAS, 0.5)
    with_tensor, gfull = eng.demux_run(ALPHAS, 0.5, want_full_ll=True)
    again = eng.demux_run(ALPHAS, 0.5)  # (the partials of the tensor run are what this one overwrites)
    rep = parity.compare_demux(without, want, ALPHAS, p)
    worst = parity.compare_full_ll(gfull, wfull, V, ALPHAS)
    print(f"V={V} C={p.C}: max |dLL| records {rep['max_abs_ll_diff']:.3e}, tensor {worst:.3e}")
    assert rep["max_abs_ll_diff"] < 1e-7 and worst < 1e-7
    assert without.tobytes() == with_tensor.tobytes() == again.tobytes()
    return wfull


def pileup_of(lens, S, V, seed, reads_of=None, gp=None):
    """cells of exactly lens[i] entries on distinct random SNPs, 1 + Poisson(0.3) random reads per entry (or reads_of(n))"""
    rng = np.random.default_rng(seed)
    base = synth.make_pileup(4, S, V, seed=seed, mean_entries=20, min_entries=5)
    cell_ptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=cell_ptr[1:])
    nnz = int(cell_ptr[-1])
    entry_snp = np.concatenate([np.sort(rng.choice(S, n, replace=False)) for n in lens] +
                               [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    nreads = 1 + rng.poisson(0.3, size=nnz) if reads_of is None else reads_of(nnz)
    entry_rptr = np.zeros(nnz + 1, dtype=np.int64)
    np.cumsum(nreads, out=entry_rptr[1:])
    R = int(entry_rptr[-1])
    reads = ((rng.integers(0, 2, R) << 7) | rng.integers(13, 41, R)).astype(np.uint8)
    return synth.Pileup(len(lens), S, cell_ptr, entry_snp, entry_rptr, reads, base.af, base.gp if gp is None else gp,
                        base.has_gp)


@pytest.mark.parametrize("V", [1, 2, 7, 16, 17, 32])
def test_few_cells_not_a_multiple_of_four(eng, V):
    """thirteen cells (the last workgroup of four cells holds one), about forty entries each: one chunk per cell, every
    shape of the slot table -- a lone sample, fewer samples than positions, all sixteen, and the sixteen-lane tiling"""
    p = synth.make_pileup(13, 500, V, seed=6100 + V, mean_entries=40, min_entries=5)
    check(eng, p, V)


SPECIAL = [0, 1, CHUNK, CHUNK + 1, 4 * CHUNK, 4 * CHUNK + 1, 8 * CHUNK + 1]  # 0, 1, 1, 2, 4, 5 and 9 chunks
FILL = [40, 300]


@pytest.mark.parametrize("V,shifts", [(16, range(9)), (20, (0, 4, 8))])
def test_chunk_counts_at_the_trip_boundaries(eng, V, shifts):
    """cells of exactly 0, 1, 192, 193, 768, 769 and 1537 entries -- no chunk, one, a full one, two, a full trip of the
    finish kernel, one more, and one more than a trip of the reduce kernel -- in a pileup of nine cells, rotated so that
    each of them is the first cell, the last one and one in the middle"""
    for r in shifts:
        lens = np.roll(np.array(SPECIAL + FILL), r).tolist()
        p = pileup_of(lens, 2000, V, seed=6200 + 16 * V + r)
        assert np.diff(p.cell_ptr).tolist() == lens
        check(eng, p, V)


@pytest.mark.parametrize("V", [16, 20])
def test_a_chunk_that_leaves_the_exponent_field(eng, V):
    """one cell of 192 entries of two or three ALT reads of quality 60 each, the last sample called hom-ref everywhere
    with (nearly) no error mixing: its singlet hypothesis loses ~2^-33 per entry, more than 2^-4094 within the one chunk,
    which the twelve exponent bits of an eight-byte partial cannot hold (the escape through the exponent array)"""
    S = 400
    rng = np.random.default_rng(6300 + V)
    G = rng.binomial(2, 0.35, size=(S, V))
    G[:, 0] = 2       # the donor of the deep cell
    G[:, V - 1] = 0   # the sample every read contradicts
    gp = synth.gt_to_gp(G.astype(np.int64), 1e-12)
    lens = [60, CHUNK, 45]
    p = pileup_of(lens, S, V, seed=6300 + V, reads_of=lambda n: 2 + rng.integers(0, 2, size=n), gp=gp)
    e0, e1 = int(p.cell_ptr[1]), int(p.cell_ptr[2])
    p.reads[p.entry_rptr[e0]:p.entry_rptr[e1]] = 0x80 | 60
    assert e1 - e0 == CHUNK  # one chunk
    want, wfull = ob.demux(p, alphas=ALPHAS, full_ll=True, nthreads=4)
    lost = wfull[1][parity.needed_ll_mask(V, ALPHAS)].min()
    print(f"V={V}: the deep cell's worst hypothesis has LL {lost:.1f}; 2^-4094 is {-4094 * np.log(2):.1f}")
    assert lost < -4094 * np.log(2)  # the precondition: otherwise no partial escapes and the test shows nothing
    check(eng, p, V)
