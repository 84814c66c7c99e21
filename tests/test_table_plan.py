"""CPU test of the host side of the three per-droplet tables (popscle_amd/csrc/table_plan.hpp): which cells go into
which batch, how a cell is cut into parts, and the order of the work items, for muxgl_demux_singlets, muxgl_fmx_singlets
and muxgl_demux_unknown.  The plan decides which slab row every part of every droplet lands in; on a device only a
budget of 1 MB reaches more than one batch.

The three callers once carried this as loops of their own.  Those loops are restated here in Python (old_*), and the
plan is held to them: the same batch ends and maxima, the same (e0, e1, row) of every item, the same cuts / cell
records.  Beside that the properties the callers' header comments promise are asserted on the plan alone.

The header is compiled into a small shared object with hipcc (plain C++: no device code, no device is touched)."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PART = 2048
DEMUX, FMX, UNKNOWN = 0, 1, 2  # the callers, as tests/csrc/table_plan_probe.cpp numbers them
SIZEOF_ITEM, SIZEOF_CELL = 24, 16
EDGES = [0, 1, 2047, 2048, 2049, 4096, 4097, 6145, 0, 5, 300, 0]
WIDTHS = [1, 3, 16, 64, 65, 300]
ALPHAS = [2, 4, 7]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    so = str(tmp_path_factory.mktemp("probe") / "table_plan_probe.so")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                        "-I", os.path.join(ROOT, "popscle_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "table_plan_probe.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    p64 = C.POINTER(C.c_int64)
    lib.probe_table_part.restype = C.c_int64
    lib.probe_table_unknown_bytes.argtypes = [C.c_int64, C.c_int, C.c_int]
    lib.probe_table_unknown_bytes.restype = C.c_uint64
    lib.probe_table_exceeds.argtypes = [C.c_double, C.c_double]
    lib.probe_table_plan.argtypes = [C.c_int, p64, C.c_int64, C.c_uint64, C.c_int, C.c_int, p64, p64, p64]
    lib.probe_table_plan.restype = C.c_int64
    lib.probe_table_fill.argtypes = [C.c_int, p64, C.c_int64, C.c_int64, p64, p64, p64]
    lib.probe_table_fill.restype = C.c_int64
    lib.probe_table_alone_message.argtypes = [C.c_int, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_char_p,
                                              C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.probe_table_alone_message.restype = None
    lib.probe_table_launch_message.argtypes = [C.c_int, C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                               C.c_char_p, C.c_size_t]
    lib.probe_table_launch_message.restype = None
    return lib


def cell_ptr_of(lens):
    cp = [0]
    for n in lens:
        cp.append(cp[-1] + n)
    return cp


# ---- the loops of the three callers before table_plan.hpp, restated
def old_parts(caller, n):
    if caller == FMX:  # fmx_singlets.hip: len > PART ? ceil(len / PART) : 1
        return (n + PART - 1) // PART if n > PART else 1
    return max(1, (n + PART - 1) // PART)  # demux_singlets.hip, demux_unknown.hip


def old_bytes_of(n, A, V):
    """demux_unknown.hip's bytes_of: the entries' weights, the slab rows (one per part) with their items, the rows of the
    three tables with the cell's record"""
    row_bytes = 8 * A * 2 * (V + 1)
    return n * A * 6 * 8 + old_parts(UNKNOWN, n) * (row_bytes + SIZEOF_ITEM) + row_bytes + SIZEOF_CELL


def old_plan(caller, cp, budget, A, V):
    """(batch ends, (max_rows, max_cells, max_cuts, max_entries), refused cell or -1); the budget is rows_cap for the
    singlet tables and bytes for the unknown-donor call, which refuses a cell that exceeds it alone"""
    Cn = len(cp) - 1
    ln = lambda c: cp[c + 1] - cp[c]
    if caller == UNKNOWN:
        cost = lambda c: old_bytes_of(ln(c), A, V)
    else:
        cost = lambda c: old_parts(caller, ln(c))
    ends, mx = [], [0, 0, 0, 0]
    c0 = 0
    while c0 < Cn:
        if caller == UNKNOWN and cost(c0) > budget:
            return None, None, c0
        used, rows, cuts, c1 = 0, 0, 0, c0
        while c1 < Cn and (c1 == c0 or used + cost(c1) <= budget):
            used += cost(c1)
            rows += old_parts(caller, ln(c1))
            cuts += old_parts(caller, ln(c1)) > 1
            c1 += 1
        ends.append(c1)
        mx = [max(mx[0], rows), max(mx[1], c1 - c0), max(mx[2], cuts), max(mx[3], cp[c1] - cp[c0])]
        c0 = c1
    return ends, tuple(mx), -1


def old_fill(caller, cp, c0, c1):
    """(items, records): the cuts (row, first, count) of the singlet tables, the (first, count) of every cell of the
    unknown-donor call"""
    items, recs = [], []
    over = c1 - c0  # first free row behind the cells' own
    for c in range(c0, c1):
        b, e = cp[c], cp[c + 1]
        n, np_ = e - b, old_parts(caller, e - b)
        if caller == FMX:
            items.append((b, b + n // np_, c - c0))
        else:
            items.append((b, min(e, b + PART), c - c0))
        if caller == UNKNOWN:
            recs.append((over, np_ - 1))
        elif np_ > 1:
            recs.append((c - c0, over, np_ - 1))
        for k in range(1, np_):
            if caller == FMX:
                items.append((b + n * k // np_, b + n * (k + 1) // np_, over))
            else:
                items.append((b + k * PART, min(e, b + (k + 1) * PART), over))
            over += 1
    return items, recs


# ---- the plan through the shim
def new_plan(lib, caller, cp, budget, A, V):
    Cn = len(cp) - 1
    arr = (C.c_int64 * len(cp))(*cp)
    ends = (C.c_int64 * max(1, Cn))()
    mx = (C.c_int64 * 4)()
    over = C.c_int64()
    n = lib.probe_table_plan(caller, arr, Cn, budget, A, V, ends, mx, C.byref(over))
    return list(ends[:n]), tuple(mx), over.value


def new_fill(lib, caller, cp, c0, c1):
    arr = (C.c_int64 * len(cp))(*cp)
    rows = sum(old_parts(caller, cp[c + 1] - cp[c]) for c in range(c0, c1))
    items = (C.c_int64 * (3 * rows))()
    w = 2 if caller == UNKNOWN else 3
    recs = (C.c_int64 * (3 * (c1 - c0)))()
    nr = C.c_int64()
    n = lib.probe_table_fill(caller, arr, c0, c1, items, recs, C.byref(nr))
    assert n == rows
    return ([tuple(items[3 * i:3 * i + 3]) for i in range(n)], [tuple(recs[w * i:w * i + w]) for i in range(nr.value)])


def cost_of(caller, n, A, V):
    return old_bytes_of(n, A, V) if caller == UNKNOWN else old_parts(caller, n)


def budgets_of(caller, lens, A, V, rng=None):
    """from "one row" (for the unknown-donor call: the largest cell alone, and one byte less, which it refuses) up to
    everything in one batch (and one unit less)"""
    costs = [cost_of(caller, n, A, V) for n in lens] or [1]
    total, big = sum(costs), max(costs)
    out = {1, 2, 3, big, big + 1, 2 * big, total // 2, total - 1, total, total + 1} if caller != UNKNOWN else \
          {big - 1, big, big + 1, big + min(costs), 2 * big, total // 2, total - 1, total, total + 1, min(costs)}
    out = sorted(b for b in out if b >= 1)
    return out if rng is None else rng.sample(out, 3)


def check(lib, caller, lens, budget, A, V, canon):
    """one (caller, pileup, budget): the plan against the restated loops, then the stated properties.  canon: the parts
    of every cell as the first budget cut them (cell -> [(e0, e1), ...] relative to the cell's start)"""
    cp = cell_ptr_of(lens)
    Cn = len(lens)
    ctx = (caller, lens, budget, A, V)
    o_ends, o_max, o_over = old_plan(caller, cp, budget, A, V)
    ends, mx, over = new_plan(lib, caller, cp, budget, A, V)
    # a cell that exceeds the budget alone is reported, the first one, where the unknown-donor call refused it
    alone = [c for c in range(Cn) if cost_of(caller, lens[c], A, V) > budget]
    assert over == (alone[0] if alone else -1), ctx
    if caller == UNKNOWN:
        assert over == o_over, ctx
        if o_over >= 0:
            return
    assert ends == o_ends and mx == o_max, ctx
    # the batches partition [0, C) into whole cells
    assert ends == sorted(set(ends)) and (ends[-1] == Cn if Cn else ends == []), ctx
    c0 = 0
    for c1 in ends:
        assert c1 > c0, ctx
        used = sum(cost_of(caller, n, A, V) for n in lens[c0:c1])
        assert used <= budget or c1 == c0 + 1, ctx  # over the budget only as a single cell
        assert c1 == Cn or used + cost_of(caller, lens[c1], A, V) > budget, ctx  # and the next cell did not fit
        items, recs = new_fill(lib, caller, cp, c0, c1)
        assert (items, recs) == old_fill(caller, cp, c0, c1), ctx + (c0, c1)
        # every row of the slab is written by exactly one item; the cells' own rows come first
        assert sorted(it[2] for it in items) == list(range(len(items))), ctx
        by_row = {it[2]: it for it in items}
        nxt = c1 - c0
        for c in range(c0, c1):
            first = by_row[c - c0]
            if caller == UNKNOWN:
                f, cnt = recs[c - c0]
            else:
                f, cnt = next(((r[1], r[2]) for r in recs if r[0] == c - c0), (nxt, 0))
            assert f == nxt or cnt == 0, ctx  # further parts in cell order
            parts = [first] + [by_row[f + k] for k in range(cnt)]
            nxt += cnt
            # the parts tile [cell_ptr[c], cell_ptr[c + 1]) in order, without gap or overlap
            assert parts[0][0] == cp[c] and parts[-1][1] == cp[c + 1], ctx
            assert all(a[1] == b[0] for a, b in zip(parts, parts[1:])), ctx
            assert all(p[0] < p[1] for p in parts) or lens[c] == 0 and len(parts) == 1, ctx
            assert all(p[1] - p[0] <= PART for p in parts), ctx
            assert len(parts) == max(1, -(-lens[c] // PART)), ctx
            # the cut of a cell depends on the cell alone: the same under every budget and batch position
            rel = [(p[0] - cp[c], p[1] - cp[c]) for p in parts]
            assert canon.setdefault(c, rel) == rel, ctx
        assert nxt == len(items), ctx
        c0 = c1


def settings():
    """(caller, A, V) of the three callers at every width (and for the unknown-donor call every alpha count)"""
    out = [(DEMUX, 0, w) for w in WIDTHS] + [(FMX, 0, w) for w in WIDTHS]
    return out + [(UNKNOWN, a, w) for a in ALPHAS for w in WIDTHS]


def test_constants(probe):
    assert probe.probe_table_part() == PART
    assert [probe.probe_table_sizes(i) for i in range(3)] == [SIZEOF_ITEM, 24, SIZEOF_CELL]  # what the kernels read
    for n in EDGES:
        assert probe.probe_table_unknown_bytes(n, 7, 65) == old_bytes_of(n, 7, 65)


def test_one_launch_limit(probe):
    # the callers' checks were (double)units / per_block >= 2147483647.0
    assert not probe.probe_table_exceeds(4.0 * 2147483646, 4.0)
    assert probe.probe_table_exceeds(4.0 * 2147483647, 4.0)
    assert not probe.probe_table_exceeds(256.0 * 2147483647 - 1, 256.0)
    assert probe.probe_table_exceeds(256.0 * 2147483647, 256.0)
    assert not probe.probe_table_exceeds(0.0, 4.0)


def test_no_cells(probe):
    for caller in (DEMUX, FMX, UNKNOWN):
        assert new_plan(probe, caller, [0], 5, 2, 3) == ([], (0, 0, 0, 0), -1)


@pytest.mark.parametrize("caller,A,V", settings())
def test_edge_lengths_at_every_budget(probe, caller, A, V):
    """The singlet tables' budget is rows: the slab budget in bytes over 8 V.  The width moves the unknown-donor call's
    bytes; for the singlet tables it only picks which row budgets are met, so every row budget is swept at every width."""
    canon = {}
    for budget in budgets_of(caller, EDGES, A, V):
        check(probe, caller, EDGES, budget, A, V, canon)
    if caller != UNKNOWN:
        for slab_bytes in (8 * V, 1 << 20, 4 << 30):  # one row, the GPU tests' 1 MB, the default
            check(probe, caller, EDGES, max(1, slab_bytes // (8 * V)), A, V, canon)


def test_the_two_policies_differ_only_inside_long_cells(probe):
    cp = cell_ptr_of(EDGES)
    d, _ = new_fill(probe, DEMUX, cp, 0, len(EDGES))
    f, _ = new_fill(probe, FMX, cp, 0, len(EDGES))
    u, _ = new_fill(probe, UNKNOWN, cp, 0, len(EDGES))
    assert d == u and [it[2] for it in d] == [it[2] for it in f]
    assert (cp[7], cp[7] + 2048, 7) in d and (cp[7], cp[7] + 6145 // 4, 7) in f  # 6145 entries: 4 parts
    assert (cp[4], cp[4] + 2048, 4) in d and (cp[4], cp[4] + 1024, 4) in f       # 2049 entries: 2048 + 1 against 1024 + 1025


def test_random_lengths(probe):
    rng = random.Random(20260)
    sets = settings()
    for i in range(240):
        n = rng.randint(1, 64)
        lens = [rng.choice([0, rng.randint(0, 30), rng.randint(0, 10000), rng.choice([2047, 2048, 2049, 4096, 4097])])
                for _ in range(n)]
        for caller in (DEMUX, FMX, UNKNOWN):
            _, A, V = rng.choice([s for s in sets if s[0] == caller])
            canon = {}
            for budget in budgets_of(caller, lens, A, V, rng):
                check(probe, caller, lens, budget, A, V, canon)


# ---- the two refusals, worded once (table_plan::alone_message, launch_message) with the words of each call
# (table_plan::shape, as the probe restates them and test_the_units_hand_in_these_words finds them in the units).  The literals are the format strings the five calls once carried, with the numbers put in:
# droplet 7 of 6145 entries, 4 alphas / rhos, 65 samples / clusters, 5 767 168 B = 5.5 MB against a budget of 1 MB, a
# largest batch of 123456789012 rows.
DEMUX_ENV, FMX_ENV = b"MUXGL_DEMUX_SLAB_MB", b"MUXGL_FMX_SLAB_MB"
CALLS = {  # name: (shapes_of number, who, noun, env)
    "demux_singlets": (0, b"muxgl_demux_singlets", b"", DEMUX_ENV),
    "fmx_singlets": (1, b"muxgl_fmx_singlets", b"", FMX_ENV),
    "demux_unknown": (2, b"muxgl_demux_unknown", b"", DEMUX_ENV),
    "fmx_unknown": (3, b"muxgl_fmx_unknown", b"", FMX_ENV),
    "demux_ambient": (4, b"muxgl_demux_ambient", b"samples", DEMUX_ENV),
    "fmx_ambient": (4, b"muxgl_fmx_ambient", b"clusters", FMX_ENV),
}


def alone_message(lib, name):
    call, who, noun, env = CALLS[name]
    out = C.create_string_buffer(512)
    lib.probe_table_alone_message(call, who, 7, 6145, 4, 65, noun, 5767168, 1 << 20, env, out, 512)
    return out.value.decode()


def launch_message(lib, name):
    call, who, noun, env = CALLS[name]
    out = C.create_string_buffer(512)
    lib.probe_table_launch_message(call, who, 123456789012, 4, 65, noun, env, out, 512)
    return out.value.decode()


@pytest.mark.parametrize("name,text", [
    ("demux_unknown", "muxgl_demux_unknown: droplet 7 alone (6145 entries x 4 alphas x 65 samples: 5.5 MB) exceeds the "
                      "budget of 1.0 MB (raise MUXGL_DEMUX_SLAB_MB)"),
    ("fmx_unknown", "muxgl_fmx_unknown: droplet 7 alone (6145 entries x 65 clusters: 5.5 MB) exceeds the budget of 1.0 MB "
                    "(raise MUXGL_FMX_SLAB_MB)"),
    ("demux_ambient", "muxgl_demux_ambient: droplet 7 alone (6145 entries x 4 rhos x 65 samples: 5.5 MB) exceeds the budget "
                      "of 1.0 MB (raise MUXGL_DEMUX_SLAB_MB)"),
    ("fmx_ambient", "muxgl_fmx_ambient: droplet 7 alone (6145 entries x 4 rhos x 65 clusters: 5.5 MB) exceeds the budget of "
                    "1.0 MB (raise MUXGL_FMX_SLAB_MB)"),
])
def test_refusal_of_a_droplet_over_the_budget_alone(probe, name, text):
    assert alone_message(probe, name) == text


def test_the_units_hand_in_these_words():
    probe_src = open(os.path.join(ROOT, "tests", "csrc", "table_plan_probe.cpp")).read()
    csrc = os.path.join(ROOT, "popscle_amd", "csrc")
    for unit, who, env, words in [
            ("demux_singlets.hip", "muxgl_demux_singlets", "MUXGL_DEMUX_SLAB_MB", 'table_plan::shape(V, "samples"), ""}'),
            ("fmx_singlets.hip", "muxgl_fmx_singlets", "MUXGL_FMX_SLAB_MB", 'table_plan::shape(K, "clusters"), ""}'),
            ("demux_unknown.hip", "muxgl_demux_unknown", "MUXGL_DEMUX_SLAB_MB",
             'table_plan::shape(V, "samples", A, "alphas"), table_plan::shape(A, "alphas", V, "samples")}'),
            ("fmx_unknown.hip", "muxgl_fmx_unknown", "MUXGL_FMX_SLAB_MB",
             'table_plan::shape(K, "clusters"), table_plan::shape(K, "clusters")}'),
            ("ambient_table.hpp", None, None,
             'table_plan::shape(W, call.noun, NR, "rhos"), table_plan::shape(NR, "rhos", W, call.noun)}')]:
        src = open(os.path.join(csrc, unit)).read()
        assert words in src and words in probe_src, unit
        if who:
            assert f'table_call call = {{"{who}", "{env}", ' in src, unit
    assert '{"muxgl_demux_ambient", h->V, "samples", h->d_gp, "MUXGL_DEMUX_SLAB_MB", ' in open(os.path.join(csrc, "demux_ambient.hip")).read()
    assert '{"muxgl_fmx_ambient", h->K, "clusters", h->d_cgp, "MUXGL_FMX_SLAB_MB", ' in open(os.path.join(csrc, "fmx_ambient.hip")).read()
    assert "table_call tc = {call.who, call.budget_env, " in open(os.path.join(csrc, "ambient_table.hpp")).read()


def test_the_singlet_tables_refuse_no_droplet(probe):
    assert alone_message(probe, "demux_singlets") == "" and alone_message(probe, "fmx_singlets") == ""


@pytest.mark.parametrize("name,text", [
    ("demux_singlets", "muxgl_demux_singlets: a batch of 123456789012 rows x 65 samples exceeds one launch "
                       "(lower MUXGL_DEMUX_SLAB_MB)"),
    ("fmx_singlets", "muxgl_fmx_singlets: a batch of 123456789012 rows x 65 clusters exceeds one launch "
                     "(lower MUXGL_FMX_SLAB_MB)"),
    ("demux_unknown", "muxgl_demux_unknown: a batch of 123456789012 rows x 65 samples x 4 alphas exceeds one launch "
                      "(lower MUXGL_DEMUX_SLAB_MB)"),
    ("fmx_unknown", "muxgl_fmx_unknown: a batch of 123456789012 rows x 65 clusters exceeds one launch "
                    "(lower MUXGL_FMX_SLAB_MB)"),
    ("demux_ambient", "muxgl_demux_ambient: a batch of 123456789012 rows x 65 samples x 4 rhos exceeds one launch "
                      "(lower MUXGL_DEMUX_SLAB_MB)"),
    ("fmx_ambient", "muxgl_fmx_ambient: a batch of 123456789012 rows x 65 clusters x 4 rhos exceeds one launch "
                    "(lower MUXGL_FMX_SLAB_MB)"),
])
def test_refusal_of_a_batch_over_one_launch(probe, name, text):
    assert launch_message(probe, name) == text


def test_lane_width(probe):
    """the power of two in 1..64 that seven loops once computed: while (W > 1 && W / 2 >= n) W /= 2, from 64"""
    assert [probe.probe_lane_width(n) for n in (0, 1, 2, 3, 33, 64, 65, 1024)] == [1, 1, 2, 4, 64, 64, 64, 64]
    for n in range(0, 200):
        w = 64
        while w > 1 and w // 2 >= n:
            w //= 2
        assert probe.probe_lane_width(n) == w
