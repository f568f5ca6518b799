"""st_intersection_aggregate over the join of line chips with polygon chips on the GPU
(mosaic_line_intersection_aggregate, mosaic_line_intersection_aggregate_geometry; k_lx_probe /
k_lx_chip_len / k_lx_clip of mosaic_amd/csrc/line_clip.hip) through LineChipTable + ChipTable +
ctx.st_intersection_aggregate / ctx.st_intersection_aggregate_length.  The wave kernel and the host
restatement (mosaic_line_intersection_aggregate_host, tests/test_line_intersection.py) run one
definition and fold in one order, so every comparison here is bitwise: keys, the uint64 view of the
lengths, and the WKB bytes."""
import ctypes

import numpy as np
import pytest

import oracle
from mosaic_amd import LineChipTable, MosaicContext, MosaicError, line_intersection_aggregate_host
from mosaic_amd import _native as N
from mosaic_amd.context import tessellate
from mosaic_amd.data import LineSet, PolygonSet
from tests import line_cases as LC
from tests import line_clip_cases as CC
from tests import line_join_cases as JC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = MosaicContext.build("H3")
    yield c
    c.close()


@pytest.fixture(scope="module")
def bng():
    c = MosaicContext.build("BNG")
    yield c
    c.close()


@pytest.fixture(scope="module")
def cells():
    """Real H3 cell ids (resolution 5) standing for the hand cases' cells: the aggregate never decodes them."""
    k = np.arange(40, dtype=np.float64)
    c = oracle.h3_point_to_index(k, 10.0 + k, 5)
    assert len(set(c.tolist())) == 40
    return [int(v) for v in c]


def last():
    n, ms = (ctypes.c_int64 * 6)(), (ctypes.c_double * 3)()
    N.check(N.lib().mosaic_line_intersection_last(n, ms))
    return list(n), list(ms)


def tables(c, lines, polys, res):
    lt = c.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], res)
    pt = c.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], res)
    return lt, pt


def same_bits(got, want):
    """Keys, the uint64 view of the lengths, status and WKB bytes."""
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(np.ascontiguousarray(got[2]).view(np.uint64), np.ascontiguousarray(want[2]).view(np.uint64))
    if len(got) > 3:
        assert np.array_equal(got[3], want[3]) and not got[3].any()
        assert got[4] == want[4]
    return True


def gpu(c, lines, polys, res, name="H3"):
    """The geometry call and the length call on fresh tables, each equal to the host's bits; returns
    the geometry call's tuple and the counters of the two calls."""
    want = line_intersection_aggregate_host(name, lines, polys, res)
    lt, pt = tables(c, lines, polys, res)
    try:
        got = c.st_intersection_aggregate(lt, pt)
        geo = last()
        short = c.st_intersection_aggregate_length(lt, pt)
        ln = last()
    finally:
        lt.close()
        pt.close()
    assert same_bits(got, want) and same_bits(short, want[:3])
    assert geo[0] == ln[0] and geo[0][4] == len(got[0])  # the two calls count alike
    return got, geo


# ---- the hand table ----
def test_hand_table(ctx, cells):
    lines, polys, want = CC.hand_chips(cells)
    got, (counts, ms) = gpu(ctx, lines, polys, 5)
    assert CC.as_dict(*got) == want
    n_core = sum(1 for h in CC.HAND for _ in h[1] if h[2])
    assert counts[0] == len(lines["index_id"]) and counts[1] == counts[0] - n_core and counts[2] == 0
    assert ms[0] > 0 and ms[1] > 0
    # every line chip against every polygon chip in one cell
    lines["index_id"][:] = cells[0]
    polys["index_id"][:] = cells[0]
    got, _ = gpu(ctx, lines, polys, 5)
    assert len(got[0]) == len(CC.HAND) ** 2


# ---- parity with the host function on the invariant workloads ----
@pytest.mark.parametrize("name", ["H3", "BNG"])
def test_invariant_workloads_equal_the_host(ctx, bng, name):
    _, _, lines, polys, res = JC.invariant_case(name)
    got, (counts, _) = gpu(ctx if name == "H3" else bng, lines, polys, res, name)
    assert len(got[0]) >= 40 and (got[2] > 0).sum() >= 20 and (got[2] == 0).sum() >= 10
    assert counts[0] > counts[1] > 0 and counts[3] > 0  # core-polygon pairs and clipped pairs, runs


def test_short_lines_against_the_zones(ctx):
    """263 NYC zones at resolution 9 against 2,000 short lines, the line chips once from the host
    producer and once from the GPU producer."""
    zones = PolygonSet.load("nyc_taxi_zones")
    polys = tessellate("H3", zones, 9)
    ls = LineSet.from_lines(LC.short_lines(LC.H3, 9, 2000, 20250117))
    pt = ctx.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], 9)
    try:
        for producer in (None, ctx):
            lines = tessellate("H3", ls, 9, ctx=producer)
            want = line_intersection_aggregate_host("H3", lines, polys, 9)
            lt = LineChipTable(ctx, lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], 9)
            got = ctx.st_intersection_aggregate(lt, pt)
            counts, _ = last()
            short = ctx.st_intersection_aggregate_length(lt, pt)
            lt.close()
            assert len(want[0]) > 500 and 0 < (want[2] > 0).sum() < len(want[2])
            assert same_bits(got, want) and same_bits(short, want[:3])
            assert counts[4] == len(got[0]) and counts[1] < counts[0] and counts[2] == 0
    finally:
        pt.close()


# ---- the smallest shapes at which the kernels can go wrong ----
def test_more_cuts_than_a_wave(ctx, cells):
    lines, polys, want = CC.comb_case(cells[0], 70)
    got, (counts, _) = gpu(ctx, lines, polys, 5)
    assert CC.as_dict(*got) == want and want[(0, 0)][0] == 35.0
    assert counts[:5] == [1, 1, 0, 35, 1]


def test_over_the_cut_cap_is_finished_on_the_host(ctx, cells):
    cap = last()[0][5]
    assert 64 < cap < 1024
    lines, polys, want = CC.comb_case(cells[0], cap + 6)
    # a second pair under the cap in the same call: the fill pass skips the first and fills the second
    more = JC.rows_of(lines) + [(0, cells[1], 1, JC.ls((-2, 4), (10, 4)))]
    polys2 = JC.columns(JC.rows_of(polys) + [(0, cells[1], 1, CC.HOLED8)])
    got, (counts, _) = gpu(ctx, JC.columns(more), polys2, 5)
    assert CC.as_dict(*got)[(0, 0)] == want[(0, 0)]
    assert CC.as_dict(*got)[(1, 1)] == (6.0, CC.runs_wkb(CC.HAND[7][5]))
    assert counts[2] >= 1 and counts[:2] == [2, 2] and counts[3] == (cap + 6) // 2 + 2


SHAPES = ["last pair", "inside", "around", "piece 67", "no piece", "chip 67", "1200 groups"]


@pytest.fixture(scope="module")
def shapes(cells):
    return JC.shape_cases(cells[0])


@pytest.mark.parametrize("name", SHAPES)
def test_shapes(ctx, shapes, name):
    """Late crossing (a 200-segment piece against a 300-vertex ring, only the last-enumerated segment
    pair crossing; the same with the piece inside, and outside), 70 pieces with only piece 67 inside,
    70 polygon chips in one cell, 1,200 groups in one cell."""
    lines, polys, _ = shapes[name]
    got, (counts, _) = gpu(ctx, lines, polys, 5)
    lengths = CC.as_dict(*got)
    if name == "last pair":
        assert 0 < lengths[(0, 0)][0] < 6.0 and len(CC.wkb_runs(lengths[(0, 0)][1])) == 1
    if name == "inside":
        assert len(CC.wkb_runs(lengths[(0, 0)][1])[0]) == 200
    if name in ("around", "no piece"):
        assert lengths[(0, 0)] == (0.0, CC.EMPTY)  # a group of length 0
    if name == "piece 67":
        assert CC.wkb_runs(lengths[(0, 0)][1]) == [[(10.0, 10.0), (20.0, 15.0)]]
    if name == "chip 67":
        assert len(lengths) == 70 and [k for (_, k), v in lengths.items() if v[0] > 0] == [66]
    if name == "1200 groups":
        assert len(lengths) == 1200 and 0 < sum(1 for v in lengths.values() if v[0] > 0) < 1200
    assert counts[4] == len(got[0]) and counts[2] == 0


def test_sum_order_two_chips_of_one_key_in_one_cell(ctx, cells):
    lines = JC.columns([(0, cells[9], 0, JC.ls((0, 1), (0.6, 1))), (0, cells[5], 0, JC.ls((0, 2), (0.1, 2))),
                        (0, cells[9], 0, JC.ls((0, 3), (0.2, 3)))])
    polys = JC.columns([(0, cells[9], 0, CC.S8), (0, cells[5], 0, CC.S8), (0, cells[9], 0, CC.TWO8)])
    got, _ = gpu(ctx, lines, polys, 5)
    # cell id first: the 0.1 of cells[5] is added first or last
    want = (((0.1 + 0.6) + 0.6) + 0.2) + 0.0 if cells[5] < cells[9] else (((0.6 + 0.6) + 0.2) + 0.0) + 0.1
    assert len(got[2]) == 1 and got[2][0] == want


def test_empty_tables_and_empty_join(ctx, cells):
    lines, polys, _ = CC.hand_chips(cells)
    for a, b in ((JC.columns([]), polys), (lines, JC.columns([]))):
        got, _ = gpu(ctx, a, b, 5)
        assert [len(x) for x in got] == [0, 0, 0, 0, 0]
    lines["index_id"][:] = cells[39]  # a cell the polygon table lacks
    got, (counts, _) = gpu(ctx, lines, polys, 5)
    assert [len(x) for x in got] == [0, 0, 0, 0, 0] and counts[:5] == [0, 0, 0, 0, 0]


def test_repeat_and_no_regression(ctx, cells):
    """Two consecutive calls return identical bits, and st_intersects_aggregate on the same tables
    answers after the new call what it answered before."""
    _, _, lines, polys, res = JC.invariant_case("H3")
    lt, pt = tables(ctx, lines, polys, res)
    try:
        before = ctx.st_intersects_aggregate(lt, pt)
        n, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 2)()
        N.check(N.lib().mosaic_line_join_last(n, ms))
        first = ctx.st_intersection_aggregate(lt, pt)
        second = ctx.st_intersection_aggregate(lt, pt)
        assert same_bits(first, second)
        n2 = (ctypes.c_int64 * 4)()
        N.check(N.lib().mosaic_line_join_last(n2, ms))
        assert list(n) == list(n2)  # the new call leaves the join's counters alone
        after = ctx.st_intersects_aggregate(lt, pt)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        # a group with a positive length is never false
        flags = JC.as_dict(*after)
        assert all(flags[g] for g, v in CC.as_dict(*first).items() if v[0] > 0)
    finally:
        lt.close()
        pt.close()


# ---- the Python surface and the errors ----
def test_sides_swapped_and_value_errors(ctx, cells):
    lines, polys, want = CC.hand_chips(cells)
    lines["polygon_key"][:] = 40 - lines["polygon_key"]
    lt, pt = tables(ctx, lines, polys, 5)
    try:
        lk, pk, ln, st, wkb = ctx.st_intersection_aggregate(lt, pt)
        pk2, lk2, ln2, st2, wkb2 = ctx.st_intersection_aggregate(pt, lt)
        assert list(zip(pk2.tolist(), lk2.tolist())) == sorted(zip(pk.tolist(), lk.tolist()))
        assert {(a, b): (v, w) for a, b, v, w in zip(lk2.tolist(), pk2.tolist(), ln2.tolist(), wkb2)} == \
               {(a, b): (v, w) for a, b, v, w in zip(lk.tolist(), pk.tolist(), ln.tolist(), wkb)}
        pk3, lk3, ln3 = ctx.st_intersection_aggregate_length(pt, lt)
        assert same_bits((pk3, lk3, ln3), (pk2, lk2, ln2))
        assert {(p, p): v for (_, p), v in CC.as_dict(lk, pk, ln, st, wkb).items()} == want
        with pytest.raises(ValueError):
            ctx.st_intersection_aggregate(lt, lt)
        with pytest.raises(ValueError):
            ctx.st_intersection_aggregate_area(lt, pt)
        # two polygon tables behave as before
        a = ctx.st_intersection_aggregate(pt, pt)
        b = ctx.st_intersection_aggregate_area(pt, pt)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) >= len(CC.HAND)
    finally:
        lt.close()
        pt.close()


def test_errors(ctx, bng, cells):
    lines, polys, _ = CC.hand_chips(cells)
    lines["is_core"][3] = 1
    lt, pt = tables(ctx, lines, polys, 5)
    lt6 = ctx.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], 6)
    bt = bng.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], 4)
    try:
        for call in (ctx.st_intersection_aggregate, ctx.st_intersection_aggregate_length):
            with pytest.raises(MosaicError) as e:
                call(lt, pt)
            assert e.value.code == N.MOSAIC_E_ARG and "line chip 3" in str(e.value)
            for table in (lt6, bt):
                with pytest.raises(MosaicError) as e:
                    call(table, pt)
                assert e.value.code == N.MOSAIC_E_ARG
    finally:
        for t in (lt, pt, lt6, bt):
            t.close()
