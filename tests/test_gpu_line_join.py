"""st_intersects_aggregate over the join of line chips with polygon chips on the GPU
(mosaic_line_chips_*, mosaic_line_intersects_aggregate; k_lj_probe / k_lj_test of
mosaic_amd/csrc/line_join.hip) through LineChipTable + ChipTable + ctx.st_intersects_aggregate.
Every decision is an exact predicate, so the GPU's key columns and flags must equal the host
restatement's (mosaic_line_intersects_aggregate_host, tests/test_line_join.py), not approximate them."""
import ctypes

import numpy as np
import pytest

import oracle
from mosaic_amd import LineChipTable, MosaicContext, MosaicError, line_intersects_aggregate_host
from mosaic_amd import _native as N
from mosaic_amd.context import tessellate
from mosaic_amd.data import LineSet, PolygonSet
from tests import line_cases as LC
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


@pytest.fixture(params=[64, 16], ids=["wave", "team16"])
def team(request):
    prev = N.lib().mosaic_line_join_team(request.param)
    yield request.param
    N.lib().mosaic_line_join_team(prev)


def tables(c, lines, polys, res):
    lt = c.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], res)
    pt = c.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], res)
    return lt, pt


def gpu(c, lines, polys, res):
    lt, pt = tables(c, lines, polys, res)
    try:
        return c.st_intersects_aggregate(lt, pt)
    finally:
        lt.close()
        pt.close()


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def last():
    n, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 2)()
    N.check(N.lib().mosaic_line_join_last(n, ms))
    return list(n), list(ms)


# ---- the hand table and the grouping cases ----
def test_hand_table(ctx, cells, team):
    lines, polys, want = JC.hand_chips(cells)
    got = gpu(ctx, lines, polys, 5)
    assert JC.as_dict(*got) == want
    assert same(got, line_intersects_aggregate_host("H3", lines, polys, 5))
    # every line against every polygon in one cell
    lines["index_id"][:] = cells[0]
    polys["index_id"][:] = cells[0]
    got = gpu(ctx, lines, polys, 5)
    assert len(got[0]) == len(JC.HAND) ** 2
    assert same(got, line_intersects_aggregate_host("H3", lines, polys, 5))


def test_grouping(ctx, cells, team):
    lines, polys, want = JC.grouping_chips(cells)
    lk, pk, fl = gpu(ctx, lines, polys, 5)
    assert JC.as_dict(lk, pk, fl) == want
    assert list(zip(lk.tolist(), pk.tolist())) == sorted(want)
    assert same((lk, pk, fl), line_intersects_aggregate_host("H3", lines, polys, 5))
    counts, ms = last()
    # line 2's cell is not in the polygon table; the other five chips find theirs; 3 x 2 + 2 x 1 chip pairs, none core
    assert counts[0] == 5 and counts[1] == 8 and 1 <= counts[2] <= 8 and counts[3] == len(want)
    assert ms[0] > 0 and ms[1] > 0


# ---- parity with the host function ----
@pytest.mark.parametrize("name", ["H3", "BNG"])
def test_invariant_workloads_equal_the_host(ctx, bng, name):
    _, _, lines, polys, res = JC.invariant_case(name)
    got = gpu(ctx if name == "H3" else bng, lines, polys, res)
    want = line_intersects_aggregate_host(name, lines, polys, res)
    assert len(want[0]) >= 20 and same(got, want)


def test_short_lines_against_the_zones(ctx, team):
    """263 NYC zones at resolution 9 against 2,000 short lines, the line chips once from the host
    producer and once from the GPU producer."""
    zones = PolygonSet.load("nyc_taxi_zones")
    polys = tessellate("H3", zones, 9)
    ls = LineSet.from_lines(LC.short_lines(LC.H3, 9, 2000, 20250117))
    pt = ctx.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], 9)
    try:
        for producer in (None, ctx):
            lines = tessellate("H3", ls, 9, ctx=producer)
            want = line_intersects_aggregate_host("H3", lines, polys, 9)
            lt = LineChipTable(ctx, lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], 9)
            got = ctx.st_intersects_aggregate(lt, pt)
            assert lt.info()["n_chips"] == len(lines["index_id"]) and lt.info()["n_pieces"] >= lt.info()["n_chips"]
            lt.close()
            assert len(want[0]) > 500 and 0 < want[2].sum() < len(want[2])
            assert same(got, want)
            counts, _ = last()
            assert counts[2] <= counts[1] and counts[3] == len(got[0]) and counts[0] <= len(lines["index_id"])
    finally:
        pt.close()


# ---- the smallest shapes at which the kernels can go wrong ----
SHAPES = ["last pair", "inside", "around", "piece 67", "no piece", "chip 67", "1200 groups"]


@pytest.fixture(scope="module")
def shapes(cells):
    return JC.shape_cases(cells[0])


@pytest.mark.parametrize("name", SHAPES)
def test_shapes(ctx, shapes, team, name):
    lines, polys, want = shapes[name]
    got = gpu(ctx, lines, polys, 5)
    host = line_intersects_aggregate_host("H3", lines, polys, 5)
    if want is not None:
        assert JC.as_dict(*got) == want
    else:
        assert len(got[0]) == 1200 and 0 < got[2].sum() < 1200  # beyond the binding's first capacity of 1,024
    assert same(got, host)
    counts, _ = last()
    assert counts[2] <= counts[1] and counts[3] == len(got[0])


def test_empty_line_table_and_empty_join(ctx, cells):
    lines, polys, _ = JC.grouping_chips(cells)
    got = gpu(ctx, JC.columns([]), polys, 5)
    assert [len(a) for a in got] == [0, 0, 0]
    lines["index_id"][:] = cells[7]  # a cell the polygon table lacks
    got = gpu(ctx, lines, polys, 5)
    assert [len(a) for a in got] == [0, 0, 0]
    assert last()[0] == [0, 0, 0, 0]


# ---- the Python surface ----
def test_sides_swapped(ctx, cells):
    lines, polys, want = JC.grouping_chips(cells)
    lt, pt = tables(ctx, lines, polys, 5)
    try:
        lk, pk, fl = ctx.st_intersects_aggregate(lt, pt)
        pk2, lk2, fl2 = ctx.st_intersects_aggregate(pt, lt)
        assert JC.as_dict(pk2, lk2, fl2) == {(p, l): f for (l, p), f in want.items()}
        assert list(zip(pk2.tolist(), lk2.tolist())) == sorted((p, l) for l, p in want)
        assert pk2.dtype == np.int32 and fl2.dtype == bool and len(lk) == len(lk2)
        with pytest.raises(ValueError):
            ctx.st_intersects_aggregate(lt, lt)
        # two polygon tables take the polygon path as before
        a, b, f = ctx.st_intersects_aggregate(pt, pt)
        assert JC.as_dict(a, b, f) == oracle.intersects_aggregate(polys, polys)
    finally:
        lt.close()
        pt.close()


def test_resolution_and_grid_mismatch(ctx, bng, cells):
    lines, polys, _ = JC.grouping_chips(cells)
    lt = ctx.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], 6)
    pt = ctx.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], 5)
    bt = bng.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], 4)
    try:
        for table in (lt, bt):
            with pytest.raises(MosaicError) as e:
                ctx.st_intersects_aggregate(table, pt)
            assert e.value.code == N.MOSAIC_E_ARG
            with pytest.raises(MosaicError):
                ctx.st_intersects_aggregate(pt, table)
    finally:
        for t in (lt, pt, bt):
            t.close()


def test_line_table_accepts_what_chip_table_accepts(ctx, bng, cells):
    lines, polys, want = JC.grouping_chips(cells)
    rows = JC.rows_of(lines)
    pt = ctx.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], 5)
    offs32 = (lines["wkb"][0].astype(np.int32), lines["wkb"][1])
    try:
        for wkb in ([r[3] for r in rows], offs32, lines["wkb"]):
            lt = LineChipTable(ctx, lines["is_core"], lines["index_id"], wkb, lines["polygon_key"], 5)
            assert lt.info()["n_chips"] == len(rows) and lt.info()["n_vertices"] == 12 and lt.info()["device_bytes"] > 0
            assert JC.as_dict(*ctx.st_intersects_aggregate(lt, pt)) == want
            lt.close()
        with pytest.raises(MosaicError) as e:
            LineChipTable(ctx, lines["is_core"], lines["index_id"], [JC.TRI] + [r[3] for r in rows[1:]], lines["polygon_key"], 5)
        assert e.value.code == N.MOSAIC_E_WKB and "line chip 0" in str(e.value)
    finally:
        pt.close()
    # string BNG ids go through bng_parse_column, as in ChipTable
    ids = [oracle.bng_point_to_index(530000.0 + 100 * k, 180000.0, 4) for k in range(3)]
    names = [oracle.bng_format(int(c)) for c in ids]
    lb = JC.columns([(0, ids[k], k, JC.ls((10, 10), (90, 90))) for k in range(3)])
    pb = JC.columns([(0, ids[k], k, JC.TRI) for k in range(2)])
    lt = LineChipTable(bng, lb["is_core"], names, lb["wkb"], lb["polygon_key"], 4)
    pt = bng.chip_table(pb["is_core"], names[:2], pb["wkb"], pb["polygon_key"], 4)
    try:
        assert JC.as_dict(*bng.st_intersects_aggregate(lt, pt)) == {(0, 0): True, (1, 1): True}
    finally:
        lt.close()
        pt.close()
