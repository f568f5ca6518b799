"""st_distance with line geometries on the GPU (mosaic_geoms_create_lines, mosaic_geoms_create_wkb_ex,
MosaicContext.geometry_table(LineSet) / geometry_table(rows, lines=True), st_distance): k_dist_small and
k_dist_block of mosaic_amd/csrc/st_distance.hip against (H), the kind-aware sequential driver compiled
by g++ (tests/test_st_distance_lines.py), bit for bit -- with every pair on k_dist_block and with the
default dispatch, with and without pruning, and with a tile of 4 segments that lines of 4, 5, 8 and 9
vertices straddle."""
import ctypes
import functools

import numpy as np
import pytest

from mosaic_amd import _native as N

from .test_st_distance import nyc35, pickups
from .test_st_distance_lines import (ANALYTIC, LCol, assert_same_bits, geom_wkb, host_distance, line, poly, pt, random_pairs,
                                     tile_pairs, trips, trips_col)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case_rows():
    """every CPU case: the analytic ones, the tile pairs and the 300 random pairs, as WKB rows in
    alternating byte orders, with (H) on them"""
    left = [c[1] for c in ANALYTIC] + list(tile_pairs()[0]) + [a for a, _ in random_pairs()]
    right = [c[2] for c in ANALYTIC] + list(tile_pairs()[1]) + [b for _, b in random_pairs()]
    rows_l = [geom_wkb(g, bool(i % 2)) for i, g in enumerate(left)]
    rows_r = [geom_wkb(g, bool(i % 3)) for i, g in enumerate(right)]
    want = host_distance(LCol.from_wkb(rows_l), LCol.from_wkb(rows_r))
    assert want[:len(ANALYTIC)].tolist() == [c[3] for c in ANALYTIC]
    return rows_l, rows_r, want


@pytest.fixture(scope="module")
def case_tables(ctx):
    rows_l, rows_r, _ = case_rows()
    lt, rt = ctx.geometry_table(rows_l, lines=True), ctx.geometry_table(rows_r, lines=True)
    yield lt, rt
    lt.close()
    rt.close()


@pytest.mark.parametrize("tile", (None, 4), ids=("tile default", "tile 4"))
@pytest.mark.parametrize("prune", (1, 0), ids=("pruned", "unpruned"))
@pytest.mark.parametrize("small_work", (None, 0), ids=("default dispatch", "all on k_dist_block"))
def test_cpu_cases(ctx, case_tables, small_work, prune, tile):
    lt, rt = case_tables
    _, _, want = case_rows()
    assert lt.info()["n_row_path"] == 0 and rt.info()["n_row_path"] == 0
    try:
        if small_work is not None:
            ctx.set_option("dist_small_work", small_work)
        if tile is not None:
            ctx.set_option("dist_tile", tile)
        ctx.set_option("dist_prune", prune)
        got = ctx.st_distance(lt, rt)
    finally:
        ctx.set_option("dist_small_work", 512)
        ctx.set_option("dist_tile", 16)
        ctx.set_option("dist_prune", 1)
    assert_same_bits(got, want, (small_work, prune, tile))
    k = len(ANALYTIC)
    assert got[:k].tolist() == [c[3] for c in ANALYTIC], [(c[0], g) for c, g in zip(ANALYTIC, got) if g != c[3]]
    assert not np.signbit(got).any()


@functools.lru_cache(maxsize=None)
def trips_host():
    """(H): 64 trips against the 35 zones (all 2,240 pairs), against 64 pickups and against themselves"""
    t = trips_col(64)
    ps = nyc35()
    x, y = pickups()
    li, ri = np.repeat(np.arange(64), len(ps)), np.tile(np.arange(len(ps)), 64)
    pi, qi = np.repeat(np.arange(64), 64), np.tile(np.arange(64), 64)
    zones, points = LCol.from_polyset(ps), LCol.from_points(x[:64], y[:64])
    return dict(zones=(li, ri, host_distance(t, zones, li, ri)), zones_first=host_distance(zones, t, ri, li),
                pickups=(pi, qi, host_distance(t, points, pi, qi)), pickups_rowwise=host_distance(t, points),
                trips=(pi, qi, host_distance(t, t, pi, qi)), trips_rowwise=host_distance(t, LCol.from_lineset(trips(64))))


def test_trips_against_zones_pickups_and_trips(ctx):
    ls, ps = trips(64), nyc35()
    x, y = pickups()
    h = trips_host()
    with ctx.geometry_table(ls) as tt, ctx.geometry_table(ps) as zt, ctx.geometry_table((x[:64].copy(), y[:64].copy())) as pt_t:
        assert tt.info() == dict(n_geoms=64, n_vertices=64 * 50, n_row_path=0)
        li, ri, want = h["zones"]
        assert (want == 0).any() and (want > 0).any()
        assert_same_bits(ctx.st_distance(tt, zt, pairs=(li, ri)), want, "trips against zones")
        assert_same_bits(ctx.st_distance(zt, tt, pairs=(ri, li)), h["zones_first"], "zones against trips")
        pi, qi, want = h["pickups"]
        assert_same_bits(ctx.st_distance(tt, pt_t, pairs=(pi, qi)), want, "trips against pickups")
        assert_same_bits(ctx.st_distance(tt, pt_t), h["pickups_rowwise"], "trips against pickups, row-wise")
        assert_same_bits(h["pickups_rowwise"], want.reshape(64, 64).diagonal(), "the two host forms")
        pi, qi, want = h["trips"]
        assert (want.reshape(64, 64).diagonal() == 0).all() and (want > 0).any()
        assert_same_bits(ctx.st_distance(tt, tt, pairs=(pi, qi)), want, "trips against trips")
        assert_same_bits(ctx.st_distance(tt, ls), h["trips_rowwise"], "trips against trips, row-wise, the LineSet given bare")
        # the same column through WKB rows with the lines flag
        with ctx.geometry_table([ls.wkb(g, bool(g % 2)) for g in range(len(ls))], lines=True) as by_wkb:
            assert by_wkb.info() == tt.info()
            assert_same_bits(ctx.st_distance(by_wkb, zt, pairs=(li, ri)), h["zones"][2], "WKB trips against zones")
        # every pair on k_dist_block, unpruned, tile 4
        try:
            ctx.set_option("dist_small_work", 0)
            ctx.set_option("dist_prune", 0)
            ctx.set_option("dist_tile", 4)
            assert_same_bits(ctx.st_distance(tt, tt, pairs=(pi, qi)), want, "trips against trips, block, unpruned, tile 4")
        finally:
            ctx.set_option("dist_small_work", 512)
            ctx.set_option("dist_prune", 1)
            ctx.set_option("dist_tile", 16)


MIXED = ["LINESTRING (0 0, 0 9)", None, "LINESTRING EMPTY", "POINT (0 0)", "LINESTRING (3 3)", "GEOMETRYCOLLECTION EMPTY",
         "MULTILINESTRING ((50 0, 60 0), EMPTY, (0 0, 0 9))", "POLYGON ((0 0, 10 0, 10 10, 0 10, 0 0))", "POINT EMPTY",
         "LINESTRING (0 0, 10 0, 10 10, 0 10, 0 0)"]


def test_status_in_a_mixed_column(ctx):
    from mosaic_amd import RowPathRequired

    ok, null, path = N.ROW_OK, N.ROW_NULL, N.ROW_PATH
    other = ctx.geometry_table((np.full(len(MIXED), 3.0), np.full(len(MIXED), 4.0)))
    with ctx.geometry_table(MIXED, lines=True) as table:
        assert table.info() == dict(n_geoms=10, n_vertices=2 + 1 + 4 + 5 + 5, n_row_path=3)
        d, st = ctx.st_distance(table, other, return_status=True)
        assert st.tolist() == [ok, null, ok, ok, path, path, ok, ok, path, ok]
        assert np.isnan(d[st != ok]).all()
        assert d[st == ok].tolist() == [3.0, 0.0, 5.0, 3.0, 0.0, 3.0]  # the closed line does not hold (3 4); the polygon does
        with pytest.raises(RowPathRequired) as e:
            ctx.st_distance(other, table)
        assert e.value.rows.tolist() == [4, 5, 8]
        # WKB rows of the same column
        rows = [None if t is None else _row(t) for t in MIXED]
        with ctx.geometry_table(rows, lines=True) as by_wkb:
            assert by_wkb.info() == table.info()
            d2, st2 = ctx.st_distance(by_wkb, other, return_status=True)
            assert st2.tolist() == st.tolist()
            assert_same_bits(d2, d, "WKB rows")
    # without lines=True the table is what it was: line rows are rows for the row path
    with ctx.geometry_table(MIXED) as plain:
        assert plain.info() == dict(n_geoms=10, n_vertices=1 + 5, n_row_path=7)
        d, st = ctx.st_distance(plain, other, return_status=True)
        assert st.tolist() == [path, null, path, ok, path, path, path, ok, path, path]
        assert d[[3, 7]].tolist() == [5.0, 0.0] and np.isnan(d[st != ok]).all()
    other.close()


def _row(text):
    from mosaic_amd.context import _wkt_row_wkb

    return _wkt_row_wkb(text, lines=True)


def _create(ctx, entry, rows, *flags):
    lens = np.array([len(r) for r in rows], np.int64)
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(rows), np.uint8).copy()
    h = ctypes.c_void_p()
    rc = getattr(N.lib(), entry)(ctx.handle, len(rows), N.ptr(offs), N.ptr(data), None, *flags, ctypes.byref(h))
    if rc:
        return rc, None
    n, v, p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    N.check(N.lib().mosaic_geoms_info(h, ctypes.byref(n), ctypes.byref(v), ctypes.byref(p)))
    N.check(N.lib().mosaic_geoms_destroy(h))
    return 0, (n.value, v.value, p.value)


def test_c_entries(ctx):
    rows = [geom_wkb(g) for g in (line([(0, 0), (0, 9)]), line([(0, 0), (1, 1)], [(5, 5), (6, 6), (7, 5)]), pt(1, 2), poly([[(0, 0), (1, 0), (1, 1), (0, 0)]]),
                                  line([]))]
    assert _create(ctx, "mosaic_geoms_create_wkb", rows) == (0, (5, 5, 3))
    assert _create(ctx, "mosaic_geoms_create_wkb_ex", rows, 0) == (0, (5, 5, 3))
    assert _create(ctx, "mosaic_geoms_create_wkb_ex", rows, N.GEOMS_LINES) == (0, (5, 12, 0))
    assert _create(ctx, "mosaic_geoms_create_wkb_ex", rows, 2)[0] == N.MOSAIC_E_ARG
    # mosaic_geoms_create_lines: inconsistent offsets
    xy = np.zeros((4, 2))
    h = ctypes.c_void_p()
    for geom_lines, line_offsets in (([0, 2, 1], [0, 2, 4]), ([0, 1, 2], [0, 3, 2]), ([1, 1, 2], [0, 2, 4])):
        gl, lo = np.array(geom_lines, np.int64), np.array(line_offsets, np.int64)
        assert N.lib().mosaic_geoms_create_lines(ctx.handle, 2, N.ptr(gl), N.ptr(lo), N.ptr(xy), ctypes.byref(h)) == N.MOSAIC_E_ARG
        assert not h
    # a one-vertex component is a row for the row path; an empty LineSet is an empty column
    from mosaic_amd.data import LineSet

    with ctx.geometry_table(LineSet.from_lines([[[(0, 0), (1, 1)]], [[(3, 3)]], [], [[(0, 0), (1, 0)], [(7, 7)]]])) as t:
        assert t.info() == dict(n_geoms=4, n_vertices=2, n_row_path=2)
        d, st = ctx.st_distance(t, "POINT (0 1)", return_status=True)
        assert st.tolist() == [N.ROW_OK, N.ROW_PATH, N.ROW_OK, N.ROW_PATH] and d[0] == np.sqrt(0.5) and d[2] == 0.0
    with ctx.geometry_table(LineSet.from_lines([])) as t:
        assert t.info() == dict(n_geoms=0, n_vertices=0, n_row_path=0)
