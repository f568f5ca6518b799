"""GridRingNeighbours and the approximate SpatialKNN with line geometries on the GPU: trips (a LineSet)
as candidates of pickup points and of zones, and as landmarks against point candidates -- the
reference's documented case of building polygons against trip linestrings
(docs/source/models/spatial-knn.rst:113-152).  Every row is compared with the host pieces of
tests/test_st_distance_lines.py: host lineFill chips, host k-rings, the kind-aware host distance,
rn::neighbours and tests/test_ring_neighbours.py's literal_knn."""
import numpy as np
import pytest

from .test_ring_neighbours import as_rows, knn_columns_as_rows, pickups64, reorder
from .test_st_distance_lines import (KNN_PARAMS, N_CANDIDATE_TRIPS, LCol, SQ, TRI, assert_knn_case_is_telling, geom_wkb,
                                     host_neighbours, knn_case, line, poly, restate, trips_side)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


def gpu_neighbours(ctx, left, right, index, rows, cells, keep_self=False):
    l, c, d, un = ctx.grid_ring_neighbours(left, right, index, rows, cells, keep_self)
    return as_rows(l, c, d), set(np.flatnonzero(un).tolist())


@pytest.mark.parametrize("it", (1, 2))
def test_pickups_against_trips(ctx, it):
    """64 pickups as landmarks, 200 trips as candidates, H3 res 8: the LineSet is given bare, its chips
    come from the GPU's lineFill, and the rows equal rn::neighbours over the host's line chips"""
    p, t = pickups64(), trips_side(N_CANDIDATE_TRIPS)
    rows, cells = p.ring_rows(it)
    want = host_neighbours((t.chips[1], t.chips[2]), p.col, t.col, rows, cells)
    chips = ctx.grid_tessellateexplode(t.geoms, 8, cells_only=True)
    assert sorted(zip(chips["index_id"].tolist(), chips["polygon_key"].tolist())) == sorted(zip(t.chips[1].tolist(), t.chips[2].tolist()))
    with ctx.cell_index(dict(index_id=chips["index_id"], polygon_key=chips["polygon_key"])) as index:
        got = gpu_neighbours(ctx, p.geoms, t.geoms, index, rows, cells)
        assert got == want
        with ctx.geometry_table(t.geoms) as table:
            assert gpu_neighbours(ctx, p.geoms, table, index, rows, cells) == want
    assert want == (reorder(restate(p, t, rows, cells)[0]), restate(p, t, rows, cells)[1])
    if it == 2:
        assert want[0] and want[1]


def test_self_match_with_lines(ctx):
    """a line against the identical line is a self match; a closed line against the polygon with the same
    vertex sequence is not"""
    left_rows = [geom_wkb(line(SQ), True), geom_wkb(poly([SQ]), True)]
    right_rows = [geom_wkb(line(SQ), False), geom_wkb(poly([SQ])), geom_wkb(line(SQ, TRI)), geom_wkb(line(SQ[::-1]))]
    chips = (np.full(4, 7, np.int64), np.arange(4, dtype=np.int32))
    rows, cells = [0, 1], [7, 7]
    left, right = ctx.geometry_table(left_rows, lines=True), ctx.geometry_table(right_rows, lines=True)
    index = ctx.cell_index(chips)
    try:
        hl, hr = LCol.from_wkb(left_rows), LCol.from_wkb(right_rows)
        for keep in (False, True):
            assert gpu_neighbours(ctx, left, right, index, rows, cells, keep) == host_neighbours(chips, hl, hr, rows, cells, keep)
        got, _ = gpu_neighbours(ctx, left, right, index, rows, cells)
        assert [(l, c) for l, c, _ in got] == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3)]
    finally:
        for t in (left, right, index):
            t.close()


@pytest.mark.parametrize("name", ("pickups-trips", "zones-trips", "trips-pickups"))
def test_spatial_knn_against_literal(ctx, name):
    from mosaic_amd import SpatialKNN

    left, right, lit = knn_case(name)
    assert_knn_case_is_telling(lit)
    with SpatialKNN(ctx, right.geoms, **KNN_PARAMS) as model:
        got = model.transform(left.geoms)
        assert knn_columns_as_rows(got) == lit[0]
        assert [a.tolist() for a in model.active_sets] == lit[1]
        assert model.metrics()["match_count"] == float(len(lit[0]))
