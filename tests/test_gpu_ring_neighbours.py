"""GridRingNeighbours and the approximate SpatialKNN on the GPU (mosaic_cell_index_*,
mosaic_ring_neighbours, MosaicContext.cell_index / grid_ring_neighbours, mosaic_amd.knn.SpatialKNN):
the kernels of mosaic_amd/csrc/ring_neighbours.hip against (H), the header's sequential driver compiled
by g++, and (B), the Python restatement, both of tests/test_ring_neighbours.py -- equal row lists,
identical distance bits.  The primitive joins on the cells' int64 values alone, so the probe shapes use
made-up cell ids; the index is a sorted array (no hash table, hence no option that shrinks one)."""
import numpy as np
import pytest

from mosaic_amd import _native as N

from .test_ring_neighbours import (FLOAT_MAX, KNN_PARAMS, HostIndex, Side, as_rows, assert_knn_case_is_telling, host_neighbours,
                                   knn_case, knn_columns_as_rows, literal_knn, literal_step, non_ok_case, pickups64, reorder, restate,
                                   zones8)
from .test_st_distance import HostCol, geom_wkb, pickups, poly, pt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


def gpu_neighbours(ctx, left, right, index, rows, cells, keep_self=False):
    l, c, d, un = ctx.grid_ring_neighbours(left, right, index, rows, cells, keep_self)
    assert l.dtype == np.int64 and c.dtype == np.int64 and d.dtype == np.float64 and un.dtype == bool
    return as_rows(l, c, d), set(np.flatnonzero(un).tolist())


# ---- the probe: made-up cells over point columns ----
N_CAND = 68
CELL_ONE, CELL_TWO, CELL_MANY = 200, 300, 400           # 1, 2 and 65 candidates
MISS_BELOW, MISS_BETWEEN, MISS_ABOVE = 50, 250, 500     # a cell with no candidate: below, between, above the indexed ones
PROBE_CELLS = (CELL_ONE, MISS_BELOW, CELL_TWO, CELL_MANY, MISS_BETWEEN, CELL_ONE, MISS_ABOVE)
N_LAND = 5


@pytest.fixture(scope="module")
def probe(ctx):
    """candidate row 0 in CELL_ONE, rows 1-2 in CELL_TWO, rows 3-67 in CELL_MANY (chips shuffled, some twice)"""
    rng = np.random.default_rng(5)
    cx, cy = rng.integers(-1000, 1000, N_CAND).astype(np.float64), rng.integers(-1000, 1000, N_CAND).astype(np.float64)
    lx, ly = rng.integers(-1000, 1000, N_LAND).astype(np.float64), rng.integers(-1000, 1000, N_LAND).astype(np.float64)
    keys = np.arange(N_CAND, dtype=np.int32)
    cells = np.where(keys == 0, CELL_ONE, np.where(keys <= 2, CELL_TWO, CELL_MANY)).astype(np.int64)
    order = rng.permutation(np.r_[np.arange(N_CAND), np.arange(0, N_CAND, 7)])
    cells, keys = cells[order], keys[order]
    host = dict(index=HostIndex(cells, keys), left=HostCol.from_points(lx, ly), right=HostCol.from_points(cx, cy))
    assert (host["index"].n_cells, host["index"].n_entries, host["index"].max_per_cell) == (3, N_CAND, 65)
    left, right = ctx.geometry_table((lx, ly)), ctx.geometry_table((cx, cy))
    index = ctx.cell_index((cells, keys))
    yield dict(host=host, left=left, right=right, index=index)
    for t in (left, right, index):
        t.close()


def probe_rows(n):
    """n (landmark, cell) rows: every landmark meets every kind of cell, rows repeat from 35 on"""
    i = np.arange(n)
    return (i % N_LAND).astype(np.int64), np.array(PROBE_CELLS, np.int64)[(i // N_LAND) % len(PROBE_CELLS)]


def test_cell_index_info(ctx, probe):
    assert probe["index"].info() == dict(n_cells=3, n_entries=N_CAND, max_per_cell=65)
    z = zones8()
    with ctx.cell_index(dict(index_id=z.chips[1], polygon_key=z.chips[2])) as ix:
        h = z.host_index()
        assert ix.info() == dict(n_cells=h.n_cells, n_entries=h.n_entries, max_per_cell=h.max_per_cell)
    with ctx.cell_index(np.zeros(0, np.int64)) as empty:
        assert empty.info() == dict(n_cells=0, n_entries=0, max_per_cell=0)
        assert gpu_neighbours(ctx, probe["left"], probe["right"], empty, [0, 1], [CELL_ONE, CELL_TWO]) == ([], {0, 1})


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_probe_row_counts(ctx, probe, n):
    rows, cells = probe_rows(n)
    h = probe["host"]
    want = host_neighbours(h["index"], h["left"], h["right"], rows, cells)
    got = gpu_neighbours(ctx, probe["left"], probe["right"], probe["index"], rows, cells)
    assert got == want
    if n >= 64:
        assert len(want[0]) == N_LAND * N_CAND and want[1] == set(range(N_LAND))  # 257 rows, 340 distinct pairs


def test_probe_each_cell_kind_and_unmatched(ctx, probe):
    h = probe["host"]
    for cell, n_cand in ((CELL_ONE, 1), (CELL_TWO, 2), (CELL_MANY, 65), (MISS_BELOW, 0), (MISS_BETWEEN, 0), (MISS_ABOVE, 0)):
        got = gpu_neighbours(ctx, probe["left"], probe["right"], probe["index"], [3], [cell])
        assert got == host_neighbours(h["index"], h["left"], h["right"], [3], [cell])
        assert len(got[0]) == n_cand and got[1] == (set() if n_cand else {3})
    # landmark 1: only cells without a chip -> the flag and no row; landmark 2: only indexed cells -> rows, no flag;
    # landmark 4: both; landmarks 0 and 3: no row given at all
    rows = [1, 1, 2, 2, 2, 4, 4, 2]
    cells = [MISS_BELOW, MISS_ABOVE, CELL_ONE, CELL_TWO, CELL_ONE, CELL_MANY, MISS_BETWEEN, CELL_TWO]
    got, un = gpu_neighbours(ctx, probe["left"], probe["right"], probe["index"], rows, cells)
    assert (got, un) == host_neighbours(h["index"], h["left"], h["right"], rows, cells)
    assert un == {1, 4} and {l for l, _, _ in got} == {2, 4}
    assert sorted(c for l, c, _ in got if l == 2) == [0, 1, 2]  # the duplicate rows add nothing


def test_probe_device_rows(ctx, probe):
    import torch

    rows, cells = probe_rows(257)
    h = probe["host"]
    dev = torch.device("cuda", ctx.device)
    got = gpu_neighbours(ctx, probe["left"], probe["right"], probe["index"], torch.from_numpy(rows).to(dev),
                         torch.from_numpy(cells).to(dev))
    assert got == host_neighbours(h["index"], h["left"], h["right"], rows, cells)


# ---- real chips: de-duplication, self matches, ties ----
@pytest.fixture(scope="module")
def nyc(ctx):
    z, p = zones8(), pickups64()
    tabs = dict(zones=ctx.geometry_table(z.geoms), pickups=ctx.geometry_table(p.geoms))
    idx = dict(zones=ctx.cell_index(dict(index_id=z.chips[1], polygon_key=z.chips[2])), pickups=ctx.cell_index(p.chips[1]))
    yield dict(z=z, p=p, tabs=tabs, idx=idx)
    for t in list(tabs.values()) + list(idx.values()):
        t.close()


@pytest.mark.parametrize("it", (1, 2, 3))
def test_pickups_against_zones(ctx, nyc, it):
    p, z = nyc["p"], nyc["z"]
    rows, cells = p.ring_rows(it)
    want, want_un = restate(p, z, rows, cells)
    got = gpu_neighbours(ctx, nyc["tabs"]["pickups"], nyc["tabs"]["zones"], nyc["idx"]["zones"], rows, cells)
    assert got == (reorder(want), want_un)
    if it == 1:
        # one zone spans several cells of one pickup's ring: more hits than pairs, each pair once
        by_cell = z.by_cell()
        hits = sum(len(by_cell.get(c, ())) for c in cells.tolist())
        assert hits > len(want) == len({(l, c) for l, _, c in want})


def test_zones_against_pickups_with_duplicate_rows(ctx, nyc):
    p, z = nyc["p"], nyc["z"]
    rows, cells = z.ring_rows(2)
    rows, cells = np.concatenate([rows, rows[::3]]), np.concatenate([cells, cells[::3]])
    want, want_un = restate(z, p, rows, cells)
    assert want and want_un
    assert gpu_neighbours(ctx, nyc["tabs"]["zones"], nyc["tabs"]["pickups"], nyc["idx"]["pickups"], rows, cells) == \
        (reorder(want), want_un)


@pytest.mark.parametrize("it", (1, 2))
def test_zones_against_zones_self_matches(ctx, nyc, it):
    z = nyc["z"]
    rows, cells = z.ring_rows(it)
    t, ix = nyc["tabs"]["zones"], nyc["idx"]["zones"]
    want, want_un = restate(z, z, rows, cells)
    assert gpu_neighbours(ctx, t, t, ix, rows, cells) == (reorder(want), want_un)
    assert all(l != c for l, _, c in want)
    kept, _ = restate(z, z, rows, cells, keep_self=True)
    assert gpu_neighbours(ctx, t, t, ix, rows, cells, keep_self=True) == (reorder(kept), want_un)
    if it == 1:
        assert {(l, c) for l, _, c in kept} - {(l, c) for l, _, c in want} == {(g, g) for g in range(z.n)}


def test_self_match_is_exact_content(ctx):
    """candidates of one cell: the landmark's geometry, the same again, the same as WKB in the other byte
    order, the same ring from another start vertex, a multipolygon with the geometry as its first part"""
    sq = [(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)]
    rot = sq[1:] + [sq[1]]
    land = [poly([sq])]
    cand = [poly([sq]), poly([sq]), poly([sq]), poly([rot]), poly([sq], [[(20, 20), (30, 20), (30, 30), (20, 20)]])]
    order = [True, True, False, True, True]  # big-endian, except candidate 2
    left = ctx.geometry_table([geom_wkb(g, True) for g in land])
    right = ctx.geometry_table([geom_wkb(g, be) for g, be in zip(cand, order)])
    index = ctx.cell_index((np.full(len(cand), 9, np.int64), np.arange(len(cand), dtype=np.int32)))
    try:
        got, un = gpu_neighbours(ctx, left, right, index, [0], [9])
        assert [(l, c) for l, c, _ in got] == [(0, 3), (0, 4)] and un == set()
        assert all(b == 0 for _, _, b in got)  # distance 0.0: a tie, ordered by the candidate row
        kept, _ = gpu_neighbours(ctx, left, right, index, [0], [9], keep_self=True)
        assert [(l, c) for l, c, _ in kept] == [(0, c) for c in range(len(cand))]
        hl = HostCol.from_wkb([geom_wkb(g, True) for g in land])
        hr = HostCol.from_wkb([geom_wkb(g, be) for g, be in zip(cand, order)])
        hi = HostIndex(np.full(len(cand), 9, np.int64), np.arange(len(cand)))
        assert (got, un) == host_neighbours(hi, hl, hr, [0], [9])
        assert (kept, un) == host_neighbours(hi, hl, hr, [0], [9], keep_self=True)
    finally:
        for t in (left, right, index):
            t.close()


def test_null_and_row_path_rows_are_no_self_matches(ctx):
    """null rows and LineStrings on both sides: stored as empty geometries, yet no self matches; their
    pairs stay with distance NaN and sort last"""
    left_rows, right_rows, want = non_ok_case()
    left, right = ctx.geometry_table(left_rows), ctx.geometry_table(right_rows)
    index = ctx.cell_index(np.full(len(right_rows), 7, np.int64))
    try:
        rows, cells = np.arange(len(left_rows)), np.full(len(left_rows), 7, np.int64)
        assert gpu_neighbours(ctx, left, right, index, rows, cells) == (want, set())
        assert gpu_neighbours(ctx, left, right, index, rows, cells, keep_self=True) == ([(0, 0, 0)] + want, set())
        hi = HostIndex(np.full(len(right_rows), 7, np.int64), np.arange(len(right_rows)))
        assert (want, set()) == host_neighbours(hi, HostCol.from_wkb(left_rows), HostCol.from_wkb(right_rows), rows, cells)
    finally:
        for t in (left, right, index):
            t.close()


def test_ties_are_ordered_by_candidate_row(ctx):
    """two polygon candidates hold the landmark point (distance 0.0 twice), a third lies apart and a
    point candidate lies nearer than it; chips in another order than the rows"""
    big = [(0, 0), (100, 0), (100, 100), (0, 100), (0, 0)]
    small = [(40, 40), (60, 40), (60, 60), (40, 60), (40, 40)]
    far = [(200, 0), (300, 0), (300, 100), (200, 100), (200, 0)]
    cand = [poly([far]), poly([big]), pt(50, 58), poly([small])]
    left = ctx.geometry_table((np.array([50.0]), np.array([50.0])))
    right = ctx.geometry_table([geom_wkb(g) for g in cand])
    index = ctx.cell_index((np.array([4, 4, 4, 4], np.int64), np.array([3, 0, 2, 1], np.int32)))
    try:
        l, c, d, un = ctx.grid_ring_neighbours(left, right, index, [0, 0], [4, 4])
        assert c.tolist() == [1, 3, 2, 0] and d.tolist() == [0.0, 0.0, 8.0, 150.0] and not un.any()
    finally:
        for t in (left, right, index):
            t.close()


def test_errors(ctx, probe):
    from mosaic_amd import MosaicError

    for rows in ([0, N_LAND], [-1, 0]):
        with pytest.raises(MosaicError) as e:
            ctx.grid_ring_neighbours(probe["left"], probe["right"], probe["index"], rows, [CELL_ONE, CELL_ONE])
        assert e.value.code == N.MOSAIC_E_ARG
    with ctx.cell_index((np.array([1, 2], np.int64), np.array([0, N_CAND], np.int32))) as beyond:
        with pytest.raises(MosaicError) as e:
            ctx.grid_ring_neighbours(probe["left"], probe["right"], beyond, [0], [1])
        assert e.value.code == N.MOSAIC_E_ARG
    with pytest.raises(MosaicError) as e:
        ctx.cell_index((np.array([1, 2], np.int64), np.array([0, -1], np.int32)))
    assert e.value.code == N.MOSAIC_E_ARG


# ---- SpatialKNN ----
@pytest.mark.parametrize("name", ("pickups-zones", "zones-zones"))
def test_spatial_knn_against_literal(ctx, name):
    from mosaic_amd import SpatialKNN

    left, right, lit = knn_case(name)
    assert_knn_case_is_telling(lit)
    with SpatialKNN(ctx, right.geoms, **KNN_PARAMS) as model:
        got = model.transform(left.geoms)
        assert knn_columns_as_rows(got) == lit[0]
        assert [a.tolist() for a in model.active_sets] == lit[1]
        m = model.metrics()
        assert m == dict(match_count=float(len(lit[0])), max_neighbours=float(max(r[4] for r in lit[0])),
                         max_radius=float(got["distance"].max()), min_radius=float(got["distance"].min()),
                         convergence_iteration=float(max(r[3] for r in lit[0])))
        # the candidates' column and index are kept: a second transform gives the same rows
        assert knn_columns_as_rows(model.transform(left.geoms)) == lit[0]


def test_spatial_knn_reference_assertions(ctx):
    """SpatialKNNBehaviors.scala:57-61 on zones against zones.  Three of the 35 zones find no other zone
    within the 4 iterations of the cases above; literal_knn reaches every landmark with 8."""
    from mosaic_amd import SpatialKNN

    z = zones8()
    p = dict(KNN_PARAMS, max_iterations=8, early_stop_iterations=3)
    final, actives, _ = literal_knn(z.n, literal_step(z, z), p["k_neighbours"], p["max_iterations"], p["early_stop_iterations"],
                                    p["distance_threshold"])
    assert {r[0] for r in final} == set(range(z.n))
    with SpatialKNN(ctx, z.geoms, **p) as model:
        got = model.transform(z.geoms)
    assert knn_columns_as_rows(got) == final
    assert got["distance"].max() <= p["distance_threshold"]
    assert got["iteration"].max() <= p["max_iterations"]
    assert got["neighbour_number"].max() <= p["k_neighbours"]
    assert set(got["landmark_row"].tolist()) == set(range(z.n))


def test_spatial_knn_early_stop(ctx):
    """three point candidates and k = 5: the matches stop growing and the early-stop counter ends the run"""
    from mosaic_amd import SpatialKNN

    x, y = pickups()
    left = Side("H3", (x[:8].copy(), y[:8].copy()), 8)
    right = Side("H3", (x[:3].copy(), y[:3].copy()), 8)
    final, actives, _ = literal_knn(left.n, literal_step(left, right), 5, 12, 1, FLOAT_MAX)
    assert 3 <= len(actives) < 12 and actives[-1]
    with SpatialKNN(ctx, right.geoms, k_neighbours=5, index_resolution=8, max_iterations=12, early_stop_iterations=1) as model:
        got = model.transform(left.geoms)
        assert knn_columns_as_rows(got) == final
        assert [a.tolist() for a in model.active_sets] == actives


def test_spatial_knn_distance_threshold(ctx):
    from mosaic_amd import SpatialKNN

    left, right, lit = knn_case("pickups-zones")
    positive = sorted(np.array([r[2] for r in lit[0]], np.int64).view(np.float64))
    thr = float(positive[len(positive) // 2])
    p = dict(KNN_PARAMS, distance_threshold=thr)
    final, actives, _ = literal_knn(left.n, literal_step(left, right), p["k_neighbours"], p["max_iterations"],
                                    p["early_stop_iterations"], thr)
    assert 0 < len(final) < len(lit[0])
    with SpatialKNN(ctx, right.geoms, **p) as model:
        got = model.transform(left.geoms)
        assert knn_columns_as_rows(got) == final and got["distance"].max() <= thr
        assert [a.tolist() for a in model.active_sets] == actives
