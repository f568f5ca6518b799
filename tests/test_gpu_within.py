"""The distance-within join and SpatialKNN.transform_exact on the GPU (mosaic_within_candidates,
mosaic_within_neighbours, MosaicContext.st_dwithin_candidates / st_dwithin_join): the kernels k_wn_count /
k_wn_emit of mosaic_amd/csrc/ring_neighbours.hip and the shared tail against (H), the header's sequential
driver over all pairs compiled by g++, and (B), the Python restatement, both of tests/test_within.py --
equal row lists, identical distance bits, equal candidate counts."""
import ctypes
import math

import numpy as np
import pytest

from mosaic_amd import _native as N

from . import test_st_distance_lines as TL
from .test_ring_neighbours import FLOAT_MAX, knn_columns_as_rows, pickups64
from .test_st_distance import HostCol, bits, geom_wkb, poly, pt
from .test_within import (INF, NAN, WSide, all_pairs, assert_exact_case_is_telling, brute_knn, exact_case, exact_columns_as_rows,
                          host_candidates, host_within, literal_exact, non_ok_case, restate, row_medians, side)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


def gpu_within(ctx, left, right, radius, rows=None, keep_self=True):
    l, c, d = ctx.st_dwithin_join(left, right, radius, rows, keep_self)
    assert l.dtype == np.int64 and c.dtype == np.int64 and d.dtype == np.float64
    return list(zip(l.tolist(), c.tolist(), bits(d).tolist()))


def gpu_counts(ctx, left, right, radius, rows=None):
    k = ctx.st_dwithin_candidates(left, right, radius, rows)
    assert k.dtype == np.int64
    return k.tolist()


# ---- the filter kernels: integer-coordinate point columns ----
N_LAND = 257
CANDS = (0, 1, 3, 4, 5, 9)          # with within_tile = 4: none, below, at and above one tile, three tiles
R_NONE, R_SOME, R_ALL = 0.5, 14.0, 1000.0


@pytest.fixture(scope="module")
def probe(ctx):
    """landmarks on even, candidates on odd integer coordinates: no distance below 1"""
    rng = np.random.default_rng(17)
    lx, ly = 2.0 * rng.integers(-10, 10, N_LAND), 2.0 * rng.integers(-10, 10, N_LAND)
    cx, cy = 2.0 * rng.integers(-10, 10, 1030) + 1, 2.0 * rng.integers(-10, 10, 1030) + 1
    host = dict(left=HostCol.from_points(lx, ly), right={m: HostCol.from_points(cx[:m], cy[:m]) for m in CANDS + (1030,)})
    left = ctx.geometry_table((lx, ly))
    right = {m: ctx.geometry_table((cx[:m].copy(), cy[:m].copy())) for m in CANDS + (1030,)}
    yield dict(host=host, left=left, right=right)
    for t in [left] + list(right.values()):
        t.close()


def probe_rows(n):
    """n of the 257 landmark rows, ascending with gaps (all of them: None), and a radius of each kind in turn"""
    rows = None if n == N_LAND else np.sort(np.random.default_rng(n).choice(N_LAND, n, replace=False)).astype(np.int64)
    radius = np.array([R_NONE, R_SOME, R_ALL])[np.arange(n) % 3]
    return rows, radius


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_filter_row_and_candidate_counts(ctx, probe, n):
    rows, radius = probe_rows(n)
    h = probe["host"]
    try:
        ctx.set_option("within_tile", 4)
        for m in CANDS:
            want = host_within(h["left"], h["right"][m], radius, rows)
            want_k = host_candidates(h["left"], h["right"][m], radius, rows).tolist()
            for slices in (1, 3):
                ctx.set_option("within_slices", slices)
                assert gpu_within(ctx, probe["left"], probe["right"][m], radius, rows) == want, (m, slices)
                assert gpu_counts(ctx, probe["left"], probe["right"][m], radius, rows) == want_k, (m, slices)
            if n >= 63 and m == 9:
                per = {}
                for l, _, _ in want:
                    per[l] = per.get(l, 0) + 1
                ask = list(range(N_LAND)) if rows is None else rows.tolist()
                kept = [per.get(l, 0) for l in ask]
                assert all(k == 0 for k in kept[0::3]) and any(0 < k < m for k in kept[1::3]) and all(k == m for k in kept[2::3])
    finally:
        ctx.set_option("within_tile", 256)
        ctx.set_option("within_slices", 0)


def test_filter_defaults_on_257_by_1030(ctx, probe):
    """the default tile and automatic slices: 257 rows are two workgroups, 1030 candidates five tiles"""
    rows, radius = probe_rows(N_LAND)
    radius = np.where(radius == R_SOME, 3.0, radius)
    h = probe["host"]
    want = host_within(h["left"], h["right"][1030], radius)
    assert 0 < len(want) < N_LAND * 1030
    assert gpu_within(ctx, probe["left"], probe["right"][1030], radius) == want
    assert gpu_counts(ctx, probe["left"], probe["right"][1030], radius) == host_candidates(h["left"], h["right"][1030], radius).tolist()
    assert gpu_within(ctx, probe["left"], probe["right"][1030], radius, keep_self=False) == want  # no landmark is a candidate


def test_device_resident_rows_and_radius(ctx, probe):
    import torch

    rows, radius = probe_rows(65)
    h = probe["host"]
    dev = torch.device("cuda", ctx.device)
    want = host_within(h["left"], h["right"][9], radius, rows)
    assert gpu_within(ctx, probe["left"], probe["right"][9], torch.from_numpy(radius).to(dev), torch.from_numpy(rows).to(dev)) == want
    assert gpu_counts(ctx, probe["left"], probe["right"][9], torch.from_numpy(radius).to(dev), torch.from_numpy(rows).to(dev)) == \
        host_candidates(h["left"], h["right"][9], radius, rows).tolist()
    assert gpu_within(ctx, probe["left"], probe["right"][9], torch.tensor(R_ALL, dtype=torch.float64, device=dev)) == \
        host_within(h["left"], h["right"][9], R_ALL)


def test_distance_ties_are_ordered_by_candidate_row(ctx):
    cand = [(3, 4), (5, 0), (4, 3), (0, 5), (6, 0), (0, -5)]
    left = ctx.geometry_table((np.array([0.0]), np.array([0.0])))
    right = ctx.geometry_table((np.array([c[0] for c in cand], np.float64), np.array([c[1] for c in cand], np.float64)))
    try:
        l, c, d = ctx.st_dwithin_join(left, right, 6.0)
        assert c.tolist() == [0, 1, 2, 3, 5, 4] and d.tolist() == [5.0] * 5 + [6.0]
        assert ctx.st_dwithin_join(left, right, 5.0)[1].tolist() == [0, 1, 2, 3, 5]
        assert ctx.st_dwithin_join(left, right, math.nextafter(5.0, 0.0))[1].tolist() == []
    finally:
        left.close()
        right.close()


# ---- real geometries: polygon and line sides, radii of every kind, self matches ----
@pytest.fixture(scope="module")
def tabs(ctx):
    from .test_ring_neighbours import zones8

    t = dict(zones=ctx.geometry_table(zones8().geoms), pickups=ctx.geometry_table(pickups64().geoms),
             trips=ctx.geometry_table(TL.trips(24)))
    yield t
    for v in t.values():
        v.close()


def check_gpu(ctx, tabs, names, radius, rows=None, keep_self=True):
    left, right = side(names[0]), side(names[1])
    want = restate(left, right, all_pairs(*names), radius, rows, keep_self)
    assert gpu_within(ctx, tabs[names[0]], tabs[names[1]], radius, rows, keep_self) == want
    counts = gpu_counts(ctx, tabs[names[0]], tabs[names[1]], radius, rows)
    assert counts == host_candidates(left.col, right.col, radius, rows).tolist()
    return want


@pytest.mark.parametrize("names", (("pickups", "zones"), ("zones", "zones"), ("trips", "zones")))
def test_polygon_and_line_sides(ctx, tabs, names):
    right = side(names[1])
    med = row_medians(all_pairs(*names), right.eligible)
    assert check_gpu(ctx, tabs, names, med)
    check_gpu(ctx, tabs, names, 0.0)
    assert len(check_gpu(ctx, tabs, names, INF)) == side(names[0]).n * right.n
    rows = list(range(1, side(names[0]).n, 3))
    check_gpu(ctx, tabs, names, med[rows], rows=rows, keep_self=False)


def test_self_matches(ctx, tabs):
    names = ("zones", "zones")
    z = side("zones")
    med = row_medians(all_pairs(*names), z.eligible)
    kept = check_gpu(ctx, tabs, names, med)
    want = check_gpu(ctx, tabs, names, med, keep_self=False)
    assert {(l, c) for l, c, _ in kept} - {(l, c) for l, c, _ in want} == {(g, g) for g in range(z.n)}
    zero = check_gpu(ctx, tabs, names, 0.0, keep_self=False)
    assert zero and all(b == 0 for _, _, b in zero)


def test_radius_kinds(ctx, tabs):
    names = ("pickups", "zones")
    left = side("pickups")
    D = all_pairs(*names)
    l0 = 5
    tie = float(np.sort(D[l0])[D.shape[1] // 2])
    kept = check_gpu(ctx, tabs, names, tie, rows=[l0])
    assert kept[-1][2] == int(bits([tie])[0])
    assert check_gpu(ctx, tabs, names, math.nextafter(tie, 0.0), rows=[l0]) == kept[:-1]
    for radius in (FLOAT_MAX, INF):
        assert len(check_gpu(ctx, tabs, names, radius)) == D.size
    for radius in (NAN, -1.0, -INF):
        assert check_gpu(ctx, tabs, names, radius) == []
    assert check_gpu(ctx, tabs, names, -0.0) == check_gpu(ctx, tabs, names, 0.0)
    kinds = np.array([0.0, tie, NAN, -1.0, INF, FLOAT_MAX, math.nextafter(tie, 0.0), 1e-3])
    radius = kinds[np.arange(left.n) % len(kinds)]
    check_gpu(ctx, tabs, names, radius)
    for rows in ([0], [left.n - 1], [3, 4, 9, 40]):
        check_gpu(ctx, tabs, names, radius[rows], rows=rows)


def test_null_row_path_and_empty_rows_never_pair(ctx):
    rows, models = non_ok_case()
    col = HostCol.from_wkb(rows)
    tab = ctx.geometry_table(rows)
    five = int(bits([5.0])[0])
    try:
        for radius in (INF, FLOAT_MAX, 5.0):
            assert gpu_within(ctx, tab, tab, radius) == [(0, 0, 0), (0, 4, five), (4, 4, 0), (4, 0, five)]
            assert gpu_within(ctx, tab, tab, radius, keep_self=False) == [(0, 4, five), (4, 0, five)]
            assert gpu_within(ctx, tab, tab, radius) == host_within(col, col, radius)
        assert gpu_within(ctx, tab, tab, 0.0) == [(0, 0, 0), (4, 4, 0)]
        assert gpu_counts(ctx, tab, tab, INF) == [2, 0, 0, 0, 2] == host_candidates(col, col, INF).tolist()
    finally:
        tab.close()


# ---- errors write nothing ----
def test_errors_write_nothing(ctx, probe):
    from mosaic_amd import MosaicError

    left, right = probe["left"], probe["right"][9]
    for rows in ([1, 1], [2, 1], [0, 5, 4], [-1, 0], [0, N_LAND]):
        with pytest.raises(MosaicError) as e:
            ctx.st_dwithin_join(left, right, 1.0, rows)
        assert e.value.code == N.MOSAIC_E_ARG
        with pytest.raises(MosaicError) as e:
            ctx.st_dwithin_candidates(left, right, 1.0, rows)
        assert e.value.code == N.MOSAIC_E_ARG
    lib = N.lib()
    rows, radius = np.array([2, 1], np.int64), np.ones(2)
    h = ctypes.c_void_p()
    assert lib.mosaic_within_neighbours(ctx.handle, left.handle, right.handle, N.ptr(rows), N.ptr(radius), 2, 1,
                                        ctypes.byref(h)) == N.MOSAIC_E_ARG and not h
    counts = np.full(2, -7, np.int64)
    assert lib.mosaic_within_candidates(ctx.handle, left.handle, right.handle, N.ptr(rows), N.ptr(radius), 2,
                                        N.ptr(counts)) == N.MOSAIC_E_ARG and (counts == -7).all()
    # rows == NULL asks for rows 0 .. n - 1 of the landmark column
    radius = np.ones(N_LAND + 1)
    assert lib.mosaic_within_neighbours(ctx.handle, left.handle, right.handle, None, N.ptr(radius), N_LAND + 1, 1,
                                        ctypes.byref(h)) == N.MOSAIC_E_ARG and not h
    with pytest.raises(ValueError):
        ctx.st_dwithin_join(left, right, np.ones(3))  # one radius per requested row


def test_null_context_is_refused_before_any_device_work():
    lib = N.lib()
    out = ctypes.c_int(0)
    assert lib.mosaic_resolution(N.GRID_H3, 16, ctypes.byref(out)) == N.MOSAIC_E_RES
    before = lib.mosaic_last_error()
    h = ctypes.c_void_p()
    assert lib.mosaic_within_neighbours(None, None, None, None, None, 0, 1, ctypes.byref(h)) == N.MOSAIC_E_ARG and not h
    msg = lib.mosaic_last_error()
    assert msg and msg != before and b"null context" in msg
    assert lib.mosaic_within_candidates(None, None, None, None, None, 0, None) == N.MOSAIC_E_ARG
    assert b"within_candidates" in lib.mosaic_last_error()


# ---- SpatialKNN.transform_exact ----
@pytest.mark.parametrize("name, budget", (("pickups-zones", 1 << 24), ("pickups-zones", 20), ("zones-zones", 20)))
def test_transform_exact_equals_the_brute_force(ctx, name, budget):
    from mosaic_amd import SpatialKNN

    left, right, wl, wr, D, lit, p = exact_case(name)
    k = p["k_neighbours"]
    brute = brute_knn(wl, wr, D, k, FLOAT_MAX)
    if name == "pickups-zones":
        assert_exact_case_is_telling(lit, brute, k)
    with SpatialKNN(ctx, right.geoms, **p) as model:
        approx = knn_columns_as_rows(model.transform(left.geoms))
        assert approx == lit[0]  # transform returns what it returned before
        got = model.transform_exact(left.geoms, pair_budget=budget)
        rows = exact_columns_as_rows(got)
        assert [(l, c, b, number) for l, c, b, _, number in rows] == brute
        assert rows == literal_exact(wl, wr, D, lit[2], lit[1], k, FLOAT_MAX)
        assert [a.tolist() for a in model.active_sets] == lit[1]
        stats = model.exact_stats
        assert stats["ring_radius"] + stats["threshold_radius"] == left.n and stats["threshold_radius"] > 0
        assert stats["pairs_within"] >= len(rows) and stats["candidate_pairs"] >= stats["pairs_within"]
        if budget < 1 << 24:
            assert stats["batches"] >= 3 and budget < wr.n  # a landmark with the threshold radius exceeds the budget alone
        else:
            assert stats["batches"] == 1
        m = model.metrics()
        assert m["match_count"] == float(len(rows)) and m["max_neighbours"] == float(k)
        assert m["max_radius"] == float(got["distance"].max()) and m["convergence_iteration"] == float(got["iteration"].max())
        assert knn_columns_as_rows(model.transform(left.geoms)) == lit[0]  # and still does


def test_transform_exact_distance_threshold(ctx):
    from mosaic_amd import SpatialKNN

    thr = 0.004
    left, right, wl, wr, D, lit, p = exact_case("pickups-zones", thr)
    brute = brute_knn(wl, wr, D, p["k_neighbours"], thr)
    assert 0 < len(brute) < len(brute_knn(wl, wr, D, p["k_neighbours"], FLOAT_MAX))
    with SpatialKNN(ctx, right.geoms, **p) as model:
        rows = exact_columns_as_rows(model.transform_exact(left.geoms))
    assert [(l, c, b, number) for l, c, b, _, number in rows] == brute
    assert rows == literal_exact(wl, wr, D, lit[2], lit[1], p["k_neighbours"], thr)


def test_transform_exact_trips_against_pickups(ctx):
    """40 trips (a LineSet) as landmarks, the 64 pickups as candidates"""
    from mosaic_amd import SpatialKNN

    ls = TL.trips(40)
    wl = WSide(TL.LCol.from_lineset(ls), [("line", ls.lines(g)) for g in range(len(ls))])
    pk = pickups64()
    wr = WSide(pk.col, pk.models)
    D = TL.host_distance(wl.col, wr.col, np.repeat(np.arange(wl.n), wr.n), np.tile(np.arange(wr.n), wl.n)).reshape(wl.n, wr.n)
    brute = brute_knn(wl, wr, D, 3, FLOAT_MAX)
    assert len(brute) == 3 * wl.n
    with SpatialKNN(ctx, pk.geoms, k_neighbours=3, index_resolution=8, max_iterations=2) as model:
        got = model.transform_exact(ls, pair_budget=100)
        rows = exact_columns_as_rows(got)
        assert [(l, c, b, number) for l, c, b, _, number in rows] == brute
        assert model.exact_stats["batches"] >= 3
        last = {l: max(i + 1 for i, a in enumerate(model.active_sets) if l in a.tolist()) for l in range(wl.n)}
        assert all(1 <= it <= last[l] + 1 for l, _, _, it, _ in rows)
