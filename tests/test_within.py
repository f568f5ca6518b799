"""The distance-within join (mosaic_within_candidates / mosaic_within_neighbours, MosaicContext.st_dwithin_join)
and SpatialKNN.transform_exact, CPU side: the header's sequential driver rn::within and the filter's count
rn::within_candidates (mosaic_amd/csrc/ring_neighbours.h, compiled by g++ as tests/native/within_host.cpp
-- source (H) below) and the numpy bookkeeping of mosaic_amd/knn.py.  The kernels are checked against (H)
in tests/test_gpu_within.py.

Expected values never come from the code under test:
  (B) a Python restatement over all pairs: eligibility and self matches decided on the tests' own
      geometry models, tests/test_st_distance_lines.py's kind-aware host_distance for the values, a
      comparison of the distance's and the radius' bits, and `sorted` for the order.
  np_box_lower_bound: dist::box_lower_bound's formula in numpy (f64, no fused operation: the same bits).
  brute_knn / literal_exact: every landmark's first k of all candidates, and transform_exact's dataflow,
      in plain Python lists, dicts and sets fed from (B).
All comparisons are exact: equal row lists, identical distance bits."""
import ctypes
import functools
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from mosaic_amd import _native as N
from mosaic_amd import knn as K

from tests import test_st_distance_lines as TL
from tests.test_ring_neighbours import (FLOAT_MAX, Side, host_neighbours, literal_knn, literal_step, london4, pickups64, zones8)
from tests.test_st_distance import HostCol, bits, geom_wkb, pickups, poly, pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mosaic_within_candidates", "mosaic_within_neighbours", "mosaic_within_neighbours_last_ms")
INF = float("inf")
NAN = float("nan")


# ---- (H) the host library ----
@functools.lru_cache(maxsize=None)
def wn_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="wn_host_"), "libwn.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "within_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    for name, args, res in (("wn_within", [vp, vp, vp, vp, i64, ctypes.c_int], vp),
                            ("wn_candidates", [vp, vp, vp, vp, i64, vp], ctypes.c_int),
                            ("wn_result_info", [vp, vp], None), ("wn_result_export", [vp, vp, vp, vp, vp], None),
                            ("wn_result_free", [vp], None), ("wn_boxes", [vp, vp], None)):
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    return lib


def radii_for(radius, n):
    r = np.asarray(radius, np.float64)
    return np.full(n, float(r)) if r.ndim == 0 else np.ascontiguousarray(r)


def host_within(left, right, radius, rows=None, keep_self=True):
    """(H): [(landmark, candidate, distance bits)] in the result's order.  ``left`` / ``right``: host columns."""
    rows = None if rows is None else np.ascontiguousarray(rows, np.int64)
    n = left.n if rows is None else len(rows)
    radius = radii_for(radius, n)
    assert len(radius) == n
    lib = wn_lib()
    h = lib.wn_within(left.handle, right.handle, N.ptr(rows), N.ptr(radius), n, int(keep_self))
    if not h:
        raise IndexError("rows out of range or not strictly ascending")
    try:
        info = np.zeros(2, np.int64)
        lib.wn_result_info(h, N.ptr(info))
        m, n_left = int(info[0]), int(info[1])
        assert n_left == left.n
        l, c, d = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.float64)
        un = np.ones(max(n_left, 1), np.uint8)
        lib.wn_result_export(h, N.ptr(l), N.ptr(c), N.ptr(d), N.ptr(un))
        assert not un[:n_left].any()  # unmatched is all zero
    finally:
        lib.wn_result_free(h)
    return list(zip(l[:m].tolist(), c[:m].tolist(), bits(d[:m]).tolist()))


def host_candidates(left, right, radius, rows=None):
    """(H): the filter's count per requested row"""
    rows = None if rows is None else np.ascontiguousarray(rows, np.int64)
    n = left.n if rows is None else len(rows)
    radius = radii_for(radius, n)
    counts = np.full(max(n, 1), -7, np.int64)
    if wn_lib().wn_candidates(left.handle, right.handle, N.ptr(rows), N.ptr(radius), n, N.ptr(counts)):
        assert (counts == -7).all()  # nothing written
        raise IndexError("rows out of range or not strictly ascending")
    return counts[:n]


def boxes(col):
    out = np.zeros((max(col.n, 1), 4), np.float64)
    wn_lib().wn_boxes(col.handle, N.ptr(out))
    return out[:col.n]


def np_box_lower_bound(a, b):
    """dist::box_lower_bound (mosaic_amd/csrc/st_distance.h) of boxes a[..., 4] and b[..., 4], broadcast"""
    a0, a1, a2, a3 = (a[..., i] for i in range(4))
    b0, b1, b2, b3 = (b[..., i] for i in range(4))
    with np.errstate(invalid="ignore"):
        dx = np.where(b0 > a2, b0 - a2, 0.0)
        dx = np.where(a0 > b2, a0 - b2, dx)
        dy = np.where(b1 > a3, b1 - a3, 0.0)
        dy = np.where(a1 > b3, a1 - b3, dy)
        ex = np.where(a2 > b2, a2, b2) - np.where(a0 < b0, a0, b0)
        ey = np.where(a3 > b3, a3, b3) - np.where(a1 < b1, a1, b1)
        gap = np.sqrt(dx * dx + dy * dy)
        return gap * (1.0 - 2.0 ** -50) - (ex + ey) * 2.0 ** -47


# ---- the sides of a join: geometry models (None: a null or row-path row), a host column ----
class WSide:
    def __init__(self, col, models):
        self.col, self.models, self.n = col, models, len(models)
        assert col.n == self.n
        self.flat = [None if g is None else TL.flat(g) for g in models]
        self.eligible = np.array([g is not None and len(TL.facets_of(g)[0]) > 0 for g in models], bool)


@functools.lru_cache(maxsize=None)
def side(name):
    if name in ("zones", "pickups", "london"):
        s = {"zones": zones8, "pickups": pickups64, "london": london4}[name]()
        return WSide(s.col, s.models)
    if name == "trips":
        ls = TL.trips(24)
        return WSide(TL.LCol.from_lineset(ls), [("line", ls.lines(g)) for g in range(len(ls))])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def all_pairs(left_name, right_name):
    """(B)'s values: the kind-aware host distance of every (left row, right row), NaN where a row is not OK"""
    left, right = side(left_name), side(right_name)
    li, ri = np.repeat(np.arange(left.n), right.n), np.tile(np.arange(right.n), left.n)
    return TL.host_distance(left.col, right.col, li, ri).reshape(left.n, right.n)


def restate(left, right, D, radius, rows=None, keep_self=True):
    """(B): [(landmark, candidate, distance bits)] ordered; D: the distances of all pairs"""
    rows = list(range(left.n)) if rows is None else list(rows)
    radius = radii_for(radius, len(rows)).tolist()
    out = []
    for l, r in zip(rows, radius):
        if not left.eligible[l] or not r >= 0:
            continue
        rb = int(bits([r + 0.0])[0])
        for c in range(right.n):
            if not right.eligible[c]:
                continue
            if not keep_self and left.flat[l] == right.flat[c]:
                continue
            b = int(bits([D[l, c]])[0])
            if b <= rb:
                out.append((l, b, c))
    return [(l, c, b) for l, b, c in sorted(out)]


def np_candidates(left, right, radius, rows=None):
    rows = np.arange(left.n) if rows is None else np.asarray(rows, np.int64)
    radius = radii_for(radius, len(rows))
    lb = np_box_lower_bound(boxes(left.col)[rows][:, None, :], boxes(right.col)[None, :, :])
    with np.errstate(invalid="ignore"):
        ok = (lb <= radius[:, None]) & right.eligible[None, :] & left.eligible[rows][:, None] & (radius >= 0)[:, None]
    return ok.sum(axis=1).astype(np.int64)


def check(left, right, D, radius, rows=None, keep_self=True):
    """(H) = (B), the count = the numpy restatement, and the count covers the pairs"""
    want = restate(left, right, D, radius, rows, keep_self)
    got = host_within(left.col, right.col, radius, rows, keep_self)
    assert got == want
    counts = host_candidates(left.col, right.col, radius, rows)
    assert counts.tolist() == np_candidates(left, right, radius, rows).tolist()
    ask = list(range(left.n)) if rows is None else list(rows)
    kept = restate(left, right, D, radius, rows, True)
    per_row = {l: 0 for l in ask}
    for l, _, _ in kept:
        per_row[l] += 1
    assert all(counts[i] >= per_row[l] for i, l in enumerate(ask))
    return want


def row_medians(D, eligible):
    """per row, the median of the row's distances to the eligible candidates: a tie with one of them"""
    out = np.zeros(D.shape[0])
    for l in range(D.shape[0]):
        v = np.sort(D[l][eligible & ~np.isnan(D[l])])
        out[l] = v[len(v) // 2] if len(v) else 0.0
    return out


# ---- tests: exports ----
def test_library_exports_new_symbols():
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in N.EXPORTS
    assert lib.mosaic_abi_version() == 4


def test_null_context_is_refused_without_a_device():
    lib = N.lib()
    out = ctypes.c_int(0)
    assert lib.mosaic_resolution(N.GRID_H3, 16, ctypes.byref(out)) == N.MOSAIC_E_RES
    before = lib.mosaic_last_error()
    h = ctypes.c_void_p()
    assert lib.mosaic_within_neighbours(None, None, None, None, None, 0, 1, ctypes.byref(h)) == N.MOSAIC_E_ARG and not h
    msg = lib.mosaic_last_error()
    assert msg and msg != before and b"within_neighbours: null context" in msg
    assert lib.mosaic_within_candidates(None, None, None, None, None, 0, None) == N.MOSAIC_E_ARG
    assert b"within_candidates: null context" in lib.mosaic_last_error()


# ---- (H) against (B) ----
@pytest.mark.parametrize("names", (("pickups", "zones"), ("zones", "pickups"), ("london", "london"), ("trips", "zones"),
                                   ("pickups", "trips")))
def test_host_against_restatement(names):
    left, right = side(names[0]), side(names[1])
    D = all_pairs(*names)
    med = row_medians(D, right.eligible)
    want = check(left, right, D, med)
    per = {}
    for l, _, _ in want:
        per[l] = per.get(l, 0) + 1
    assert any(0 < v < right.n for v in per.values())  # some, not all
    assert len(check(left, right, D, INF)) == left.n * right.n
    check(left, right, D, 0.0)
    rows = list(range(1, left.n, 3))
    check(left, right, D, med[rows], rows=rows)
    check(left, right, D, float(np.median(med)), rows=rows, keep_self=False)


def test_host_zones_against_zones_self_matches():
    z = side("zones")
    D = all_pairs("zones", "zones")
    med = row_medians(D, z.eligible)
    kept = check(z, z, D, med)
    want = check(z, z, D, med, keep_self=False)
    assert {(l, c) for l, c, _ in kept} - {(l, c) for l, c, _ in want} == {(g, g) for g in range(z.n)}
    # radius 0: the zones that touch or overlap, ties ordered by the candidate row
    zero = check(z, z, D, 0.0, keep_self=False)
    assert zero and all(b == 0 for _, _, b in zero) and [(l, c) for l, c, _ in zero] == sorted((l, c) for l, c, _ in zero)
    assert len({l for l, _, _ in zero}) < len(zero)  # some landmark has two


# ---- rows that never pair ----
def non_ok_case():
    """(WKB rows, models): a point, a null row, a LineString (a row-path row in a column without the lines
    flag), an empty polygon (ROW_OK without a facet), a second point"""
    from mosaic_amd.context import _wkt_row_wkb

    line_a = struct.pack("<BII", 1, 2, 2) + struct.pack("<4d", 0, 0, 1, 1)
    rows = [geom_wkb(pt(0, 0)), None, line_a, _wkt_row_wkb("POLYGON EMPTY"), geom_wkb(pt(3, 4))]
    models = [pt(0, 0), None, None, ("polygon", []), pt(3, 4)]
    return rows, models


def test_host_null_row_path_and_empty_rows_never_pair():
    rows, models = non_ok_case()
    col = HostCol.from_wkb(rows)
    st, facets = col.status()
    assert st.tolist() == [N.ROW_OK, N.ROW_NULL, N.ROW_PATH, N.ROW_OK, N.ROW_OK] and facets.tolist() == [1, 0, 0, 0, 1]
    s = WSide(col, models)
    assert s.eligible.tolist() == [True, False, False, False, True]
    n = s.n
    D = TL.host_distance(col, col, np.repeat(np.arange(n), n), np.tile(np.arange(n), n)).reshape(n, n)
    assert D[0, 3] == 0.0 and D[3, 4] == 0.0  # the artefact that must not leak
    five = int(bits([5.0])[0])
    for radius in (INF, FLOAT_MAX, 5.0):
        assert check(s, s, D, radius) == [(0, 0, 0), (0, 4, five), (4, 4, 0), (4, 0, five)]
        assert check(s, s, D, radius, keep_self=False) == [(0, 4, five), (4, 0, five)]
    assert check(s, s, D, 0.0) == [(0, 0, 0), (4, 4, 0)]
    assert host_candidates(col, col, INF).tolist() == [2, 0, 0, 0, 2]
    # the empty box alone would pass the bound at radius +inf: the eligibility rule keeps it out
    b = boxes(col)
    assert b[3].tolist() == [INF, INF, -INF, -INF] and np_box_lower_bound(b[0], b[3]) <= INF


# ---- radii ----
def test_radius_kinds():
    left, right = side("pickups"), side("zones")
    D = all_pairs("pickups", "zones")
    l0 = 5
    order = np.argsort(D[l0], kind="stable")
    c_tie = int(order[len(order) // 2])
    tie = float(D[l0, c_tie])
    assert tie > 0
    kept = check(left, right, D, tie, rows=[l0])
    assert (l0, c_tie, int(bits([tie])[0])) == kept[-1]  # the radius is the exact bits of a pair's distance: kept
    below = check(left, right, D, math.nextafter(tie, 0.0), rows=[l0])
    assert below == kept[:-1]  # one ulp less: dropped
    assert len(check(left, right, D, FLOAT_MAX)) == left.n * right.n
    assert len(check(left, right, D, INF)) == left.n * right.n
    assert check(left, right, D, NAN) == [] and check(left, right, D, -1.0) == [] and check(left, right, D, -INF) == []
    assert host_candidates(left.col, right.col, NAN).tolist() == [0] * left.n
    assert check(left, right, D, -0.0) == check(left, right, D, 0.0)
    # per-row arrays of every kind, and subsets of the rows
    kinds = np.array([0.0, tie, NAN, -1.0, INF, FLOAT_MAX, math.nextafter(tie, 0.0), 1e-3])
    radius = kinds[np.arange(left.n) % len(kinds)]
    want = check(left, right, D, radius)
    assert {l for l, _, _ in want}.isdisjoint({l for l in range(left.n) if l % len(kinds) in (2, 3)})
    for rows in ([0], [left.n - 1], [3, 4, 9, 40], list(range(0, left.n, 2))):
        check(left, right, D, radius[rows], rows=rows)
    assert check(left, right, D, np.zeros(0), rows=[]) == []


def test_row_errors_write_nothing():
    left, right = side("pickups"), side("zones")
    for rows in ([1, 1], [2, 1], [0, 5, 4], [-1, 0], [0, left.n], [left.n]):
        with pytest.raises(IndexError):
            host_within(left.col, right.col, 1.0, rows=rows)
        with pytest.raises(IndexError):
            host_candidates(left.col, right.col, 1.0, rows=rows)  # asserts that the counts are untouched
    # rows == NULL asks for rows 0 .. n - 1: more than the column holds is an error
    radius = np.ones(left.n + 1)
    assert not wn_lib().wn_within(left.col.handle, right.col.handle, None, N.ptr(radius), left.n + 1, 1)
    counts = np.full(left.n + 1, -7, np.int64)
    assert wn_lib().wn_candidates(left.col.handle, right.col.handle, None, N.ptr(radius), left.n + 1, N.ptr(counts)) == 1
    assert (counts == -7).all()


# ---- the filter can drop no pair ----
def assert_bound_below_distance(left, right, D):
    lb = np_box_lower_bound(boxes(left.col)[:, None, :], boxes(right.col)[None, :, :])
    ok = left.eligible[:, None] & right.eligible[None, :]
    assert ok.any()
    bad = np.argwhere(ok & ~(lb <= D))
    assert len(bad) == 0, (bad[:4].tolist(), lb[ok & ~(lb <= D)][:4], D[ok & ~(lb <= D)][:4])


@pytest.mark.parametrize("names", (("pickups", "zones"), ("zones", "zones"), ("london", "london"), ("trips", "zones"),
                                   ("pickups", "trips")))
def test_filter_safety_on_the_fixtures(names):
    assert_bound_below_distance(side(names[0]), side(names[1]), all_pairs(*names))


def test_filter_safety_on_strained_shapes():
    """shapes built to strain the bound: a point 1e-12 beside a segment one degree long, far from both ends;
    an axis-parallel segment lying on the other box's side; the same near (-74, 40.7) and near (5e5, 2e5)"""
    for ox, oy, unit in ((-74.0, 40.7, 1.0), (5e5, 2e5, 1e4), (0.0, 0.0, 1.0)):
        geoms = [
            TL.line([(ox, oy), (ox + unit, oy + unit)]),                       # a diagonal one unit long
            pt(ox + 0.5 * unit + 1e-12 * unit, oy + 0.5 * unit),               # 1e-12 beside its middle
            pt(ox + 0.25 * unit, oy + 0.25 * unit - 1e-12 * unit),
            TL.line([(ox + unit, oy), (ox + unit, oy + unit)]),                # on the first box's right side
            TL.line([(ox, oy + unit), (ox + unit, oy + unit)]),                # on its top side
            TL.line([(ox + unit, oy + unit), (ox + 2 * unit, oy + unit)]),     # touching its corner
            poly([[(ox, oy), (ox + unit, oy), (ox + unit, oy + unit), (ox, oy + unit), (ox, oy)]]),
            pt(ox + unit + 1e-9 * unit, oy + 0.5 * unit),                      # just outside the square
            pt(ox + 0.5 * unit, oy + 0.5 * unit),                              # inside it: distance 0
            TL.line([(ox + 1.5 * unit, oy - unit), (ox + 1.5 * unit, oy + 3 * unit)]),
            pt(ox + 3 * unit, oy + 4 * unit),
        ]
        col = TL.LCol.from_geoms(geoms)
        s = WSide(col, geoms)
        assert s.eligible.all()
        n = s.n
        D = TL.host_distance(col, col, np.repeat(np.arange(n), n), np.tile(np.arange(n), n)).reshape(n, n)
        assert 0 < D[0, 1] < 1e-11 * unit and D[6, 8] == 0.0 and D[0, 3] == 0.0
        assert_bound_below_distance(s, s, D)
        # and the join at radii that sit on those distances
        for radius in (0.0, float(D[0, 1]), math.nextafter(float(D[0, 1]), 0.0), float(D[6, 7]), unit):
            check(s, s, D, radius)
            check(s, s, D, radius, keep_self=False)


# ---- SpatialKNN.transform_exact: the numpy steps against literal Python ----
def literal_exact_radius(M, n, k, threshold):
    radius, from_ring = [], []
    for l in range(n):
        near = {}
        for ll, c, d, _ in M:
            if ll == l and d <= threshold:  # False for NaN
                near[c] = d
        ds = sorted(near.values())
        from_ring.append(len(ds) >= k)
        radius.append(ds[k - 1] if len(ds) >= k else threshold)
    return radius, from_ring


def literal_exact(left, right, D, M, actives, k, threshold):
    """transform_exact's rows [(l, c, distance bits, iteration, neighbour_number)] from (B)"""
    radius, _ = literal_exact_radius(M, left.n, k, threshold)
    rows = restate(left, right, D, radius, keep_self=False)
    first = {}
    for l, c, _, it in M:
        first[(l, c)] = min(it, first.get((l, c), it))
    last_active = {l: max(i + 1 for i, a in enumerate(actives) if l in a) for l in range(left.n)}
    out, number = [], {}
    for l, c, b in rows:
        number[l] = number.get(l, 0) + 1
        if number[l] <= k:
            out.append((l, c, b, first.get((l, c), last_active[l] + 1), number[l]))
    return out


def brute_knn(left, right, D, k, threshold):
    """every landmark's first k of all eligible candidates that are no self match and lie within the threshold,
    by (distance bits, candidate row): [(l, c, distance bits, neighbour_number)]"""
    tb = int(bits([threshold])[0])
    out = []
    for l in range(left.n):
        if not left.eligible[l]:
            continue
        mine = sorted((int(bits([D[l, c]])[0]), c) for c in range(right.n)
                      if right.eligible[c] and left.flat[l] != right.flat[c])
        out += [(l, c, b, i + 1) for i, (b, c) in enumerate(mine[:k]) if b <= tb]
    return out


def exact_columns_as_rows(m):
    return list(zip(m["landmark_row"].tolist(), m["candidate_row"].tolist(), bits(m["distance"]).tolist(),
                    m["iteration"].tolist(), m["neighbour_number"].tolist()))


def host_exact(left_side, right_side, params, pair_budget):
    """transform_exact's dataflow driven from the host primitives: (H) for the rings and for the join"""
    def step(active, it):
        rows, cells = left_side.ring_rows(it, active.tolist())
        got, un = host_neighbours(right_side.host_index(), left_side.col, right_side.col, rows, cells)
        unmatched = np.zeros(left_side.n, bool)
        unmatched[sorted(un)] = True
        l, c, b = (np.array([r[i] for r in got], np.int64) for i in range(3))
        return l, c, b.view(np.float64), unmatched

    k, thr = params["k_neighbours"], params["distance_threshold"]
    matches, actives = K.knn_iterate(left_side.n, step, k, params["max_iterations"], params["early_stop_iterations"], thr)
    radius, from_ring = K.knn_exact_radius(matches, left_side.n, k, thr)
    counts = host_candidates(left_side.col, right_side.col, radius)
    batches = K.knn_exact_batches(counts, pair_budget)
    parts = [host_within(left_side.col, right_side.col, radius[a:b], rows=np.arange(a, b), keep_self=False) for a, b in batches]
    rows = [r for p in parts for r in p]
    within = (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64),
              np.array([r[2] for r in rows], np.int64).view(np.float64))
    return K.knn_exact_result(within, matches, actives, left_side.n, k), (radius, from_ring, counts, batches, matches, actives)


# The telling case: pickups against the 35 zones at res 8, k = 3, one iteration.  literal_knn's approximate
# result differs from the brute force in both ways (assert_exact_case_is_telling).
EXACT_PARAMS = dict(k_neighbours=3, index_resolution=8, max_iterations=1, early_stop_iterations=1, distance_threshold=FLOAT_MAX)


@functools.lru_cache(maxsize=None)
def exact_case(name, threshold=FLOAT_MAX):
    """(left Side, right Side, their WSides, D, literal_knn's approximate result, the parameters)"""
    p = dict(EXACT_PARAMS, distance_threshold=threshold)
    if name == "pickups-zones":
        left, right, names = pickups64(), zones8(), ("pickups", "zones")
    elif name == "zones-zones":
        left, right, names = zones8(), zones8(), ("zones", "zones")
        p["max_iterations"] = 2
    elif name == "few-points":  # two point candidates, fewer than k
        x, y = pickups()
        left, right, names = pickups64(), Side("H3", (x[80:82].copy(), y[80:82].copy()), 8), None
    else:
        raise KeyError(name)
    wl, wr = WSide(left.col, left.models), WSide(right.col, right.models)
    if names:
        D = all_pairs(*names)
    else:
        D = TL.host_distance(wl.col, wr.col, np.repeat(np.arange(wl.n), wr.n), np.tile(np.arange(wr.n), wl.n)).reshape(wl.n, wr.n)
    lit = literal_knn(left.n, literal_step(left, right), p["k_neighbours"], p["max_iterations"], p["early_stop_iterations"],
                      p["distance_threshold"])
    return left, right, wl, wr, D, lit, p


def assert_exact_case_is_telling(lit, brute, k):
    """the approximate result misses the brute force in both ways"""
    approx, want = {}, {}
    for l, c, _, _, _ in lit[0]:
        approx.setdefault(l, []).append(c)
    for l, c, _, _ in brute:
        want.setdefault(l, []).append(c)
    assert all(len(v) == k for v in want.values())
    assert any(len(approx.get(l, [])) < k for l in want), "no landmark has fewer than k rows"
    assert any(len(approx.get(l, [])) == k and not set(approx[l]) <= set(want[l]) for l in want), \
        "no landmark has k rows with a wrong candidate"


def test_knn_exact_radius_batches_and_result_against_literal():
    left, right, wl, wr, D, lit, p = exact_case("pickups-zones")
    k = p["k_neighbours"]
    final, actives, M = lit
    m = (np.array([r[0] for r in M], np.int64), np.array([r[1] for r in M], np.int64),
         np.array([r[2] for r in M], np.float64), np.array([r[3] for r in M], np.int32))
    for thr in (FLOAT_MAX, float(np.median(m[2]))):
        radius, from_ring = K.knn_exact_radius(m, left.n, k, thr)
        want_r, want_f = literal_exact_radius(M, left.n, k, thr)
        assert bits(radius).tolist() == bits(want_r).tolist() and from_ring.tolist() == want_f
        assert any(want_f) and not all(want_f)
        rows = restate(wl, wr, D, want_r, keep_self=False)
        within = (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64),
                  np.array([r[2] for r in rows], np.int64).view(np.float64))
        got = K.knn_exact_result(within, m, [np.array(a, np.int64) for a in actives], left.n, k)
        assert exact_columns_as_rows(got) == literal_exact(wl, wr, D, M, actives, k, thr)
    # a NaN distance and a pair matched twice count for nothing and once
    mm = (np.array([0, 0, 0, 0, 1]), np.array([7, 7, 8, 9, 7]), np.array([2.0, 2.0, NAN, 1.0, 3.0]), np.array([1, 2, 1, 2, 1]))
    radius, from_ring = K.knn_exact_radius(mm, 3, 2, 10.0)
    assert radius.tolist() == [2.0, 10.0, 10.0] and from_ring.tolist() == [True, False, False]
    assert K.knn_exact_radius(mm, 3, 2, 1.5)[0].tolist() == [1.5, 1.5, 1.5]
    # batches: consecutive rows while the sum stays within the budget; a row over it is alone
    assert K.knn_exact_batches([3, 3, 3, 10, 1, 1, 0, 5], 6) == [(0, 2), (2, 3), (3, 4), (4, 7), (7, 8)]
    assert K.knn_exact_batches([], 6) == [] and K.knn_exact_batches([0, 0], 0) == [(0, 2)]
    assert K.knn_exact_batches([7], 6) == [(0, 1)] and K.knn_exact_batches([6, 1], 6) == [(0, 1), (1, 2)]


@pytest.mark.parametrize("name, threshold, budget", (("pickups-zones", FLOAT_MAX, 1 << 24), ("pickups-zones", FLOAT_MAX, 20),
                                                      ("pickups-zones", 0.004, 1 << 24), ("zones-zones", FLOAT_MAX, 20),
                                                      ("few-points", FLOAT_MAX, 1 << 24)))
def test_transform_exact_dataflow_equals_the_brute_force(name, threshold, budget):
    left, right, wl, wr, D, lit, p = exact_case(name, threshold)
    k = p["k_neighbours"]
    brute = brute_knn(wl, wr, D, k, threshold)
    if name == "pickups-zones" and threshold == FLOAT_MAX:
        assert_exact_case_is_telling(lit, brute, k)
    got, (radius, from_ring, counts, batches, matches, actives) = host_exact(left, right, p, budget)
    rows = exact_columns_as_rows(got)
    assert [(l, c, b, number) for l, c, b, _, number in rows] == brute
    assert rows == literal_exact(wl, wr, D, lit[2], lit[1], k, threshold)
    assert [a.tolist() for a in actives] == lit[1]
    assert len({(l, c) for l, c, _, _, _ in rows}) == len(rows)  # each (landmark, candidate) once
    if threshold != FLOAT_MAX:
        full = brute_knn(wl, wr, D, k, FLOAT_MAX)
        assert 0 < len(brute) < len(full) and not from_ring.all()
    if name == "few-points":
        assert len(brute) == 2 * left.n and not from_ring.any()  # every landmark gets both candidates
    if budget < 1 << 24:
        assert len(batches) >= 3 and any(b - a == 1 and counts[a] > budget for a, b in batches)
        assert batches[0][0] == 0 and batches[-1][1] == left.n and all(x[1] == y[0] for x, y in zip(batches, batches[1:]))
    # the new iteration value: a pair the rings never matched carries its landmark's last active iteration + 1
    matched = {(l, c) for l, c, _, _ in lit[2]}
    fresh = [r for r in rows if (r[0], r[1]) not in matched]
    if name == "pickups-zones" and threshold == FLOAT_MAX:
        assert fresh and all(it == 2 for _, _, _, it, _ in fresh)
