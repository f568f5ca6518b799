"""GridRingNeighbours (models/knn/GridRingNeighbours.scala:121-160) and the approximate SpatialKNN
(models/knn/SpatialKNN.scala, models/core/IterativeTransformer.scala), CPU side: the header's sequential
driver rn::neighbours (mosaic_amd/csrc/ring_neighbours.h, compiled by g++ as
tests/native/ring_neighbours_host.cpp -- source (H) below) and the numpy bookkeeping of
mosaic_amd/knn.py.  The kernels are checked against (H) and (B) in tests/test_gpu_ring_neighbours.py.

Expected values never come from the code under test:
  (B) an independent Python restatement of one iteration: a dict from cell to candidate set built
      from the host producer's chips (tessellate(..., ctx=None), or the oracle's cell of each point),
      Python sets for the pairs and for `unmatched`, a self match decided on the tests' own geometry
      models (equal parts, rings and vertex bytes), tests/test_st_distance.py's host_distance for the
      values and `sorted` for the order.  The landmarks' ring cells are tests/test_geometry_kring.py's
      brute force over the oracle's k-rings.
  literal_knn: SpatialKNN's dataflow in plain Python lists, dicts and sets, fed from (B).
All comparisons are exact: equal row lists, identical distance bits."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from mosaic_amd import _native as N
from mosaic_amd import knn as K
from mosaic_amd.data import PolygonSet

from tests.test_geometry_kring import brute, chips_of
from tests.test_st_distance import HostCol, bits, host_distance, nyc35, pickups, polyset_geom, pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mosaic_cell_index_create", "mosaic_cell_index_info", "mosaic_cell_index_destroy", "mosaic_ring_neighbours",
               "mosaic_neighbours_info", "mosaic_neighbours_export", "mosaic_neighbours_destroy",
               "mosaic_ring_neighbours_last_ms")
FLOAT_MAX = float(np.finfo(np.float64).max)  # Double.MaxValue, the reference's default distanceThreshold


# ---- (H) the host library ----
@functools.lru_cache(maxsize=None)
def rn_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="rn_host_"), "librn.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "ring_neighbours_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    for name, args, res in (("rn_index_create", [vp, vp, i64], vp), ("rn_index_info", [vp, vp], None),
                            ("rn_index_free", [vp], None), ("rn_neighbours", [vp, vp, vp, vp, vp, i64, ctypes.c_int], vp),
                            ("rn_result_info", [vp, vp], None), ("rn_result_export", [vp, vp, vp, vp, vp], None),
                            ("rn_result_free", [vp], None), ("rn_same_geometry", [vp, i64, vp, i64], ctypes.c_int)):
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    return lib


class HostIndex:
    """the header's cell index over chips (cells, candidate rows)"""

    def __init__(self, cells, keys):
        cells, keys = np.ascontiguousarray(cells, np.int64), np.ascontiguousarray(keys, np.int32)
        self.handle = rn_lib().rn_index_create(N.ptr(cells), N.ptr(keys), len(cells))
        if not self.handle:
            raise ValueError("negative key")
        info = np.zeros(3, np.int64)
        rn_lib().rn_index_info(self.handle, N.ptr(info))
        self.n_cells, self.n_entries, self.max_per_cell = (int(v) for v in info)

    def __del__(self):
        try:
            if self.handle:
                rn_lib().rn_index_free(self.handle)
        except Exception:
            pass


def host_neighbours(index, left, right, rows, cells, keep_self=False):
    """(H): ([(landmark, candidate, distance bits)] in the result's order, set of unmatched landmarks)"""
    rows, cells = np.ascontiguousarray(rows, np.int64), np.ascontiguousarray(cells, np.int64)
    assert len(rows) == len(cells)
    h = rn_lib().rn_neighbours(index.handle, left.handle, right.handle, N.ptr(rows), N.ptr(cells), len(rows), int(keep_self))
    if not h:
        raise IndexError("row index out of range")
    try:
        info = np.zeros(2, np.int64)
        rn_lib().rn_result_info(h, N.ptr(info))
        n, n_left = int(info[0]), int(info[1])
        assert n_left == left.n
        l, c, d = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.float64)
        un = np.zeros(max(n_left, 1), np.uint8)
        rn_lib().rn_result_export(h, N.ptr(l), N.ptr(c), N.ptr(d), N.ptr(un))
    finally:
        rn_lib().rn_result_free(h)
    return as_rows(l[:n], c[:n], d[:n]), set(np.flatnonzero(un[:n_left]).tolist())


def as_rows(l, c, d):
    return list(zip(np.asarray(l).tolist(), np.asarray(c).tolist(), bits(d).tolist()))


# ---- the sides of a join: geometry models, a host column, chips from the host producer ----
def flat(g):
    """the geometry's flat content: part kinds, rings, vertex bytes"""
    kind, parts = g
    if kind == "point":
        return tuple(("point", np.asarray(p, np.float64).tobytes()) for p in parts)
    return tuple(("polygon", tuple(np.asarray(r, np.float64).tobytes() for r in part)) for part in parts)


class Side:
    """``geoms``: a PolygonSet or (x, y) point arrays"""

    def __init__(self, grid, geoms, res, col=None):
        self.grid, self.res, self.geoms = grid, res, geoms
        if hasattr(geoms, "geom_parts"):
            self.models = [polyset_geom(geoms, g) for g in range(len(geoms))]
            self.col = col or HostCol.from_polyset(geoms)
            self.chips = chips_of(grid, geoms, res)
        else:
            x, y = (np.ascontiguousarray(v, np.float64) for v in geoms)
            self.models = [pt(a, b) for a, b in zip(x, y)]
            self.col = col or HostCol.from_points(x, y)
            if grid == "H3":
                cells = np.asarray(oracle.h3_point_to_index(x, y, res), np.int64)
            else:
                cells = np.array([int(oracle.bng_point_to_index(a, b, res)) for a, b in zip(x, y)], np.int64)
            self.chips = (np.zeros(len(x), np.uint8), cells, np.arange(len(x), dtype=np.int32), len(x))
        self.n = len(self.models)
        self.flat = [flat(g) for g in self.models]

    @functools.lru_cache(maxsize=None)
    def rings(self, it):
        """per landmark, the sorted cells of iteration `it`: the 1-ring, or the `it`-loop"""
        want = brute(self.grid, *self.chips, it)
        return [sorted(w[0] if it == 1 else w[2]) for w in want]

    def ring_rows(self, it, active=None):
        rings = self.rings(it)
        active = range(self.n) if active is None else active
        rows = [l for l in active for _ in rings[l]]
        cells = [c for l in active for c in rings[l]]
        return np.array(rows, np.int64), np.array(cells, np.int64)

    @functools.lru_cache(maxsize=None)
    def host_index(self):
        return HostIndex(self.chips[1], self.chips[2])

    @functools.lru_cache(maxsize=None)
    def by_cell(self):
        d = {}
        for cell, key in zip(self.chips[1].tolist(), self.chips[2].tolist()):
            d.setdefault(cell, set()).add(key)
        return d


def restate(left, right, rows, cells, keep_self=False):
    """(B): ([(landmark, candidate, distance bits)] ordered, set of unmatched landmarks)"""
    by_cell = right.by_cell()
    pairs, unmatched = set(), set()
    for l, cell in zip(np.asarray(rows).tolist(), np.asarray(cells).tolist()):
        if cell in by_cell:
            pairs |= {(l, c) for c in by_cell[cell]}
        else:
            unmatched.add(l)
    if not keep_self:
        pairs = {(l, c) for l, c in pairs if left.flat[l] != right.flat[c]}
    pl = sorted(pairs)
    d = host_distance(left.col, right.col, [p[0] for p in pl], [p[1] for p in pl]) if pl else np.zeros(0)
    return sorted((l, int(b), c) for (l, c), b in zip(pl, bits(d).tolist())), unmatched


def reorder(rows):
    """(l, bits, c) -> (l, c, bits), the layout of as_rows"""
    return [(l, c, b) for l, b, c in rows]


def check_iteration(left, right, it, keep_self=False, duplicates=False):
    rows, cells = left.ring_rows(it)
    if duplicates:
        rows, cells = np.concatenate([rows, rows[::3]]), np.concatenate([cells, cells[::3]])
    want, want_un = restate(left, right, rows, cells, keep_self)
    got, got_un = host_neighbours(right.host_index(), left.col, right.col, rows, cells, keep_self)
    assert got == reorder(want), (it, keep_self)
    assert got_un == want_un, (it, keep_self)
    return want, want_un


# ---- fixtures, computed once and never modified ----
@functools.lru_cache(maxsize=None)
def zones8():
    return Side("H3", nyc35(), 8)


@functools.lru_cache(maxsize=None)
def pickups64():
    x, y = pickups()
    return Side("H3", (x[:64].copy(), y[:64].copy()), 8)


@functools.lru_cache(maxsize=None)
def london4():
    return Side("BNG", PolygonSet.load("london_postcodes_bng").subset(range(6)), 4)


# ---- literal_knn: SpatialKNN.scala:136-164, 202-235 and IterativeTransformer.scala:49-84 in plain Python ----
def literal_knn(n, step, k, max_iterations, early_stop, threshold):
    """``step(active, it)`` -> ([(l, c, distance as float)], set of unmatched landmarks).  Returns the
    final rows [(l, c, distance bits, iteration, neighbour_number)], the active set of every iteration
    run, and the match list M."""
    M, null, active, actives = [], set(), list(range(n)), []
    count, prev_cond, prev_distinct = 0, False, 0
    for it in range(1, max_iterations + 1):
        actives.append(list(active))
        rows, unmatched = step(active, it)
        M += [(l, c, d, it) for l, c, d in rows]
        null |= set(unmatched)
        within = {}
        for l, c, d, _ in M:
            if d <= threshold:
                within[l] = within.get(l, 0) + 1
        # (a match within the threshold or a null row) and match_count - 1 < k, the null row counted in
        nxt = [l for l in range(n) if (within.get(l, 0) > 0 or l in null) and within.get(l, 0) <= k]
        distinct = len({(l, c) for l, c, _, _ in M})
        cond = len(active) == len(nxt) and distinct == prev_distinct and distinct > 0
        prev_distinct = distinct
        count = 0 if cond != prev_cond else count + 1
        prev_cond = cond
        active = nxt
        if cond and count == early_stop:
            break
        if not active:  # M can no longer change
            break
    final = []
    for l in range(n):
        mine = sorted((d, c, it) for ll, c, d, it in M if ll == l)
        for number, (d, c, it) in enumerate(mine, 1):
            if number <= k and d <= threshold:
                final.append((l, c, int(bits([d])[0]), it, number))
    return final, actives, M


def literal_step(left, right):
    def step(active, it):
        rows, cells = left.ring_rows(it, active)
        want, un = restate(left, right, rows, cells)
        return [(l, c, float(np.array([b], np.int64).view(np.float64)[0])) for l, b, c in want], un
    return step


def knn_columns_as_rows(m):
    return list(zip(m["landmark_row"].tolist(), m["candidate_row"].tolist(), bits(m["distance"]).tolist(),
                    m["iteration"].tolist(), m["neighbour_number"].tolist()))


# The end-to-end cases.  With 12 zones as candidates (res 8, k = 3, 4 iterations, early stop 1) every
# landmark is still active after iteration 1 (literal_knn's active sets: 64, 64, 58, 37 pickups; 12, 12,
# 12, 8 zones), so the candidates are all 35 zones: 64, 11, 6, 3 pickups and 35, 20, 14, 7 zones stay
# active, and literal_knn's own result shows a landmark leaving the active set after iteration 1, one
# still active at the last iteration and a pair matched in two iterations (assert_knn_case_is_telling).
KNN_PARAMS = dict(k_neighbours=3, index_resolution=8, max_iterations=4, early_stop_iterations=1, distance_threshold=FLOAT_MAX)


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """(left Side, right Side, literal_knn's result)"""
    left, right = {"pickups-zones": (pickups64(), zones8()), "zones-zones": (zones8(), zones8())}[name]
    p = KNN_PARAMS
    lit = literal_knn(left.n, literal_step(left, right), p["k_neighbours"], p["max_iterations"], p["early_stop_iterations"],
                      p["distance_threshold"])
    return left, right, lit


def assert_knn_case_is_telling(lit):
    final, actives, M = lit
    assert len(actives) >= 2 and set(actives[0]) - set(actives[1]), "no landmark leaves the active set after iteration 1"
    assert len(actives) == KNN_PARAMS["max_iterations"] and actives[-1], "no landmark is active at the last iteration"
    seen = {}
    for l, c, _, it in M:
        seen.setdefault((l, c), set()).add(it)
    assert any(len(v) >= 2 for v in seen.values()), "no pair is matched in two iterations"
    assert final


# ---- tests ----
def test_library_exports_new_symbols():
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in N.EXPORTS


def test_abi_version_unchanged():
    assert N.lib().mosaic_abi_version() == 4


def test_host_index():
    ix = HostIndex([7, 5, 7, 7, 9, 5], [2, 0, 2, 1, 4, 0])
    assert (ix.n_cells, ix.n_entries, ix.max_per_cell) == (3, 4, 2)
    with pytest.raises(ValueError):
        HostIndex([1, 2], [0, -1])
    z = zones8()
    ix = z.host_index()
    by_cell = z.by_cell()
    assert (ix.n_cells, ix.n_entries, ix.max_per_cell) == (len(by_cell), sum(len(v) for v in by_cell.values()),
                                                          max(len(v) for v in by_cell.values()))
    assert ix.max_per_cell >= 2  # a border cell shared by neighbouring zones


@pytest.mark.parametrize("it", (1, 2, 3))
def test_host_pickups_against_zones(it):
    want, un = check_iteration(pickups64(), zones8(), it)
    if it == 1:
        assert want and un and len(un) < 64  # matches, null rows and landmarks without one


@pytest.mark.parametrize("it", (1, 2))
def test_host_zones_against_pickups(it):
    want, un = check_iteration(zones8(), pickups64(), it, duplicates=True)
    assert want and un


@pytest.mark.parametrize("it", (1, 2, 3))
def test_host_zones_against_zones_drops_self_matches(it):
    z = zones8()
    want, _ = check_iteration(z, z, it)
    assert all(l != c for l, _, c in want)
    kept, _ = check_iteration(z, z, it, keep_self=True)
    if it == 1:
        assert {(l, c) for l, _, c in kept} - {(l, c) for l, _, c in want} == {(g, g) for g in range(z.n)}
        # neighbouring zones touch: distance 0.0 ties, ordered by the candidate row
        zero = [(l, c) for l, b, c in want if b == 0]
        assert zero == sorted(zero) and len({l for l, _ in zero}) < len(zero)  # some landmark has two
    else:
        assert len(kept) == len(want)  # a k-loop holds no cell of the zone's own chips: no self match to drop


def test_host_london_bng():
    z = london4()
    for it in (1, 2):
        want, _ = check_iteration(z, z, it)
        assert want
        check_iteration(z, z, it, keep_self=True)


def test_same_geometry_is_exact():
    from tests.test_st_distance import geom_wkb, poly

    sq = [(0, 0), (10, 0), (10, 10), (0, 10), (0, 0)]
    rot = sq[1:] + [sq[1]]
    geoms = [poly([sq]), poly([sq]), poly([rot]), poly([sq], [[(20, 20), (30, 20), (30, 30), (20, 20)]]), pt(1, 2), pt(1, 2),
             pt(1, -2), pt(1, 2, 3, 4), poly([[(0, 0), (10, 0), (10, 10), (0, 10.000000000000002), (0, 0)]])]
    big = HostCol.from_wkb([geom_wkb(g, True) for g in geoms])
    little = HostCol.from_wkb([geom_wkb(g, False) for g in geoms])
    for a in range(len(geoms)):
        for b in range(len(geoms)):
            want = int(flat(geoms[a]) == flat(geoms[b]))
            assert rn_lib().rn_same_geometry(big.handle, a, big.handle, b) == want, (a, b)
            assert rn_lib().rn_same_geometry(big.handle, a, little.handle, b) == want, (a, b)  # the other byte order
    assert flat(geoms[0]) == flat(geoms[1]) != flat(geoms[2])  # the rotated ring is another geometry


NAN_BITS = 0x7ff8000000000000


def non_ok_case():
    """(landmark WKB rows, candidate WKB rows, expected [(l, c, distance bits)]): a point, a null row and two
    different LineStrings (row-path rows) on both sides, plus a second point among the candidates, all
    candidates in cell 7.  Null and row-path rows are stored as empty geometries, alike; only the two
    equal points are a self match.  Every pair with a side that is not MOSAIC_ROW_OK stays, with
    distance NaN, after the numbers and by candidate row."""
    import struct

    from tests.test_st_distance import geom_wkb

    line_a = struct.pack("<BII", 1, 2, 2) + struct.pack("<4d", 0, 0, 1, 1)
    line_b = struct.pack("<BII", 1, 2, 2) + struct.pack("<4d", 5, 5, 9, 9)
    left = [geom_wkb(pt(0, 0)), None, line_a, line_b]
    right = [geom_wkb(pt(0, 0)), None, line_a, line_b, geom_wkb(pt(3, 4))]
    five = int(bits([5.0])[0])
    want = [(0, 4, five), (0, 1, NAN_BITS), (0, 2, NAN_BITS), (0, 3, NAN_BITS)]
    want += [(l, c, NAN_BITS) for l in (1, 2, 3) for c in range(5)]
    return left, right, want


def test_host_null_and_row_path_rows_are_no_self_matches():
    left, right, want = non_ok_case()
    hl, hr = HostCol.from_wkb(left), HostCol.from_wkb(right)
    assert hl.status()[0].tolist() == [N.ROW_OK, N.ROW_NULL, N.ROW_PATH, N.ROW_PATH]
    index = HostIndex(np.full(len(right), 7, np.int64), np.arange(len(right)))
    rows, cells = np.arange(len(left)), np.full(len(left), 7, np.int64)
    assert host_neighbours(index, hl, hr, rows, cells) == (want, set())
    kept, _ = host_neighbours(index, hl, hr, rows, cells, keep_self=True)
    assert kept == [(0, 0, 0)] + want


def test_host_errors_write_nothing():
    p, z = pickups64(), zones8()
    rows, cells = p.ring_rows(1)
    for bad in (-1, p.n):
        r = rows.copy()
        r[5] = bad
        with pytest.raises(IndexError):
            host_neighbours(z.host_index(), p.col, z.col, r, cells)
    # an index naming a row outside the candidate column
    with pytest.raises(IndexError):
        host_neighbours(HostIndex(z.chips[1], z.chips[2] + 1), p.col, z.col, rows, cells)
    # no rows: no pairs, nothing unmatched
    assert host_neighbours(z.host_index(), p.col, z.col, [], []) == ([], set())


@pytest.mark.parametrize("name", ("pickups-zones", "zones-zones"))
def test_knn_bookkeeping_against_literal(name):
    left, right, lit = knn_case(name)
    assert_knn_case_is_telling(lit)

    def step(active, it):  # the host driver, restricted to the active landmarks
        rows, cells = left.ring_rows(it, active.tolist())
        got, un = host_neighbours(right.host_index(), left.col, right.col, rows, cells)
        unmatched = np.zeros(left.n, bool)
        unmatched[sorted(un)] = True
        l, c, b = (np.array([r[i] for r in got], np.int64) for i in range(3))
        return l, c, b.view(np.float64), unmatched

    p = KNN_PARAMS
    matches, actives = K.knn_iterate(left.n, step, p["k_neighbours"], p["max_iterations"], p["early_stop_iterations"],
                                     p["distance_threshold"])
    assert [a.tolist() for a in actives] == lit[1]
    assert sorted(zip(matches[0].tolist(), matches[1].tolist(), bits(matches[2]).tolist(), matches[3].tolist())) == \
        sorted((l, c, int(bits([d])[0]), it) for l, c, d, it in lit[2])
    assert knn_columns_as_rows(K.knn_result(matches, p["k_neighbours"], p["distance_threshold"])) == lit[0]
    # a distance threshold cuts after the rank: neighbour numbers keep their gaps
    thr = float(np.median(matches[2][matches[2] > 0])) if (matches[2] > 0).any() else 0.0
    cut = K.knn_result(matches, p["k_neighbours"], thr)
    full = K.knn_result(matches, p["k_neighbours"], FLOAT_MAX)
    keep = full["distance"] <= thr
    assert knn_columns_as_rows(cut) == [r for r, k in zip(knn_columns_as_rows(full), keep) if k]


def test_literal_knn_early_stop():
    """three point candidates, k = 5: the matches stop growing and the early-stop counter ends the run
    (IterativeTransformer.scala:66-72: the counter restarts when the condition changes, so with
    earlyStopIterations = 1 the run ends at the second iteration in a row whose condition holds)"""
    x, y = pickups()
    left = Side("H3", (x[:8].copy(), y[:8].copy()), 8)
    right = Side("H3", (x[:3].copy(), y[:3].copy()), 8)
    final, actives, M = literal_knn(left.n, literal_step(left, right), 5, 12, 1, FLOAT_MAX)
    assert 3 <= len(actives) < 12 and actives[-1]  # ended by the counter, not by max_iterations or an empty set
    distinct = [len({(l, c) for l, c, _, it in M if it <= i}) for i in range(1, len(actives) + 1)]
    assert distinct[-1] == distinct[-2] == distinct[-3] > 0


def test_plumbing_errors():
    from mosaic_amd import SpatialKNN

    with pytest.raises(NotImplementedError, match="st_buffer"):
        SpatialKNN(None, nyc35(), index_resolution=8, approximate=False)
    with pytest.raises(TypeError):
        SpatialKNN(None, [b"\x01\x01\x00\x00\x00" + b"\0" * 16], index_resolution=8)
    with pytest.raises(TypeError):
        SpatialKNN(None, "POINT (1 2)", index_resolution=8)
    model = SpatialKNN(None, nyc35(), k_neighbours=2, index_resolution=8, max_iterations=3, early_stop_iterations=1,
                       distance_threshold=1.0)
    assert (model.k_neighbours, model.max_iterations, model.early_stop_iterations, model.distance_threshold,
            model.approximate) == (2, 3, 1, 1.0, True)
    with pytest.raises(TypeError):
        model.transform(["POINT (1 2)"])
    with pytest.raises(RuntimeError):
        model.metrics()
    with pytest.raises(ValueError, match="different lengths"):
        K.grid_ring_neighbours(None, None, None, None, [0, 1], [5])
