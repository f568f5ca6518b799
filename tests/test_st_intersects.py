"""st_intersects (JTS 1.19 Geometry.intersects for Point / MultiPoint / LineString / MultiLineString /
Polygon / MultiPolygon on either side), CPU side: the sequential driver isect::intersects of
mosaic_amd/csrc/st_intersects.h compiled by g++ as tests/native/st_intersects_host.cpp -- source (H) --
plus the Python plumbing that needs no device.  The kernels are checked against (H) in
tests/test_gpu_st_intersects.py.

Expected values never come from the code under test: the truth table and the explicit cases carry
theirs by construction, and every case is also put to (E), the exact oracle of tests/intersects_cases.py
(integers and Fractions; every vertex is located, not only a component's first).
"""
import struct
import types

import numpy as np
import pytest

from mosaic_amd import _native as N
from mosaic_amd import wkb as W

from tests import intersects_cases as C
from tests.intersects_cases import (EXPLICIT, KINDS, exact_intersects, host_intersects, host_pair, kernel_cases, kind_name,
                                    random_pairs, truth_table)
from tests.test_st_distance import SQ, poly, pt
from tests.test_st_distance_lines import LCol, geom_wkb, line
from tests.test_st_distance_lines import host_distance as host_distance_lines

NEW_SYMBOLS = ("mosaic_st_intersects", "mosaic_st_intersects_last_split")


def test_library_exports_new_symbols():
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in N.EXPORTS
    assert lib.mosaic_abi_version() == 4  # adding a symbol breaks no caller


def test_documented_example():
    name, a, b, want = EXPLICIT[0]
    assert name == "docs example" and want is True
    assert host_pair(a, b) is True and host_pair(b, a) is True and exact_intersects(a, b) is True


@pytest.mark.parametrize("case", EXPLICIT, ids=[c[0] for c in EXPLICIT])
def test_explicit(case):
    name, a, b, want = case
    assert exact_intersects(a, b) is want
    assert host_pair(a, b) is want and host_pair(b, a) is want


def test_point_facets_in_segments_intersect():
    """pip::segments_intersect on (v, v) facets, as the header's comment derives it"""
    f = C.host_segments_intersect
    seg = ((0.0, 0.0), (9.0, 6.0))
    for p, want in (((3.0, 2.0), True), ((0.0, 0.0), True), ((9.0, 6.0), True), ((12.0, 8.0), False), ((-3.0, -2.0), False),
                    ((3.0, 2.5), False), ((3.0, np.nextafter(2.0, 3.0)), False)):
        assert f(p, p, *seg) is want and f(*seg, p, p) is want, p
    assert f((3.0, 4.0), (3.0, 4.0), (3.0, 4.0), (3.0, 4.0)) is True
    assert f((3.0, 4.0), (3.0, 4.0), (3.0, 5.0), (3.0, 5.0)) is False
    # a point one ulp off a long sloped segment: the double-double path decides
    big = ((-1048576.0, -699051.0), (1048575.0, 699050.0))
    mid = ((big[0][0] + big[1][0]) / 2, (big[0][1] + big[1][1]) / 2)  # (-0.5, -0.5): exactly on the segment
    assert f(mid, mid, *big) is True
    off = (mid[0], np.nextafter(mid[1], 1.0))
    assert f(off, off, *big) is False and f(*big, off, off) is False


def test_truth_table():
    table = truth_table()
    got = host_intersects(LCol.from_geoms([c[1] for c in table]), LCol.from_geoms([c[2] for c in table]))
    bad = [(c[0], bool(g)) for c, g in zip(table, got) if bool(g) is not c[3]]
    assert not bad, bad
    for name, a, b, want in table:
        assert exact_intersects(a, b) is want, name
    # every ordered pair of kinds sees every situation that exists for it
    seen = {}
    for name, a, b, _ in table:
        seen.setdefault((kind_name(a), kind_name(b)), set()).add(name.split(": ")[1].split(", the big")[0])
    assert set(seen) == {(x, y) for x in KINDS for y in KINDS}
    everything = {"disjoint, disjoint boxes", "disjoint, meeting boxes", "touching at a vertex", "touching along an edge",
                  "crossing", "contained without boundary contact", "inside a hole", "on a hole's ring"}
    for (x, y), names in seen.items():
        bx, by = x.replace("multi", ""), y.replace("multi", "")
        want = {"disjoint, disjoint boxes", "touching at a vertex"}
        if (x, y) != ("point", "point"):
            want.add("disjoint, meeting boxes")
        if (bx, by) != ("point", "point"):
            want.add("touching along an edge")  # for a point: on an edge's interior
        if "point" not in (bx, by):
            want.add("crossing")
        if "polygon" in (bx, by):
            want |= {"contained without boundary contact", "inside a hole", "on a hole's ring"}
        assert names == want, (x, y, names ^ want)
        if bx != "point" and by != "point" and "polygon" in (bx, by):
            assert names == everything


def test_kernel_cases_against_exact():
    cases = kernel_cases()
    got = host_intersects(LCol.from_geoms([c[1] for c in cases]), LCol.from_geoms([c[2] for c in cases]))
    for (name, a, b), g in zip(cases, got):
        assert exact_intersects(a, b) is bool(g), name
        if "false" in name or "hole" in name and "ring" not in name:
            assert not g, name
        elif "only" in name or "cross" in name or "through" in name or "decides" in name:
            assert g, name
    for name, a, b in cases:
        if "last segment" in name or "closing segment" in name or name.startswith("the same"):
            assert C._last_segments_only(a, b), name
    assert got.any() and not got.all()


def test_host_against_exact_random():
    pairs = random_pairs()
    got = host_intersects(LCol.from_geoms([a for a, _ in pairs]), LCol.from_geoms([b for _, b in pairs]))
    bad = [k for k, (a, b) in enumerate(pairs) if exact_intersects(a, b) is not bool(got[k])]
    assert not bad, bad
    kinds = {(kind_name(a), kind_name(b)) for a, b in pairs}
    assert len(kinds) == 36, sorted(kinds)
    assert 80 <= int(got.sum()) <= len(pairs) - 80
    # the near-touching half has both answers too
    near = got[1::2]
    assert 30 <= int(near.sum()) <= len(near) - 30


# Two-vertex lines AB and PQ with P = A + t (B - A) rounded: an endpoint within an ulp of the other
# segment.  Found by a seeded search (numpy default_rng(20251022): A, B uniform in [-100, 100]^2, t in
# [0.05, 0.95], Q = P + uniform(-50, 50)^2, 100,000 trials, trials 24 and 234): 17,160 trials had
# st_distance == 0.0 on disjoint lines and 526 a positive distance on lines that cross.
DISTANCE_ZERO_BUT_DISJOINT = (
    line([(-83.59315655965995, -89.39694649568631), (-34.10269330921281, 67.37745433085385)]),
    line([(-60.45573995677882, -16.102934147601076), (-85.04388539722731, -18.078686360212913)]))
DISTANCE_POSITIVE_BUT_CROSSING = (
    line([(60.97186128663469, 35.199033765037996), (-90.58089597245723, -50.070334528471186)]),
    line([(-34.75446788077005, -18.660254345481952), (-21.174312757871313, 6.461176416839116)]))


def test_st_distance_equal_zero_is_another_function():
    """st_distance(...) == 0.0 decides from rounded quotients; the predicate from exact orientation signs"""
    a, b = DISTANCE_ZERO_BUT_DISJOINT
    assert exact_intersects(a, b) is False and host_pair(a, b) is False and host_pair(b, a) is False
    assert host_distance_lines(LCol.from_geoms([a]), LCol.from_geoms([b])).tolist() == [0.0]
    a, b = DISTANCE_POSITIVE_BUT_CROSSING
    assert exact_intersects(a, b) is True and host_pair(a, b) is True and host_pair(b, a) is True
    d = host_distance_lines(LCol.from_geoms([a]), LCol.from_geoms([b]))[0]
    assert 0.0 < d < 1e-13


def test_host_restatements_agree_on_the_invariant_workloads():
    """the inputs of the GPU file's invariant tests: the aggregates' host twins over the chip joins and
    the flat host driver agree on every one of the 35 x 35 and 60 x 35 pairs, none left out"""
    import oracle
    from mosaic_amd import line_intersects_aggregate_host
    from mosaic_amd.data import LineSet
    from tests import line_join_cases as JC

    zones, moved, left, right, _ = C.invariant_zones()
    keys = ("index_id", "is_core", "polygon_key", "wkb")
    agg = oracle.intersects_aggregate({k: left[k] for k in keys}, {k: right[k] for k in keys})
    li, ri = C.all_pairs(len(zones), len(moved))
    flat = host_intersects(LCol.from_polyset(zones), LCol.from_polyset(moved), li, ri)
    assert {(int(a), int(b)) for a, b in zip(li[flat], ri[flat])} == {k for k, f in agg.items() if f}
    assert 35 < int(flat.sum()) < len(agg) < len(flat)
    # the line fixture against the zones
    geoms, zones, lines, polys, res = JC.invariant_case("H3")
    lk, pk, fl = line_intersects_aggregate_host("H3", lines, polys, res)
    li, ri = C.all_pairs(len(geoms), len(zones))
    flat = host_intersects(LCol.from_lineset(LineSet.from_lines(geoms)), LCol.from_polyset(zones), li, ri)
    assert {(int(a), int(b)) for a, b in zip(li[flat], ri[flat])} == {(int(a), int(b)) for a, b, f in zip(lk, pk, fl) if f}
    assert 20 < int(flat.sum()) < len(lk) < len(flat)


def test_empty_rows_are_served_and_false():
    rows = [line([]), line(), poly([]), ("point", [])]
    other = [pt(1, 1), poly([SQ]), line([(0, 0), (5, 5)]), pt(0, 0)]
    for l, r in ((rows, other), (other, rows)):
        got, st = host_intersects(LCol.from_geoms(l), LCol.from_geoms(r), return_status=True)
        assert st.tolist() == [N.ROW_OK] * 4 and not got.any()
    # st_distance says 0.0 on the same pairs
    assert host_distance_lines(LCol.from_geoms(rows), LCol.from_geoms(other)).tolist() == [0.0] * 4


def test_status_and_errors():
    one_vertex = struct.pack("<BII", 1, 2, 1) + struct.pack("<2d", 3, 3)
    collection = struct.pack("<BI", 1, 7) + struct.pack("<I", 0)
    rows = [geom_wkb(line([(0, 0), (0, 9)])), None, geom_wkb(line([])), collection, W.point_wkb(float("nan"), float("nan")),
            one_vertex, geom_wkb(poly([SQ])), geom_wkb(pt(0, 4))]
    col = LCol.from_wkb(rows)
    other = LCol.from_geoms([pt(0, 4)] * len(rows))
    ok, null, path = N.ROW_OK, N.ROW_NULL, N.ROW_PATH
    got, st = host_intersects(col, other, return_status=True)
    assert st.tolist() == [ok, null, ok, path, path, path, ok, ok]
    assert got.tolist() == [True, False, False, False, False, False, True, True]
    got2, st2 = host_intersects(other, col, return_status=True)
    assert st2.tolist() == st.tolist() and got2.tolist() == got.tolist()
    # a line row in a column built without the lines flag stays a row for the row path
    plain = LCol.from_wkb(rows, flags=0)
    got, st = host_intersects(plain, other, return_status=True)
    assert st.tolist() == [path, null, path, path, path, path, ok, ok]
    assert got.tolist() == [False] * 6 + [True, True]
    # pair lists; an out-of-range row index writes nothing
    li, ri = [6, 0, 7, 6], [0, 1, 2, 7]
    assert host_intersects(col, other, li, ri).tolist() == [True, True, True, True]
    for li, ri in (([0, 8], [0, 0]), ([0, 0], [0, -1]), ([-1], [0])):
        with pytest.raises(IndexError):
            host_intersects(col, other, li, ri)


def test_python_plumbing_without_a_device(monkeypatch):
    """MosaicContext.st_intersects and st_distance share one argument path (_pair_call); here it runs
    with the host library behind the two C entries"""
    from mosaic_amd import RowPathRequired
    from mosaic_amd.context import GeometryTable, MosaicContext

    hl = C.host_lib()
    calls = []

    def entry(fn):
        def call(ctx, lh, rh, li, ri, n, out, status):
            calls.append((fn, li is None, n))
            return getattr(hl, fn)(lh, rh, li, ri, n, out, status, 2)
        return call

    fake = types.SimpleNamespace(mosaic_st_intersects=entry("si_intersects"), mosaic_st_distance=entry("sdl_distance"),
                                 mosaic_last_error=lambda: b"row index out of range")
    monkeypatch.setattr(N, "lib", lambda: fake)

    class HostTable(GeometryTable):  # a table whose handle is a column of the host library
        def __init__(self, col):
            self.col, self.handle, self.n_geoms, self.ctx = col, col.handle, col.n, None

        def close(self):
            self.handle = None

    def table(geoms):
        return HostTable(LCol.from_geoms(geoms))

    ctx = MosaicContext.__new__(MosaicContext)
    ctx.handle = None
    lt = table([poly([SQ]), line([(20, 0), (30, 0)]), pt(5, 5), line([])])
    rt = table([pt(5, 5), pt(25, 0), pt(5, 6), pt(1, 1)])
    got = ctx.st_intersects(lt, rt)
    assert got.dtype == np.bool_ and got.tolist() == [True, True, False, False] and calls[-1] == ("si_intersects", True, 4)
    # a single geometry is broadcast, on either side
    one = table([pt(5, 5)])
    assert ctx.st_intersects(lt, one).tolist() == [True, False, True, False] and calls[-1] == ("si_intersects", False, 4)
    assert ctx.st_intersects(one, lt).tolist() == [True, False, True, False]
    # a pair list
    got, st = ctx.st_intersects(lt, rt, pairs=([0, 0, 1, 2], [0, 3, 1, 0]), return_status=True)
    assert got.tolist() == [True, True, True, True] and st.tolist() == [N.ROW_OK] * 4 and got.dtype == np.bool_
    assert ctx.st_intersects(lt, rt, pairs=(np.zeros(0, np.int64), np.zeros(0, np.int64))).tolist() == []
    with pytest.raises(ValueError, match="different lengths"):
        ctx.st_intersects(lt, rt, pairs=([0, 1], [0]))
    with pytest.raises(ValueError, match="row-wise st_intersects of 4 and 2 rows"):
        ctx.st_intersects(lt, table([pt(0, 0), pt(1, 1)]))
    with pytest.raises(N.MosaicError):
        ctx.st_intersects(lt, rt, pairs=([4], [0]))
    # null and row-path rows
    mixed = HostTable(LCol.from_wkb([None, struct.pack("<BI", 1, 7) + struct.pack("<I", 0), geom_wkb(pt(5, 5)), geom_wkb(pt(1, 1))]))
    got, st = ctx.st_intersects(mixed, rt, return_status=True)
    assert st.tolist() == [N.ROW_NULL, N.ROW_PATH, N.ROW_OK, N.ROW_OK] and got.tolist() == [False, False, False, True]
    with pytest.raises(RowPathRequired) as e:
        ctx.st_intersects(mixed, rt)
    assert e.value.rows.tolist() == [1]
    # st_distance goes the same way and is what it was
    d = ctx.st_distance(lt, rt)
    assert d.dtype == np.float64 and d.tolist() == [0.0, 0.0, 1.0, 0.0] and calls[-1] == ("sdl_distance", True, 4)
    with pytest.raises(ValueError, match="row-wise st_distance of 4 and 2 rows"):
        ctx.st_distance(lt, table([pt(0, 0), pt(1, 1)]))
    assert "ST_Intersects.scala" in MosaicContext.st_intersects.__doc__ and "MosaicGeometryJTS.intersects" in MosaicContext.st_intersects.__doc__
