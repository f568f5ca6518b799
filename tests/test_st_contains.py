"""st_contains / st_within over geometry columns (JTS 1.19 Geometry.contains for Point / MultiPoint /
LineString / MultiLineString / Polygon / MultiPolygon on either side), CPU side: the sequential driver
contains::contains of mosaic_amd/csrc/st_contains.h compiled by g++ as tests/native/st_contains_host.cpp
-- source (H) -- plus the Python plumbing that needs no device.  The kernels are checked against (H) in
tests/test_gpu_st_contains.py.

The requirement: wherever the status is OK, out equals (E), the exact oracle of tests/contains_cases.py;
wherever it is PAIR_UNDECIDED, out is 0.  The hand-made cases pin the status as well.
"""
import struct
import types

import numpy as np
import pytest

from mosaic_amd import _native as N
from mosaic_amd import wkb as W

from tests import contains_cases as C
from tests.contains_cases import (HAND, OK, UNDECIDED, clean_pairs, exact_contains, exact_touch_without_crossing, host_contains,
                                  host_pair, kernel_cases, lattice_pairs)
from tests.test_st_distance import HOLE, SQ, poly, pt
from tests.test_st_distance_lines import LCol, geom_wkb, line

NEW_SYMBOLS = ("mosaic_st_contains_geoms", "mosaic_st_contains_last_split")


def test_library_exports_new_symbols():
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in N.EXPORTS
    assert lib.mosaic_abi_version() == 4  # adding a symbol breaks no caller
    assert N.PAIR_UNDECIDED == UNDECIDED == 3 and UNDECIDED not in (N.ROW_NULL, N.ROW_OK, N.ROW_PATH)
    header = open(C.ROOT + "/include/mosaic_hip.h").read()
    assert "#define MOSAIC_PAIR_UNDECIDED 3" in header


def test_entry_refuses_a_null_context():
    lib = N.lib()
    assert lib.mosaic_st_contains_geoms(None, None, None, None, None, 0, None, None) == N.MOSAIC_E_ARG
    assert lib.mosaic_last_error()
    five = np.full(5, -1, np.int64)
    assert lib.mosaic_st_contains_last_split(N.ptr(five)) == 0 and five.tolist() == [0] * 5
    assert lib.mosaic_st_contains_last_split(None) == N.MOSAIC_E_ARG


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made(case):
    name, a, b, status, out, oracle, swapped_status = case
    assert exact_contains(a, b) is bool(oracle), "the case table's oracle column"
    if status == OK:
        assert out == oracle
    else:
        assert out == 0
    assert host_pair(a, b) == (bool(out), status)
    # the sides swapped
    got, st = host_pair(b, a)
    assert st == swapped_status
    assert got is (exact_contains(b, a) if st == OK else False)


def test_facet_contact():
    """contains::facet_contact: 0 apart, 1 contact, 2 a proper crossing; a point facet never crosses"""
    f = C.host_facet_contact
    seg = ((0.0, 0.0), (10.0, 0.0))
    assert f(*seg, (5.0, -1.0), (5.0, 1.0)) == 2 and f((5.0, -1.0), (5.0, 1.0), *seg) == 2
    assert f(*seg, (5.0, 0.0), (5.0, 1.0)) == 1  # ends on the segment
    assert f(*seg, (10.0, -1.0), (10.0, 1.0)) == 1  # through an end
    assert f(*seg, (2.0, 0.0), (8.0, 0.0)) == 1 and f(*seg, (12.0, 0.0), (18.0, 0.0)) == 0  # collinear
    assert f(*seg, (5.0, 1.0), (5.0, 2.0)) == 0
    for p, want in (((3.0, 0.0), 1), ((0.0, 0.0), 1), ((3.0, 1.0), 0), ((12.0, 0.0), 0)):
        assert f(p, p, *seg) == want and f(*seg, p, p) == want
    # one ulp decides between a crossing and a touch on a long sloped segment (the double-double path)
    big = ((-1048576.0, -699051.0), (1048575.0, 699050.0))
    mid = (-0.5, -0.5)
    assert f(*big, mid, (0.0, 5.0)) == 1
    assert f(*big, (mid[0], float(np.nextafter(mid[1], -1.0))), (0.0, 5.0)) == 2
    assert f(*big, (mid[0], float(np.nextafter(mid[1], 1.0))), (0.0, 5.0)) == 0


def check_against_oracle(pairs, got, st):
    """OK => out equals (E); UNDECIDED => out 0.  Returns the oracle's values."""
    want = np.array([exact_contains(a, b) for a, b in pairs])
    assert set(st.tolist()) <= {OK, UNDECIDED}
    bad = [k for k in range(len(pairs)) if (st[k] == OK and bool(got[k]) is not bool(want[k])) or (st[k] != OK and got[k])]
    assert not bad, bad[:10]
    return want


def test_kernel_shapes_against_exact():
    cases = kernel_cases()
    pairs = [(c[1], c[2]) for c in cases]
    got, st, how = host_contains(LCol.from_geoms([a for a, _ in pairs]), LCol.from_geoms([b for _, b in pairs]), return_how=True)
    want = check_against_oracle(pairs, got, st)
    by_name = {c[0]: (bool(g), int(s), int(h)) for c, g, s, h in zip(cases, got, st, how)}
    assert by_name["building inside"] == (True, OK, C.HOW_CLEAR)
    assert by_name["building inside the hole"] == (False, OK, C.HOW_CLEAR)
    assert by_name["building across the shell"] == (False, OK, C.HOW_OUT)
    assert by_name["building across the hole's ring"] == (False, OK, C.HOW_OUT)
    assert by_name["building covering the hole"] == (False, OK, C.HOW_CLEAR)
    assert by_name["building outside, in the box's corner"] == (False, OK, C.HOW_CLEAR)
    assert by_name["trip of 130 inside"] == (True, OK, C.HOW_CLEAR)
    assert by_name["trip of 130 through the hole"] == (False, OK, C.HOW_OUT)
    assert by_name["trip of 130 leaving through the shell"] == (False, OK, C.HOW_OUT)
    assert by_name["the zone with itself"] == (False, UNDECIDED, C.HOW_TOUCH)
    assert by_name["multipoint of 60 inside"] == (True, OK, C.HOW_POINTS_IN)
    assert by_name["multipoint of 60, the last one in the hole"] == (False, OK, C.HOW_POINTS_OUT)
    assert by_name["multipoint of 60, all on the shell's vertices"] == (False, OK, C.HOW_POINTS_IN)
    assert by_name["multipoints of 60 and 59"] == (True, OK, C.HOW_POINTS_IN)
    assert by_name["multipoints of 60 and 59, one missing"] == (False, OK, C.HOW_POINTS_OUT)
    assert by_name["a 40-ring in the 300-ring, hole uncovered"] == (True, OK, C.HOW_CLEAR)
    assert want.any() and not want.all()


def test_clean_generator():
    """zones on the even lattice, buildings and lines on the odd one: nothing touches without crossing, so
    nothing may be undecided, and every answer equals the oracle's"""
    pairs = [(a, b) for a, b, _ in clean_pairs()]
    assert 200 <= len(pairs) <= 400
    assert not any(exact_touch_without_crossing(a, b) for a, b in pairs)  # (E) finds no contact without a crossing
    for a, b in pairs:  # the lattices
        assert all(c % 2 == 0 for v in C.vertices(a) for c in v) and all(c % 2 == 1 for v in C.vertices(b) for c in v)
    got, st, how = host_contains(LCol.from_geoms([a for a, _ in pairs]), LCol.from_geoms([b for _, b in pairs]), return_how=True)
    assert (st == OK).all(), np.flatnonzero(st != OK)[:10]  # the cap: zero undecided pairs
    want = check_against_oracle(pairs, got, st)
    assert min(int(want.sum()), int((~want).sum())) >= len(pairs) // 4, int(want.sum())
    # every way of deciding step 5 occurs, with lines and polygons, holes and second parts
    assert {C.HOW_BOX, C.HOW_OUT, C.HOW_CLEAR} <= set(how.tolist())
    assert {b[0] for _, b in pairs} == {"line", "polygon"}
    clear0 = [k for k in range(len(pairs)) if how[k] == C.HOW_CLEAR and not got[k]]
    assert any(clean_pairs()[k][2] == "around the hole" for k in clear0) and any(clean_pairs()[k][2] == "in the hole" for k in clear0)
    # rings of 5 to 40 vertices, some of them a whole number of 3-segment tiles
    facets = [len(a[1][0][0]) - 1 for a, _ in pairs]
    assert min(facets) <= 6 and max(facets) >= 30 and any(f % 3 == 0 for f in facets) and any(f % 3 for f in facets)


def test_shared_lattice_generator():
    """one coarse lattice on both sides: touches abound; OK => the oracle's value, UNDECIDED => 0"""
    pairs = list(lattice_pairs())
    got, st, how = host_contains(LCol.from_geoms([a for a, _ in pairs]), LCol.from_geoms([b for _, b in pairs]), return_how=True)
    want = check_against_oracle(pairs, got, st)
    n_ok, n_un = int((st == OK).sum()), int((st == UNDECIDED).sum())
    print(f"shared lattice: {len(pairs)} pairs, {n_un} undecided ({n_un / len(pairs):.0%}), of them {int(want[st == UNDECIDED].sum())} "
          f"contained by the oracle; {int(got.sum())} contained and decided")
    assert n_ok >= 1 and n_un >= 1
    assert got.any() and {C.HOW_KINDS, C.HOW_TOUCH, C.HOW_OUT, C.HOW_CLEAR, C.HOW_POINTS_IN, C.HOW_POINTS_OUT} <= set(how.tolist())
    assert want[st == UNDECIDED].any() and not want[st == UNDECIDED].all()  # both answers hide among the undecided


def test_point_rows_equal_the_point_form():
    """step 3 on POINT rows against the CPU oracle of the point form (oracle/pip.c, what ctx.st_contains is
    checked against): identical on every one of the 35 NYC zones against the golden pickups and generated points"""
    import oracle
    from mosaic_amd.data import PolygonSet, quickstart_points
    from tests.test_st_distance import pickups

    zones = PolygonSet.load("nyc_taxi_zones_35")
    qx, qy = quickstart_points(zones, 200, seed=11)
    x, y = np.concatenate([pickups()[0], qx]), np.concatenate([pickups()[1], qy])
    zi, pi = C.all_pairs(len(zones), len(x))
    got, st = host_contains(LCol.from_polyset(zones), LCol.from_points(x, y), zi, pi)
    assert (st == OK).all()
    blobs = [W.geometry_wkb(zones.parts(g)) for g in range(len(zones))]
    want = np.array([oracle.wkb_contains(blobs[g], x[k], y[k]) for g, k in zip(zi, pi)])
    assert np.array_equal(got, want) and 100 < int(got.sum()) <= len(x)


def test_status_and_errors():
    one_vertex = struct.pack("<BII", 1, 2, 1) + struct.pack("<2d", 3, 3)
    collection = struct.pack("<BI", 1, 7) + struct.pack("<I", 0)
    rows = [geom_wkb(poly([SQ])), None, geom_wkb(line([])), collection, W.point_wkb(float("nan"), float("nan")),
            one_vertex, geom_wkb(line([(0, 0), (9, 9)])), geom_wkb(pt(0, 4, 5, 5))]
    col = LCol.from_wkb(rows)
    other = LCol.from_geoms([pt(5, 5)] * len(rows))
    ok, null, path = N.ROW_OK, N.ROW_NULL, N.ROW_PATH
    got, st = host_contains(col, other)
    assert st.tolist() == [ok, null, ok, path, path, path, UNDECIDED, ok]
    assert got.tolist() == [True, False, False, False, False, False, False, True]
    got2, st2 = host_contains(other, col)
    assert st2.tolist() == [ok, null, ok, path, path, path, ok, ok]  # the box ends the line; the multipoint sticks out
    assert not got2.any()
    # a line row in a column built without the lines flag stays a row for the row path
    plain = LCol.from_wkb(rows, flags=0)
    got, st = host_contains(plain, other)
    assert st.tolist() == [ok, null, path, path, path, path, path, ok]
    assert got.tolist() == [True] + [False] * 6 + [True]
    # pair lists; an out-of-range row index writes nothing
    li, ri = [0, 7, 0, 6], [0, 1, 2, 7]
    got, st = host_contains(col, other, li, ri)
    assert got.tolist() == [True, True, True, False] and st.tolist() == [ok, ok, ok, UNDECIDED]
    for li, ri in (([0, 8], [0, 0]), ([0, 0], [0, -1]), ([-1], [0])):
        with pytest.raises(IndexError):
            host_contains(col, other, li, ri)


def test_python_plumbing_without_a_device(monkeypatch):
    """MosaicContext.st_contains_geoms / st_within_geoms go through st_intersects' argument path
    (_pair_call); here they run with the host library behind the C entry"""
    from mosaic_amd import RowPathRequired
    from mosaic_amd.context import GeometryTable, MosaicContext

    hl = C.host_lib()
    calls = []

    def entry(ctx, lh, rh, li, ri, n, out, status):
        calls.append((li is None, n))
        return hl.sc_contains(lh, rh, li, ri, n, out, status, None, 2)

    fake = types.SimpleNamespace(mosaic_st_contains_geoms=entry, mosaic_last_error=lambda: b"row index out of range")
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
    zones = table([poly([SQ, HOLE]), poly([SQ]), poly([SQ]), poly([SQ])])
    things = table([pt(1, 1), line([(1, 1), (9, 9)]), poly([[(2, 2), (4, 2), (4, 4), (2, 2)]]), pt(5, 20)])
    got = ctx.st_contains_geoms(zones, things)
    assert got.dtype == np.bool_ and got.tolist() == [True, True, True, False] and calls[-1] == (True, 4)
    assert ctx.st_within_geoms(things, zones).tolist() == [True, True, True, False]
    # a single geometry is broadcast, on either side
    one = table([poly([SQ])])
    assert ctx.st_contains_geoms(one, things).tolist() == [True, True, True, False] and calls[-1] == (False, 4)
    assert ctx.st_within_geoms(things, one).tolist() == [True, True, True, False]
    # a pair list: (left row, right row) as given, also for st_within
    got, st = ctx.st_contains_geoms(zones, things, pairs=([0, 1, 1], [2, 0, 3]), return_status=True)
    assert got.tolist() == [False, True, False] and st.tolist() == [OK] * 3 and got.dtype == np.bool_
    got, st = ctx.st_within_geoms(things, zones, pairs=([2, 0, 3], [0, 1, 1]), return_status=True)
    assert got.tolist() == [False, True, False] and st.tolist() == [OK] * 3
    assert ctx.st_contains_geoms(zones, things, pairs=(np.zeros(0, np.int64), np.zeros(0, np.int64))).tolist() == []
    with pytest.raises(ValueError, match="row-wise st_contains of 4 and 2 rows"):
        ctx.st_contains_geoms(zones, table([pt(0, 0), pt(1, 1)]))
    with pytest.raises(N.MosaicError):
        ctx.st_contains_geoms(zones, things, pairs=([4], [0]))
    # undecided pairs and row-path rows: reported by status, raised without it
    touching = HostTable(LCol.from_wkb([geom_wkb(line([(5, 5), (10, 5)])), None, geom_wkb(poly([SQ])), geom_wkb(pt(1, 1))]))
    mixed = HostTable(LCol.from_wkb([geom_wkb(poly([SQ])), geom_wkb(poly([SQ])), struct.pack("<BI", 1, 7) + struct.pack("<I", 0),
                                     geom_wkb(line([(0, 0), (9, 9)]))]))
    got, st = ctx.st_contains_geoms(mixed, touching, return_status=True)
    assert st.tolist() == [UNDECIDED, N.ROW_NULL, N.ROW_PATH, UNDECIDED] and not got.any()
    with pytest.raises(RowPathRequired) as e:
        ctx.st_contains_geoms(mixed, touching)
    assert e.value.rows.tolist() == [0, 2, 3]
    assert "ST_Contains.scala" in MosaicContext.st_contains_geoms.__doc__ and "PAIR_UNDECIDED" in MosaicContext.st_contains_geoms.__doc__
