"""st_distance with line geometries (JTS 1.19 DistanceOp extended to LineString / MultiLineString: a
component line is an open run of segments that is never closed and never contains anything), CPU
side: the kind-aware sequential driver of mosaic_amd/csrc/st_distance.h, the column builder's opt-in
line decode and LineSet form (geoms_build.h) and ring_neighbours.h over such columns, compiled by g++
as tests/native/st_distance_lines_host.cpp -- source (H) below -- plus the Python plumbing that needs
no device.  The kernels are checked against (H) in tests/test_gpu_st_distance_lines.py and
tests/test_gpu_knn_lines.py.

Expected values never come from the code under test.  The sources are those of
tests/test_st_distance.py, extended with lines as open rings that never contain:
  (E) exact: the fractions.Fraction brute force on integer coordinates |c| <= 2^20; the arithmetic
      per facet pair is that file's, so its 3-ulp bound holds unchanged, and zero agrees exactly.
  (N) the numpy restatement, bit-identical by construction.
The analytic cases carry their value worked out by hand.
"""
import ctypes
import functools
import os
import struct
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from mosaic_amd import _native as N
from mosaic_amd import wkb as W
from mosaic_amd.data import LineSet

from tests import test_st_distance as T
from tests.test_st_distance import HOLE, SQ, assert_same_bits, bits, poly, pt, sqrt_rounded, ulps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mosaic_geoms_create_wkb_ex", "mosaic_geoms_create_lines")
HOST_THREADS = T.HOST_THREADS
LINES = 1  # MOSAIC_GEOMS_LINES


# ---- geometries: those of tests/test_st_distance.py and ("line", [component line, ...]) ----
def line(*lines):
    return ("line", [[tuple(map(float, v)) for v in ln] for ln in lines])


def geom_wkb(g, big_endian=True):
    if g[0] != "line":
        return T.geom_wkb(g, big_endian)
    lines = g[1]
    return W.linestring_wkb(lines[0], big_endian) if len(lines) == 1 else W.multilinestring_wkb(lines, big_endian)


def as_rings(g):
    """a line geometry as open rings, one per non-empty component (the model of the facets and of the
    components' first coordinates); other geometries as they are"""
    return ("polygon", [[ln] for ln in g[1] if ln]) if g[0] == "line" else g


def facets_of(g):
    return T.facets_of(as_rings(g))


def contained(a, b):
    """a polygon part of a holds the first coordinate of a component of b, exactly; a line holds nothing"""
    return a[0] == "polygon" and T.exact_contained(a, as_rings(b))


def exact_distance2(a, b):
    """(E): the exact squared distance (Fraction)"""
    fa, fb = [np.atleast_1d(v) for v in facets_of(a)], [np.atleast_1d(v) for v in facets_of(b)]
    if len(fa[0]) == 0 or len(fb[0]) == 0:
        return Fraction(0)
    if contained(a, b) or contained(b, a):
        return Fraction(0)
    sa = [(T.exact((fa[0][i], fa[1][i])), T.exact((fa[2][i], fa[3][i]))) for i in range(len(fa[0]))]
    sb = [(T.exact((fb[0][j], fb[1][j])), T.exact((fb[2][j], fb[3][j]))) for j in range(len(fb[0]))]
    best = None
    for p, q in sa:
        for r, s in sb:
            if T._segments_meet(p, q, r, s):
                return Fraction(0)
            d = min(T._pt_seg2(p, r, s), T._pt_seg2(q, r, s), T._pt_seg2(r, p, q), T._pt_seg2(s, p, q))
            if best is None or d < best:
                best = d
    return best


def numpy_distance(a, b):
    """(N)"""
    fa, fb = facets_of(a), facets_of(b)
    if len(fa[0]) == 0 or len(fb[0]) == 0:
        return 0.0
    if contained(a, b) or contained(b, a):
        return 0.0
    best = np.inf
    for i0 in range(0, len(fa[0]), 256):
        left = [v[i0:i0 + 256, None] for v in fa]
        best = min(best, float(T.n_seg_seg(*left, *[v[None, :] for v in fb]).min()))
    return best


# ---- (H) the host library ----
@functools.lru_cache(maxsize=None)
def host_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="sdl_host_"), "libsdl.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-pthread",
                    "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "st_distance_lines_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    for name, args, res in (("sdl_col_wkb", [i64, vp, vp, vp, ctypes.c_uint32], vp), ("sdl_col_lines", [i64, vp, vp, vp], vp),
                            ("sdl_col_arrays", [i64, vp, vp, vp, vp], vp), ("sdl_col_points", [vp, vp, i64], vp),
                            ("sdl_col_info", [vp, vp], None), ("sdl_col_status", [vp, vp, vp], None),
                            ("sdl_col_part_kinds", [vp, vp], None), ("sdl_col_free", [vp], None),
                            ("sdl_distance", [vp, vp, vp, vp, i64, vp, vp, i32], i32),
                            ("sdl_neighbours", [vp, vp, i64, vp, vp, vp, vp, i64, i32], vp),
                            ("sdl_result_info", [vp, vp], None), ("sdl_result_export", [vp, vp, vp, vp, vp], None),
                            ("sdl_result_free", [vp], None), ("sdl_same_geometry", [vp, i64, vp, i64], i32)):
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    return lib


class LCol:
    """a geometry column of the host library"""

    def __init__(self, handle):
        assert handle
        self.handle = handle
        info = np.zeros(4, np.int64)
        host_lib().sdl_col_info(handle, N.ptr(info))
        self.n, self.n_vertices, self.n_row_path, self.n_parts = (int(v) for v in info)

    @classmethod
    def from_wkb(cls, rows, flags=LINES):
        """rows: WKB bytes or None"""
        lens = np.array([0 if r is None else len(r) for r in rows], np.int64)
        offs = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        data = np.frombuffer(b"".join(r or b"" for r in rows) or b"\0", np.uint8).copy()
        valid = np.array([r is not None for r in rows], np.uint8)
        return cls(host_lib().sdl_col_wkb(len(rows), N.ptr(offs), N.ptr(data), N.ptr(valid), flags))

    @classmethod
    def from_geoms(cls, geoms):
        """through the WKB decode with the lines flag, alternating byte order"""
        return cls.from_wkb([geom_wkb(g, bool(i % 2)) for i, g in enumerate(geoms)])

    @classmethod
    def from_lineset(cls, ls):
        h = host_lib().sdl_col_lines(len(ls), N.ptr(ls.geom_lines), N.ptr(ls.line_offsets), N.ptr(ls.xy))
        if not h:
            raise ValueError("inconsistent offsets")
        return cls(h)

    @classmethod
    def from_polyset(cls, ps):
        return cls(host_lib().sdl_col_arrays(len(ps), N.ptr(ps.geom_parts), N.ptr(ps.part_rings), N.ptr(ps.ring_offsets),
                                             N.ptr(ps.xy)))

    @classmethod
    def from_points(cls, x, y):
        x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
        return cls(host_lib().sdl_col_points(N.ptr(x), N.ptr(y), len(x)))

    def status(self):
        st, fc = np.zeros(max(self.n, 1), np.int32), np.zeros(max(self.n, 1), np.uint32)
        host_lib().sdl_col_status(self.handle, N.ptr(st), N.ptr(fc))
        return st[:self.n], fc[:self.n]

    def part_kinds(self):
        k = np.zeros(max(self.n_parts, 1), np.uint8)
        host_lib().sdl_col_part_kinds(self.handle, N.ptr(k))
        return k[:self.n_parts].tolist()

    def __del__(self):
        try:
            host_lib().sdl_col_free(self.handle)
        except Exception:
            pass


def host_distance(left, right, li=None, ri=None, threads=HOST_THREADS, return_status=False):
    """the kind-aware dist::distance over two columns (LCol, or a HostCol of tests/test_st_distance.py:
    the same GeomColumn behind the handle)"""
    if li is None:
        assert left.n == right.n
        n = left.n
    else:
        li, ri = np.ascontiguousarray(li, np.int64), np.ascontiguousarray(ri, np.int64)
        n = len(li)
    out = np.full(max(n, 1), -1.0)
    st = np.full(max(n, 1), -1, np.int32)
    rc = host_lib().sdl_distance(left.handle, right.handle, N.ptr(li), N.ptr(ri), n, N.ptr(out), N.ptr(st), threads)
    if rc:
        raise IndexError("row index out of range")
    return (out[:n], st[:n]) if return_status else out[:n]


def host_pair(a, b):
    return float(host_distance(LCol.from_geoms([a]), LCol.from_geoms([b]))[0])


def host_neighbours(chips, left, right, rows, cells, keep_self=False):
    """rn::neighbours over the candidates' chips (cells, keys): ([(landmark, candidate, distance bits)] in
    the result's order, set of unmatched landmarks)"""
    ids, keys = np.ascontiguousarray(chips[0], np.int64), np.ascontiguousarray(chips[1], np.int32)
    rows, cells = np.ascontiguousarray(rows, np.int64), np.ascontiguousarray(cells, np.int64)
    assert len(rows) == len(cells) and len(ids) == len(keys)
    lib = host_lib()
    h = lib.sdl_neighbours(N.ptr(ids), N.ptr(keys), len(ids), left.handle, right.handle, N.ptr(rows), N.ptr(cells), len(rows),
                           int(keep_self))
    if not h:
        raise IndexError("row index out of range")
    try:
        info = np.zeros(2, np.int64)
        lib.sdl_result_info(h, N.ptr(info))
        n, n_left = int(info[0]), int(info[1])
        l, c, d = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.float64)
        un = np.zeros(max(n_left, 1), np.uint8)
        lib.sdl_result_export(h, N.ptr(l), N.ptr(c), N.ptr(d), N.ptr(un))
    finally:
        lib.sdl_result_free(h)
    return list(zip(l[:n].tolist(), c[:n].tolist(), bits(d[:n]).tolist())), set(np.flatnonzero(un[:n_left]).tolist())


# ---- the analytic cases: (name, left, right, expected); the GPU file runs them too ----
TRI = [(4, 4), (6, 4), (6, 6), (4, 4)]
C_SHAPE = [(0, 0), (10, 0), (10, 10), (0, 10)]  # SQ without its closing segment (0 10)-(0 0)
ANALYTIC = (
    # a line part never contains: fails if a closed LineString is taken for a ring with an interior
    ("point strictly inside a closed line", line(SQ), pt(5, 4), 4.0),
    ("point strictly inside a closed line, point first", pt(3, 5), line(SQ), 3.0),
    ("polygon inside a closed line", poly([TRI]), line(SQ), 4.0),
    ("closed line around a polygon", line(SQ), poly([TRI]), 4.0),
    ("closed line inside a closed line", line(TRI), line(SQ), 4.0),
    # a line part is a component: its first coordinate is located in every polygon part of the other side
    ("line inside a polygon", line([(1, 1), (2, 2)]), poly([SQ]), 0.0),
    ("polygon around a line", poly([SQ]), line([(8, 1), (9, 3), (7, 2)]), 0.0),
    ("line from the polygon's boundary outwards", line([(10, 5), (15, 5)]), poly([SQ]), 0.0),
    ("line from a polygon's vertex outwards", poly([SQ]), line([(10, 10), (15, 12)]), 0.0),
    ("line inside a hole", line([(4, 5), (6, 5)]), poly([SQ, HOLE]), 1.0),
    ("line inside a hole, polygon first", poly([SQ, HOLE]), line([(5, 6.5), (5, 5)]), 0.5),
    ("second component inside the polygon", line([(20, 20), (30, 20)], [(1, 1), (2, 2)]), poly([SQ]), 0.0),
    ("second component inside the second part", poly([[(50, 50), (60, 50), (60, 60), (50, 50)]], [SQ]),
     line([(20, 20), (30, 20)], [(1, 1), (2, 2)]), 0.0),
    ("line from outside across the boundary", line([(-5, 5), (5, 5)]), poly([SQ]), 0.0),
    ("line from outside across the whole polygon", poly([SQ]), line([(-5, 5), (15, 6)]), 0.0),
    ("line outside a polygon", line([(13, -4), (13, 4), (20, 4)]), poly([SQ]), 3.0),
    # nothing closes a line: fails if the segment (0 10)-(0 0) is added
    ("point on the missing closing segment", line(C_SHAPE), pt(0, 5), 5.0),
    ("line through the missing closing segment", line([(-5, 5), (5, 5)]), line(C_SHAPE), 5.0),
    # two-vertex lines
    ("crossing", line([(0, 0), (4, 4)]), line([(0, 4), (4, 0)]), 0.0),
    ("T-touching", line([(0, 0), (4, 0)]), line([(2, 0), (2, 3)]), 0.0),
    ("end to end", line([(0, 0), (1, 0)]), line([(1, 0), (2, 5)]), 0.0),
    ("parallel", line([(0, 0), (4, 0)]), line([(0, 3), (4, 3)]), 3.0),
    ("collinear and overlapping", line([(0, 0), (4, 0)]), line([(2, 0), (6, 0)]), 0.0),
    ("collinear and disjoint", line([(0, 0), (2, 0)]), line([(5, 0), (9, 0)]), 3.0),
    ("zero-length line and point", line([(1, 2), (1, 2)]), pt(4, 6), 5.0),
    ("line and zero-length line", line([(0, 0), (0, 9)]), line([(3, 4), (3, 4)]), 3.0),
    ("zero-length lines", line([(1, 2), (1, 2)]), line([(4, 6), (4, 6)]), 5.0),
    ("point and line", pt(3, 4), line([(0, 0), (0, 9)]), 3.0),
    ("multipoint and multiline", pt(100, 100, 3, 4), line([(50, 0), (60, 0)], [(0, 0), (0, 9)]), 3.0),
    # empties
    ("LINESTRING EMPTY on the left", line([]), pt(1, 1), 0.0),
    ("MULTILINESTRING EMPTY on the right", poly([SQ]), line(), 0.0),
    ("empty line and empty polygon", line([]), poly([]), 0.0),
    ("multiline with an empty member", line([], [(0, 0), (0, 9)]), pt(3, 4), 3.0),
    ("multiline with an empty member last", pt(3, 4), line([(0, 0), (0, 9)], []), 3.0),
)


def zigzag(n, x0, y0, dx=7, dy=5):
    """an integer polyline of n vertices"""
    return [(x0 + dx * i, y0 + (dy if i % 2 else 0) + i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def tile_pairs():
    """lines of 4, 5, 8 and 9 vertices (3, 4, 7, 8 segments: around one and two tiles of 4) against each
    other, a point, a polygon and a closed line, apart and crossing"""
    sizes = (2, 4, 5, 8, 9)
    left, right = [], []
    for a in sizes:
        for b in sizes:
            for off in (40, 3):
                left.append(line(zigzag(a, 0, 0)))
                right.append(line(zigzag(b, 2, off, dx=5, dy=-4)))
        for other in (pt(11, 30), pt(14, 2), poly([[(0, 20), (60, 20), (30, 50), (0, 20)]]), poly([[(-9, -9), (90, -9), (90, 30), (-9, 30), (-9, -9)]]),
                      line([(0, 20), (60, 20), (30, 50), (0, 20)]), line(zigzag(a, 0, 0), zigzag(9, 1, 25))):
            left.append(line(zigzag(a, 0, 0)))
            right.append(other)
            left.append(other)
            right.append(line(zigzag(a, 0, 0)))
    return tuple(left), tuple(right)


# ---- seeded random integer geometries, |c| <= 2^20: {point, multipoint, line, multiline, polygon with a hole}^2 ----
def walk(rng, cx, cy, radius, n):
    p = np.array([cx, cy]) + rng.uniform(-0.5 * radius, 0.5 * radius, 2)
    out = []
    for _ in range(n):
        out.append((float(round(p[0])), float(round(p[1]))))
        p = p + rng.uniform(-0.4 * radius, 0.4 * radius, 2)
    return out


def random_geom(rng, cx, cy):
    kind = int(rng.integers(0, 5))
    radius = float(rng.integers(2000, 120000))
    if kind == 0:
        return pt(round(cx), round(cy))
    if kind == 1:
        k = int(rng.integers(2, 6))
        return pt(*[float(round(c)) for c in (np.array([cx, cy]) + rng.uniform(-radius, radius, (k, 2))).ravel()])
    if kind == 2:
        ln = walk(rng, cx, cy, radius, int(rng.integers(2, 12)))
        if rng.integers(0, 4) == 0:
            ln = ln + ln[:1]  # a closed line
        return line(ln)
    if kind == 3:
        return line(*[walk(rng, cx + 1.5 * radius * j, cy, radius, int(rng.integers(2, 9))) for j in range(int(rng.integers(2, 4)))])
    return poly([T.star(rng, cx, cy, radius, int(rng.integers(5, 24))),
                 T.star(rng, cx, cy, 0.4 * radius, int(rng.integers(4, 10)), lo=0.4)])


def kind_of(g):
    return (g[0], min(len(g[1]), 2))


@functools.lru_cache(maxsize=None)
def random_pairs(n=300, seed=20250612):
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        cx, cy = rng.uniform(-200000, 200000, 2)
        a = random_geom(rng, cx, cy)
        spread = (20000, 120000, 250000)[int(rng.integers(0, 3))]  # inside / overlapping / apart
        b = random_geom(rng, cx + rng.uniform(-spread, spread), cy + rng.uniform(-spread, spread))
        pairs.append((a, b))
    assert all(abs(c) <= 2 ** 20 for a, b in pairs for g in (a, b) for v in facets_of(g) for c in np.atleast_1d(v))
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def random_host():
    pairs = random_pairs()
    return host_distance(LCol.from_geoms([a for a, _ in pairs]), LCol.from_geoms([b for _, b in pairs]))


# ---- tests ----
def test_library_exports_new_symbols():
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in N.EXPORTS
    assert N.GEOMS_LINES == LINES


def test_abi_version_unchanged():
    assert N.lib().mosaic_abi_version() == 4


@pytest.mark.parametrize("case", ANALYTIC, ids=[c[0] for c in ANALYTIC])
def test_analytic(case):
    name, a, b, want = case
    got = host_pair(a, b)
    assert got == want and not np.signbit(got)
    # and the sources agree on it
    assert numpy_distance(a, b) == want
    assert sqrt_rounded(exact_distance2(a, b)) == want


def test_closed_line_is_no_container_but_the_kind_blind_driver_takes_it_for_one():
    """why the definition needs the part kinds: the form without them, kept for columns of points and
    polygons, would put a point inside a closed line at 0"""
    col, p = LCol.from_geoms([line(SQ)]), LCol.from_geoms([pt(5, 4)])
    assert host_distance(col, p).tolist() == [4.0]
    assert T.host_distance(col, p).tolist() == [0.0]  # tests/native/st_distance_host.cpp: every part may contain
    assert col.part_kinds() == [2] and p.part_kinds() == [1] and LCol.from_geoms([poly([SQ], [TRI])]).part_kinds() == [0, 0]


def test_tile_pairs_against_numpy():
    left, right = tile_pairs()
    got = host_distance(LCol.from_geoms(left), LCol.from_geoms(right))
    assert_same_bits(got, [numpy_distance(a, b) for a, b in zip(left, right)], "tile pairs")
    assert (got == 0).any() and (got > 0).any()


def test_host_against_exact():
    pairs, got = random_pairs(), random_host()
    kinds = {(kind_of(a), kind_of(b)) for a, b in pairs}
    assert len(kinds) == 25, sorted(kinds)
    worst, zeros = 0, 0
    for k, (a, b) in enumerate(pairs):
        d2 = exact_distance2(a, b)
        if d2 == 0:
            zeros += 1
            assert got[k] == 0.0, k
        else:
            assert got[k] > 0.0, k
            worst = max(worst, ulps(got[k], sqrt_rounded(d2)))
    print(f"(H) against (E): worst {worst} ulp over {len(pairs) - zeros} positive pairs, {zeros} zeros")
    assert 20 <= zeros <= len(pairs) - 100
    assert worst <= 3
    # some zeros come from a line's first coordinate in a polygon alone, and some closed lines hold the other side
    only_contained = sum(1 for a, b in pairs if "line" in (a[0], b[0]) and (contained(a, b) or contained(b, a)))
    assert only_contained > 0


def test_host_against_numpy_random():
    pairs, got = random_pairs(), random_host()
    assert_same_bits(got, [numpy_distance(a, b) for a, b in pairs], "random pairs")


def test_lineset_column():
    geoms = [[[(0, 0), (4, 0), (4, 3)]], [[(0, 8), (1, 8)], [(5, 5), (6, 5), (6, 6), (5, 5)]], [], [[], [(0, 9), (3, 9)]],
             [[(1, 1)]], [[(0, 0), (1, 0)], [(7, 7)]]]
    ls = LineSet.from_lines(geoms)
    col = LCol.from_lineset(ls)
    st, facets = col.status()
    assert st.tolist() == [N.ROW_OK] * 4 + [N.ROW_PATH] * 2
    assert facets.tolist() == [2, 4, 0, 1, 0, 0]
    assert (col.n, col.n_vertices, col.n_row_path, col.n_parts) == (6, 11, 2, 4) and col.part_kinds() == [2, 2, 2, 2]
    # the same column through the WKB decode
    by_wkb = LCol.from_wkb([ls.wkb(g, bool(g % 2)) for g in range(len(ls))])
    assert by_wkb.status()[0].tolist() == st.tolist() and by_wkb.status()[1].tolist() == facets.tolist()
    assert (by_wkb.n_vertices, by_wkb.n_parts) == (col.n_vertices, col.n_parts)
    lib = host_lib()
    for g in range(4):
        assert lib.sdl_same_geometry(col.handle, g, by_wkb.handle, g) == 1
    other = LCol.from_geoms([pt(0, 4)] * len(geoms))
    d, s = host_distance(col, other, return_status=True)
    assert s.tolist() == st.tolist() and np.isnan(d[4:]).all()
    assert d[:4].tolist() == [4.0, 4.0, 0.0, 5.0]
    # inconsistent offsets
    for bad in (LineSet(ls.xy, ls.line_offsets, [0, 2, 1]), LineSet(ls.xy, [0, 3, 2], [0, 1, 2])):
        with pytest.raises(ValueError):
            LCol.from_lineset(bad)


def test_status_and_wkb_variants():
    one_vertex = struct.pack("<BII", 1, 2, 1) + struct.pack("<2d", 3, 3)
    rows = [geom_wkb(line([(0, 0), (0, 9)])), None, geom_wkb(line([])), geom_wkb(line()), one_vertex,
            W.multilinestring_wkb([[(0.0, 0.0), (0.0, 9.0)], [(7.0, 7.0)]]), struct.pack("<BI", 1, 7) + struct.pack("<I", 0),  # collection
            W.point_wkb(float("nan"), float("nan")), b"\x01\x02\x00", geom_wkb(line([], [(0, 0), (0, 9)]), False),
            struct.pack("<BII", 1, 2, 3) + struct.pack("<4d", 0, 0, 1, 1)]  # a LineString cut short
    col = LCol.from_wkb(rows)
    st, facets = col.status()
    assert st.tolist() == [N.ROW_OK, N.ROW_NULL, N.ROW_OK, N.ROW_OK, N.ROW_PATH, N.ROW_PATH, N.ROW_PATH, N.ROW_PATH, N.ROW_PATH,
                           N.ROW_OK, N.ROW_PATH]
    assert facets.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0] and col.n_row_path == 6 and col.n_vertices == 4 and col.n_parts == 2
    d, s = host_distance(col, LCol.from_geoms([pt(3, 4)] * len(rows)), return_status=True)
    assert s.tolist() == st.tolist() and np.isnan(d[s != N.ROW_OK]).all()
    assert d[[0, 2, 3, 9]].tolist() == [3.0, 0.0, 0.0, 3.0]
    # without the flag the same rows are rows for the row path, as before: through the builder's old
    # entry (tests/native/st_distance_host.cpp) and through the new one with flags 0
    for plain in (T.HostCol.from_wkb(rows), LCol.from_wkb(rows, flags=0)):
        st0, facets0 = plain.status()
        assert st0.tolist() == [N.ROW_PATH, N.ROW_NULL] + [N.ROW_PATH] * 9
        assert not facets0.any() and plain.n_row_path == 10 and plain.n_vertices == 0
    # both byte orders, ISO Z / ZM and EWKB Z / SRID variants decode to the same rows
    ln = [(0.0, 0.0), (0.0, 9.0), (2.0, 11.0)]
    iso_z = struct.pack(">BII", 0, 1002, 3) + b"".join(struct.pack(">ddd", x, y, 77.0) for x, y in ln)
    iso_zm = struct.pack("<BII", 1, 3002, 3) + b"".join(struct.pack("<dddd", x, y, 77.0, 88.0) for x, y in ln)
    ewkb = struct.pack("<BIII", 1, 0x80000000 | 0x20000000 | 2, 4326, 3) + b"".join(struct.pack("<ddd", x, y, 5.0) for x, y in ln)
    multi_z = struct.pack(">BII", 0, 1005, 2) + struct.pack(">BII", 0, 1002, 0) + iso_z
    v = LCol.from_wkb([W.linestring_wkb(ln, True), W.linestring_wkb(ln, False), iso_z, iso_zm, ewkb, multi_z])
    assert v.status()[0].tolist() == [N.ROW_OK] * 6 and v.status()[1].tolist() == [2] * 6 and v.n_vertices == 18
    for g in range(1, 6):
        assert host_lib().sdl_same_geometry(v.handle, 0, v.handle, g) == 1
    assert host_distance(v, LCol.from_geoms([pt(3, 4)] * 6)).tolist() == [3.0] * 6
    assert T.HostCol.from_wkb([iso_z, multi_z]).status()[0].tolist() == [N.ROW_PATH] * 2


def test_ring_neighbours_self_match_with_lines():
    """an identical line on both sides is a self match; a closed line against the polygon with the same
    vertex sequence is not (the part kinds differ), nor is the line with one more component"""
    left = LCol.from_geoms([line(SQ), poly([SQ])])
    right = LCol.from_wkb([geom_wkb(line(SQ), False), geom_wkb(poly([SQ])), geom_wkb(line(SQ, TRI)), geom_wkb(line(SQ[::-1]))])
    chips = (np.full(4, 7, np.int64), np.arange(4, dtype=np.int32))
    rows, cells = [0, 1], [7, 7]
    got, un = host_neighbours(chips, left, right, rows, cells)
    zero, four = 0, int(bits([4.0])[0])
    # line SQ: itself dropped; the polygon holds its first vertex (0); SQ + TRI shares SQ (0); reversed SQ (0)
    # polygon SQ: itself dropped; line SQ starts on its boundary (0); TRI lies inside it (0)
    assert got == [(0, 1, zero), (0, 2, zero), (0, 3, zero), (1, 0, zero), (1, 2, zero), (1, 3, zero)] and un == set()
    kept, _ = host_neighbours(chips, left, right, rows, cells, keep_self=True)
    assert [(l, c) for l, c, _ in kept] == [(l, c) for l in (0, 1) for c in range(4)] and all(b == zero for _, _, b in kept)
    lib = host_lib()
    assert lib.sdl_same_geometry(left.handle, 0, right.handle, 0) == 1 and lib.sdl_same_geometry(left.handle, 0, right.handle, 1) == 0
    assert lib.sdl_same_geometry(left.handle, 1, right.handle, 1) == 1 and lib.sdl_same_geometry(left.handle, 0, right.handle, 3) == 0
    # the distances are the kind-aware ones: a polygon inside a closed line is 4 away from it
    got, _ = host_neighbours((np.array([7], np.int64), np.array([0], np.int32)), LCol.from_geoms([poly([TRI])]),
                             LCol.from_geoms([line(SQ)]), [0], [7])
    assert got == [(0, 0, four)]


def test_python_plumbing_without_a_device():
    from mosaic_amd import SpatialKNN
    from mosaic_amd.context import _WKB_ROW_PATH, _wkt_row_wkb

    assert W.read_wkb(_WKB_ROW_PATH) == ("linestring", [[]])  # LINESTRING EMPTY: a served row once lines are
    texts = ["LINESTRING (0 0, 0 9)", "MULTILINESTRING ((50 0, 60 0), (0 0, 0 9))", "LINESTRING EMPTY", "MULTILINESTRING EMPTY",
             "MULTILINESTRING (EMPTY, (0 0, 0 9))", "POINT (3 4)", "GEOMETRYCOLLECTION EMPTY", "LINESTRING (0 0, 1", "POINT EMPTY",
             "LINESTRING (3 3)"]
    rows = [_wkt_row_wkb(t, lines=True) for t in texts]
    marker = rows[6]
    assert marker == rows[7] and marker != _WKB_ROW_PATH and marker not in rows[:6]
    assert struct.unpack(">BII", marker) == (0, 7, 0)  # GEOMETRYCOLLECTION EMPTY
    assert W.read_wkb(rows[0]) == ("linestring", [[(0.0, 0.0), (0.0, 9.0)]])
    assert W.read_wkb(rows[1]) == ("linestring", [[(50.0, 0.0), (60.0, 0.0)], [(0.0, 0.0), (0.0, 9.0)]])
    col = LCol.from_wkb(rows)
    st, facets = col.status()
    assert st.tolist() == [N.ROW_OK] * 6 + [N.ROW_PATH] * 4
    assert facets.tolist() == [1, 2, 0, 0, 1, 1, 0, 0, 0, 0]
    d = host_distance(col, LCol.from_geoms([pt(3, 4)] * len(rows)))
    assert d[:6].tolist() == [3.0, 3.0, 0.0, 0.0, 3.0, 0.0]
    # lines=False is the conversion as it was: line text is the LINESTRING EMPTY marker
    assert [_wkt_row_wkb(t) for t in texts[:5]] == [_WKB_ROW_PATH] * 5 and _wkt_row_wkb(texts[6]) == _WKB_ROW_PATH
    assert _wkt_row_wkb(texts[5]) == rows[5] == _wkt_row_wkb(texts[5], lines=False)
    # SpatialKNN takes a LineSet on the candidate side and says so when it is given something else
    trips = LineSet.from_lines([[[(0, 0), (1, 1)]]])
    model = SpatialKNN(None, trips, k_neighbours=3, index_resolution=8)
    assert model.candidates is trips
    with pytest.raises(TypeError, match="LineSet"):
        SpatialKNN(None, "LINESTRING (0 0, 1 1)", index_resolution=8)
    with pytest.raises(NotImplementedError):
        SpatialKNN(None, trips, index_resolution=8, approximate=False)


# ---- trips: seeded LineSets, their host columns and host line chips; the sides of the KNN cases ----
@functools.lru_cache(maxsize=None)
def trips(n):
    """n seeded 50-vertex random walks in the NYC bbox (the generator of tools/kbench_lines.py)"""
    from tools.kbench_lines import trips as make

    return make(n)


@functools.lru_cache(maxsize=None)
def trips_col(n):
    return LCol.from_lineset(trips(n))


def flat(g):
    """the geometry's flat content: part kinds, rings, vertex bytes"""
    if g[0] == "line":
        return tuple(("line", np.asarray(ln, np.float64).tobytes()) for ln in g[1] if ln)
    from tests.test_ring_neighbours import flat as flat_rn

    return flat_rn(g)


def line_side(ls, res):
    """a LineSet as a side of the KNN model (tests/test_ring_neighbours.py's Side): its host column and the
    host producer's line chips (Mosaic.lineFill, all non-core), from which Side draws the host k-rings"""
    from mosaic_amd.context import tessellate
    from tests.test_ring_neighbours import Side

    side = Side.__new__(Side)
    side.grid, side.res, side.geoms = "H3", res, ls
    side.models = [("line", ls.lines(g)) for g in range(len(ls))]
    side.col = LCol.from_lineset(ls)
    t = tessellate("H3", ls, res, ctx=None, cells_only=True)
    side.chips = (np.array(t["is_core"], np.uint8), np.array(t["index_id"], np.int64), np.array(t["polygon_key"], np.int32), len(ls))
    assert not side.chips[0].any()
    side.n = len(side.models)
    side.flat = [flat(g) for g in side.models]
    return side


@functools.lru_cache(maxsize=None)
def trips_side(n, res=8):
    return line_side(trips(n), res)


def restate(left, right, rows, cells, keep_self=False):
    """tests/test_ring_neighbours.py's (B) with the kind-aware host distance: ([(landmark, distance bits,
    candidate)] ordered, set of unmatched landmarks)"""
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


def literal_step(left, right):
    def step(active, it):
        rows, cells = left.ring_rows(it, active)
        want, un = restate(left, right, rows, cells)
        return [(l, c, float(np.array([b], np.int64).view(np.float64)[0])) for l, b, c in want], un
    return step


KNN_PARAMS = dict(k_neighbours=3, index_resolution=8, max_iterations=6)  # early stop 3, no threshold: the model's defaults
N_CANDIDATE_TRIPS = 200


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """(left Side, right Side, literal_knn's result) of the three line cases"""
    from tests.test_ring_neighbours import FLOAT_MAX, literal_knn, pickups64, zones8

    left, right = {"pickups-trips": (pickups64, lambda: trips_side(N_CANDIDATE_TRIPS)),
                   "zones-trips": (zones8, lambda: trips_side(N_CANDIDATE_TRIPS)),
                   "trips-pickups": (lambda: trips_side(64), pickups64)}[name]
    left, right = left(), right()
    lit = literal_knn(left.n, literal_step(left, right), KNN_PARAMS["k_neighbours"], KNN_PARAMS["max_iterations"], 3, FLOAT_MAX)
    return left, right, lit


def assert_knn_case_is_telling(lit):
    final, actives, M = lit
    assert len(actives) >= 2 and actives[1], "one iteration only"
    filled = {}
    for l, _, _, _, number in final:
        filled[l] = max(filled.get(l, 0), number)
    assert any(v == KNN_PARAMS["k_neighbours"] for v in filled.values()), "no landmark fills its k"


@pytest.mark.parametrize("it", (1, 2))
def test_host_pickups_against_trips(it):
    """rn::neighbours over line candidates against the Python restatement"""
    from tests.test_ring_neighbours import pickups64, reorder

    left, right = pickups64(), trips_side(N_CANDIDATE_TRIPS)
    rows, cells = left.ring_rows(it)
    want, want_un = restate(left, right, rows, cells)
    got, got_un = host_neighbours((right.chips[1], right.chips[2]), left.col, right.col, rows, cells)
    assert got == reorder(want) and got_un == want_un
    if it == 2:
        assert want and want_un


@pytest.mark.parametrize("name", ("pickups-trips", "zones-trips", "trips-pickups"))
def test_knn_line_cases_are_telling(name):
    left, right, lit = knn_case(name)
    assert_knn_case_is_telling(lit)
    final = lit[0]
    d = np.array([r[2] for r in final], np.int64).view(np.float64)
    assert not np.isnan(d).any()
    if name == "zones-trips":
        assert (d == 0).any() and (d > 0).any()  # trips that cross a zone or start inside it, and trips apart
