"""What tests/test_st_contains.py (CPU) and tests/test_gpu_st_contains.py share: the host library (H)
built from tests/native/st_contains_host.cpp, the exact oracle (E) and the case lists.

(E) is independent of the definition in mosaic_amd/csrc/st_contains.h: DE-9IM `T*****FF*` evaluated in
`fractions.Fraction` on a set of sample points that meets every cell of the arrangement of the two
geometries -- every segment of each side is noded at its intersection points with the other side's
segments; the nodes, the sub-segment midpoints, the points of point geometries and, next to every
sub-segment midpoint, one point strictly inside the face on either side of it are located in both
geometries.  contains(A, B) holds iff no sample that is in B (interior or boundary) is in A's exterior
and some sample is interior to both.  It assumes valid geometries (rings that do not cross, parts that
touch at single points), which is what the cases are.

Geometries are those of tests/test_st_distance_lines.py: ("point", ...), ("line", ...), ("polygon", ...).
"""
import ctypes
import functools
import math
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

from mosaic_amd import _native as N

from tests import test_st_distance as T
from tests.intersects_cases import all_pairs, circle, translated, vertices, zigzag
from tests.test_st_distance import HOLE, SQ, poly, pt
from tests.test_st_distance_lines import LCol, geom_wkb, line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_THREADS = T.HOST_THREADS
OK, UNDECIDED = N.ROW_OK, 3  # MOSAIC_ROW_OK, MOSAIC_PAIR_UNDECIDED
# contains::kHow* of st_contains.h
HOW_EMPTY, HOW_BOX, HOW_KINDS, HOW_POINTS_OUT, HOW_POINTS_IN, HOW_OUT, HOW_CLEAR, HOW_TOUCH = range(8)


# ---- (H) the host library ----
@functools.lru_cache(maxsize=None)
def host_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="sc_host_"), "libsc.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-pthread",
                    "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "native"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "st_contains_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.sc_contains.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i32]
    lib.sc_contains.restype = i32
    lib.sc_facet_contact.argtypes = [vp]
    lib.sc_facet_contact.restype = i32
    lib.si_intersects.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32]
    lib.si_intersects.restype = i32
    return lib


def host_contains(left, right, li=None, ri=None, threads=HOST_THREADS, return_how=False):
    """contains::contains over two columns (LCol): (out as bool, status), with return_how also the
    kHow* code of every pair (-1 on null and row-path rows)"""
    if li is None:
        assert left.n == right.n
        n = left.n
    else:
        li, ri = np.ascontiguousarray(li, np.int64), np.ascontiguousarray(ri, np.int64)
        n = len(li)
    out = np.full(max(n, 1), 7, np.uint8)
    st = np.full(max(n, 1), -1, np.int32)
    how = np.full(max(n, 1), -2, np.int32)
    rc = host_lib().sc_contains(left.handle, right.handle, N.ptr(li), N.ptr(ri), n, N.ptr(out), N.ptr(st), N.ptr(how), threads)
    if rc:
        assert (out == 7).all() and (st == -1).all()  # nothing written
        raise IndexError("row index out of range")
    assert set(out[:n].tolist()) <= {0, 1}
    assert not (out[:n][st[:n] != OK]).any()  # out is 0 wherever the status is not OK
    return (out[:n].astype(bool), st[:n], how[:n]) if return_how else (out[:n].astype(bool), st[:n])


def host_pair(a, b):
    """(out, status) of one pair"""
    out, st = host_contains(LCol.from_geoms([a]), LCol.from_geoms([b]))
    return bool(out[0]), int(st[0])


def host_facet_contact(p1, p2, q1, q2):
    c = np.array([*p1, *p2, *q1, *q2], np.float64)
    return int(host_lib().sc_facet_contact(N.ptr(c)))


def expected_split(st, how, work, small_work):
    """mosaic_st_contains_last_split's five counts from the host definition's statuses and kHow* codes and
    the pairs' work (facets x facets): ended in plan, decided by a crossing or something outside, decided
    without contact, undecided, served by a workgroup"""
    st, how, work = np.asarray(st), np.asarray(how), np.asarray(work, np.uint64)
    points = (how == HOW_POINTS_OUT) | (how == HOW_POINTS_IN)
    routed = ((how >= HOW_OUT) | (points & (work > small_work))) & (st != N.ROW_NULL) & (st != N.ROW_PATH)
    undecided = st == UNDECIDED
    return (int((~routed & ~undecided).sum()), int((routed & ((how == HOW_OUT) | (how == HOW_POINTS_OUT))).sum()),
            int((routed & ((how == HOW_CLEAR) | (how == HOW_POINTS_IN))).sum()), int(undecided.sum()),
            int((routed & (work > small_work)).sum()))


# ---- (E) exact ----
def _x(v):
    return (Fraction(v[0]), Fraction(v[1]))


def _cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _sign(v):
    return (v > 0) - (v < 0)


class _Ring:
    """a vertex list with a float copy for the y-range prefilter of `locate`"""

    def __init__(self, verts):
        self.v = [_x(p) for p in verts]
        f = np.array(verts, np.float64).reshape(-1, 2)
        self.ylo, self.yhi = np.minimum(f[:-1, 1], f[1:, 1]), np.maximum(f[:-1, 1], f[1:, 1])

    def edges_near(self, p):
        y = float(p[1])
        lo, hi = np.nextafter(y, -np.inf), np.nextafter(y, np.inf)
        return np.flatnonzero((self.ylo <= hi) & (self.yhi >= lo))

    def on(self, p):
        for i in self.edges_near(p):
            a, b = self.v[i], self.v[i + 1]
            if (_cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])):
                return True
        return False

    def locate(self, p):
        """1 inside, 0 on the ring, -1 outside"""
        if self.on(p):
            return 0
        inside = False
        for i in self.edges_near(p):
            a, b = self.v[i], self.v[i + 1]
            if (a[1] > p[1]) != (b[1] > p[1]):
                lo, hi = (a, b) if a[1] < b[1] else (b, a)
                if _cross(lo, hi, p) > 0:  # p is left of the upward edge: the ray to its right crosses it
                    inside = not inside
        return 1 if inside else -1


class _Geom:
    def __init__(self, g):
        self.kind, members = g
        self.points, self.lines, self.parts = [], [], []
        if self.kind == "point":
            self.points = [_x(p) for p in members]
        elif self.kind == "line":
            self.lines = [_Ring(ln) for ln in members if len(ln) >= 2]
        else:
            self.parts = [[_Ring(r) for r in part if len(r) >= 2] for part in members if part and len(part[0]) >= 2]
        self.rings = self.lines + [r for part in self.parts for r in part]
        self.segs = [(r.v[i], r.v[i + 1]) for r in self.rings for i in range(len(r.v) - 1)]
        allv = self.points + [p for r in self.rings for p in r.v]
        self.empty = not allv
        if allv:
            self.box = (min(p[0] for p in allv), min(p[1] for p in allv), max(p[0] for p in allv), max(p[1] for p in allv))
        # the segments as doubles (the inputs are doubles, so these are exact) for the prefilters
        self.f = np.array([[float(c) for p in s for c in p] for s in self.segs], np.float64).reshape(-1, 4)
        self.lo = np.minimum(self.f[:, :2], self.f[:, 2:])
        self.hi = np.maximum(self.f[:, :2], self.f[:, 2:])

    def in_box(self, p):
        return self.box[0] <= p[0] <= self.box[2] and self.box[1] <= p[1] <= self.box[3]

    def segs_in_box(self, lo, hi):
        """indices of the segments whose box meets the box lo .. hi (doubles: exact)"""
        return np.flatnonzero((self.lo[:, 0] <= hi[0]) & (self.hi[:, 0] >= lo[0]) & (self.lo[:, 1] <= hi[1]) & (self.hi[:, 1] >= lo[1]))

    def locate(self, p):
        """'I', 'B' or 'E'"""
        if self.kind == "point":
            return "I" if p in self.points else "E"
        if self.kind == "line":
            if not any(r.on(p) for r in self.lines):
                return "E"
            ends = sum((r.v[0] == p) + (r.v[-1] == p) for r in self.lines)  # the Mod-2 rule: a closed line has no boundary
            return "B" if ends % 2 else "I"
        seen = "E"
        for part in self.parts:
            loc = part[0].locate(p)
            if loc == 0:
                seen = "B"
            elif loc > 0:
                holes = [h.locate(p) for h in part[1:]]
                if 0 in holes:
                    seen = "B"
                elif 1 not in holes:
                    return "I"
        return seen


def _line_hits(m, m2, c, d):
    """the points of segment cd on the line through m and m2 (both ends if cd lies on it)"""
    d1, d2 = _cross(m, m2, c), _cross(m, m2, d)
    if d1 == 0 and d2 == 0:
        return [c, d]
    if _sign(d1) * _sign(d2) <= 0:
        s = Fraction(d1) / (d1 - d2)
        return [(c[0] + s * (d[0] - c[0]), c[1] + s * (d[1] - c[1]))]
    return []


def _node_params(a, b, other):
    """parameters t in [0, 1] of the points of segment ab that are intersection points with a segment of `other`"""
    if a == b:
        return [Fraction(0)]
    ts = {Fraction(0), Fraction(1)}
    dx, dy = b[0] - a[0], b[1] - a[1]
    l2 = dx * dx + dy * dy
    fa, fb = (float(a[0]), float(a[1])), (float(b[0]), float(b[1]))
    for k in other.segs_in_box((min(fa[0], fb[0]), min(fa[1], fb[1])), (max(fa[0], fb[0]), max(fa[1], fb[1]))):
        for p in _line_hits(a, b, *other.segs[k]):
            t = Fraction((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) / l2
            if 0 <= t <= 1:
                ts.add(t)
    return sorted(ts)


def _face_point(m, n, geoms):
    """a point m + tau n, tau > 0, with nothing of the geometries on the open way from m to it or at it"""
    best = None
    m2 = (m[0] + n[0], m[1] + n[1])
    nn = n[0] * n[0] + n[1] * n[1]
    mf, nf = (float(m[0]), float(m[1])), (float(n[0]), float(n[1]))
    for g in geoms:
        if not len(g.f):
            continue
        # doubles first: the signed areas of the segments' ends against the ray's line, with a generous margin
        d1 = nf[0] * (g.f[:, 1] - mf[1]) - nf[1] * (g.f[:, 0] - mf[0])
        d2 = nf[0] * (g.f[:, 3] - mf[1]) - nf[1] * (g.f[:, 2] - mf[0])
        tol = 1e-9 * (abs(nf[0]) + abs(nf[1])) * (np.abs(g.f - np.tile(mf, 2)).max() + 1.0)
        for k in np.flatnonzero(((d1 <= tol) & (d2 >= -tol)) | ((d1 >= -tol) & (d2 <= tol))):
            for p in _line_hits(m, m2, *g.segs[k]):
                tau = Fraction((p[0] - m[0]) * n[0] + (p[1] - m[1]) * n[1]) / nn
                if tau > 0 and (best is None or tau < best):
                    best = tau
    tau = Fraction(1) if best is None else best / 2
    return (m[0] + tau * n[0], m[1] + tau * n[1])


def _samples(ga, gb):
    """the sample points that can lie in B: those of B's cells, and those of A's cells inside B's box"""
    pts = [p for p in ga.points if gb.in_box(p)] + list(gb.points)
    areal = bool(ga.parts) or bool(gb.parts)
    blo, bhi = (float(gb.box[0]), float(gb.box[1])), (float(gb.box[2]), float(gb.box[3]))
    for x, y, idx in ((ga, gb, ga.segs_in_box(blo, bhi)), (gb, ga, range(len(gb.segs)))):
        for k in idx:
            a, b = x.segs[k]
            ts = _node_params(a, b, y)
            nodes = [(a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])) for t in ts]
            pts.extend(nodes)
            for p, q in zip(nodes, nodes[1:]):
                m = ((p[0] + q[0]) / 2, (p[1] + q[1]) / 2)
                if not gb.in_box(m):
                    continue
                pts.append(m)
                if areal:
                    n = (-(b[1] - a[1]), b[0] - a[0])
                    pts.append(_face_point(m, n, (ga, gb)))
                    pts.append(_face_point(m, (-n[0], -n[1]), (ga, gb)))
    return pts


@functools.lru_cache(maxsize=64)
def _geom_of(g):
    return _Geom(g)


@functools.lru_cache(maxsize=None)
def _exact_contains(a, b):
    ga, gb = _geom_of(a), _geom_of(b)
    if ga.empty or gb.empty:
        return False
    if gb.box[0] < ga.box[0] or gb.box[1] < ga.box[1] or gb.box[2] > ga.box[2] or gb.box[3] > ga.box[3]:
        return False  # a point of B outside A's box is in A's exterior
    shared = False
    for p in _samples(ga, gb):
        if not gb.in_box(p):
            continue
        lb = gb.locate(p)
        if lb == "E":
            continue
        la = ga.locate(p)
        if la == "E":
            return False
        if la == "I" and lb == "I":
            shared = True
    return shared


def _frozen(g):
    kind, members = g
    if kind == "point":
        return (kind, tuple(tuple(p) for p in members))
    if kind == "line":
        return (kind, tuple(tuple(tuple(p) for p in ln) for ln in members))
    return (kind, tuple(tuple(tuple(tuple(p) for p in ring) for ring in part) for part in members))


def exact_contains(a, b):
    """(E): JTS Geometry.contains(a, b) as DE-9IM T*****FF*, exactly"""
    return _exact_contains(_frozen(a), _frozen(b))


@functools.lru_cache(maxsize=None)
def _exact_touch(a, b):
    ga, gb = _Geom(a), _Geom(b)
    for g in (ga, gb):  # points count as zero-length segments
        g.segs = g.segs + [(p, p) for p in g.points]
        g.f = np.array([[float(c) for p in s for c in p] for s in g.segs], np.float64).reshape(-1, 4)
        g.lo, g.hi = np.minimum(g.f[:, :2], g.f[:, 2:]), np.maximum(g.f[:, :2], g.f[:, 2:])
    for k, (p, q) in enumerate(ga.segs):
        for j in gb.segs_in_box(ga.lo[k], ga.hi[k]):
            r, s = gb.segs[j]
            if T._segments_meet(p, q, r, s):
                o = [_sign(_cross(p, q, r)), _sign(_cross(p, q, s)), _sign(_cross(r, s, p)), _sign(_cross(r, s, q))]
                if not (o[0] * o[1] < 0 and o[2] * o[3] < 0):
                    return True
    return False


def exact_touch_without_crossing(a, b):
    """some segment of a meets a segment of b in a way that is not a proper crossing (the contact that
    the clean generator excludes), exactly"""
    return _exact_touch(_frozen(a), _frozen(b))


# ---- hand-made cases: (name, A, B, status, out, oracle, swapped status) ----
# `out` is what the engine must say for contains(A, B): the oracle's value where the status is OK, 0 where
# it is UNDECIDED; `oracle` records (E)'s value, which a later change that decides the touching pairs will
# need.  Every case also runs as contains(B, A) with the pinned `swapped status`.
SMALL = [(2, 2), (4, 2), (4, 4), (2, 4), (2, 2)]
TRI = [(4, 4), (6, 4), (6, 6), (4, 4)]
FAR = [(50, 50), (60, 50), (60, 60), (50, 50)]
NEXT = [(10, 10), (20, 10), (20, 20), (10, 20), (10, 10)]  # shares the vertex (10 10) with SQ
NOTCH = [(0, 0), (10, 0), (10, 10), (6, 10), (5, 4), (4, 10), (0, 10), (0, 0)]  # SQ with a notch from the top down to (5 4)
ULP = float(np.nextafter(10.0, 11.0))
HAND = (
    # decided 1
    ("square in square", poly([SQ]), poly([SMALL]), OK, 1, 1, OK),
    ("building in a zone with a hole, beside the hole", poly([SQ, HOLE]), poly([[(1, 1), (2, 1), (2, 2), (1, 2), (1, 1)]]), OK, 1, 1, OK),
    ("line inside", poly([SQ]), line([(1, 1), (5, 2), (8, 8)]), OK, 1, 1, OK),
    ("multiline inside a zone with a hole", poly([SQ, HOLE]), line([(1, 1), (1, 9)], [(8, 1), (9, 9), (8, 9)]), OK, 1, 1, OK),
    ("multipoint inside", poly([SQ, HOLE]), pt(1, 1, 8, 8, 2, 5), OK, 1, 1, OK),
    ("multipoint inside and on the boundary", poly([SQ]), pt(0, 5, 1, 1), OK, 1, 1, OK),
    ("polygon inside one part of a multipolygon", poly([FAR], [SQ]), poly([[(1, 1), (2, 1), (2, 2), (1, 1)]]), OK, 1, 1, OK),
    ("multipolygon inside two parts of a multipolygon", poly([SQ], [[(20, 0), (30, 0), (30, 10), (20, 10), (20, 0)]]),
     poly([SMALL], [[(22, 2), (24, 2), (24, 4), (22, 2)]]), OK, 1, 1, OK),
    ("a polygon with a hole, beside the zone's hole", poly([SQ, HOLE]),
     poly([[(0.5, 0.5), (2.5, 0.5), (2.5, 2.5), (0.5, 2.5), (0.5, 0.5)], [(1, 1), (2, 1), (2, 2), (1, 1)]]), OK, 1, 1, OK),
    ("an annulus around the zone's hole, which lies in the annulus' hole", poly([SQ, HOLE]),
     poly([[(1, 1), (9, 1), (9, 9), (1, 9), (1, 1)], [(2, 2), (8, 2), (8, 8), (2, 8), (2, 2)]]), OK, 1, 1, OK),
    # decided 0
    ("a crossing line", poly([SQ, HOLE]), line([(1, 5), (9, 5)]), OK, 0, 0, OK),
    ("a crossing line leaving the box", poly([SQ]), line([(5, 5), (15, 5)]), OK, 0, 0, OK),
    ("a polygon overlapping an edge", poly([SQ, HOLE]), poly([[(1, 4), (5, 4), (5, 6), (1, 6), (1, 4)]]), OK, 0, 0, OK),
    ("a polygon overlapping an edge of a notch", poly([NOTCH]), poly([[(3, 7), (7, 7), (7, 9), (3, 9), (3, 7)]]), OK, 0, 0, OK),
    ("B covering a hole of A without touching it", poly([SQ, HOLE]), poly([[(2, 2), (8, 2), (8, 8), (2, 8), (2, 2)]]), OK, 0, 0, OK),
    ("B inside a hole of A", poly([SQ, HOLE]), poly([TRI]), OK, 0, 0, OK),
    ("a line inside a hole of A", poly([SQ, HOLE]), line([(4, 4), (6, 5)]), OK, 0, 0, OK),
    ("B with its first vertex inside and a later one outside", poly([SQ, HOLE]), line([(1, 1), (5, 5)]), OK, 0, 0, OK),
    ("a polygon with its first vertex inside and a later one outside", poly([SQ, HOLE]),
     poly([[(1, 1), (2, 1), (5, 5), (1, 2), (1, 1)]]), OK, 0, 0, OK),
    ("a line through a notch with a vertex outside", poly([NOTCH]), line([(2, 8), (5, 8), (8, 8)]), OK, 0, 0, OK),
    ("a line through a notch without a vertex outside", poly([NOTCH]), line([(2, 8), (8, 8)]), OK, 0, 0, OK),
    ("a second part outside", poly([FAR], [SQ]), poly([SMALL], [[(20, 20), (30, 20), (30, 30), (20, 20)]]), OK, 0, 0, OK),
    ("multipoint: one point outside", poly([SQ, HOLE]), pt(1, 1, 5, 5), OK, 0, 0, OK),
    ("multipoint: all points on the boundary", poly([SQ, HOLE]), pt(0, 5, 10, 5, 3, 5), OK, 0, 0, OK),
    ("a point on the shared vertex of two parts", poly([SQ], [NEXT]), pt(10, 10), OK, 0, 0, OK),
    ("LINESTRING EMPTY on the right", poly([SQ]), line([]), OK, 0, 0, OK),
    ("POLYGON EMPTY on the left", poly([]), pt(1, 1), OK, 0, 0, OK),
    ("two empties", line(), ("point", []), OK, 0, 0, OK),
    ("B's box sticking out of A's box by one ulp", poly([SQ]), poly([[(1, 1), (ULP, 5), (1, 9), (1, 1)]]), OK, 0, 0, OK),
    ("a point one ulp outside", poly([SQ]), pt(ULP, 5), OK, 0, 0, OK),
    # undecided: the boundaries touch, nothing crosses, no vertex is outside
    ("A with itself", poly([SQ]), poly([SQ]), UNDECIDED, 0, 1, UNDECIDED),
    ("B sharing an edge from inside", poly([SQ]), poly([[(0, 2), (4, 2), (4, 6), (0, 6), (0, 2)]]), UNDECIDED, 0, 1, OK),
    ("a line ending on the boundary from inside", poly([SQ]), line([(5, 5), (10, 5)]), UNDECIDED, 0, 1, OK),
    ("a line running along the boundary", poly([SQ]), line([(2, 0), (8, 0)]), UNDECIDED, 0, 0, OK),
    ("B filling a hole of A exactly", poly([SQ, HOLE]), poly([HOLE]), UNDECIDED, 0, 0, OK),
    ("a line touching a hole's vertex from inside", poly([SQ, HOLE]), line([(1, 1), (3, 3)]), UNDECIDED, 0, 1, OK),
    # undecided: the left side is not polygonal and the right side not points only
    ("a line on a line", line([(0, 0), (10, 0)]), line([(2, 0), (8, 0)]), UNDECIDED, 0, 1, OK),
    ("a point in a line", line([(0, 0), (10, 0)]), pt(5, 0), UNDECIDED, 0, 1, OK),
    ("a zero-length line on a multipoint", pt(1, 1, 2, 2), line([(1, 1), (1, 1)]), UNDECIDED, 0, 1, OK),
    ("a closed line around a polygon", line(SQ), poly([SMALL]), UNDECIDED, 0, 0, OK),
    # degenerate facets: the list of st_intersects.h
    ("a point on a vertex", poly([SQ]), pt(10, 0), OK, 0, 0, OK),
    ("a point on a segment's interior", poly([SQ]), pt(4, 0), OK, 0, 0, OK),
    ("a point on a segment's interior and one inside", poly([SQ]), pt(4, 0, 5, 5), OK, 1, 1, OK),
    ("a point on a hole's ring", poly([SQ, HOLE]), pt(3, 5), OK, 0, 0, OK),
    ("a zero-length line inside", poly([SQ]), line([(3, 4), (3, 4)]), OK, 1, 1, OK),
    ("a zero-length line on the boundary", poly([SQ]), line([(10, 5), (10, 5)]), UNDECIDED, 0, 0, OK),
    ("a zero-length line outside, in the box", poly([NOTCH]), line([(5, 8), (5, 8)]), OK, 0, 0, OK),
    ("two equal points", pt(3, 4), pt(3, 4), OK, 1, 1, OK),
    ("a multipoint holding a point", pt(3, 4, 5, 5), pt(5, 5), OK, 1, 1, OK),
    ("a multipoint missing a point", pt(3, 4, 6, 6), pt(3, 4, 4, 5), OK, 0, 0, OK),
    ("minus zero equals zero", pt(0.0, 1, 2, 2), pt(-0.0, 1), OK, 1, 1, OK),
)


def hand_pairs():
    """(A, B) of every hand-made case, then (B, A) of every case"""
    return tuple((c[1], c[2]) for c in HAND) + tuple((c[2], c[1]) for c in HAND)


# ---- shapes for the workgroup kernel: a zone of 300 + 40 vertices against buildings of 5 and a trip of 130 ----
@functools.lru_cache(maxsize=None)
def kernel_cases():
    """(name, A, B): a ring beyond one 256-lane sweep; expectations come from (E) and from (H)"""
    zone = poly([circle(300, 1000), circle(40, 200, cx=300)])

    def box(cx, cy, h):
        return poly([[(cx - h, cy - h), (cx + h, cy - h), (cx + h, cy + h), (cx - h, cy + h), (cx - h, cy - h)]])

    trip_in = line(zigzag(130, -650, -301, dx=4, dy=7))
    trip_hole = line(zigzag(130, -230, 1, dx=7, dy=5))          # runs through the hole
    trip_out = line(zigzag(130, 500, 601, dx=3, dy=9))          # ends beyond the shell, inside its box
    cases = [
        ("building inside", zone, box(-401, 3, 7)),
        ("building inside the hole", zone, box(301, 1, 9)),
        ("building across the shell", zone, box(707, 705, 30)),
        ("building across the hole's ring", zone, box(101, 3, 15)),
        ("building covering the hole", zone, box(301, 1, 251)),
        ("building outside, in the box's corner", zone, box(901, 901, 9)),
        ("trip of 130 inside", zone, trip_in),
        ("trip of 130 through the hole", zone, trip_hole),
        ("trip of 130 leaving through the shell", zone, trip_out),
        ("the zone with itself", zone, zone),
        ("multipoint of 60 inside", zone, pt(*[c for k in range(60) for c in (-700 + 7 * k, -5 * k + 11)])),
        ("multipoint of 60, the last one in the hole", zone, pt(*[c for k in range(59) for c in (-700 + 7 * k, -5 * k + 11)], 300, 0)),
        ("multipoint of 60, all on the shell's vertices", zone, pt(*[c for v in circle(300, 1000)[:60] for c in v])),
        ("multipoints of 60 and 59", pt(*[c for k in range(60) for c in (3 * k, 2 * k)]), pt(*[c for k in range(59) for c in (3 * k, 2 * k)])),
        ("multipoints of 60 and 59, one missing", pt(*[c for k in range(60) for c in (3 * k, 2 * k)]),
         pt(*[c for k in range(58) for c in (3 * k, 2 * k)], 3, 3)),
        ("a 40-ring in the 300-ring, hole uncovered", poly([circle(300, 1000)]), poly([circle(40, 200, cx=300)])),
    ]
    return tuple(cases)


# ---- generated cases ----
def _lattice(ring, odd):
    """the ring's vertices moved to the even or the odd integer lattice, consecutive duplicates dropped"""
    out = []
    for x, y in ring:
        v = (2.0 * round((x - odd) / 2) + odd, 2.0 * round((y - odd) / 2) + odd)
        if not out or out[-1] != v:
            out.append(v)
    return out


def _star(rng, cx, cy, radius, n, odd, lo=0.6):
    ring = _lattice(T.star(rng, cx, cy, radius, n, lo=lo)[:-1], odd)
    if ring[0] == ring[-1]:
        ring.pop()
    return ring + ring[:1]


def _walk(rng, cx, cy, radius, n):
    v = np.array([cx, cy]) + rng.uniform(-radius, radius, (n, 2)) * 0.7
    return _lattice([tuple(p) for p in v], 1)


def _simple(ring):
    """no two non-adjacent segments of the closed ring meet, and no zero-length segment"""
    seg = list(zip(ring, ring[1:]))
    n = len(seg)
    if n < 3 or any(a == b for a, b in seg):
        return False
    for i in range(n):
        for j in range(i + 2, n):
            if i == 0 and j == n - 1:
                continue
            if T._segments_meet(T.exact(seg[i][0]), T.exact(seg[i][1]), T.exact(seg[j][0]), T.exact(seg[j][1])):
                return False
    return True


PLACES = ("inside", "inside", "inside", "in the hole", "around the hole", "across the shell", "across the hole", "in the box's corner", "far")


def _clean_pair(rng, k):
    radius = float(rng.integers(300, 900))
    cx, cy = (float(v) for v in rng.integers(-2000, 2000, 2))
    n = int(rng.integers(5, 40))
    shell = _star(rng, cx, cy, radius, n, 0)
    hx, hy, hr = cx + 0.3 * radius, cy, 0.12 * radius
    with_hole = k % 3 != 0
    rings = [shell] + ([_star(rng, hx, hy, hr, int(rng.integers(4, 12)), 0)] if with_hole else [])
    parts = [rings]
    if k % 5 == 0:  # a second part, far to the right
        parts.append([_star(rng, cx + 3 * radius, cy, 0.5 * radius, int(rng.integers(5, 16)), 0)])
    zone = poly(*parts)
    place = PLACES[int(rng.integers(0, len(PLACES)))]
    if not with_hole and "hole" in place:
        place = "inside"
    r = 0.05 * radius
    if place == "inside":
        bx, by = cx - 0.3 * radius, cy + float(rng.uniform(-0.1, 0.1)) * radius
        r = float(rng.uniform(0.03, 0.12)) * radius
    elif place == "in the hole":
        bx, by, r = hx, hy, 0.3 * hr
    elif place == "around the hole":
        bx, by, r = hx, hy, 2.2 * hr
    elif place == "across the shell":
        bx, by = shell[int(rng.integers(0, len(shell) - 1))]
        r = float(rng.uniform(0.05, 0.15)) * radius
    elif place == "across the hole":
        bx, by = hx + hr * 0.8, hy
        r = 0.5 * hr
    elif place == "in the box's corner":
        bx, by = cx + 0.93 * radius * (1 if rng.integers(0, 2) else -1), cy + 0.93 * radius * (1 if rng.integers(0, 2) else -1)
        r = 0.03 * radius
    else:
        bx, by = cx + 4.0 * radius, cy - 2.0 * radius
    if k % 4 == 3:
        b = line(_walk(rng, bx, by, r, int(rng.integers(2, 9))))
        if any(p == q for p, q in zip(b[1][0], b[1][0][1:])) or len(b[1][0]) < 2:
            return None
    else:
        nb = int(rng.integers(4, 12))
        ring = _star(rng, bx, by, r, max(nb, 9) if place == "around the hole" else nb, 1, lo=0.75 if place == "around the hole" else 0.6)
        if not _simple(ring):
            return None
        b = poly([ring])
    if not all(_simple(ring) for part in zone[1] for ring in part):
        return None
    if with_hole and (exact_touch_or_cross_rings(shell, rings[1]) or
                      T._ring_locate([T.exact(v) for v in shell], T.exact(rings[1][0])) != 1):
        return None  # the hole lies strictly inside the shell
    if exact_touch_without_crossing(zone, b):
        return None  # the clean set holds no contact without a crossing
    return zone, b, place


def exact_touch_or_cross_rings(r1, r2):
    return any(T._segments_meet(T.exact(a), T.exact(b), T.exact(c), T.exact(d)) for a, b in zip(r1, r1[1:]) for c, d in zip(r2, r2[1:]))


@functools.lru_cache(maxsize=None)
def clean_pairs(n=240, seed=20251101):
    """(zone, building or line, placement): zones on the even integer lattice, buildings and lines on the odd
    one, placed strictly inside, strictly outside or across the zone's rings; a draw with a contact that is
    no proper crossing (a vertex on an edge, an edge through a vertex) is drawn again"""
    rng = np.random.default_rng(seed)
    out, k = [], 0
    while len(out) < n:
        p = _clean_pair(rng, k)
        k += 1
        if p is not None:
            out.append(p)
    return tuple(out)


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


@functools.lru_cache(maxsize=None)
def lattice_pairs(n=300, seed=20251102):
    """(A, B) on one coarse lattice (0 .. 12), so touches abound: rectangles, rectangles with a rectangular
    hole, two-part multipolygons, short lines and multipoints on either side"""
    rng = np.random.default_rng(seed)

    def span(lo, hi, least=1):
        a = int(rng.integers(lo, hi - least + 1))
        return a, int(rng.integers(a + least, hi + 1))

    def shape(big):
        kind = int(rng.integers(0, 10))
        lo, hi = (0, 12) if big else (1, 11)
        x0, x1 = span(lo, hi, 4 if big else 1)
        y0, y1 = span(lo, hi, 4 if big else 1)
        if kind < 5 or (big and kind < 8):
            rings = [_rect(x0, y0, x1, y1)]
            if x1 - x0 >= 4 and y1 - y0 >= 4 and rng.integers(0, 2):
                hx0, hx1 = span(x0 + 1, x1 - 1)
                hy0, hy1 = span(y0 + 1, y1 - 1)
                rings.append(_rect(hx0, hy0, hx1, hy1))
            if big and kind == 7 and x1 <= 10 and y1 <= 10:
                return poly(rings, [_rect(x1, y1, 12, 12)])  # a second part that touches the first at a vertex
            return poly(rings)
        if kind < 8 or (big and kind == 8):
            k = int(rng.integers(2, 5))
            v = [(float(rng.integers(x0, x1 + 1)), float(rng.integers(y0, y1 + 1))) for _ in range(k)]
            v = [p for i, p in enumerate(v) if i == 0 or p != v[i - 1]]
            return line(v) if len(v) >= 2 else pt(*v[0])
        k = int(rng.integers(1, 4))
        return pt(*[float(c) for _ in range(k) for c in (rng.integers(x0, x1 + 1), rng.integers(y0, y1 + 1))])

    return tuple((shape(True), shape(False)) for _ in range(n))


# ---- buildings against the 35 NYC zones: real coordinates, for the end-to-end test ----
@functools.lru_cache(maxsize=None)
def zone_buildings(n=150, seed=20251103):
    """(zones as a PolygonSet, buildings, contained): star-shaped buildings of 4 to 8 vertices on the 2^-24
    degree lattice, around a point of a zone's box, around a vertex of its shell (across the boundary), or
    far away; contained[k] = the zones that (E) says contain building k.  Only zones whose box covers the
    building's are put to (E): a building that sticks out of a zone's box is not contained."""
    from mosaic_amd.data import PolygonSet

    zones = PolygonSet.load("nyc_taxi_zones_35")
    geoms = [_frozen(("polygon", zones.parts(g))) for g in range(len(zones))]
    boxes = []
    for g in geoms:
        v = np.array([p for part in g[1] for ring in part for p in ring])
        boxes.append((v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()))
    rng = np.random.default_rng(seed)
    q = 2.0 ** -24
    buildings, contained = [], []
    while len(buildings) < n:
        z = int(rng.integers(0, len(zones)))
        x0, y0, x1, y1 = boxes[z]
        mode = int(rng.integers(0, 4))
        if mode < 2:
            cx, cy = rng.uniform(x0, x1), rng.uniform(y0, y1)
        elif mode == 2:
            shell = geoms[z][1][0][0]
            cx, cy = shell[int(rng.integers(0, len(shell)))]
        else:
            cx, cy = x1 + 0.5, y1 + 0.5
        r = float(rng.uniform(5e-5, 6e-4))
        k = int(rng.integers(4, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.6 * r, r, k)
        ring = [(float(np.round((cx + a * math.cos(t)) / q) * q), float(np.round((cy + a * math.sin(t)) / q) * q)) for a, t in zip(rad, ang)]
        ring = ring + ring[:1]
        if not _simple(ring):
            continue
        b = poly([ring])
        bx = np.array(ring)
        inside = [g for g in range(len(zones)) if boxes[g][0] <= bx[:, 0].min() and boxes[g][1] <= bx[:, 1].min() and
                  boxes[g][2] >= bx[:, 0].max() and boxes[g][3] >= bx[:, 1].max()]
        if any(exact_touch_without_crossing(geoms[g], b) for g in inside):
            continue  # clean: no contact without a crossing (it does not happen on these coordinates)
        buildings.append(b)
        contained.append(tuple(g for g in inside if exact_contains(geoms[g], b)))
    return zones, tuple(buildings), tuple(contained)


@functools.lru_cache(maxsize=None)
def all_cases():
    """every case list as (left geometries, right geometries): hand-made both ways, kernel shapes, clean, lattice"""
    pairs = list(hand_pairs()) + [(c[1], c[2]) for c in kernel_cases()] + [(a, b) for a, b, _ in clean_pairs()] + list(lattice_pairs())
    return tuple(a for a, _ in pairs), tuple(b for _, b in pairs)


@functools.lru_cache(maxsize=None)
def case_rows():
    """all_cases as WKB rows in alternating byte orders, with (H) on them: (rows_l, rows_r, out, status, how, work)"""
    left, right = all_cases()
    rows_l = [geom_wkb(g, bool(i % 2)) for i, g in enumerate(left)]
    rows_r = [geom_wkb(g, bool(i % 3)) for i, g in enumerate(right)]
    hl, hr = LCol.from_wkb(rows_l), LCol.from_wkb(rows_r)
    out, st, how = host_contains(hl, hr, return_how=True)
    work = hl.status()[1].astype(np.uint64) * hr.status()[1].astype(np.uint64)
    return rows_l, rows_r, out, st, how, work
