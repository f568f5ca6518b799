"""What tests/test_st_intersects.py (CPU) and tests/test_gpu_st_intersects.py share: the host library
(H) built from tests/native/st_intersects_host.cpp, the exact oracle (E) and the case lists.

(E) is independent of the code under test: tests/test_st_distance.py's `_segments_meet` / `_in_part`
on integers and Fractions.  Two geometries intersect iff two facets meet or some vertex -- every
vertex is tried, not only a component's first -- lies in or on a polygon part of the other side.

Geometries are those of tests/test_st_distance_lines.py: ("point", ...), ("line", ...), ("polygon", ...).
"""
import ctypes
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

from mosaic_amd import _native as N

from tests import test_st_distance as T
from tests import test_st_distance_lines as TL
from tests.test_st_distance import HOLE, SQ, poly, pt
from tests.test_st_distance_lines import LCol, geom_wkb, line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_THREADS = T.HOST_THREADS
KINDS = ("point", "multipoint", "line", "multiline", "polygon", "multipolygon")


# ---- (H) the host library ----
@functools.lru_cache(maxsize=None)
def host_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="si_host_"), "libsi.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-pthread",
                    "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "st_intersects_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.si_intersects.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32]
    lib.si_intersects.restype = i32
    lib.si_segments_intersect.argtypes = [vp]
    lib.si_segments_intersect.restype = i32
    lib.sdl_distance.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32]
    lib.sdl_distance.restype = i32
    return lib


def host_intersects(left, right, li=None, ri=None, threads=HOST_THREADS, return_status=False):
    """isect::intersects over two columns (LCol: the GeomColumn behind the handle is the one this
    library was compiled with)"""
    if li is None:
        assert left.n == right.n
        n = left.n
    else:
        li, ri = np.ascontiguousarray(li, np.int64), np.ascontiguousarray(ri, np.int64)
        n = len(li)
    out = np.full(max(n, 1), 7, np.uint8)
    st = np.full(max(n, 1), -1, np.int32)
    rc = host_lib().si_intersects(left.handle, right.handle, N.ptr(li), N.ptr(ri), n, N.ptr(out), N.ptr(st), threads)
    if rc:
        assert (out == 7).all() and (st == -1).all()  # nothing written
        raise IndexError("row index out of range")
    assert set(out[:n].tolist()) <= {0, 1}
    return (out[:n].astype(bool), st[:n]) if return_status else out[:n].astype(bool)


def host_pair(a, b):
    return bool(host_intersects(LCol.from_geoms([a]), LCol.from_geoms([b]))[0])


def host_segments_intersect(p1, p2, q1, q2):
    c = np.array([*p1, *p2, *q1, *q2], np.float64)
    return bool(host_lib().si_segments_intersect(N.ptr(c)))


# ---- (E) exact ----
def components(g):
    """[(is_polygon, rings)]: a point is one ring of one vertex, a component line one open ring"""
    kind, members = g
    if kind == "point":
        return [(False, [[p]]) for p in members]
    if kind == "line":
        return [(False, [ln]) for ln in members if ln]
    return [(True, [r for r in part if r]) for part in members if part and part[0]]


def exact_facets(g):
    out = []
    for _, rings in components(g):
        for ring in rings:
            e = [T.exact(v) for v in ring]
            out.extend([(e[0], e[0])] if len(e) == 1 else list(zip(e, e[1:])))
    return out


def exact_intersects(a, b):
    fa, fb = exact_facets(a), exact_facets(b)
    if not fa or not fb:
        return False
    if any(T._segments_meet(p, q, r, s) for p, q in fa for r, s in fb):
        return True
    for x, y in ((a, b), (b, a)):
        parts = [[[T.exact(v) for v in ring] for ring in rings] for is_poly, rings in components(x) if is_poly]
        verts = [T.exact(v) for _, rings in components(y) for ring in rings for v in ring]
        if any(T._in_part(part, v) for part in parts for v in verts):
            return True
    return False


# ---- the truth table: a small shape of every kind placed against a big shape of every kind ----
# The small shape hangs on an anchor P and lies in the cone P + s d + t n, s >= t >= 0: the point P, the
# line P, P + 2d, P + 2d + 2n, or the triangle on those three.  A multi kind puts a far decoy first, so
# the only hit is on the last member.
SPIKE = [(0, 0), (10, 0), (10, 10), (14, 14), (0, 10), (0, 0)]  # SQ with a spike: its box is larger than it
BIG_LINE = [(0, 0), (10, 0), (10, 10)]


def small(kind, P, d=(1, 0), n=(0, 1)):
    base = kind.replace("multi", "")

    def one(P):
        a = np.array(P, float)
        b = a + 2 * np.array(d, float)
        c = b + 2 * np.array(n, float)
        a, b, c = tuple(a.tolist()), tuple(b.tolist()), tuple(c.tolist())
        return a if base == "point" else [a, b, c] if base == "line" else [[a, b, c, a]]

    members = ([one((-200, -200))] if kind.startswith("multi") else []) + [one(P)]
    if base == "point":
        return pt(*[c for m in members for c in m])
    return line(*members) if base == "line" else poly(*members)


def big(kind):
    base = kind.replace("multi", "")
    multi = kind.startswith("multi")
    if base == "point":
        return pt(300, 300, 10, 10) if multi else pt(10, 10)
    if base == "line":
        return line([(300, 300), (310, 300)], BIG_LINE) if multi else line(BIG_LINE)
    decoy = [[(300, 300), (310, 300), (310, 310), (300, 300)]]
    return poly(decoy, [SPIKE, HOLE]) if multi else poly([SPIKE, HOLE])


def _situations(ks, kb):
    """(situation, anchor, d, n, expected) for a small shape of kind ks against big(kb)"""
    s, b = ks.replace("multi", ""), kb.replace("multi", "")
    out = [("disjoint, disjoint boxes", (-50, -50), (1, 0), (0, 1), False)]
    if b == "point":
        if s == "point":
            if ks != "point" or kb != "point":  # the boxes of two single points meet only if the points are equal
                out.append(("disjoint, meeting boxes", (12, 12), (1, 0), (0, 1), False))
        else:
            out.append(("disjoint, meeting boxes", (9, 8.5), (1, 0), (0, 1), False))
        out.append(("touching at a vertex", (10, 10), (1, 0), (0, 1), True))
        return out
    out.append(("disjoint, meeting boxes", (2, 4) if b == "line" else (11.5, 2), (1, 0), (0, 1), False))
    if b == "line":
        out.append(("touching at a vertex", (10, 10), (1, 0), (0, 1), True))
    else:
        out.append(("touching at a vertex", (10, 0), (1, 0), (0, -1), True))
    out.append(("touching along an edge", (3, 0), (1, 0), (0, -1), True))  # a point: on the edge's interior
    if s != "point":
        out.append(("crossing", (4, -1), (0, 1), (1, 0), True))
    if b == "polygon":
        out.append(("contained without boundary contact", (0.5, 0.5), (1, 0), (0, 1), True))
        out.append(("inside a hole", (4, 4), (1, 0), (0, 1), False))
        out.append(("on a hole's ring", (3, 4), (1, 0), (0, 1), True))
    return out


@functools.lru_cache(maxsize=None)
def truth_table():
    """(name, left, right, expected): every situation in both orders"""
    cases = []
    for ks in KINDS:
        for kb in KINDS:
            for name, P, d, n, want in _situations(ks, kb):
                a, b = small(ks, P, d, n), big(kb)
                cases.append((f"{ks} / {kb}: {name}", a, b, want))
                cases.append((f"{kb} / {ks}: {name}, the big shape first", b, a, want))
    return tuple(cases)


def kind_name(g):
    return ("multi" if len(g[1]) != 1 else "") + g[0]


TRI = [(4, 4), (6, 4), (6, 6), (4, 4)]
FAR = [(50, 50), (60, 50), (60, 60), (50, 50)]
EXPLICIT = (
    # docs/source/api/spatial-functions.rst gives POLYGON ((0 0, 0 3, 3 3, 3 0)) and POLYGON ((2 2, 2 4, 4 4, 4 2)): JTS
    # rejects an unclosed ring ("Points of LinearRing do not form a closed linestring"), so the rings are closed here
    ("docs example", poly([[(0, 0), (0, 3), (3, 3), (3, 0), (0, 0)]]), poly([[(2, 2), (2, 4), (4, 4), (4, 2), (2, 2)]]), True),
    # the (v, v) facets
    ("point on a segment's interior", pt(4, 0), line([(0, 0), (10, 0)]), True),
    ("point on a sloped segment's interior", line([(0, 0), (9, 6)]), pt(3, 2), True),
    ("point on a vertex", pt(10, 0), line([(0, 0), (10, 0), (10, 5)]), True),
    ("point collinear with a segment but beyond it", pt(12, 0), line([(0, 0), (10, 0)]), False),
    ("point collinear with a sloped segment but beyond it", line([(0, 0), (9, 6)]), pt(12, 8), False),
    ("point beside a segment", pt(4, 1), line([(0, 0), (10, 0)]), False),
    ("two equal points", pt(3, 4), pt(3, 4), True),
    ("two unequal points", pt(3, 4), pt(3, 5), False),
    ("zero-length line on a point", line([(3, 4), (3, 4)]), pt(3, 4), True),
    # a line never contains
    ("closed line around a point", line(SQ), pt(5, 4), False),
    ("point inside a closed line", pt(5, 4), line(SQ), False),
    ("closed line around a polygon", line(SQ), poly([TRI]), False),
    ("closed line around a closed line", line(SQ), line(TRI), False),
    ("nothing closes a line", line([(0, 0), (10, 0), (10, 10), (0, 10)]), line([(-5, 5), (5, 5)]), False),
    # each polygon part is located on its own
    ("three parts, the only hit in the last", poly([FAR], [[(80, 80), (90, 80), (90, 90), (80, 80)]], [SQ, HOLE]), pt(1, 1), True),
    ("three parts, the only hit in the last, point first", pt(1, 1), poly([FAR], [[(80, 80), (90, 80), (90, 90), (80, 80)]], [SQ, HOLE]), True),
    ("three parts around a point in the last part's hole", poly([FAR], [[(80, 80), (90, 80), (90, 90), (80, 80)]], [SQ, HOLE]), pt(5, 5), False),
    ("polygon around a polygon", poly([SQ]), poly([[(1, 1), (2, 1), (2, 2), (1, 1)]]), True),
    ("polygon inside a polygon", poly([[(1, 1), (2, 1), (2, 2), (1, 1)]]), poly([SQ]), True),
    ("polygon around the other's shell, in its hole", poly([TRI]), poly([SQ, HOLE]), False),
    ("polygon filling a hole exactly", poly([HOLE]), poly([SQ, HOLE]), True),
    ("collinear overlapping segments", line([(0, 0), (4, 0)]), line([(2, 0), (6, 0)]), True),
    ("collinear disjoint segments", line([(0, 0), (2, 0)]), line([(5, 0), (9, 0)]), False),
    ("second component inside the second part", poly([FAR], [SQ]), line([(20, 20), (30, 20)], [(1, 1), (2, 2)]), True),
    # empties: false, where st_distance says 0.0
    ("LINESTRING EMPTY on the left", line([]), pt(1, 1), False),
    ("MULTILINESTRING EMPTY on the right", poly([SQ]), line(), False),
    ("POLYGON EMPTY on the left", poly([]), poly([SQ]), False),
    ("empty multipoint on the right", pt(1, 1), ("point", []), False),
    ("two empties", line([]), poly([]), False),
    ("multiline with an empty member", line([], [(0, 0), (0, 9)]), pt(0, 4), True),
)


# ---- shapes that reach every branch of the workgroup kernel ----
def circle(n, radius, cx=0, cy=0):
    ring = [(float(round(cx + radius * math.cos(2 * math.pi * k / n))), float(round(cy + radius * math.sin(2 * math.pi * k / n))))
            for k in range(n)]
    return ring + ring[:1]


def zigzag(n, x0, y0, dx=7, dy=5):
    return [(float(x0 + dx * i), float(y0 + (dy if i % 2 else 0))) for i in range(n)]


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """(name, left, right): rings of 5 to 40 vertices and one of 300; expectations come from (E)"""
    rng = np.random.default_rng(20251020)
    ring300 = circle(300, 1000)
    star40 = T.star(rng, 0, 0, 300, 39)
    star25 = T.star(rng, 0, 0, 900, 24)
    star9 = T.star(rng, 0, 0, 40, 8)
    frame = poly([circle(36, 1000), circle(30, 800)])  # a ring around (0, 0) with a wide hole
    cases = [
        ("300-ring around a 40-star: containment only", poly([ring300]), poly([star40])),
        ("40-star inside a 300-ring: containment only, flipped", poly([star40]), poly([ring300])),
        ("300-ring crossed by a 25-star", poly([ring300]), poly([star25])),
        ("25-star crossing a 300-ring", poly([star25]), poly([ring300])),
        ("300-ring and a 9-star in its box's corner: false after every block", poly([ring300]),
         poly([[(x + 880, y + 880) for x, y in star9]])),
        ("9-star in the corner first", poly([[(x + 880, y + 880) for x, y in star9]]), poly([ring300])),
        ("40-star in the frame's hole: false", frame, poly([star40])),
        ("the frame around a 40-star, star first", poly([star40]), frame),
        ("25-star across the frame's hole ring", frame, poly([star25])),
        ("300-ring and a long zigzag through it", poly([ring300]), line(zigzag(40, -1200, 3, dx=61))),
        ("long zigzag inside the 300-ring: its first vertex decides", line(zigzag(40, -100, 3, dx=5)), poly([ring300])),
        ("long zigzag inside the frame's hole", frame, line(zigzag(40, -100, 3, dx=5))),
        ("multipoint of 40 around the frame, the last one on its hole ring",
         pt(*[c for k in range(39) for c in (3 * k - 60, 2 * k)], 800, 0), frame),
        ("multipoint of 40 in the frame's hole", frame, pt(*[c for k in range(40) for c in (3 * k - 60, 2 * k)])),
    ]
    # the only meeting segments are the last segment of the last ring of each side
    za = [zigzag(7, 0, 100), zigzag(9, 0, 200), zigzag(6, 0, 0) + [(40.0, -20.0)]]
    zb = [zigzag(5, 300, 100), zigzag(8, 300, 200), [(300.0, -50.0), (200.0, -60.0), (100.0, -60.0), (38.0, -30.0), (38.0, -2.0)]]
    cases.append(("multilines: only the last segments of the last lines cross", line(*za), line(*zb)))
    cases.append(("multilines: only the last segments cross, the longer side first", line(*zb), line(*za)))
    mp = poly([[(x + 3000, y) for x, y in star25]], [[(20, 0), (30, 0), (30, 10), (20, 10), (5, 5), (20, 0)]])
    ml = line(zigzag(9, -400, 50), [(-90.0, 40.0), (-60.0, 30.0), (-30.0, 3.0), (14.0, 3.0)])
    cases.append(("multipolygon's closing segment crossed by the multiline's last segment", mp, ml))
    cases.append(("the same, line first", ml, mp))
    return tuple(cases)


def _last_segments_only(a, b):
    """of all facet pairs only (last, last) meet"""
    fa, fb = exact_facets(a), exact_facets(b)
    hits = [(i, j) for i, (p, q) in enumerate(fa) for j, (r, s) in enumerate(fb) if T._segments_meet(p, q, r, s)]
    return hits == [(len(fa) - 1, len(fb) - 1)]


# ---- seeded random integer geometries, |c| <= 2^20, all six kinds, with near-touching placements ----
def random_geom(rng, cx, cy):
    if rng.integers(0, 6) < 5:
        return TL.random_geom(rng, cx, cy)
    radius = float(rng.integers(2000, 60000))
    return poly([T.star(rng, cx, cy, radius, int(rng.integers(5, 14)))],
                [T.star(rng, cx + 2.5 * radius, cy, radius, int(rng.integers(5, 24))),
                 T.star(rng, cx + 2.5 * radius, cy, 0.4 * radius, int(rng.integers(4, 10)), lo=0.4)])


def vertices(g):
    return [v for _, rings in components(g) for ring in rings for v in ring]


def translated(g, dx, dy):
    kind, members = g
    mv = lambda v: (v[0] + dx, v[1] + dy)
    if kind == "point":
        return (kind, [mv(v) for v in members])
    if kind == "line":
        return (kind, [[mv(v) for v in ln] for ln in members])
    return (kind, [[[mv(v) for v in ring] for ring in part] for part in members])


def near_touching(rng, a, b):
    """b moved so that one of its vertices is a lattice point of one of a's facets, or one unit off it"""
    fa = exact_facets(a)
    (px, py), (qx, qy) = fa[int(rng.integers(0, len(fa)))]
    g = math.gcd(int(qx - px), int(qy - py))
    k = int(rng.integers(0, g + 1)) if g else 0
    tx, ty = (px + (qx - px) // g * k, py + (qy - py) // g * k) if g else (px, py)
    tx, ty = tx + int(rng.integers(-1, 2)), ty + int(rng.integers(-1, 2))
    vb = vertices(b)
    vx, vy = vb[int(rng.integers(0, len(vb)))]
    return translated(b, float(tx - vx), float(ty - vy))


@functools.lru_cache(maxsize=None)
def random_pairs(n=400, seed=20251021):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(n):
        cx, cy = rng.uniform(-200000, 200000, 2)
        a = random_geom(rng, cx, cy)
        spread = (20000, 120000, 250000)[int(rng.integers(0, 3))]  # inside / overlapping / apart
        b = random_geom(rng, cx + rng.uniform(-spread, spread), cy + rng.uniform(-spread, spread))
        if k % 2:
            b = near_touching(rng, a, b)
        pairs.append((a, b))
    assert all(abs(c) <= 2 ** 20 for a, b in pairs for g in (a, b) for v in vertices(g) for c in v)
    return tuple(pairs)


# ---- the reference's invariant (intersectsBehaviour, ST_IntersectsBehaviors.scala:13-61) ----
INVARIANT_SEED, INVARIANT_RES = 20251023, 8


@functools.lru_cache(maxsize=None)
def invariant_zones():
    """(zones, moved, left chips, right chips, resolution): the 35 NYC zones and a copy with every zone
    translated by (sqrt(area u 0.1), sqrt(area u' 0.1)), u, u' seeded uniforms, as the reference's
    st_translate(wkt, sqrt(st_area * rand() * 0.1), sqrt(st_area * rand() * 0.1)) does"""
    from mosaic_amd.context import tessellate
    from mosaic_amd.data import PolygonSet

    zones = PolygonSet.load("nyc_taxi_zones_35")
    rng = np.random.default_rng(INVARIANT_SEED)
    xy = np.array(zones.xy, np.float64).reshape(-1, 2).copy()
    for g in range(len(zones)):
        area = 0.0
        for part in zones.parts(g):
            for k, ring in enumerate(part):
                r = np.array(ring)
                a = 0.5 * abs(float(np.sum(r[:-1, 0] * r[1:, 1] - r[1:, 0] * r[:-1, 1])))
                area += a if k == 0 else -a
        v0 = int(zones.ring_offsets[zones.part_rings[zones.geom_parts[g]]])
        v1 = int(zones.ring_offsets[zones.part_rings[zones.geom_parts[g + 1]]])
        xy[v0:v1] += np.sqrt(area * rng.random(2) * 0.1)
    moved = PolygonSet(xy.reshape(np.shape(zones.xy)), zones.ring_offsets, zones.part_rings, zones.geom_parts, zones.names)
    return zones, moved, tessellate("H3", zones, INVARIANT_RES), tessellate("H3", moved, INVARIANT_RES), INVARIANT_RES


def all_pairs(n_left, n_right):
    return np.repeat(np.arange(n_left), n_right), np.tile(np.arange(n_right), n_left)


@functools.lru_cache(maxsize=None)
def all_cases():
    """every case of the CPU file as (left geometries, right geometries)"""
    left = [c[1] for c in truth_table()] + [c[1] for c in EXPLICIT] + [c[1] for c in kernel_cases()] + [a for a, _ in random_pairs()]
    right = [c[2] for c in truth_table()] + [c[2] for c in EXPLICIT] + [c[2] for c in kernel_cases()] + [b for _, b in random_pairs()]
    return tuple(left), tuple(right)


@functools.lru_cache(maxsize=None)
def case_rows():
    """all_cases as WKB rows in alternating byte orders, with (H) on them"""
    left, right = all_cases()
    rows_l = [geom_wkb(g, bool(i % 2)) for i, g in enumerate(left)]
    rows_r = [geom_wkb(g, bool(i % 3)) for i, g in enumerate(right)]
    want = host_intersects(LCol.from_wkb(rows_l), LCol.from_wkb(rows_r))
    return rows_l, rows_r, want
