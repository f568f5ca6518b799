"""What tests/test_st_measures.py (CPU) and tests/test_gpu_st_measures.py share: the host library (H)
built from tests/native/st_measures_host.cpp, the exact oracle (E) with its error bounds, and the case
lists.  Geometries are those of tests/test_st_distance_lines.py: ("point", ...), ("line", ...),
("polygon", ...).

(E) works in fractions.Fraction on the doubles as given: the shoelace area and the area centroid are
rationals; lengths are square roots taken to 2^-200 relative.  None of it shares code with
mosaic_amd/csrc/st_measures.h.
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
from tests.test_st_distance import HOLE, SQ, poly, pt
from tests.test_st_distance_lines import LCol, geom_wkb, line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_THREADS = T.HOST_THREADS
NEW_SYMBOLS = ("mosaic_st_measures", "mosaic_st_measures_last_split")
FIELDS = ("area", "length", "cx", "cy", "numpoints", "xmin", "ymin", "xmax", "ymax")
U = Fraction(1, 2 ** 53)  # unit roundoff


# ---- (H) the host library ----
@functools.lru_cache(maxsize=None)
def host_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="sm_host_"), "libsm.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-pthread",
                    "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "native", "st_measures_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.sm_measures.argtypes = [vp, vp, i64] + [vp] * 10 + [i32]
    lib.sm_measures.restype = i32
    lib.sm_is_ccw.argtypes = [vp, i64]
    lib.sm_is_ccw.restype = i32
    return lib


def host_measures(col, rows=None, fields=FIELDS, threads=HOST_THREADS):
    """meas::measure over the rows of a column (LCol): a dict of arrays, "status" included"""
    if rows is not None:
        rows = np.ascontiguousarray(rows, np.int64)
    n = col.n if rows is None else len(rows)
    out = {f: np.full(max(n, 1), -7, np.int64) if f == "numpoints" else np.full(max(n, 1), -7.0) for f in fields}
    st = np.full(max(n, 1), -1, np.int32)
    rc = host_lib().sm_measures(col.handle, N.ptr(rows), n, *[N.ptr(out.get(f)) for f in FIELDS], N.ptr(st), threads)
    if rc:
        raise IndexError("row index out of range")
    res = {f: a[:n] for f, a in out.items()}
    res["status"] = st[:n]
    return res


def host_one(g):
    m = host_measures(LCol.from_geoms([g]))
    return {k: v[0] for k, v in m.items()}


def host_is_ccw(ring):
    xy = np.ascontiguousarray(ring, np.float64).reshape(-1)
    return bool(host_lib().sm_is_ccw(N.ptr(xy), len(xy) // 2))


# ---- (E) exact ----
def fr(v):
    return Fraction(float(v[0])), Fraction(float(v[1]))


def components(g):
    """[(kind, rings)] with kind "point" / "line" / "polygon"; empty members dropped as the column drops them"""
    kind, members = g
    if kind == "point":
        return [("point", [[p]]) for p in members]
    if kind == "line":
        return [("line", [ln]) for ln in members if ln]
    return [("polygon", [r for r in part]) for part in members if part]


def sqrt_frac(v, k=200):
    """sqrt of the Fraction v from below, within 2^-k relative for v >= 2^-k"""
    if v == 0:
        return Fraction(0)
    s = 0
    while v < 1:  # scale up by 4^s
        v *= 4
        s += 1
    return Fraction(math.isqrt((v.numerator << (2 * k)) // v.denominator), 1 << (k + s))


def gamma(k):
    """the accumulated bound of k roundings, (1 + u)^k - 1 <= k u / (1 - k u)"""
    return k * U / (1 - k * U)


def exact_area(g):
    """(area, bound): the exact shoelace area and the forward error bound of the ring recursion"""
    area, terms, longest, n_rings = Fraction(0), Fraction(0), 0, 0
    for kind, rings in components(g):
        if kind != "polygon":
            continue
        for k, ring in enumerate(rings):
            e = [fr(v) for v in ring]
            n_rings += 1
            if len(e) < 3:
                continue
            t = [(e[i][0] - e[0][0]) * (e[i - 1][1] - e[i + 1][1]) for i in range(1, len(e) - 1)]
            a = abs(sum(t)) / 2
            area += a if k == 0 else -a
            terms += sum(abs(x) for x in t) / 2
            longest = max(longest, len(t))
    # a term is rounded 3 times (two differences, one product), then passes at most `longest` additions
    # in its ring and one addition or subtraction per ring and per part of the fold (<= 2 n_rings)
    return area, gamma(3 + longest + 2 * n_rings) * terms


def exact_length(g):
    total, longest, n_rings = Fraction(0), 0, 0
    for kind, rings in components(g):
        if kind == "point":
            continue
        for ring in rings:
            e = [fr(v) for v in ring]
            n_rings += 1
            longest = max(longest, len(e) - 1)
            for a, b in zip(e, e[1:]):
                total += sqrt_frac((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)
    # a segment: dx and dy rounded once each and squared (2 + 1 roundings on each square), one addition,
    # one square root that halves what came before: (1 + u)^4 under the root, (1 + u)^3 after it; then
    # the additions of its ring, of the part and of the geometry.  All terms are >= 0.
    return total, gamma(3 + longest + 2 * n_rings) * total + total / 2 ** 150


def _quotient_bound(s, e_s, a, e_a, roundings):
    """|fl(S^ / A^ ...) - S / A| for |S^ - S| <= e_s, |A^ - A| <= e_a and `roundings` roundings in the
    division chain: (e_s + |S / A| e_a) / (|A| - e_a), then gamma(roundings) of the perturbed quotient"""
    assert abs(a) > e_a, "the case is too ill-conditioned to bound"
    q = s / a
    d = (e_s + abs(q) * e_a) / (abs(a) - e_a)
    return d + gamma(roundings) * (abs(q) + d)


def exact_centroid(g):
    """((cx, cy), (bound x, bound y)) or (None, None) for an empty geometry: JTS's rule -- area part if the
    signed area sum is not 0, else the line part if the length is not 0, else the mean of the points"""
    comps = components(g)
    # area part: sum over polygon rings of the signed triangles on the part's base point
    sx = sy = a2 = Fraction(0)
    mag_x = mag_y = mag_a = Fraction(0)
    n_seg = 0
    for kind, rings in comps:
        if kind != "polygon":
            continue
        base = fr(rings[0][0]) if rings[0] else None
        for k, ring in enumerate(rings):
            e = [fr(v) for v in ring]
            if not e:
                continue
            shoelace = sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(e, e[1:]))
            # JTS adds a shell's triangles positively when it is clockwise: with its own orientation sign the
            # shell counts |area|, and a hole counts -|area|.  A ring of zero area contributes zero either way.
            sign = (-1 if shoelace > 0 else 1) * (1 if k == 0 else -1)
            for p, q in zip(e, e[1:]):
                ab, cd = (p[0] - base[0]) * (q[1] - base[1]), (q[0] - base[0]) * (p[1] - base[1])
                t = sign * (ab - cd)
                cx, cy = base[0] + p[0] + q[0], base[1] + p[1] + q[1]
                sx += t * cx
                sy += t * cy
                a2 += t
                mt = abs(ab) + abs(cd)
                mag_a += mt
                mag_x += mt * (abs(base[0]) + abs(p[0]) + abs(q[0]))
                mag_y += mt * (abs(base[1]) + abs(p[1]) + abs(q[1]))
                n_seg += 1
    if a2 != 0:
        # area2: 2 differences + 1 product on each side and the difference: 4 roundings against |ab| + |cd|;
        # the triangle's centre sum: 2; their product: 1; then one addition per segment of the geometry.
        # The result is cg3 / 3 / areasum2: two more roundings.
        e_s_k, e_a_k = gamma(7 + n_seg), gamma(4 + n_seg)
        # exact value: (sx / a2) / 3; the sign convention cancels in the quotient
        bx = _quotient_bound(sx, e_s_k * mag_x, 3 * a2, 3 * e_a_k * mag_a, 2)
        by = _quotient_bound(sy, e_s_k * mag_y, 3 * a2, 3 * e_a_k * mag_a, 2)
        return (sx / (3 * a2), sy / (3 * a2)), (bx, by)
    # line part
    lx = ly = total = Fraction(0)
    mag_lx = mag_ly = Fraction(0)
    n_seg = n_runs = 0
    points = []
    for kind, rings in comps:
        if kind == "point":
            points.append(fr(rings[0][0]))
            continue
        for ring in rings:
            e = [fr(v) for v in ring]
            if not e:
                continue
            run = Fraction(0)
            for a, b in zip(e, e[1:]):
                d = sqrt_frac((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)
                run += d
                lx += d * (a[0] + b[0]) / 2
                ly += d * (a[1] + b[1]) / 2
                mag_lx += d * (abs(a[0]) + abs(b[0])) / 2
                mag_ly += d * (abs(a[1]) + abs(b[1])) / 2
                n_seg += 1
            n_runs += 1
            total += run
            if run == 0:
                points.append(e[0])
    if total != 0:
        # a length: 3 roundings (exact_length); the midpoint: 1; their product: 1; the additions; one division
        e_s_k, e_l_k = gamma(5 + n_seg) + Fraction(1, 2 ** 150), gamma(3 + n_seg + n_runs) + Fraction(1, 2 ** 150)
        return (lx / total, ly / total), (_quotient_bound(lx, e_s_k * mag_lx, total, e_l_k * total, 1),
                                          _quotient_bound(ly, e_s_k * mag_ly, total, e_l_k * total, 1))
    if points:
        n = len(points)
        px, py = sum(p[0] for p in points), sum(p[1] for p in points)
        ex = gamma(n) * sum(abs(p[0]) for p in points)
        ey = gamma(n) * sum(abs(p[1]) for p in points)
        return (px / n, py / n), (_quotient_bound(px, ex, Fraction(n), Fraction(0), 1),
                                  _quotient_bound(py, ey, Fraction(n), Fraction(0), 1))
    return None, None


def numpoints_of(g):
    return sum(len(r) for _, rings in components(g) for r in rings)


def bounds_of(g):
    vs = [v for _, rings in components(g) for r in rings for v in r]
    if not vs:
        return None
    xs, ys = [v[0] for v in vs], [v[1] for v in vs]
    return min(xs), min(ys), max(xs), max(ys)


def python_ring_area(ring):
    """the ring recursion, transcribed: bit-identical by construction"""
    n = len(ring)
    if n < 3:
        return 0.0
    s = 0.0
    x0 = ring[0][0]
    for i in range(1, n - 1):
        s += (ring[i][0] - x0) * (ring[i - 1][1] - ring[i + 1][1])
    return s / 2.0


def python_area(parts):
    area = 0.0
    for rings in parts:
        a = 0.0
        for k, ring in enumerate(rings):
            r = abs(python_ring_area(ring))
            a = a + r if k == 0 else a - r
        area += a
    return area


# ---- the case table ----
DOCS_POLYGON = poly([[(30, 10), (40, 40), (20, 40), (10, 20), (30, 10)]])
DOCS = dict(area=550.0, length=96.34413615167959, numpoints=5, cx=25.454545454545453, cy=26.96969696969697,
            xmin=10.0, ymin=10.0, xmax=40.0, ymax=40.0)
CW_SQ = SQ[::-1]
TRI = [(4, 4), (6, 4), (6, 6), (4, 4)]
CASES = (
    ("docs polygon", DOCS_POLYGON),
    ("ccw square", poly([SQ])),
    ("cw square", poly([CW_SQ])),
    ("ccw square with a ccw hole", poly([SQ, HOLE])),
    ("ccw square with a cw hole", poly([SQ, HOLE[::-1]])),
    ("cw square with a cw hole", poly([CW_SQ, HOLE[::-1]])),
    ("two holes", poly([[(0, 0), (20, 0), (20, 10), (0, 10), (0, 0)], HOLE, [(12, 3), (17, 3), (17, 8), (12, 3)]])),
    ("multipolygon, mixed orientations", poly([SQ, HOLE], [[(x + 30, y + 5) for x, y in CW_SQ]], [[(x - 40, y) for x, y in TRI]])),
    ("zero-area polygon: the line part decides", poly([[(0, 0), (10, 0), (20, 0), (10, 0), (0, 0)]])),
    ("zero-area polygon on a slope", poly([[(1, 1), (5, 3), (9, 5), (1, 1)]])),
    ("polygon of one repeated vertex: the point part decides", poly([[(3, 4), (3, 4), (3, 4), (3, 4)]])),
    ("repeated vertices in a ring", poly([[(0, 0), (10, 0), (10, 0), (10, 10), (10, 10), (0, 10), (0, 0), (0, 0)]])),
    ("flat top: isCCW walks equal y", poly([[(0, 0), (10, 0), (10, 10), (6, 10), (3, 10), (0, 10), (0, 0)]])),
    ("spike at the top: upHi == downHi", poly([[(0, 0), (10, 0), (5, 5), (5, 12), (5, 5), (0, 0)]])),
    ("point", pt(3, 4)),
    ("multipoint", pt(0, 0, 10, 0, 10, 10, 1, 7)),
    ("empty multipoint", ("point", [])),
    ("line", line([(0, 0), (3, 4), (3, 10)])),
    ("closed line: no area", line(SQ)),
    ("zero-length line: the point part decides", line([(3, 4), (3, 4)])),
    ("line with a zero-length segment", line([(0, 0), (0, 0), (6, 8)])),
    ("multiline", line([(0, 0), (10, 0)], [(20, 5), (20, 9), (23, 13)])),
    ("multiline with a zero-length member", line([(5, 5), (5, 5)], [(0, 0), (8, 6)])),
    ("multiline of zero-length members", line([(5, 5), (5, 5)], [(1, 9), (1, 9), (1, 9)])),
    ("multiline with an empty member", line([], [(0, 0), (0, 9)])),
    ("LINESTRING EMPTY", line([])),
    ("MULTILINESTRING EMPTY", line()),
    ("POLYGON EMPTY", poly([])),
    ("near the antimeridian and the pole",
     poly([[(179.99999, 89.99999), (-179.99999, 89.99999), (-179.99999, -89.99999), (179.99999, -89.99999), (179.99999, 89.99999)]])),
    ("a sliver at +180 / +90", poly([[(179.9999990, 89.9999990), (179.9999999, 89.9999990), (179.9999999, 89.9999999),
                                       (179.9999990, 89.9999999), (179.9999990, 89.9999990)]])),
    ("a sliver at -180 / -90", poly([[(-179.9999990, -89.9999990), (-179.9999990, -89.9999999), (-179.9999999, -89.9999999),
                                       (-179.9999999, -89.9999990), (-179.9999990, -89.9999990)]])),
    ("BNG metres", poly([[(530123.25, 180456.5), (530987.75, 180461.0), (530990.5, 181200.125), (530119.0, 181190.75),
                          (530123.25, 180456.5)],
                         [(530400.0, 180700.0), (530600.0, 180700.0), (530600.0, 180900.5), (530400.0, 180700.0)]])),
    ("BNG line", line([(651234.5, 1213456.25), (651240.0, 1213460.75), (651300.125, 1213400.0)])),
)


def star_f(rng, cx, cy, radius, n):
    """a star-shaped ring with fractional coordinates; consecutive vertices are less than a half turn apart
    as seen from the centre, so the ring is simple and its orientation is the sign of its shoelace sum"""
    ang = (np.arange(n) + rng.uniform(0.3, 0.7, n)) * (2 * np.pi / n)
    rad = rng.uniform(0.5 * radius, radius, n)
    ring = [(float(cx + r * math.cos(t)), float(cy + r * math.sin(t))) for r, t in zip(rad, ang)]
    return ring + ring[:1]


def random_geom(rng):
    kind = int(rng.integers(0, 7))
    cx, cy = (rng.uniform(-180, 180), rng.uniform(-85, 85)) if rng.integers(0, 2) else (rng.uniform(0, 7e5), rng.uniform(0, 1.3e6))
    radius = float(rng.uniform(1e-3, 2.0)) if abs(cx) <= 180 and abs(cy) <= 90 else float(rng.uniform(5, 5e4))
    flip = lambda ring: ring[::-1] if rng.integers(0, 2) else ring
    if kind == 0:
        return pt(cx, cy)
    if kind == 1:
        return pt(*(np.array([cx, cy]) + rng.uniform(-radius, radius, (int(rng.integers(2, 7)), 2))).ravel())
    if kind == 2:
        return line([tuple(v) for v in np.array([cx, cy]) + rng.uniform(-radius, radius, (int(rng.integers(2, 30)), 2))])
    if kind == 3:
        return line(*[[tuple(v) for v in np.array([cx, cy]) + rng.uniform(-radius, radius, (int(rng.integers(2, 12)), 2))]
                      for _ in range(int(rng.integers(2, 5)))])
    if kind == 4:
        return poly([flip(star_f(rng, cx, cy, radius, int(rng.integers(3, 40))))])
    if kind == 5:
        return poly([flip(star_f(rng, cx, cy, radius, int(rng.integers(6, 40)))),
                     flip(star_f(rng, cx, cy, 0.3 * radius, int(rng.integers(3, 12))))])
    return poly([flip(star_f(rng, cx, cy, radius, int(rng.integers(4, 20))))],
                [flip(star_f(rng, cx + 3 * radius, cy, radius, int(rng.integers(6, 24)))),
                 flip(star_f(rng, cx + 3 * radius, cy, 0.3 * radius, int(rng.integers(3, 9))))],
                [flip(star_f(rng, cx, cy + 3 * radius, radius, int(rng.integers(3, 9))))])


@functools.lru_cache(maxsize=None)
def random_geoms(n=300, seed=20251101):
    rng = np.random.default_rng(seed)
    return tuple(random_geom(rng) for _ in range(n))


@functools.lru_cache(maxsize=None)
def case_rows():
    """the case table and the random geometries as WKB rows in alternating byte orders, with (H) on them"""
    geoms = [g for _, g in CASES] + list(random_geoms())
    rows = [geom_wkb(g, bool(i % 2)) for i, g in enumerate(geoms)]
    return rows, host_measures(LCol.from_wkb(rows))


# ---- the ring-size column of the GPU tests ----
RING_SIZES = (4, 5, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def ring_size_rows():
    """(rows, (H)): polygons whose shells have RING_SIZES stored vertices, single parts and multiparts
    with holes, one ring of 3,001 vertices, and a null row, an empty row and a row-path row among them;
    the first and the last rows are polygons"""
    rng = np.random.default_rng(20251102)
    ring = lambda n, cx=0.0, cy=0.0, r=1.0: star_f(rng, cx, cy, r, n - 1)
    rows = []
    for k, n in enumerate(RING_SIZES):
        rows.append(poly([ring(n, 10 * k, 0)]))
        rows.append(poly([ring(n, 10 * k, 50), ring(5, 10 * k, 50, 0.2)[::-1]], [ring(n + 1, 10 * k + 4, 50)[::-1]]))
        if k == 3:
            rows += [None, poly([]), "path"]
    rows.append(poly([ring(3001, -50, -50, 20.0), ring(64, -50, -50, 3.0)]))
    rows.append(poly([ring(7, 0, -100)]))
    wkb = [None if g is None else b"\x01\x07\x00\x00\x00\x00\x00\x00\x00" if g == "path" else geom_wkb(g, bool(i % 2))
           for i, g in enumerate(rows)]  # "path": GEOMETRYCOLLECTION EMPTY
    return wkb, host_measures(LCol.from_wkb(wkb))


# ---- the analyzer's oracle composition ----
BNG_EDGE = {-1: 500000, 1: 100000, -2: 50000, 2: 10000, -3: 5000, 3: 1000, -4: 500, 4: 100, -5: 50, 5: 10, -6: 5, 6: 1}


@functools.lru_cache(maxsize=None)
def nyc_oracle_inputs():
    """(areas, [(res, cell areas)]) on the 263 NYC zones: (H) areas; per resolution the python_area of the
    closed h3ToGeoBoundary ring (degrees) of the oracle's cell under oracle.jts_centroid"""
    import oracle
    from mosaic_amd.data import PolygonSet

    zones = PolygonSet.load("nyc_taxi_zones")
    areas = host_measures(LCol.from_polyset(zones), fields=("area",))["area"]
    cents = np.array([oracle.jts_centroid(zones.parts(g)) for g in range(len(zones))])
    cell_areas = []
    for res in range(16):
        cells = oracle.h3_point_to_index(cents[:, 0], cents[:, 1], res)
        a = []
        for c in cells.tolist():
            b = [(math.degrees(lng), math.degrees(lat)) for lat, lng in oracle.h3_to_geo_boundary(c)]
            a.append(python_area([[b + b[:1]]]))
        cell_areas.append((res, np.array(a)))
    return areas, cell_areas
