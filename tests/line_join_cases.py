"""TEST INFRASTRUCTURE ONLY: st_intersects_aggregate over the join of line chips with polygon chips,
restated in Python, and the cases the host and GPU tests share.

The reference folds ``l.is_core || p.is_core || l.wkb intersects p.wkb`` with OR over the equi-join of
two grid_tessellateexplode outputs on index_id, grouped by (line row, polygon row)
(ST_IntersectsAggregate.scala:28-39); ``intersects`` is JTS Geometry.intersects: the closed point sets
share a point.  Restated on decoded geometries:

* ``intersects(pieces, parts)``: a segment of a piece meets a ring segment, or the first vertex of a
  piece (every point item is a piece) is not exterior to a polygon part.  ``exact=True`` decides both
  with the rationals of oracle/exact.py (the hand cases); ``exact=False`` takes the oracle's C segment
  predicate behind a numpy segment-box filter and exact.locate_in_polygon (the volume cases).
* ``join``: the join, the grouping and the OR.
"""
import math
import struct

import numpy as np

import oracle
from mosaic_amd import wkb as W
from oracle import exact
from tests import line_cases as LC


# ---- the semantics ----
def pieces_of(blob):
    """A line chip's WKB as pieces (lists of points); a piece of one point is a point item."""
    blob = bytes(blob)
    if not blob:
        return []
    kind, g = W.read_wkb(blob)
    if kind == "point":
        return [] if math.isnan(g[0]) or math.isnan(g[1]) else [[g]]
    if kind == "multipoint":
        return [[p] for p in g if not (math.isnan(p[0]) or math.isnan(p[1]))]
    assert kind == "linestring", kind
    return [ln for ln in g if ln]


def parts_of(blob):
    blob = bytes(blob)
    if not blob:
        return []
    kind, g = W.read_wkb(blob)
    assert kind == "polygon", kind
    return g


def _box(points):
    xs, ys = [p[0] for p in points], [p[1] for p in points]
    return min(xs), min(ys), max(xs), max(ys)


def _meet(a, b):
    return not (a[2] < b[0] or b[2] < a[0] or a[3] < b[1] or b[3] < a[1])


def intersects(pieces, parts, exact_segments=True):
    rings = [r for rings in parts for r in rings if r]
    if not pieces or not rings:
        return False
    if not _meet(_box([p for ln in pieces for p in ln]), _box([p for r in rings for p in r])):
        return False
    for ln in pieces:
        if len(ln) < 2:
            continue
        lb = _box(ln)
        for r in rings:
            if len(r) < 2 or not _meet(lb, _box(r)):
                continue
            if exact_segments:
                if any(exact.segments_intersect(a, b, c, d) for a, b in zip(ln, ln[1:]) for c, d in zip(r, r[1:])):
                    return True
                continue
            q = np.asarray(r, np.float64)
            qx0, qx1 = np.minimum(q[:-1, 0], q[1:, 0]), np.maximum(q[:-1, 0], q[1:, 0])
            qy0, qy1 = np.minimum(q[:-1, 1], q[1:, 1]), np.maximum(q[:-1, 1], q[1:, 1])
            for a, b in zip(ln, ln[1:]):
                near = ~((qx1 < min(a[0], b[0])) | (qx0 > max(a[0], b[0])) | (qy1 < min(a[1], b[1])) | (qy0 > max(a[1], b[1])))
                for j in np.nonzero(near)[0]:
                    if oracle.segments_intersect(a, b, r[j], r[j + 1]):
                        return True
    return any(exact.locate_in_polygon(ln[0], rings) != exact.EXTERIOR for ln in pieces for rings in parts if rings and rings[0])


def rows_of(chips):
    """Chip columns as rows (is_core, cell, key, wkb bytes)."""
    offs, data = chips["wkb"]
    data = np.asarray(data, np.uint8).tobytes()
    return [(bool(chips["is_core"][i]), int(chips["index_id"][i]), int(chips["polygon_key"][i]),
             data[int(offs[i]):int(offs[i + 1])]) for i in range(len(chips["index_id"]))]


def join(line_chips, polygon_chips, exact_segments=True):
    """{(line key, polygon key): flag} of the chip join."""
    by_cell = {}
    for core, cell, key, blob in rows_of(polygon_chips):
        by_cell.setdefault(cell, []).append((core, key, blob))
    out = {}
    for lcore, cell, lkey, lblob in rows_of(line_chips):
        for pcore, pkey, pblob in by_cell.get(cell, ()):
            g = (lkey, pkey)
            if out.get(g):
                continue
            out[g] = lcore or pcore or intersects(pieces_of(lblob), parts_of(pblob), exact_segments)
    return out


def as_dict(keys_a, keys_b, flags):
    return {(int(a), int(b)): bool(f) for a, b, f in zip(keys_a, keys_b, flags)}


# ---- chip columns from rows (is_core, cell, key, wkb) ----
def columns(rows):
    blobs = [r[3] for r in rows]
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    data = np.frombuffer(b"".join(blobs), np.uint8)
    return dict(is_core=np.array([r[0] for r in rows], np.uint8), index_id=np.array([r[1] for r in rows], np.int64),
                polygon_key=np.array([r[2] for r in rows], np.int32), wkb=(offs, data if len(data) else np.zeros(1, np.uint8)))


# ---- the hand table: one cell id stands for a 100 x 100 square ----
def ring(*pts):
    return [tuple(map(float, p)) for p in pts] + [tuple(map(float, pts[0]))]


def square(x0, y0, s):
    return ring((x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s))


TRI = W.geometry_wkb([[ring((0, 0), (100, 0), (0, 100))]])
HOLED = W.geometry_wkb([[square(0, 0, 100), square(40, 40, 20)]])
TWO = W.geometry_wkb([[square(0, 0, 10)], [square(50, 50, 40)]])
EMPTY_LINE = struct.pack(">BII", 0, 2, 0)


def ls(*pts):
    return W.linestring_wkb([tuple(map(float, p)) for p in pts])


# (name, line is_core, line wkb, polygon is_core, polygon wkb, expected flag)
HAND = [
    ("polygon chip core, line far away", 0, ls((900, 900), (950, 950)), 1, TRI, True),
    ("line table is_core", 1, ls((900, 900), (950, 950)), 0, TRI, True),
    ("line crossing the hypotenuse", 0, ls((10, 10), (90, 90)), 0, TRI, True),
    ("line wholly inside", 0, ls((10, 10), (20, 30), (30, 20)), 0, TRI, True),
    ("line wholly in the other half", 0, ls((60, 60), (90, 90), (95, 70)), 0, TRI, False),
    ("line ending on vertex (100, 0)", 0, ls((150, 50), (100, 0)), 0, TRI, True),
    ("line collinear with the hypotenuse", 0, ls((75, 25), (25, 75)), 0, TRI, True),
    ("point on the boundary", 0, W.point_wkb(50.0, 50.0), 0, TRI, True),
    ("point outside", 0, W.point_wkb(50.5, 50.0), 0, TRI, False),
    ("multipoint, second point inside", 0, W.multipoint_wkb([(80.0, 80.0), (20.0, 20.0)]), 0, TRI, True),
    ("multilinestring, second piece inside", 0,
     W.multilinestring_wkb([[(60.0, 60.0), (90.0, 90.0)], [(10.0, 10.0), (20.0, 15.0)]]), 0, TRI, True),
    ("line inside the hole", 0, ls((45, 45), (55, 50), (50, 55)), 0, HOLED, False),
    ("line along the hole's edge", 0, ls((42, 40), (58, 40)), 0, HOLED, True),
    ("multipolygon, line inside its second part", 0, ls((60, 60), (70, 65)), 0, TWO, True),
    ("empty line against a border chip", 0, EMPTY_LINE, 0, TRI, False),
    ("empty line against a core chip", 0, EMPTY_LINE, 1, TRI, True),
]


def hand_chips(cells):
    """The hand table as two chip sets: row k has line key k, polygon key k and its own cell cells[k]."""
    assert len(cells) >= len(HAND)
    lines = columns([(h[1], int(cells[k]), k, h[2]) for k, h in enumerate(HAND)])
    polys = columns([(h[3], int(cells[k]), k, h[4]) for k, h in enumerate(HAND)])
    return lines, polys, {(k, k): h[5] for k, h in enumerate(HAND)}


def grouping_chips(cells):
    """Line 0 x polygon 0 in two cells (false, true): one true group; line 1 x polygon 0 in two cells
    (false, false): one false group; line 2 in a cell the polygons lack: no group; line 3 x polygon 1:
    true.  Rows are given out of key order."""
    c0, c1, c2 = (int(c) for c in cells[:3])
    lines = columns([(0, c0, 3, ls((10, 10), (20, 20))), (0, c0, 1, ls((60, 60), (90, 90))), (0, c1, 1, ls((70, 70), (80, 90))),
                     (0, c0, 0, ls((60, 60), (90, 90))), (0, c1, 0, ls((10, 10), (90, 90))), (0, c2, 2, ls((10, 10), (20, 20)))])
    polys = columns([(0, c1, 0, TRI), (0, c0, 1, TRI), (0, c0, 0, TRI)])
    want = {(0, 0): True, (0, 1): False, (1, 0): False, (1, 1): False, (3, 0): True, (3, 1): True}
    return lines, polys, want


# ---- the reference's invariant (intersectsBehaviour, ST_IntersectsBehaviors.scala:13-61) on lines ----
def walks_in(grid, res, n, seed, bbox):
    """line_cases.random_walks with every component line translated so that its first vertex falls at
    a seeded place inside `bbox` (the generator's own origins are NYC midtown and a field outside
    London); coordinates stay rounded to 1e-6 degrees / 1 m."""
    rng = np.random.default_rng(seed + 1)
    digits = 6 if grid == LC.H3 else 0
    out = []
    for lines in LC.random_walks(grid, res, n, seed):
        moved = []
        for ln in lines:
            tx = rng.uniform(bbox[0], bbox[2]) - ln[0][0]
            ty = rng.uniform(bbox[1], bbox[3]) - ln[0][1]
            moved.append(LC.clean([(round(x + tx, digits), round(y + ty, digits)) for x, y in ln]))
        out.append(moved)
    assert all(len(ln) >= 2 for lines in out for ln in lines)
    return out


def flat(geoms, zones):
    """{(line, polygon): intersects(line geometry, polygon)} on the original geometries."""
    parts = [zones.parts(k) for k in range(len(zones))]
    return {(g, k): intersects(lines, parts[k], exact_segments=False) for g, lines in enumerate(geoms) for k in range(len(zones))}


_invariant = {}


def invariant_case(name):
    """(line geometries, zones, line chips, polygon chips, resolution) of the invariant workloads, built
    once: the 35 NYC zones at H3 resolution 8 and the London postcode areas at BNG resolution 4, each
    against 60 seeded walks placed inside the zones' bounding box."""
    from mosaic_amd.context import tessellate
    from mosaic_amd.data import LineSet, PolygonSet

    if name not in _invariant:
        if name == "H3":
            zones, grid, res, seed = PolygonSet.load("nyc_taxi_zones_35"), LC.H3, 8, 20250308
        else:
            zones, grid, res, seed = PolygonSet.load("london_postcodes_bng"), LC.BNG, 4, 20250313
        geoms = walks_in(grid, res, 60, seed, zones.bbox())
        _invariant[name] = (geoms, zones, tessellate(name, LineSet.from_lines(geoms), res), tessellate(name, zones, res), res)
    return _invariant[name]


# ---- the smallest shapes at which the GPU kernels can go wrong (one cell id each) ----
def _circle(n, r, a0=0.0, a1=2 * math.pi, closed=False):
    pts = [(r * math.cos(a0 + (a1 - a0) * k / (n if closed else n - 1)), r * math.sin(a0 + (a1 - a0) * k / (n if closed else n - 1)))
           for k in range(n)]
    return pts + [pts[0]] if closed else pts


def shape_cases(cell):
    """{name: (line chips, polygon chips, expected groups)}.

    last pair      a piece of 200 vertices against a ring of 300: the only meeting segment pair is the
                   last one enumerated (last line segment x last ring segment), and the piece starts outside
    inside         the same ring, no segment meets, the piece's first vertex inside (step 4 after a full scan)
    around         the same ring, the piece around it: boxes meet, nothing else does
    piece 67       a chip of 70 one-segment pieces, only piece 67 inside the triangle (more than 64 step-4 tasks)
    chip 67        one cell holding 70 small squares with their own keys, a line inside the 67th only
    1200 groups    40 line keys x 30 polygon keys in one cell
    """
    cell = int(cell)
    n_ring = 299  # 300 vertices with the closing one
    ring_pts = _circle(n_ring, 100.0, closed=True)
    ring300 = W.geometry_wkb([[ring_pts]])
    # the last ring segment runs from vertex 298 to vertex 0; its midpoint lies at this angle
    mid = 2 * math.pi * (n_ring - 0.5) / n_ring
    outer = _circle(199, 130.0, mid - 1.5, mid)
    last = outer + [(95.0 * math.cos(mid), 95.0 * math.sin(mid))]
    meeting = [(i, j) for i in range(len(last) - 1) for j in range(len(ring_pts) - 1)
               if oracle.segments_intersect(last[i], last[i + 1], ring_pts[j], ring_pts[j + 1])]
    assert meeting == [(len(last) - 2, len(ring_pts) - 2)] and len(last) == 200 and len(ring_pts) == 300
    assert exact.locate_in_polygon(last[0], [ring_pts]) == exact.EXTERIOR
    inside = _circle(200, 50.0, 0.0, 6.0)
    around = _circle(200, 130.0, 0.0, 6.0)
    cases = {}
    for name, ln, want in (("last pair", last, True), ("inside", inside, True), ("around", around, False)):
        cases[name] = (columns([(0, cell, 0, W.linestring_wkb(ln))]), columns([(0, cell, 0, ring300)]), {(0, 0): want})
    pieces = [[(60.0 + 0.1 * k, 60.0), (90.0, 90.0 - 0.1 * k)] for k in range(70)]
    pieces[67] = [(10.0, 10.0), (20.0, 15.0)]
    cases["piece 67"] = (columns([(0, cell, 0, W.multilinestring_wkb(pieces))]), columns([(0, cell, 0, TRI)]), {(0, 0): True})
    pieces[67] = [(61.0, 61.0), (62.0, 63.0)]
    cases["no piece"] = (columns([(0, cell, 0, W.multilinestring_wkb(pieces))]), columns([(0, cell, 0, TRI)]), {(0, 0): False})
    squares = columns([(0, cell, k, W.geometry_wkb([[square(10.0 * k, 0.0, 5.0)]])) for k in range(70)])
    cases["chip 67"] = (columns([(0, cell, 0, ls((661, 1), (663, 3), (662, 4)))]), squares, {(0, k): k == 66 for k in range(70)})
    lines = columns([(0, cell, i, ls((2.5 + 10 * (i % 30), -1 if i % 3 else 1), (2.5 + 10 * (i % 30) + (i // 30) * 10, 2.5)))
                     for i in range(40)])
    polys = columns([(0, cell, k, W.geometry_wkb([[square(10.0 * k, 0.0, 5.0)]])) for k in range(30)])
    cases["1200 groups"] = (lines, polys, None)
    return cases
