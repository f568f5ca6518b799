"""TEST INFRASTRUCTURE ONLY: st_intersection_aggregate over the join of line chips with polygon chips
("how much of each trip lies in each zone"), restated in Python, an independent exact answer on the
original geometries, and the cases the host and GPU tests share.

* ``join``: the definition of mosaic_amd/csrc/line_clip.h -- per joined chip pair the whole line chip
  (polygon chip core) or clip(line chip, polygon chip); cuts by a restatement of JTS's
  RobustLineIntersector arithmetic in Python floats (IEEE doubles, no contraction) with orientation
  signs from the rationals of oracle/exact.py; midpoints located by exact.locate_in_polygon; lengths
  and runs folded in the definition's order.  Bit for bit what the host and the GPU return.
* ``flat_lengths``: the length of (original line n original polygon) in fractions.Fraction: crossing
  parameters of every segment against every ring edge, midpoints classified by
  exact.locate_in_polygon, math.sqrt of the exact squared length of each segment's inside part.
  Nothing of the chips, the cells or the clip's arithmetic enters it.
"""
import math
import struct
from fractions import Fraction

import numpy as np

from mosaic_amd import wkb as W
from oracle import exact
from tests import line_join_cases as JC

EMPTY = struct.pack(">BII", 0, 2, 0)  # LINESTRING EMPTY


# ---- JTS RobustLineIntersector.computeIntersect (llclip::meet), in Python floats ----
def _pt_dist(p, a):
    dx, dy = p[0] - a[0], p[1] - a[1]
    return math.sqrt(dx * dx + dy * dy)


def _point_to_segment(p, a, b):
    if a == b:
        return _pt_dist(p, a)
    len2 = (b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1])
    r = ((p[0] - a[0]) * (b[0] - a[0]) + (p[1] - a[1]) * (b[1] - a[1])) / len2
    if r <= 0.0:
        return _pt_dist(p, a)
    if r >= 1.0:
        return _pt_dist(p, b)
    s = ((a[1] - p[1]) * (b[0] - a[0]) - (a[0] - p[0]) * (b[1] - a[1])) / len2
    return abs(s) * math.sqrt(len2)


def _nearest_endpoint(p1, p2, q1, q2):
    best, md = p1, _point_to_segment(p1, q1, q2)
    for cand, d in ((p2, _point_to_segment(p2, q1, q2)), (q1, _point_to_segment(q1, p1, p2)), (q2, _point_to_segment(q2, p1, p2))):
        if d < md:
            md, best = d, cand
    return best


def _in_env(r, a, b):
    return min(a[0], b[0]) <= r[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= r[1] <= max(a[1], b[1])


def _intersection(p1, p2, q1, q2):
    min_x, max_x = max(min(p1[0], p2[0]), min(q1[0], q2[0])), min(max(p1[0], p2[0]), max(q1[0], q2[0]))
    min_y, max_y = max(min(p1[1], p2[1]), min(q1[1], q2[1])), min(max(p1[1], p2[1]), max(q1[1], q2[1]))
    midx, midy = (min_x + max_x) / 2.0, (min_y + max_y) / 2.0
    p1x, p1y, p2x, p2y = p1[0] - midx, p1[1] - midy, p2[0] - midx, p2[1] - midy
    q1x, q1y, q2x, q2y = q1[0] - midx, q1[1] - midy, q2[0] - midx, q2[1] - midy
    px, py, pw = p1y - p2y, p2x - p1x, p1x * p2y - p2x * p1y
    qx, qy, qw = q1y - q2y, q2x - q1x, q1x * q2y - q2x * q1y
    x, y, w = py * qw - qy * pw, qx * pw - px * qw, px * qy - qx * py
    try:
        xi, yi = x / w, y / w
        bad = math.isnan(xi) or math.isinf(xi) or math.isnan(yi) or math.isinf(yi)
    except ZeroDivisionError:
        bad = True
    r = _nearest_endpoint(p1, p2, q1, q2) if bad else (xi + midx, yi + midy)
    if not (_in_env(r, p1, p2) and _in_env(r, q1, q2)):
        r = _nearest_endpoint(p1, p2, q1, q2)
    return r


def meet(a, b, c, d):
    """The points where segment a-b meets segment c-d (0 to 2), as llclip::meet returns them."""
    if max(a[0], b[0]) < min(c[0], d[0]) or min(a[0], b[0]) > max(c[0], d[0]) or max(a[1], b[1]) < min(c[1], d[1]) or \
            min(a[1], b[1]) > max(c[1], d[1]):
        return []
    pq1, pq2 = exact.orientation(a, b, c), exact.orientation(a, b, d)
    if (pq1 > 0 and pq2 > 0) or (pq1 < 0 and pq2 < 0):
        return []
    qp1, qp2 = exact.orientation(c, d, a), exact.orientation(c, d, b)
    if (qp1 > 0 and qp2 > 0) or (qp1 < 0 and qp2 < 0):
        return []
    if pq1 == 0 and pq2 == 0 and qp1 == 0 and qp2 == 0:
        c_in, d_in, a_in, b_in = _in_env(c, a, b), _in_env(d, a, b), _in_env(a, c, d), _in_env(b, c, d)
        out = []
        if c_in and d_in:
            out = [c, d]
        elif a_in and b_in:
            out = [a, b]
        elif c_in and a_in:
            out = [c] + ([a] if c != a or not d_in else [])
        elif c_in and b_in:
            out = [c] + ([b] if c != b or not d_in else [])
        elif d_in and a_in:
            out = [d] + ([a] if d != a or not c_in else [])
        elif d_in and b_in:
            out = [d] + ([b] if d != b or not c_in else [])
        if len(out) == 2 and out[0] == out[1]:
            out = out[:1]
        return out
    if pq1 == 0 or pq2 == 0 or qp1 == 0 or qp2 == 0:
        if a == c or a == d:
            return [a]
        if b == c or b == d:
            return [b]
        return [c if pq1 == 0 else d if pq2 == 0 else a if qp1 == 0 else b]
    return [_intersection(a, b, c, d)]


# ---- the definition ----
def _bits(p):
    return struct.pack(">dd", *p)


def _box(a, b):
    return min(a[0], b[0]), min(a[1], b[1]), max(a[0], b[0]), max(a[1], b[1])


def _dedup(pts):
    return [p for k, p in enumerate(pts) if k == 0 or _bits(p) != _bits(pts[k - 1])]


def clip(pieces, parts):
    """clip(line chip, polygon chip): (length, runs as lists of points)."""
    rings = [r for rings in parts for r in rings if r]
    if not pieces or not parts or not rings:
        return 0.0, []
    gb = JC._box([p for r in rings for p in r])
    if not JC._meet(JC._box([p for ln in pieces for p in ln]), gb):
        return 0.0, []
    ring_np = [(np.asarray(r, np.float64), JC._box(r)) for rings in parts for r in rings if len(r) >= 2]
    total, runs = 0.0, []
    for ln in pieces:
        if len(ln) < 2:
            continue
        run = None  # [first segment, last segment, first cut, last cut]

        def close():
            nonlocal run
            if run:
                pts = _dedup([run[2]] + ln[run[0] + 1:run[1] + 1] + [run[3]])
                if len(pts) >= 2:
                    runs.append(pts)
            run = None

        for i, (a, b) in enumerate(zip(ln, ln[1:])):
            if a == b:
                continue
            sb = _box(a, b)
            if not JC._meet(sb, gb):
                close()
                continue
            cuts = [a, b]
            for q, rb in ring_np:
                if not JC._meet(sb, rb):
                    continue
                near = ~((np.maximum(q[:-1, 0], q[1:, 0]) < sb[0]) | (np.minimum(q[:-1, 0], q[1:, 0]) > sb[2]) |
                         (np.maximum(q[:-1, 1], q[1:, 1]) < sb[1]) | (np.minimum(q[:-1, 1], q[1:, 1]) > sb[3]))
                for j in np.nonzero(near)[0]:
                    cuts += meet(a, b, (float(q[j, 0]), float(q[j, 1])), (float(q[j + 1, 0]), float(q[j + 1, 1])))
            cuts.sort(key=lambda p: ((p[0] - a[0]) * (b[0] - a[0]) + (p[1] - a[1]) * (b[1] - a[1]), p[0], p[1], _bits(p)))
            cuts = _dedup(cuts)
            for p, q in zip(cuts, cuts[1:]):
                mid = ((p[0] + q[0]) / 2.0, (p[1] + q[1]) / 2.0)
                if any(exact.locate_in_polygon(mid, rs) != exact.EXTERIOR for rs in parts):
                    total += _pt_dist(q, p)
                    if run is None:
                        run = [i, i, p, q]
                    run[1], run[3] = i, q
                else:
                    close()
        close()
    return total, runs


def whole(pieces):
    """The whole line chip: (length, its pieces of at least 2 vertices)."""
    total, runs = 0.0, []
    for ln in pieces:
        if len(ln) < 2:
            continue
        for a, b in zip(ln, ln[1:]):
            total += _pt_dist(b, a)
        pts = _dedup(ln)
        if len(pts) >= 2:
            runs.append(pts)
    return total, runs


def runs_wkb(runs):
    if not runs:
        return EMPTY
    return W.linestring_wkb(runs[0]) if len(runs) == 1 else W.multilinestring_wkb(runs)


def wkb_runs(blob):
    """The runs of a result WKB (LINESTRING EMPTY: none)."""
    kind, g = W.read_wkb(blob)
    assert kind == "linestring", kind
    return [ln for ln in g if ln]


def join(line_chips, polygon_chips):
    """{(line key, polygon key): (length, wkb, run counts per pair)} of the chip join, folded in the
    order (cell id, line chip row, polygon chip row)."""
    by_cell = {}
    for j, (core, cell, key, blob) in enumerate(JC.rows_of(polygon_chips)):
        by_cell.setdefault(cell, []).append((j, core, key, blob))
    pairs = {}
    parts_cache = {}
    for i, (lcore, cell, lkey, lblob) in enumerate(JC.rows_of(line_chips)):
        pieces = None
        for j, pcore, pkey, pblob in by_cell.get(cell, ()):
            assert not lcore
            if pieces is None:
                pieces = JC.pieces_of(lblob)
            if pcore:
                ln, runs = whole(pieces)
            else:
                if j not in parts_cache:
                    parts_cache[j] = JC.parts_of(pblob)
                ln, runs = clip(pieces, parts_cache[j])
            pairs.setdefault((lkey, pkey), []).append(((cell, i, j), ln, runs))
    out = {}
    for g, items in pairs.items():
        items.sort(key=lambda t: t[0])
        total, runs = 0.0, []
        for _, ln, rs in items:
            total += ln
            runs += rs
        out[g] = (total, runs_wkb(runs), [len(rs) for _, _, rs in items])
    return out


def as_dict(lk, pk, length, status, wkb):
    assert not np.asarray(status).any()
    return {(int(a), int(b)): (float(v), w) for a, b, v, w in zip(lk, pk, length, wkb)}


def resum(blob, run_counts):
    """A group's length from its WKB: per pair (run_counts: runs per pair, in order) the segment
    lengths in order, then the pairs' sums in order -- the fold of the definition."""
    runs = wkb_runs(blob)
    assert sum(run_counts) == len(runs)
    total, k = 0.0, 0
    for n in run_counts:
        pair = 0.0
        for r in runs[k:k + n]:
            for a, b in zip(r, r[1:]):
                pair += _pt_dist(b, a)
        total += pair
        k += n
    return total


# ---- the independent exact answer on the original geometries ----
def _seg_params(a, b, edges):
    """Parameters in [0, 1] where segment a-b (Fractions) meets the ring edges, exactly."""
    ax, ay, bx, by = a[0], a[1], b[0], b[1]
    dx, dy = bx - ax, by - ay
    ts = {Fraction(0), Fraction(1)}
    for c, d in edges:
        cx, cy, ex, ey = Fraction(c[0]), Fraction(c[1]), Fraction(d[0]) - Fraction(c[0]), Fraction(d[1]) - Fraction(c[1])
        den = dx * ey - dy * ex
        wx, wy = cx - ax, cy - ay
        if den != 0:
            t, u = (wx * ey - wy * ex) / den, (wx * dy - wy * dx) / den
            if 0 <= t <= 1 and 0 <= u <= 1:
                ts.add(t)
        elif wx * dy - wy * dx == 0:  # collinear: the edge's ends, where they fall on the segment
            l2 = dx * dx + dy * dy
            for q in ((cx, cy), (cx + ex, cy + ey)):
                t = ((q[0] - ax) * dx + (q[1] - ay) * dy) / l2
                if 0 <= t <= 1:
                    ts.add(t)
    return sorted(ts)


def flat_length(lines, parts):
    """Length of (MULTI)LINESTRING `lines` inside the polygon `parts` (closed set), exact up to the
    final square roots: per segment math.sqrt of the exact squared length of its inside part."""
    rings = [r for rs in parts for r in rs if len(r) >= 2]
    if not rings:
        return 0.0
    gb = JC._box([p for r in rings for p in r])
    arr = [(np.asarray(r, np.float64), r) for r in rings]
    total = 0.0
    for ln in lines:
        for a, b in zip(ln, ln[1:]):
            if a == b or not JC._meet(_box(a, b), gb):
                continue
            sb = _box(a, b)
            edges = []
            for q, r in arr:
                near = ~((np.maximum(q[:-1, 0], q[1:, 0]) < sb[0]) | (np.minimum(q[:-1, 0], q[1:, 0]) > sb[2]) |
                         (np.maximum(q[:-1, 1], q[1:, 1]) < sb[1]) | (np.minimum(q[:-1, 1], q[1:, 1]) > sb[3]))
                edges += [(r[j], r[j + 1]) for j in np.nonzero(near)[0]]
            fa, fb = (Fraction(a[0]), Fraction(a[1])), (Fraction(b[0]), Fraction(b[1]))
            ts = _seg_params(fa, fb, edges)
            inside = Fraction(0)
            for t0, t1 in zip(ts, ts[1:]):
                tm = (t0 + t1) / 2
                mid = (fa[0] + tm * (fb[0] - fa[0]), fa[1] + tm * (fb[1] - fa[1]))
                if any(exact.locate_in_polygon(mid, rs) != exact.EXTERIOR for rs in parts):
                    inside += t1 - t0
            if inside:
                l2 = (fb[0] - fa[0]) ** 2 + (fb[1] - fa[1]) ** 2
                total += math.sqrt(inside * inside * l2)
    return total


_flat = {}


def flat_lengths(name):
    """{(line, polygon): exact length} of the invariant workload `name` (JC.invariant_case), computed
    once; pairs whose boxes do not meet are absent (length 0)."""
    if name not in _flat:
        geoms, zones = JC.invariant_case(name)[:2]
        parts = [zones.parts(k) for k in range(len(zones))]
        boxes = [JC._box([p for rs in ps for r in rs for p in r]) for ps in parts]
        out = {}
        for g, lines in enumerate(geoms):
            lb = JC._box([p for ln in lines for p in ln])
            for k, ps in enumerate(parts):
                if JC._meet(lb, boxes[k]):
                    out[(g, k)] = flat_length(lines, ps)
        _flat[name] = out
    return _flat[name]


def max_coordinate(name):
    geoms, zones = JC.invariant_case(name)[:2]
    m = max(abs(c) for lines in geoms for ln in lines for p in ln for c in p)
    return max(m, max(abs(c) for k in range(len(zones)) for rs in zones.parts(k) for r in rs for p in r for c in p))


def bound(name):
    """The reference's own 1e-8 (ST_IntersectionBehaviors.scala:68) in degrees; in metres the same
    figure scaled by coordinate magnitude, 1e-8 * max|coordinate| / 180."""
    return 1e-8 if name == "H3" else 1e-8 * max_coordinate(name) / 180.0


# ---- the hand table: exactly representable cuts (axis-aligned and 3-4-5 geometry, dyadic coordinates) ----
S8 = W.geometry_wkb([[JC.square(0, 0, 8)]])
HOLED8 = W.geometry_wkb([[JC.square(0, 0, 8), JC.square(3, 3, 2)]])
TRI8 = W.geometry_wkb([[JC.ring((0, 0), (8, 0), (0, 8))]])
TWO8 = W.geometry_wkb([[JC.square(0, 0, 2)], [JC.square(4, 4, 4)]])
ls = JC.ls


def _f(*pts):
    return [tuple(map(float, p)) for p in pts]


# (name, line chips of the key [wkb ...], polygon is_core, polygon wkb, length, runs)
HAND = [
    ("through a square", [ls((-2, 4), (10, 4))], 0, S8, 8.0, [_f((0, 4), (8, 4))]),
    ("through a square, 3-4-5", [ls((-3, 0), (9, 16))], 0, S8, 5.0, [_f((0, 4), (3, 8))]),
    ("wholly inside", [ls((1, 1), (4, 5), (7, 1))], 0, S8, 10.0, [_f((1, 1), (4, 5), (7, 1))]),
    ("wholly outside, boxes overlap", [ls((5, 5), (8, 8))], 0, TRI8, 0.0, []),
    ("ending on the boundary", [ls((4, 4), (8, 4))], 0, S8, 4.0, [_f((4, 4), (8, 4))]),
    ("touching at a vertex only", [ls((6, 10), (10, 6))], 0, S8, 0.0, []),
    ("collinear stretch along an edge", [ls((-2, 0), (10, 0))], 0, S8, 8.0, [_f((0, 0), (8, 0))]),
    ("through a hole", [ls((-2, 4), (10, 4))], 0, HOLED8, 6.0, [_f((0, 4), (3, 4)), _f((5, 4), (8, 4))]),
    ("a run over three segments", [ls((-2, 2), (2, 2), (2, 6), (10, 6))], 0, S8, 12.0, [_f((0, 2), (2, 2), (2, 6), (8, 6))]),
    ("the second piece only", [W.multilinestring_wkb([_f((10, 10), (12, 12)), _f((1, 1), (4, 5))])], 0, S8, 5.0, [_f((1, 1), (4, 5))]),
    ("the second polygon part only", [ls((5, 5), (5, 7))], 0, TWO8, 2.0, [_f((5, 5), (5, 7))]),
    ("multipoint chip", [W.multipoint_wkb([(1.0, 1.0), (2.0, 2.0)])], 0, S8, 0.0, []),
    ("core polygon chip without geometry", [ls((100, 100), (103, 104), (103, 110))], 1, b"", 11.0, [_f((100, 100), (103, 104), (103, 110))]),
    ("two line chips of one key in one cell", [ls((1, 1), (4, 5)), ls((1, 2), (1, 6))], 0, S8, 9.0, [_f((1, 1), (4, 5)), _f((1, 2), (1, 6))]),
    ("core polygon chip, points and a line", [W.multipoint_wkb([(1.0, 1.0)]), ls((0, 0), (0, 2))], 1, S8, 2.0, [_f((0, 0), (0, 2))]),
]


def hand_chips(cells):
    """The hand table as two chip sets: case k has line key k, polygon key k and its own cell cells[k]."""
    assert len(cells) >= len(HAND)
    lines = JC.columns([(0, int(cells[k]), k, blob) for k, h in enumerate(HAND) for blob in h[1]])
    polys = JC.columns([(h[2], int(cells[k]), k, h[3]) for k, h in enumerate(HAND)])
    return lines, polys, {(k, k): (h[4], runs_wkb(h[5])) for k, h in enumerate(HAND)}


# ---- the smallest shapes at which the GPU kernels can go wrong (one cell id each) ----
def comb(teeth, depth=4.0):
    """A comb polygon: a spine y in [-2, 0] over x in [0, 2 * teeth] with `teeth` unit-wide teeth
    rising to y = depth at x in [2k + 0.5, 2k + 1.5]; the line y = 1 crosses 2 * teeth ring edges."""
    pts = [(0.0, -2.0), (2.0 * teeth, -2.0), (2.0 * teeth, 0.0)]
    for k in range(teeth - 1, -1, -1):
        pts += [(2.0 * k + 1.5, 0.0), (2.0 * k + 1.5, depth), (2.0 * k + 0.5, depth), (2.0 * k + 0.5, 0.0)]
    pts += [(0.0, 0.0)]
    return W.geometry_wkb([[JC.ring(*pts)]])


def comb_case(cell, crossings):
    """One segment at y = 1 with `crossings` (even) crossings of a comb: every tooth is a run of length 1."""
    teeth = crossings // 2
    lines = JC.columns([(0, int(cell), 0, ls((-1, 1), (2 * teeth + 1, 1)))])
    polys = JC.columns([(0, int(cell), 0, comb(teeth))])
    runs = [_f((2 * k + 0.5, 1), (2 * k + 1.5, 1)) for k in range(teeth)]
    return lines, polys, {(0, 0): (float(teeth), runs_wkb(runs))}
