"""TEST INFRASTRUCTURE ONLY: Mosaic.lineFill restated in Python, and the seeded line generators.

The reference (core/Mosaic.scala:89-97, 146-194) flattens a line geometry, and lineDecompose walks each
component breadth-first from pointToIndex(first vertex): a cell belongs to the result when
``line.intersection(indexToGeometry(cell))`` is not empty, the kRing(1) of every such cell is tried,
and the start cell's ring is tried once when its own intersection is empty (``newTraversed.size ==
1``).  ``traverse`` below is that walk over the whole line (not the engine's per-segment spans), with

* exact orientation signs (oracle/chip_clip.py ``orient``: a float filter, then oracle/exact.py-style
  rationals) where the engine uses JTS's DD signs;
* the crossing formula of oracle/chip_clip.py (``intersection``, ``_meet``, ``_locate``);
* cells from oracle.h3_point_to_index / h3_to_geo_boundary / h3_ring1, oracle.bng_point_to_index /
  bng_kring / bng_cell_wkb.

``chip`` is JTS's overlay of a line with an area as the issue states it: the line cut at every point
where it meets the cell's boundary, a piece kept when its midpoint is inside or on the cell, each kept
piece one LineString in the line's direction, contacts that end no kept piece isolated points; pieces
win over points (divergence (a)); the line is not noded at its own crossings (divergence (b)).  Rows:
component order, then the position (segment, parameter) where the chip begins, then the cell id.
"""
import math
import os
import struct
import subprocess

import numpy as np

import oracle
from oracle import chip_clip as cc

H3, BNG = oracle.GRID_H3, oracle.GRID_BNG
_cells = {}


def cell_poly(grid, cid):
    key = (grid, int(cid))
    if key not in _cells:
        if grid == H3:
            _cells[key] = [(b * 180.0 / math.pi, a * 180.0 / math.pi) for a, b in oracle.h3_to_geo_boundary(int(cid))]
        else:
            v = struct.unpack(">10d", oracle.bng_cell_wkb(int(cid))[13:])
            _cells[key] = [(v[2 * i], v[2 * i + 1]) for i in range(4)]
    return _cells[key]


def point_cell(grid, res, p):
    if grid == H3:
        return int(oracle.h3_point_to_index(np.array([p[0]]), np.array([p[1]]), res)[0])
    return int(oracle.bng_point_to_index(p[0], p[1], res))


def ring1(grid, cid):
    r = oracle.h3_ring1(cid) if grid == H3 else oracle.bng_kring(cid, 1)
    return [int(c) for c in r]


def clean(line):
    out = []
    for p in line:
        p = (float(p[0]), float(p[1]))
        if not out or out[-1] != p:
            out.append(p)
    return out


def chip(line, C):
    """line n C for a cleaned line: None, or (kind, items, begin): kind 'lines' with a list of point
    lists, or 'points' with a list of points; begin = (segment, parameter) where the chip starts."""
    x0, x1 = min(p[0] for p in C), max(p[0] for p in C)
    y0, y1 = min(p[1] for p in C), max(p[1] for p in C)
    nodes = [(line[0], (0, 0.0), cc._locate(line[0], C) == 1, True)]  # point, position, on the boundary, a vertex
    kept = []
    for s in range(len(line) - 1):
        a, b = line[s], line[s + 1]
        ev = []
        far = max(a[0], b[0]) < x0 or min(a[0], b[0]) > x1 or max(a[1], b[1]) < y0 or min(a[1], b[1]) > y1
        if not far:
            dx, dy = b[0] - a[0], b[1] - a[1]
            for j in range(len(C)):
                for q in cc._meet(a, b, C[j], C[(j + 1) % len(C)]):
                    if q == a or q == b or any(q == e[1] for e in ev):
                        continue
                    ev.append(((q[0] - a[0]) / dx if abs(dx) >= abs(dy) else (q[1] - a[1]) / dy, q))
            ev.sort(key=lambda e: e[0])
        seq = [(a, None)] + [(q, t) for t, q in ev] + [(b, None)]
        for i in range(len(seq) - 1):
            p0, p1 = seq[i][0], seq[i + 1][0]
            mid = ((p0[0] + p1[0]) / 2, (p0[1] + p1[1]) / 2)
            kept.append((not far) and cc._locate(mid, C) != 0)
            if i + 1 < len(seq) - 1:
                nodes.append((p1, (s, seq[i + 1][1]), True, False))
            else:
                nodes.append((b, (s + 1, 0.0), (not far) and cc._locate(b, C) == 1, True))
    pieces, points, cur, begin_piece, begin_point = [], [], None, None, None
    for i, (p, pos, on, vertex) in enumerate(nodes):
        before = i > 0 and kept[i - 1]
        after = i < len(kept) and kept[i]
        if cur is not None:
            cur.append(p)
            if on or not after:
                pieces.append(cur)
                cur = None
        if after and cur is None:
            cur = [p]
            if begin_piece is None:
                begin_piece = pos
        if on and not before and not after and p not in points:
            points.append(p)
            if begin_point is None:
                begin_point = pos
    if pieces:
        return "lines", pieces, begin_piece
    if points:
        return "points", points, begin_point
    return None


def chip_wkb(kind, items):
    if kind == "lines":
        one = [struct.pack(">BII", 0, 2, len(p)) + b"".join(struct.pack(">dd", *q) for q in p) for p in items]
        return one[0] if len(one) == 1 else struct.pack(">BII", 0, 5, len(one)) + b"".join(one)
    one = [struct.pack(">BIdd", 0, 1, *q) for q in items]
    return one[0] if len(one) == 1 else struct.pack(">BII", 0, 4, len(one)) + b"".join(one)


def traverse(grid, res, line):
    """lineDecompose's traversal: {cell: chip} over a cleaned line."""
    start = point_cell(grid, res, line[0])
    queue, seen, out = [start], {start}, {}
    first = True
    while queue:
        nxt = []
        for c in queue:
            got = chip(line, cell_poly(grid, c))
            if got is not None:
                out[c] = got
            if got is not None or first:
                for nb in ring1(grid, c):
                    if nb not in seen:
                        seen.add(nb)
                        nxt.append(nb)
        first = False
        queue = nxt
    return out


def line_fill(grid, res, geoms):
    """Rows (key, cell, wkb) of grid_tessellateexplode over line geometries (lists of component lines)."""
    rows = []
    for g, lines in enumerate(geoms):
        for line in lines:
            line = clean(line)
            if not line:
                continue
            assert len(line) >= 2
            chips = traverse(grid, res, line)
            order = sorted(chips, key=lambda c: (chips[c][2][0], chips[c][2][1], c % (1 << 64)))
            rows += [(g, c, chip_wkb(chips[c][0], chips[c][1])) for c in order]
    return rows


def piece_count(grid, line, cid):
    """Items (pieces, else distinct isolated points) of a cleaned line's chip in a cell."""
    got = chip(line, cell_poly(grid, cid))
    return 0 if got is None else len(got[1])


def rows_of(chips):
    """Chip columns (mosaic_amd.tessellate) as the rows line_fill returns."""
    offs, data = chips["wkb"]
    data = np.asarray(data, np.uint8).tobytes()
    return [(int(chips["polygon_key"][i]), int(chips["index_id"][i]), data[int(offs[i]):int(offs[i + 1])])
            for i in range(len(chips["index_id"]))]


# ---- generators (seeded; coordinates rounded to 1e-6 degrees / 1 m so DD and exact signs agree) ----
def random_walks(grid, res, n, seed):
    """n geometries: random walks of 2..40 vertices spanning 1 to about 20 cells; every fifth is a
    MultiLineString of two or three walks."""
    rng = np.random.default_rng(seed)
    if grid == H3:
        step = {8: 0.004, 9: 0.0015}[res]
        origin, spread, digits = (-73.98, 40.75), 0.2, 6
    else:
        step = {3: 400.0, 4: 40.0}[res]
        origin, spread, digits = (400000.0, 300000.0), 50000.0, 0

    def walk():
        nv = int(rng.integers(2, 41))
        scale = step * float(rng.choice([0.05 if grid == H3 else 0.3, 0.3, 1.0, 3.0]))
        p = np.asarray(origin) + rng.uniform(-spread, spread, 2)
        heading = rng.uniform(0, 2 * np.pi)
        pts = [p]
        for _ in range(nv - 1):
            heading += rng.normal(0, 0.7)
            p = p + scale * rng.uniform(0.2, 1.0) * np.array([np.cos(heading), np.sin(heading)])
            pts.append(p)
        pts = np.round(np.asarray(pts), digits)
        return [(float(x), float(y)) for x, y in pts]

    geoms = []
    for g in range(n):
        geoms.append([walk() for _ in range(int(rng.integers(2, 4)) if g % 5 == 4 else 1)])
    return geoms


def length(points):
    return sum(math.hypot(b[0] - a[0], b[1] - a[1]) for a, b in zip(points, points[1:]))


def short_lines(grid, res, n, seed):
    """n geometries of one line of 2..8 vertices, each spanning a few cells (every 50th a MultiLineString)."""
    rng = np.random.default_rng(seed)
    if grid == H3:
        step, origin, spread, digits = {9: 0.002}[res], (-73.98, 40.75), 0.2, 6
    else:
        step, origin, spread, digits = {4: 60.0}[res], (400000.0, 300000.0), 50000.0, 0

    def one():
        nv = int(rng.integers(2, 9))
        p = np.asarray(origin) + rng.uniform(-spread, spread, 2)
        pts = p + np.cumsum(rng.normal(0, step, (nv, 2)), axis=0)
        pts = np.round(pts, digits)
        pts[1:][(pts[1:] == pts[:-1]).all(axis=1)] += 10.0 ** -digits  # (no line of one distinct vertex)
        return [(float(x), float(y)) for x, y in pts]

    return [[one() for _ in range(2 if g % 50 == 49 else 1)] for g in range(n)]


def bng_degenerates():
    """The exact BNG cases of tests/test_line_fill.py (integer metres, 1 km grid) as one batch."""
    return [
        [[(400100.0, 300000.0), (400900.0, 300000.0)]],
        [[(399500.0, 299500.0), (400500.0, 300500.0)]],
        [[(400200.0, 300500.0), (400500.0, 301000.0), (400800.0, 300500.0)]],
        [[(400200.0, 300500.0), (400500.0, 300800.0), (400500.0, 301500.0), (400800.0, 301500.0), (400800.0, 301000.0)]],
        [[(400200.0, 300200.0), (400800.0, 300800.0), (400800.0, 300200.0), (400200.0, 300800.0), (400200.0, 300200.0)]],
        [[(400100.0, 300100.0), (400900.0, 300100.0)], [(400100.0, 300900.0), (400900.0, 300900.0)]],
        [[(400100.0, 300100.0)] * 2 + [(400500.0, 300500.0)] * 3 + [(401500.0, 300500.0)] * 2],
    ]


def item_count(blob):
    """Pieces (or isolated points) of a chip's WKB."""
    (t,) = struct.unpack(">I", blob[1:5])
    return struct.unpack(">I", blob[5:9])[0] if t in (4, 5) else 1


# ---- inputs that reach the device walk's hand-off, its second walk and the error order ----
# H3 cells are as wide in degrees of longitude as 1 / cos(lat): along a segment near a pole the spans,
# sized by the start vertex's cell, come to cells several times narrower than themselves, and a walk
# tries more than lineclip::kWalkCap cells.  No walk of these meets a cell that is no planar polygon.
# (a, b, the spans span_count cuts a-b into)
_POLAR = {
    8: [((0.0, 89.9), (175.0, 89.5), 23)],
    9: [((0.0, 89.9), (175.0, 89.5), 56), ((0.0, 89.9), (-175.0, 89.5), 56), ((10.0, 89.6), (175.0, 88.6), 153),
        ((0.0, 89.0), (150.0, 86.5), 359)],
    10: [((-170.0, 89.9), (0.0, 89.5), 145), ((0.0, 87.0), (170.0, 80.0), 3146)],
}
POLAR_SMALL_SPANS = 153  # segments of at most this many spans are cheap enough for the Python restatement


def polar_segments(res, max_spans=None):
    """(a, b, spans): high-latitude H3 segments of which at least one span's walk tries more than
    kWalkCap cells; max_spans leaves out those cut into more spans."""
    for a, b, k in _POLAR[res]:
        if max_spans is None or k <= max_spans:
            yield a, b, k


def polar_batch(res):
    """Every polar segment of the resolution as its own geometry, a MultiLineString of two polar
    components (the first segment and the same reversed, which is cut into other spans) and an ordinary
    line in New York."""
    segs = [[a, b] for a, b, _ in polar_segments(res)]
    return [[s] for s in segs] + [[segs[0], segs[0][::-1]], [[(-73.98, 40.75), (-73.95, 40.77), (-73.9, 40.8)]]]


BNG_CORNER_DIAGONAL = [(400000.0, 300000.0), (410000.0, 310000.0)]  # resolution 4: through a lattice corner every 100 m


def bng_corner_lines():
    """The corner diagonal, three copies shifted by whole 100 m cells (every span of these emits more than
    lineclip::kSlot cells: the line touches two diagonal cells at every corner) and one shifted by half a
    cell, which passes through no corner."""
    a, b = BNG_CORNER_DIAGONAL
    shifts = [(0.0, 0.0), (300.0, 0.0), (0.0, 700.0), (-1100.0, 400.0), (50.0, 0.0)]
    return [[[(a[0] + dx, a[1] + dy), (b[0] + dx, b[1] + dy)]] for dx, dy in shifts]


# H3 resolution 5: the walk of A comes to a cell that is no planar polygon while span_count is fine with
# it; B's span_count itself fails (its first vertex's cell holds the pole).
ERROR_ORDINARY = [(-73.98, 40.75), (-73.9, 40.8)]
ERROR_A = [(0.0, 89.8), (170.0, 89.0)]
ERROR_B = [(0.0, 89.9), (175.0, 89.5)]


def error_batches():
    """Batches whose first bad geometry is number 1, found by the walk in one and by span_count in the other."""
    return [[[ERROR_ORDINARY], [ERROR_A], [ERROR_B]], [[ERROR_ORDINARY], [ERROR_B], [ERROR_A]]]


def segments_of(geoms):
    """The segments (ax, ay, bx, by) both producers walk, in their order: cleaned lines, geometry by geometry."""
    out = []
    for lines in geoms:
        for line in lines:
            line = clean(line)
            out += [(*a, *b) for a, b in zip(line, line[1:])]
    return out


def build_linewalk_caps(root, out_dir, sanitize=False):
    """Compiles tests/native/linewalk_caps_host.cpp; the program's path."""
    exe = os.path.join(str(out_dir), "linewalk_caps_san" if sanitize else "linewalk_caps")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I",
                    os.path.join(root, "mosaic_amd", "csrc"), "-o", exe,
                    os.path.join(root, "tests", "native", "linewalk_caps_host.cpp")], check=True)
    return exe


def walk_counts(exe, work_dir, grid, res, segments):
    """tests/native/linewalk_caps_host.cpp over segments (ax, ay, bx, by): (caps, per segment (K, spans)) with
    caps = dict(walk_cap, slot, items), K = -1 where span_count fails and spans = [(status, cells, bad)]."""
    path = os.path.join(str(work_dir), "linewalk_caps.bin")
    with open(path, "wb") as f:
        np.array([0 if grid == H3 else 1, res, len(segments)], np.int64).tofile(f)
        np.asarray(segments, np.float64).reshape(-1, 4).tofile(f)
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
    head = out[0].split()
    assert head[0] == "caps"
    caps = dict(walk_cap=int(head[1]), slot=int(head[2]), items=int(head[3]))
    segs = []
    for ln in out[1:]:
        t = ln.split()
        if t[0] == "segment":
            assert int(t[1]) == len(segs)
            segs.append((int(t[2]), []))
        else:
            segs[-1][1].append((int(t[0]), int(t[1]), int(t[2])))
    assert len(segs) == len(segments) and all(k < 0 or k == len(sp) for k, sp in segs)
    return caps, segs


def walk_totals(segs):
    """Of walk_counts' segments: spans, spans that need more than kWalkCap tried cells, the cells those emit."""
    spans = [sp for _, rows in segs for sp in rows]
    return len(spans), sum(sp[0] == 1 for sp in spans), sum(sp[1] for sp in spans if sp[0] == 1)
