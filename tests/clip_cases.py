"""Inputs that drive the GPU border clip (k_tess_clip_ll) to its hand-off paths, and the host helper
that predicts a lane's verdict (tests/native/llclip_caps_host.cpp: llclip::clip with the device's
workspace).  Shared by tests/test_clip_caps.py (CPU) and tests/test_gpu_clip_handoff.py (GPU)."""
import math
import os
import subprocess

import numpy as np

import oracle
from mosaic_amd.data import PolygonSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_D64 = (64 << 20) // (6 * 64 * 16)  # candidates per chunk of the H3 session at densify 64: 10,922


def one_ring_each(rings):
    """A PolygonSet of single-shell geometries (closed rings)."""
    xy = np.vstack(rings)
    ro = np.zeros(len(rings) + 1, np.int64)
    ro[1:] = np.cumsum([len(r) for r in rings])
    idx = np.arange(len(rings) + 1, dtype=np.int64)
    return PolygonSet(np.ascontiguousarray(xy, np.float64), ro, idx.copy(), idx.copy())


def concat(a, b):
    """Geometries of a, then those of b."""
    return PolygonSet(np.vstack([a.xy, b.xy]),
                      np.concatenate([a.ring_offsets, b.ring_offsets[1:] + a.ring_offsets[-1]]),
                      np.concatenate([a.part_rings, b.part_rings[1:] + a.part_rings[-1]]),
                      np.concatenate([a.geom_parts, b.geom_parts[1:] + a.geom_parts[-1]]))


def comb(period, x0=-73.99, y0=40.70, width=0.02, base=0.001, top=0.02):
    """One closed counter-clockwise ring: a base bar y0 .. y0 + base over x0 .. x0 + width with
    width / period teeth of width period / 2 up to y0 + top, at x0 + t * period."""
    n = int(round(width / period))
    pts = [(x0, y0), (x0 + width, y0), (x0 + width, y0 + base)]
    for t in range(n - 1, -1, -1):
        xa = x0 + t * period
        xb = xa + period / 2
        pts += [(xb, y0 + base), (xb, y0 + top), (xa, y0 + top), (xa, y0 + base)]
    pts[-1] = pts[0]  # (the first tooth's left side runs down to (x0, y0): 4 n + 3 vertices, closed)
    return np.array(pts, np.float64)


def wavy_circles(n_geoms, n_vertices, cx=-73.9, cy=40.7, step=0.05, radius=0.012, ky=0.76, centres=None):
    """n_geoms rings of n_vertices vertices around (cx + step g, cy), or around centres[g]: radius
    radius * (1 + 0.2 sin 7a) in x, times ky in y; counter-clockwise, closed."""
    a = np.linspace(0.0, 2.0 * np.pi, n_vertices, endpoint=False)
    r = radius * (1.0 + 0.2 * np.sin(7.0 * a))
    rings = []
    for g in range(n_geoms):
        x, y = (cx + step * g, cy) if centres is None else centres[g]
        ring = np.column_stack([x + r * np.cos(a), y + ky * r * np.sin(a)])
        rings.append(np.vstack([ring, ring[:1]]))
    return one_ring_each(rings)


def h3_cell_degrees(cid):
    """indexToGeometry's vertices of an H3 cell: (lon, lat) degrees, counter-clockwise, open."""
    return [(b * 180.0 / math.pi, a * 180.0 / math.pi) for a, b in oracle.h3_to_geo_boundary(int(cid))]


def bng_squares(polys, e):
    """(geometry, square) for every e-metre grid square that meets a geometry's envelope."""
    out = []
    for g in range(len(polys)):
        r0 = polys.part_rings[polys.geom_parts[g]]
        r1 = polys.part_rings[polys.geom_parts[g + 1]]
        xy = polys.xy[polys.ring_offsets[r0]:polys.ring_offsets[r1]]
        i0, j0 = math.floor(xy[:, 0].min() / e), math.floor(xy[:, 1].min() / e)
        i1, j1 = math.floor(xy[:, 0].max() / e), math.floor(xy[:, 1].max() / e)
        for j in range(j0, j1 + 1):
            for i in range(i0, i1 + 1):
                x, y = i * e, j * e
                out.append((g, [(x, y), (x + e, y), (x + e, y + e), (x, y + e)]))
    return out


def build_caps_helper(tmp_dir):
    exe = os.path.join(str(tmp_dir), "llclip_caps")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I",
                    os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "llclip_caps_host.cpp")], check=True)
    return exe


def lane_verdicts(exe, tmp_dir, polys, cells, lonlat):
    """What a device lane decides for each (geometry, cell polygon) of cells: an int array of rows
    (status, chains, rings, vertices, polygons, is_cell); status 0 = clipped on the device."""
    path = os.path.join(str(tmp_dir), "caps_input.bin")
    cxy = np.zeros((len(cells), 32), np.float64)
    for k, (_, c) in enumerate(cells):
        cxy[k, :2 * len(c)] = np.asarray(c, np.float64).ravel()
    with open(path, "wb") as f:
        np.array([len(polys), len(polys.part_rings) - 1, len(polys.ring_offsets) - 1, len(polys.xy), len(cells),
                  int(lonlat)], np.int64).tofile(f)
        for a in (polys.geom_parts, polys.part_rings, polys.ring_offsets):
            np.ascontiguousarray(a, np.int64).tofile(f)
        np.ascontiguousarray(polys.xy, np.float64).tofile(f)
        np.array([g for g, _ in cells], np.int64).tofile(f)
        np.array([len(c) for _, c in cells], np.int64).tofile(f)
        cxy.tofile(f)
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout
    rows = np.array([[int(v) for v in line.split()] for line in out.splitlines()], np.int64).reshape(-1, 6)
    assert len(rows) == len(cells)
    return rows


def h3_border_verdicts(exe, tmp_dir, polys, chips):
    """lane_verdicts over the border chips (is_core == 0) of a host tessellation of polys."""
    border = np.nonzero(np.asarray(chips["is_core"]) == 0)[0]
    cells = [(int(chips["polygon_key"][i]), h3_cell_degrees(chips["index_id"][i])) for i in border]
    return lane_verdicts(exe, tmp_dir, polys, cells, True)
