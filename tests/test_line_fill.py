"""Mosaic.lineFill on the host (mosaic_tessellate_lines, mosaic_amd/csrc/lineclip.h): chips of
LineString / MultiLineString geometries against the Python restatement of the reference's traversal
and of JTS's line / area overlay (tests/line_cases.py).

Unpinned: nothing here runs JTS, and the reference's own tests (MosaicExplodeBehaviors.scala:143-208)
assert row counts only, so the piece order and direction are the restatement's, derived from JTS's
algorithm.  Pinned divergences: (a) mixed cells give their pieces, (b) self-crossings do not split
pieces, (c) a cell over the antimeridian is MOSAIC_E_ARG."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mosaic_amd import IllegalStateException, MosaicError
from mosaic_amd import _native as N
from mosaic_amd import wkb as W
from mosaic_amd.context import tessellate
from mosaic_amd.data import LineSet
from tests import line_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [("H3", LC.H3, 8), ("H3", LC.H3, 9), ("BNG", LC.BNG, 3), ("BNG", LC.BNG, 4)]
_walks = {}


def walks(name, grid, res):
    """(geometries, the host producer's rows, the oracle's rows), computed once per grid."""
    if (name, res) not in _walks:
        geoms = LC.random_walks(grid, res, 30, 20250117 + res)
        got = LC.rows_of(tessellate(name, LineSet.from_lines(geoms), res))
        _walks[(name, res)] = (geoms, got, LC.line_fill(grid, res, geoms))
    return _walks[(name, res)]


def host_rows(name, geoms, res, **kw):
    return LC.rows_of(tessellate(name, LineSet.from_lines(geoms), res, **kw))


def chip_lines(blob):
    kind, g = W.read_wkb(blob)
    return g if kind == "linestring" else []


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_random_walks_equal_the_oracle(name, grid, res):
    geoms, got, want = walks(name, grid, res)
    assert len(want) > len(geoms)
    assert sum(len(g) > 1 for g in geoms) >= 5  # MultiLineStrings among them
    per_line = [sum(1 for r in want if r[0] == g) / len(lines) for g, lines in enumerate(geoms)]
    assert min(per_line) >= 1 and max(per_line) >= 10  # from one cell to many
    assert got == want


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_chips_tile_the_line(name, grid, res):
    geoms, got, _ = walks(name, grid, res)
    for g, lines in enumerate(geoms):
        total = sum(LC.length(LC.clean(ln)) for ln in lines)
        # (a piece that runs along a cell side is in both cells' chips: counted once)
        pieces = {tuple(p) for r in got if r[0] == g for p in chip_lines(r[2])}
        assert abs(sum(LC.length(p) for p in pieces) - total) <= 1e-9 * total
    # every computed crossing point ends a piece in two chips of its component, bit for bit
    for g, lines in enumerate(geoms):
        if len(lines) != 1:
            continue
        verts = set(LC.clean(lines[0]))
        ends = {}
        for i, r in enumerate(x for x in got if x[0] == g):
            for p in chip_lines(r[2]):
                for q in (p[0], p[-1]):
                    if q not in verts:
                        ends.setdefault(q, set()).add(i)
        assert all(len(v) >= 2 for v in ends.values()), [k for k, v in ends.items() if len(v) < 2]


def test_reference_first_point_on_boundary():
    # MosaicExplodeBehaviors.scala:189: the first vertex lies on its cell's boundary
    text = open(os.path.join(ROOT, "tests", "golden", "line_first_point_on_boundary.wkt")).read().strip()
    ls = LineSet.from_wkt([text])
    got = LC.rows_of(tessellate("H3", ls, 8))
    assert len(got) >= 1
    assert got == LC.line_fill(LC.H3, 8, [ls.lines(0)])


# ---- exact BNG degenerates: integer metres on the 1 km grid (resolution 3) ----
def cell_at(x, y):
    return LC.point_cell(LC.BNG, 3, (x, y))


def bng3(geoms):
    got = host_rows("BNG", geoms, 3)
    assert got == LC.line_fill(LC.BNG, 3, geoms)
    return got


def test_line_along_a_cell_side_belongs_to_both_cells():
    line = [(400100.0, 300000.0), (400900.0, 300000.0)]
    got = bng3([[line]])
    assert {r[1] for r in got} == {cell_at(400500, 300500), cell_at(400500, 299500)}
    assert all(r[2] == W.linestring_wkb(line) for r in got)


def test_line_through_a_cell_corner_touches_the_diagonal_cells():
    got = bng3([[[(399500.0, 299500.0), (400500.0, 300500.0)]]])
    by_cell = {r[1]: r[2] for r in got}
    corner = W.point_wkb(400000.0, 300000.0)
    assert by_cell[cell_at(399500, 300500)] == corner and by_cell[cell_at(400500, 299500)] == corner
    assert by_cell[cell_at(399500, 299500)] == W.linestring_wkb([(399500.0, 299500.0), (400000.0, 300000.0)])
    assert by_cell[cell_at(400500, 300500)] == W.linestring_wkb([(400000.0, 300000.0), (400500.0, 300500.0)])
    assert len(got) == 4


def test_vertex_on_a_side_splits_the_piece():
    a, v, b = (400200.0, 300500.0), (400500.0, 301000.0), (400800.0, 300500.0)
    got = bng3([[[a, v, b]]])
    by_cell = {r[1]: r[2] for r in got}
    assert by_cell[cell_at(400500, 300500)] == W.multilinestring_wkb([[a, v], [v, b]])
    assert by_cell[cell_at(400500, 301500)] == W.point_wkb(*v)
    assert len(got) == 2


def test_mixed_cell_keeps_its_pieces():
    # divergence (a): the lower cell holds a piece and, where the line comes back down to end on its top
    # side, an isolated point; the reference would drop the chip (GeometryCollection -> POLYGON EMPTY)
    line = [(400200.0, 300500.0), (400500.0, 300800.0), (400500.0, 301500.0), (400800.0, 301500.0), (400800.0, 301000.0)]
    got = bng3([[line]])
    by_cell = {r[1]: r[2] for r in got}
    assert by_cell[cell_at(400500, 300500)] == W.linestring_wkb([line[0], line[1], (400500.0, 301000.0)])
    assert by_cell[cell_at(400500, 301500)] == W.linestring_wkb([(400500.0, 301000.0)] + line[2:])
    assert len(got) == 2


def test_figure_eight_is_one_linestring():
    # divergence (b): JTS would node the line at its own crossing
    line = [(400200.0, 300200.0), (400800.0, 300800.0), (400800.0, 300200.0), (400200.0, 300800.0), (400200.0, 300200.0)]
    got = bng3([[line]])
    assert got == [(0, cell_at(400500, 300500), W.linestring_wkb(line))]


def test_multilinestring_components_sharing_a_cell_give_two_rows():
    l1 = [(400100.0, 300100.0), (400900.0, 300100.0)]
    l2 = [(400100.0, 300900.0), (400900.0, 300900.0)]
    got = bng3([[l1, l2], [l1]])
    c = cell_at(400500, 300500)
    assert got == [(0, c, W.linestring_wkb(l1)), (0, c, W.linestring_wkb(l2)), (1, c, W.linestring_wkb(l1))]


def test_repeated_vertices_are_removed():
    a, b, c = (400100.0, 300100.0), (400500.0, 300500.0), (401500.0, 300500.0)
    assert bng3([[[a, a, b, b, b, c, c]]]) == bng3([[[a, b, c]]])


# ---- errors and options ----
def test_empty_component_gives_no_chips():
    l1 = [(400100.0, 300100.0), (400900.0, 300100.0)]
    assert host_rows("BNG", [[[], l1, []], [[]], [l1]], 3) == host_rows("BNG", [[l1], [], [l1]], 3)
    assert len(host_rows("BNG", [], 3)) == 0


def test_one_vertex_component_is_an_argument_error():
    for line in ([(400100.0, 300100.0)], [(400100.0, 300100.0)] * 3):
        with pytest.raises(MosaicError) as e:
            host_rows("BNG", [[[(0.0, 0.0), (5.0, 5.0)]], [line]], 3)
        assert e.value.code == N.MOSAIC_E_ARG and "geometry 1" in str(e.value)


def test_nan_is_an_illegal_state():
    for name, res in (("BNG", 3), ("H3", 9)):
        with pytest.raises(IllegalStateException) as e:
            host_rows(name, [[[(1.0, 2.0), (float("nan"), 3.0)]]], res)
        assert e.value.code == N.MOSAIC_E_NAN


def test_line_over_the_antimeridian_is_an_argument_error():
    # divergence (c)
    with pytest.raises(MosaicError) as e:
        host_rows("H3", [[[(10.0, 10.0), (10.001, 10.001)]], [[(179.95, 10.0), (179.999, 10.02)]]], 7)
    assert e.value.code == N.MOSAIC_E_ARG and "geometry 1" in str(e.value)


def test_cells_only_gives_the_same_rows_without_wkb():
    geoms, got, _ = walks("H3", LC.H3, 9)
    bare = host_rows("H3", geoms, 9, cells_only=True)
    assert [r[:2] for r in bare] == [r[:2] for r in got]
    assert all(r[2] == b"" for r in bare)


# ---- wrapper ----
def test_lineset_and_wkb_round_trips():
    geoms = [[[(1.0, 2.0), (3.5, -4.25), (5.0, 6.0)]], [[(0.0, 0.0), (1.0, 1.0)], [(2.0, 2.0), (3.0, 3.0), (4.0, 5.0)]]]
    ls = LineSet.from_lines(geoms)
    assert len(ls) == 2 and ls.lines(0) == geoms[0] and ls.lines(1) == geoms[1]
    assert ls.wkb(0) == W.linestring_wkb(geoms[0][0]) and ls.wkb(1) == W.multilinestring_wkb(geoms[1])
    for big in (True, False):
        back = LineSet.from_wkb([ls.wkb(g, big) for g in range(2)])
        assert [back.lines(g) for g in range(2)] == geoms
    text = ["LINESTRING (1 2, 3.5 -4.25, 5 6)", "MULTILINESTRING ((0 0, 1 1), (2 2, 3 3, 4 5))"]
    back = LineSet.from_wkt(text)
    assert [back.lines(g) for g in range(2)] == geoms
    assert len(LineSet.from_wkt(["LINESTRING EMPTY"]).lines(0)) == 0
    assert W.read_wkb(W.multilinestring_wkb(geoms[1])) == ("linestring", geoms[1])
    assert struct.unpack(">BI", ls.wkb(1)[:5]) == (0, 5)
    with pytest.raises(ValueError):
        LineSet.from_wkt(["POINT (1 2)"])


def test_tessellate_dispatches_on_lineset_and_abi_stays():
    line = [(400100.0, 300100.0), (400900.0, 300100.0)]
    chips = tessellate("BNG", LineSet.from_lines([[line]]), 3, ctx=None)
    assert set(chips) == {"is_core", "index_id", "polygon_key", "wkb"}
    assert chips["is_core"].tolist() == [0] and chips["polygon_key"].tolist() == [0]
    assert chips["index_id"].tolist() == [cell_at(400500, 300500)]
    assert N.lib().mosaic_abi_version() == 4
    for name in ("mosaic_tessellate_lines", "mosaic_tessellate_lines_gpu", "mosaic_tess_lines_last",
                 "mosaic_tess_lines_last_walk"):
        assert name in N.EXPORTS


# ---- the piece builder with a deliberately small workspace ----
def zigzag(n, x0=400100.0, x1=400900.0, y_lo=299900.0, y_hi=300100.0):
    """n vertices alternating across the side y = 300000 of two cells: n - 1 pieces in each."""
    xs = np.linspace(x0, x1, n).round()
    return [(float(x), y_hi if i % 2 else y_lo) for i, x in enumerate(xs)]


def caps_verdicts(exe, tmp_path, line, cells, cap):
    path = os.path.join(str(tmp_path), "caps_lines.bin")
    cxy = np.zeros((len(cells), 32))
    for k, c in enumerate(cells):
        cxy[k, :2 * len(c)] = np.asarray(c).ravel()
    with open(path, "wb") as f:
        np.array([len(line), len(cells), cap], np.int64).tofile(f)
        np.asarray(line, np.float64).tofile(f)
        np.array([len(c) for c in cells], np.int64).tofile(f)
        cxy.tofile(f)
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout
    return [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_piece_builder_reports_needs_more_exactly(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "lineclip_caps")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I",
                    os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "lineclip_caps_host.cpp")], check=True)
    cells = [LC.cell_poly(LC.BNG, cell_at(400500, 300500)), LC.cell_poly(LC.BNG, cell_at(400500, 299500)),
             LC.cell_poly(LC.BNG, cell_at(402500, 300500))]
    touching = [(400100.0 + 100 * i, 300000.0 if i % 2 else 299900.0) for i in range(14)]  # points only, above
    seen = set()
    for line in (zigzag(2), zigzag(5), zigzag(9), zigzag(10), zigzag(40), touching):
        for cap in (1, 4, 8, 0):
            rows = caps_verdicts(exe, tmp_path, line, cells, cap)
            for C, (status, n, has_piece) in zip(cells, rows):
                got = LC.chip(line, C)
                want = 0 if got is None else len(got[1])
                more = want > (cap or 8)
                assert status == (1 if more else 0)
                if not more:
                    assert n == want and has_piece == int(got is not None and got[0] == "lines")
                seen.add((more, want > 0, got is not None and got[0] == "points"))
    assert {(True, True, False), (False, True, False), (False, False, False), (True, True, True), (False, True, True)} <= seen


# ---- inputs of the device walk's hand-off, its second walk and the error order (tests/test_gpu_line_fill.py) ----
@pytest.fixture(scope="module")
def walk_caps(tmp_path_factory):
    """tests/native/linewalk_caps_host.cpp, compiled once, and once under ASan / UBSan for the small inputs:
    walk_caps(grid, res, segments, checked=False) = (constants, per segment (K, spans))."""
    d = tmp_path_factory.mktemp("linewalk")
    plain, san = LC.build_linewalk_caps(ROOT, d), LC.build_linewalk_caps(ROOT, d, sanitize=True)

    def run(grid, res, segments, checked=False):
        got = LC.walk_counts(plain, d, grid, res, segments)
        assert not checked or LC.walk_counts(san, d, grid, res, segments) == got
        return got

    return run


@pytest.mark.parametrize("res", [8, 9])
def test_polar_segments_equal_the_oracle(res):
    geoms = [[[a, b]] for a, b, _ in LC.polar_segments(res, LC.POLAR_SMALL_SPANS)]
    assert len(geoms) == {8: 1, 9: 3}[res]
    got = host_rows("H3", geoms, res)
    assert {r[0] for r in got} == set(range(len(geoms)))
    assert got == LC.line_fill(LC.H3, res, geoms)


@pytest.mark.parametrize("res", [8, 9, 10])
def test_polar_segments_need_more_than_the_walk_cap(walk_caps, res):
    """Pins that the inputs keep reaching the hand-off if a constant moves: every segment of the table has
    a span whose walk tries more than kWalkCap cells, and no walk of the GPU tests' batch (which adds a
    reversed segment and an ordinary line) meets a bad cell, so the host producer is a reference there."""
    table = list(LC.polar_segments(res))
    caps, segs = walk_caps(LC.H3, res, LC.segments_of(LC.polar_batch(res)), checked=res == 8)
    assert caps == dict(walk_cap=64, slot=8, items=8)
    assert all(k > 0 and not any(r[0] == 2 or r[2] for r in rows) and all(r[1] >= 1 for r in rows) for k, rows in segs)
    for (a, b, spans), (k, rows) in zip(table, segs):
        assert k == spans == len(rows)
        assert sum(r[0] == 1 for r in rows) >= 1, (a, b)


def test_bng_corner_diagonal_exceeds_the_slot_in_every_span(walk_caps):
    lines = LC.bng_corner_lines()
    caps, segs = walk_caps(LC.BNG, 4, LC.segments_of(lines), checked=True)
    for k, rows in segs[:4]:
        assert k == 50 and all(r[0] == 0 and not r[2] and caps["slot"] < r[1] <= caps["walk_cap"] for r in rows)
    assert segs[4][0] == 50 and all(r[0] == 0 and not r[2] for r in segs[4][1])
    # the suite's other BNG line has no such span
    _, (long_one,) = walk_caps(LC.BNG, 4, [(380013.0, 290007.0, 415021.0, 309013.0)])
    assert long_one[0] == 176 and max(r[1] for r in long_one[1]) <= caps["slot"]
    got = host_rows("BNG", lines[:1] + lines[4:], 4)
    assert got == LC.line_fill(LC.BNG, 4, lines[:1] + lines[4:])


def test_error_batches_name_the_first_bad_geometry(walk_caps):
    _, (fine, a, b) = walk_caps(LC.H3, 5, LC.segments_of([[LC.ERROR_ORDINARY], [LC.ERROR_A], [LC.ERROR_B]]), checked=True)
    assert fine[0] >= 1 and not any(r[0] or r[2] for r in fine[1])
    assert a[0] >= 1 and any(r[2] for r in a[1])  # span_count is fine with A; its walk meets a bad cell
    assert b[0] == -1  # span_count fails
    for geoms in LC.error_batches():
        with pytest.raises(MosaicError) as e:
            host_rows("H3", geoms, 5)
        assert e.value.code == N.MOSAIC_E_ARG and str(e.value).startswith("geometry 1:")
