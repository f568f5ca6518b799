"""st_intersects_aggregate over the join of line chips (Mosaic.lineFill) with polygon chips, on the
host (mosaic_line_intersects_aggregate_host, mosaic_amd/csrc/line_isect.h): "which trips cross which
zones".  Reference: ST_IntersectsAggregate.update (expressions/geometry/ST_IntersectsAggregate.scala:
28-39) decodes whatever WKB a chip holds and folds ``l.is_core || p.is_core || l.wkb intersects
p.wkb`` with OR over the equi-join on index_id; getChips sends line geometries to lineFill
(core/Mosaic.scala:21-35).  Checked against the Python restatement of tests/line_join_cases.py (exact
rationals on the hand cases) and, like the reference's intersectsBehaviour
(ST_IntersectsBehaviors.scala:13-61), against flat intersects of the original geometries."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from mosaic_amd import MosaicError, IllegalStateException, line_intersects_aggregate_host
from mosaic_amd import _native as N
from mosaic_amd import wkb as W
from tests import line_join_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [1001 + k for k in range(32)]
NEW = ["mosaic_line_chips_create", "mosaic_line_chips_info", "mosaic_line_chips_destroy", "mosaic_line_intersects_aggregate",
       "mosaic_line_join_last", "mosaic_line_join_team", "mosaic_line_intersects_aggregate_host"]


def host(lines, polys, grid="H3", res=9):
    return line_intersects_aggregate_host(grid, lines, polys, res)


# ---- the hand table ----
def test_hand_table_flags():
    lines, polys, want = JC.hand_chips(CELLS)
    lk, pk, fl = host(lines, polys)
    got = JC.as_dict(lk, pk, fl)
    for k, h in enumerate(JC.HAND):
        assert got[(k, k)] == h[5], h[0]
    assert got == want
    assert got == JC.join(lines, polys, exact_segments=True)


def test_hand_table_every_line_against_every_polygon():
    # all rows in one cell: 16 x 16 chip pairs, the same (line, polygon) keys
    lines, polys, _ = JC.hand_chips(CELLS)
    lines["index_id"][:] = 7
    polys["index_id"][:] = 7
    got = JC.as_dict(*host(lines, polys))
    assert len(got) == len(JC.HAND) ** 2
    assert got == JC.join(lines, polys, exact_segments=True)


def test_empty_line_group_exists():
    lines, polys, _ = JC.hand_chips(CELLS)
    got = JC.as_dict(*host(lines, polys))
    k = [h[0] for h in JC.HAND].index("empty line against a border chip")
    assert (k, k) in got and got[(k, k)] is False


# ---- grouping ----
def test_grouping_and_order():
    lines, polys, want = JC.grouping_chips(CELLS)
    lk, pk, fl = host(lines, polys)
    assert JC.as_dict(lk, pk, fl) == want
    assert list(zip(lk.tolist(), pk.tolist())) == sorted(want)
    assert lk.dtype == np.int32 and pk.dtype == np.int32 and fl.dtype == bool


def raw_host(lines, polys, cap):
    def cols(c):
        return [len(c["index_id"]), c["is_core"], c["index_id"], c["polygon_key"], np.ascontiguousarray(c["wkb"][0], np.int64),
                np.ascontiguousarray(c["wkb"][1], np.uint8)]

    L, P = cols(lines), cols(polys)
    lk, pk, fl = np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7, np.int32), np.zeros(max(cap, 1), np.uint8)
    n_out = ctypes.c_int64(-1)
    rc = N.lib().mosaic_line_intersects_aggregate_host(N.GRID_H3, 9, L[0], *[N.ptr(a) for a in L[1:]], P[0],
                                                       *[N.ptr(a) for a in P[1:]], N.ptr(lk), N.ptr(pk), N.ptr(fl), cap,
                                                       ctypes.byref(n_out))
    return rc, int(n_out.value), lk


def test_capacity_protocol():
    lines, polys, want = JC.grouping_chips(CELLS)
    rc, n, lk = raw_host(lines, polys, len(want) - 1)
    assert rc == N.MOSAIC_E_CAPACITY and n == len(want)
    assert (lk == -7).all()  # nothing written
    rc, n, _ = raw_host(lines, polys, 0)
    assert rc == N.MOSAIC_E_CAPACITY and n == len(want)
    rc, n, _ = raw_host(lines, polys, len(want))
    assert rc == N.MOSAIC_OK and n == len(want)


def test_empty_sides_give_no_groups():
    lines, polys, _ = JC.grouping_chips(CELLS)
    none = JC.columns([])
    for a, b in ((none, polys), (lines, none), (none, none)):
        lk, pk, fl = host(a, b)
        assert len(lk) == len(pk) == len(fl) == 0


# ---- the decoder ----
def little_endian(blob):
    """A big-endian 2D WKB geometry rewritten in little-endian byte order."""
    def geom(pos):
        assert blob[pos] == 0
        (t,) = struct.unpack_from(">I", blob, pos + 1)
        out, pos = struct.pack("<BI", 1, t), pos + 5
        if t == 1:
            return out + struct.pack("<2d", *struct.unpack_from(">2d", blob, pos)), pos + 16
        (n,) = struct.unpack_from(">I", blob, pos)
        out, pos = out + struct.pack("<I", n), pos + 4
        for _ in range(n):
            if t == 2:
                piece, pos = struct.pack("<2d", *struct.unpack_from(">2d", blob, pos)), pos + 16
            elif t == 3:
                (m,) = struct.unpack_from(">I", blob, pos)
                piece = struct.pack("<I", m) + struct.pack(f"<{2 * m}d", *struct.unpack_from(f">{2 * m}d", blob, pos + 4))
                pos += 4 + 16 * m
            else:
                piece, pos = geom(pos)
            out += piece
        return out, pos

    out, end = geom(0)
    assert end == len(blob)
    return out


def test_both_byte_orders_give_identical_results():
    lines, polys, want = JC.hand_chips(CELLS)
    assert all(r[3][0] == 0 for r in JC.rows_of(lines) + JC.rows_of(polys))
    l2 = JC.columns([(r[0], r[1], r[2], little_endian(r[3])) for r in JC.rows_of(lines)])
    p2 = JC.columns([(r[0], r[1], r[2], little_endian(r[3])) for r in JC.rows_of(polys)])
    assert W.read_wkb(JC.rows_of(l2)[2][3]) == W.read_wkb(JC.rows_of(lines)[2][3])
    for a, b in ((lines, polys), (l2, p2), (l2, polys), (lines, p2)):
        assert JC.as_dict(*host(a, b)) == want


def test_iso_z_and_ewkb_flags_are_skipped():
    line3d = struct.pack("<BII", 1, 1002, 2) + struct.pack("<6d", 10, 10, 5, 90, 90, 5)
    ewkb = struct.pack("<BIII", 1, 2 | 0x20000000 | 0x80000000, 4326, 2) + struct.pack("<6d", 10, 10, 5, 90, 90, 5)
    point_m = struct.pack(">BI3d", 0, 2001, 50.0, 50.0, 9.0)
    lines = JC.columns([(0, 5, 0, line3d), (0, 5, 1, ewkb), (0, 5, 2, point_m)])
    polys = JC.columns([(0, 5, 0, JC.TRI)])
    assert JC.as_dict(*host(lines, polys)) == {(0, 0): True, (1, 0): True, (2, 0): True}


def test_empty_geometries_are_empty_chips():
    nan = float("nan")
    empties = [b"", JC.EMPTY_LINE, W.point_wkb(nan, nan), struct.pack(">BII", 0, 4, 0), struct.pack(">BII", 0, 5, 0),
               W.multipoint_wkb([(nan, nan)]), struct.pack(">BII", 0, 5, 1) + JC.EMPTY_LINE]
    lines = JC.columns([(0, 5, k, e) for k, e in enumerate(empties)])
    polys = JC.columns([(0, 5, 0, JC.TRI), (1, 5, 1, JC.TRI)])
    got = JC.as_dict(*host(lines, polys))
    assert got == {(k, p): bool(p) for k in range(len(empties)) for p in (0, 1)}
    # a MULTIPOINT / MULTILINESTRING skips its empty members and keeps the others
    mixed = [W.multipoint_wkb([(nan, nan), (20.0, 20.0)]),
             struct.pack(">BII", 0, 5, 2) + JC.EMPTY_LINE + JC.ls((10, 10), (20, 15))]
    lines = JC.columns([(0, 5, k, e) for k, e in enumerate(mixed)])
    assert JC.as_dict(*host(lines, JC.columns([(0, 5, 0, JC.TRI)]))) == {(0, 0): True, (1, 0): True}


ML = W.multilinestring_wkb([[(1.0, 1.0), (2.0, 2.0)], [(3.0, 3.0), (4.0, 4.0)]])
BAD_ROWS = [
    ("polygon", JC.TRI, N.MOSAIC_E_WKB),
    ("multipolygon", JC.TWO, N.MOSAIC_E_WKB),
    ("geometry collection", struct.pack(">BII", 0, 7, 0), N.MOSAIC_E_WKB),
    ("unknown type", struct.pack(">BII", 0, 17, 0), N.MOSAIC_E_WKB),
    ("bad byte order", b"\x02" + ML[1:], N.MOSAIC_E_WKB),
    ("truncated", ML[:-1], N.MOSAIC_E_WKB),
    ("truncated header", ML[:3], N.MOSAIC_E_WKB),
    ("point count beyond the buffer", struct.pack(">BII", 0, 2, 1 << 30) + b"\0" * 32, N.MOSAIC_E_WKB),
    ("linestring of one point", struct.pack(">BIIdd", 0, 2, 1, 1.0, 2.0), N.MOSAIC_E_WKB),
    ("point inside a multilinestring", struct.pack(">BII", 0, 5, 1) + W.point_wkb(1.0, 2.0), N.MOSAIC_E_WKB),
    ("line inside a multipoint", struct.pack(">BII", 0, 4, 1) + JC.ls((1, 1), (2, 2)), N.MOSAIC_E_WKB),
    ("NaN inside a line", W.linestring_wkb([(1.0, 1.0), (float("nan"), 2.0)]), N.MOSAIC_E_NAN),
    ("NaN inside a multilinestring", W.multilinestring_wkb([[(1.0, 1.0), (2.0, 2.0)], [(3.0, float("nan")), (4.0, 4.0)]]),
     N.MOSAIC_E_NAN),
]


@pytest.mark.parametrize("name,blob,code", BAD_ROWS, ids=[b[0] for b in BAD_ROWS])
def test_decoder_errors_name_the_row(name, blob, code):
    good = JC.ls((10, 10), (90, 90))
    lines = JC.columns([(0, 5, 0, good), (0, 5, 1, good), (0, 5, 2, blob), (0, 5, 3, good)])
    polys = JC.columns([(0, 5, 0, JC.TRI)])
    with pytest.raises(IllegalStateException if code == N.MOSAIC_E_NAN else MosaicError) as e:
        host(lines, polys)
    assert e.value.code == code and "line chip 2" in str(e.value)


def test_negative_key_and_bad_polygon_chip():
    good = JC.ls((10, 10), (90, 90))
    polys = JC.columns([(0, 5, 0, JC.TRI)])
    with pytest.raises(MosaicError) as e:
        host(JC.columns([(0, 5, 0, good), (0, 5, -1, good)]), polys)
    assert e.value.code == N.MOSAIC_E_ARG and "line chip 1" in str(e.value)
    # the polygon side accepts what mosaic_chip_table_create accepts: a line chip there is malformed
    with pytest.raises(MosaicError) as e:
        host(JC.columns([(0, 5, 0, good)]), JC.columns([(0, 5, 0, JC.TRI), (0, 5, 1, good)]))
    assert e.value.code == N.MOSAIC_E_WKB and "polygon chip 1" in str(e.value)


def test_every_prefix_is_malformed_under_sanitizers(tmp_path):
    """Every non-empty proper prefix of a MULTILINESTRING and of a MULTIPOINT (both byte orders, with
    and without Z) returns MOSAIC_E_WKB without a sanitizer report; the empty prefix is the
    zero-length row, an empty chip by definition.  A stand-alone program: nothing is preloaded."""
    exe = os.path.join(str(tmp_path), "line_chips_prefix")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                    "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "line_chips_prefix_host.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    rows = [ln.split() for ln in run.stdout.splitlines()]
    assert len(rows) == 8
    for name, n, refused, whole, pieces, empty in rows:
        assert int(n) > 40 and n == refused, name
        assert int(whole) == N.MOSAIC_OK and int(empty) == N.MOSAIC_OK
        assert int(pieces) == (2 if name.startswith("multilinestring") else 3)


# ---- the reference's invariant on lines: the aggregate equals flat intersects of the originals ----
@pytest.mark.parametrize("name", ["H3", "BNG"])
def test_aggregate_equals_flat_intersects(name):
    """intersectsBehaviour (ST_IntersectsBehaviors.scala:13-61) carried over to lines: for every group
    the flag equals intersects(line, polygon) on the original geometries, and every intersecting pair
    is a group.  Zero disagreements: a condition, not a measurement.  (Chip clipping rounds crossing
    points, so a line grazing a zone boundary within ulps of a cell side could disagree: none of the
    seeds 20250301..20250310 (H3) and 20250301..20250316 (BNG) tried on the host gave one.  Among them
    20250308 (H3) and 20250313 (BNG) were taken for their counts of true and false groups: at BNG
    resolution 4 most chips of a postcode area are core, and few seeds give ten false groups.)"""
    geoms, zones, lines, polys, res = JC.invariant_case(name)
    lk, pk, fl = host(lines, polys, name, res)
    got = JC.as_dict(lk, pk, fl)
    truth = JC.flat(geoms, zones)
    wrong = [g for g, f in got.items() if f != truth[g]]
    assert wrong == []
    missing = [g for g, f in truth.items() if f and g not in got]
    assert missing == []
    n_true = sum(got.values())
    assert n_true >= 10 and len(got) - n_true >= 10
    assert list(zip(lk.tolist(), pk.tolist())) == sorted(got)
    # multi-component lines are among the true groups' lines
    assert any(len(geoms[g]) > 1 for (g, _), f in got.items() if f)


# ---- ABI ----
def test_new_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mosaic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert "typedef struct mosaic_line_chips mosaic_line_chips;" in text
    assert lib.mosaic_abi_version() == 4
    import mosaic_amd

    assert mosaic_amd.LineChipTable is not None and callable(mosaic_amd.line_intersects_aggregate_host)


# ---- the GPU tests' edge shapes, on the host ----
def test_edge_shapes_on_the_host():
    for name, (lines, polys, want) in JC.shape_cases(CELLS[0]).items():
        got = JC.as_dict(*host(lines, polys))
        if want is None:
            want = JC.join(lines, polys, exact_segments=True)
            assert len(want) == 1200 and 0 < sum(want.values()) < 1200
        assert got == want, name
