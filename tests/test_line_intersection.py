"""st_intersection_aggregate over the join of line chips (Mosaic.lineFill) with polygon chips, on the
host (mosaic_line_intersection_aggregate_host; mosaic_amd/csrc/line_clip.h is the definition): "how
much of each trip lies in each zone".  Reference: ST_IntersectionAggregate.update
(expressions/geometry/ST_IntersectionAggregate.scala:40-72) folds, per joined chip pair, the left chip
(right chip core) or the chips' intersection.  Checked exactly on hand cases with representable cuts,
bit for bit against the Python restatement of tests/line_clip_cases.py, and, like the reference's
intersectionBehaviour (ST_IntersectionBehaviors.scala:22-135), against the exact length of the flat
intersection of the original geometries."""
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mosaic_amd
from mosaic_amd import IllegalStateException, LineChipTable, MosaicContext, MosaicError, line_intersection_aggregate_host
from mosaic_amd import _native as N
from mosaic_amd import wkb as W
from oracle import exact
from tests import line_clip_cases as CC
from tests import line_join_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [1001 + k for k in range(32)]
NEW = ["mosaic_line_intersection_aggregate", "mosaic_line_intersection_aggregate_geometry", "mosaic_line_intersection_last",
       "mosaic_line_intersection_aggregate_host"]


def host(lines, polys, grid="H3", res=9):
    return line_intersection_aggregate_host(grid, lines, polys, res)


# ---- 1. the hand table: exact lengths and exact WKB ----
def test_hand_table_exact():
    lines, polys, want = CC.hand_chips(CELLS)
    lk, pk, ln, st, wkb = host(lines, polys)
    got = CC.as_dict(lk, pk, ln, st, wkb)
    for k, h in enumerate(CC.HAND):
        assert got[(k, k)] == want[(k, k)], h[0]
    assert got == want
    assert lk.dtype == np.int32 and pk.dtype == np.int32 and ln.dtype == np.float64 and st.dtype == np.uint8
    assert list(zip(lk.tolist(), pk.tolist())) == sorted(want)
    assert {g: v[:2] for g, v in CC.join(lines, polys).items()} == got


def test_touch_only_group_is_present_and_empty():
    lines, polys, _ = CC.hand_chips(CELLS)
    got = CC.as_dict(*host(lines, polys))
    k = [h[0] for h in CC.HAND].index("touching at a vertex only")
    assert got[(k, k)] == (0.0, CC.EMPTY) and CC.EMPTY == struct.pack(">BII", 0, 2, 0)
    k = [h[0] for h in CC.HAND].index("through a hole")
    assert W.read_wkb(got[(k, k)][1]) == ("linestring", CC.HAND[k][5]) and got[(k, k)][1][4] == 5  # MULTILINESTRING


def test_hand_table_every_line_against_every_polygon():
    # all rows in one cell: every line chip against every polygon chip; the restatement bit for bit
    lines, polys, _ = CC.hand_chips(CELLS)
    lines["index_id"][:] = 7
    polys["index_id"][:] = 7
    got = CC.as_dict(*host(lines, polys))
    assert len(got) == len(CC.HAND) ** 2
    assert {g: v[:2] for g, v in CC.join(lines, polys).items()} == got


def test_sum_order_is_cell_then_line_row_then_polygon_row():
    # one key pair over two cells and, in the second, two line chips and two polygon chips: rows given
    # out of order; lengths whose sum depends on the order of addition
    lines = JC.columns([(0, 9, 0, JC.ls((0, 1), (0.6, 1))), (0, 5, 0, JC.ls((0, 2), (0.1, 2))), (0, 9, 0, JC.ls((0, 3), (0.2, 3)))])
    polys = JC.columns([(0, 9, 0, CC.S8), (0, 5, 0, CC.S8), (0, 9, 0, CC.TWO8)])
    lk, pk, ln, st, wkb = host(lines, polys)
    assert CC.as_dict(lk, pk, ln, st, wkb) == {g: v[:2] for g, v in CC.join(lines, polys).items()}
    # cell 5: row 1 x row 1 (0.1); cell 9: row 0 x row 0 (0.6), row 0 x row 2 (0.6), row 2 x row 0 (0.2), row 2 x row 2 (0)
    assert len(ln) == 1 and ln[0] == (((0.1 + 0.6) + 0.6) + 0.2) + 0.0
    assert ln[0] not in (((0.6 + 0.6) + 0.1) + 0.2, ((0.6 + 0.6) + 0.2) + 0.1, ((0.1 + 0.6) + 0.2) + 0.6)  # (other orders: other bits)
    assert W.read_wkb(wkb[0])[1] == [[(0.0, 2.0), (0.1, 2.0)], [(0.0, 1.0), (0.6, 1.0)], [(0.0, 1.0), (0.6, 1.0)], [(0.0, 3.0), (0.2, 3.0)]]


def test_core_line_chip_is_refused():
    lines, polys, _ = CC.hand_chips(CELLS)
    lines["is_core"][3] = 1
    with pytest.raises(MosaicError) as e:
        host(lines, polys)
    assert e.value.code == N.MOSAIC_E_ARG and "line chip 3" in str(e.value)
    # a core line chip that joins nothing is no error: the reference's update never sees it
    lines["index_id"][3] = 999
    assert len(host(lines, polys)[0]) == len(CC.HAND) - 1


def test_empty_sides_give_no_groups():
    lines, polys, _ = CC.hand_chips(CELLS)
    none = JC.columns([])
    for a, b in ((none, polys), (lines, none), (none, none)):
        got = host(a, b)
        assert [len(x) for x in got] == [0, 0, 0, 0, 0]


class _HostLib:
    """The library with the GPU geometry call answered by the host function, on fake tables that hold
    their chip dicts: the Python dispatch of a line table on either side, without a GPU."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def mosaic_line_intersection_aggregate_geometry(self, ctx, lines, polys, out):
        def cols(c):
            off = np.ascontiguousarray(c["wkb"][0], dtype=np.int64)
            return [len(c["index_id"]), c["is_core"], c["index_id"], c["polygon_key"], off, np.ascontiguousarray(c["wkb"][1], np.uint8)]

        L, P = cols(lines), cols(polys)
        return self._lib.mosaic_line_intersection_aggregate_host(N.GRID_H3, 9, L[0], *[N.ptr(a) for a in L[1:]], P[0],
                                                                 *[N.ptr(a) for a in P[1:]], out)


def _fake(cls, chips):
    t = cls.__new__(cls)
    t.handle = chips
    return t


def test_line_table_on_the_right(monkeypatch):
    lines, polys, want = CC.hand_chips(CELLS)
    lines["polygon_key"][:] = 40 - lines["polygon_key"]  # the swapped order differs from the native one
    real = N.lib()
    monkeypatch.setattr(N, "lib", lambda: _HostLib(real))
    ctx = MosaicContext.__new__(MosaicContext)
    ctx.handle = None
    lt, pt = _fake(LineChipTable, lines), _fake(mosaic_amd.ChipTable, polys)
    lk, pk, ln, st, wkb = MosaicContext.st_intersection_aggregate(ctx, lt, pt)
    pk2, lk2, ln2, st2, wkb2 = MosaicContext.st_intersection_aggregate(ctx, pt, lt)
    assert list(zip(pk2.tolist(), lk2.tolist())) == sorted(zip(pk.tolist(), lk.tolist())) != list(zip(pk.tolist(), lk.tolist()))
    assert {(a, b): (v, w) for a, b, v, w in zip(lk2.tolist(), pk2.tolist(), ln2.tolist(), wkb2)} == \
           {(a, b): (v, w) for a, b, v, w in zip(lk.tolist(), pk.tolist(), ln.tolist(), wkb)}
    assert {(p, p): v for (_, p), v in CC.as_dict(lk, pk, ln, st, wkb).items()} == want
    lt.handle = pt.handle = None
    ctx.handle = None


def test_dispatcher_value_errors():
    ctx = MosaicContext.__new__(MosaicContext)
    ctx.handle = None
    lt, pt = _fake(LineChipTable, None), _fake(mosaic_amd.ChipTable, None)
    for call in (ctx.st_intersection_aggregate, ctx.st_intersection_aggregate_length):
        with pytest.raises(ValueError, match="line x line"):
            call(lt, lt)
    with pytest.raises(ValueError, match="LineChipTable"):
        ctx.st_intersection_aggregate_length(pt, pt)
    for a, b in ((lt, pt), (pt, lt), (lt, lt)):
        with pytest.raises(ValueError, match="st_intersection_aggregate_length"):
            ctx.st_intersection_aggregate_area(a, b)


# ---- 2. the reference's intersectionBehaviour invariant, carried to lines ----
@pytest.fixture(scope="module", params=["H3", "BNG"])
def workload(request):
    name = request.param
    geoms, zones, lines, polys, res = JC.invariant_case(name)
    return name, geoms, zones, lines, polys, CC.as_dict(*host(lines, polys, name, res)), CC.join(lines, polys)


def test_aggregate_length_equals_flat_length(workload):
    """For every group |aggregate length - exact length of (line n polygon)| is within the reference's
    own 1e-8 (ST_IntersectionBehaviors.scala:68) in degrees, and within the same figure scaled by
    coordinate magnitude (1e-8 * max|coordinate| / 180 = 3.05e-5 m) on the BNG; every flat-intersecting
    pair of positive length is a group.  Zero exceptions.  Measured on the host: the largest deviation
    is 4.2e-14 degrees (H3, 44 groups) and 1.0e-10 m (BNG, 75 groups)."""
    name, geoms, zones, lines, polys, got, _ = workload
    truth = CC.flat_lengths(name)
    bound = CC.bound(name)
    assert bound == 1e-8 if name == "H3" else 1e-6 < bound < 1e-4
    dev = {g: abs(v[0] - truth.get(g, 0.0)) for g, v in got.items()}
    print(f"{name}: {len(got)} groups, bound {bound:.3g}, largest deviation {max(dev.values()):.3g}")
    assert [g for g, d in dev.items() if not d <= bound] == []
    assert [g for g, v in truth.items() if v > 0 and g not in got] == []
    assert sum(1 for v in got.values() if v[0] > 0) >= 20 and sum(1 for v in got.values() if v[0] == 0.0) >= 10
    assert any(len(geoms[g]) > 1 for (g, _), v in got.items() if v[0] > 0)


def test_host_equals_the_restatement_bit_for_bit(workload):
    name, _, _, _, _, got, want = workload
    assert {g: v[:2] for g, v in want.items()} == got


# ---- 3. geometry consistency ----
def test_wkb_lengths_resum_to_the_length_column(workload):
    """The WKB's run lengths, summed as the definition folds them (per pair in run order, then the
    pairs in order; the runs per pair from the restatement), equal the length column bit for bit."""
    name, _, _, _, _, got, want = workload
    for g, (length, blob) in got.items():
        assert CC.resum(blob, want[g][2]) == length, g
        kind = struct.unpack_from(">I", blob, 1)[0]
        n_runs = len(CC.wkb_runs(blob))
        assert kind == (5 if n_runs > 1 else 2) and (n_runs > 0) == (length > 0)


def _edge_distance(p, rings):
    best = math.inf
    for r in rings:
        q = np.asarray(r, np.float64)
        a, d = q[:-1], q[1:] - q[:-1]
        l2 = (d * d).sum(1)
        t = np.clip(((p[0] - a[:, 0]) * d[:, 0] + (p[1] - a[:, 1]) * d[:, 1]) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0)
        best = min(best, float(np.hypot(a[:, 0] + t * d[:, 0] - p[0], a[:, 1] + t * d[:, 1] - p[1]).min()))
    return best


def test_run_vertices_lie_in_the_polygon(workload):
    """Every run vertex is not exterior to the group's polygon (exact.locate_in_polygon); a cut point,
    computed in floating point, may miss the boundary by no more than the bound of test 2."""
    name, _, zones, _, _, got, _ = workload
    bound = CC.bound(name)
    checked = 0
    for (_, k), (_, blob) in got.items():
        parts = zones.parts(k)
        for run in CC.wkb_runs(blob):
            assert len(run) >= 2 and all(a != b for a, b in zip(run, run[1:]))
            for p in run:
                checked += 1
                if all(exact.locate_in_polygon(p, rs) == exact.EXTERIOR for rs in parts):
                    assert _edge_distance(p, [r for rs in parts for r in rs]) <= bound, (k, p)
    assert checked > 100


def test_length_column_is_finite_and_status_zero(workload):
    name, _, _, lines, polys, got, _ = workload
    lk, pk, ln, st, wkb = host(lines, polys, name, JC.invariant_case(name)[4])
    assert np.isfinite(ln).all() and (ln >= 0).all() and not st.any() and all(w is not None for w in wkb)
    assert CC.as_dict(lk, pk, ln, st, wkb) == got  # a second call: the same bits


# ---- 4. the ABI, the decoder ----
def test_new_names_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mosaic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in N.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.mosaic_abi_version() == 4 and "#define MOSAIC_ABI_VERSION 4" in open(os.path.join(ROOT, "include", "mosaic_hip.h")).read()
    assert callable(mosaic_amd.line_intersection_aggregate_host) and "line_intersection_aggregate_host" in mosaic_amd.__all__
    assert callable(MosaicContext.st_intersection_aggregate_length)
    n, ms = (ctypes.c_int64 * 6)(), (ctypes.c_double * 3)()
    N.check(lib.mosaic_line_intersection_last(n, ms))
    assert 64 < n[5] < 1024  # kCutCap: "a few hundred"


ML = W.multilinestring_wkb([[(1.0, 1.0), (2.0, 2.0)], [(3.0, 3.0), (4.0, 4.0)]])
BAD_ROWS = [
    ("polygon", CC.S8, N.MOSAIC_E_WKB),
    ("truncated", ML[:-1], N.MOSAIC_E_WKB),
    ("linestring of one point", struct.pack(">BIIdd", 0, 2, 1, 1.0, 2.0), N.MOSAIC_E_WKB),
    ("NaN inside a line", W.linestring_wkb([(1.0, 1.0), (float("nan"), 2.0)]), N.MOSAIC_E_NAN),
]


@pytest.mark.parametrize("name,blob,code", BAD_ROWS, ids=[b[0] for b in BAD_ROWS])
def test_decoder_errors_pass_through(name, blob, code):
    good = JC.ls((1, 1), (4, 5))
    lines = JC.columns([(0, 5, 0, good), (0, 5, 1, good), (0, 5, 2, blob), (0, 5, 3, good)])
    polys = JC.columns([(0, 5, 0, CC.S8)])
    with pytest.raises(IllegalStateException if code == N.MOSAIC_E_NAN else MosaicError) as e:
        host(lines, polys)
    assert e.value.code == code and "line chip 2" in str(e.value)
    with pytest.raises(MosaicError) as e:
        host(JC.columns([(0, 5, 0, good)]), JC.columns([(0, 5, 0, CC.S8), (0, 5, 1, good)]))
    assert e.value.code == N.MOSAIC_E_WKB and "polygon chip 1" in str(e.value)


def test_empty_members_and_both_byte_orders():
    ml = struct.pack(">BII", 0, 5, 3) + JC.ls((-2, 4), (10, 4)) + JC.EMPTY_LINE + JC.ls((1, 1), (4, 5))
    le = struct.pack("<BII", 1, 5, 2) + W.linestring_wkb([(-2.0, 4.0), (10.0, 4.0)], big_endian=False) + \
        W.linestring_wkb([(1.0, 1.0), (4.0, 5.0)], big_endian=False)
    want = (13.0, W.multilinestring_wkb([[(0.0, 4.0), (8.0, 4.0)], [(1.0, 1.0), (4.0, 5.0)]]))
    for blob in (ml, le):
        got = CC.as_dict(*host(JC.columns([(0, 5, 0, blob)]), JC.columns([(0, 5, 0, CC.S8)])))
        assert got == {(0, 0): want}


# ---- the GPU tests' edge shapes, on the host ----
def test_combs_on_the_host():
    n, _ = (ctypes.c_int64 * 6)(), None
    N.check(N.lib().mosaic_line_intersection_last(n, None))
    for crossings in (70, int(n[5]) + 6):
        lines, polys, want = CC.comb_case(CELLS[0], crossings)
        assert CC.as_dict(*host(lines, polys)) == want
        assert want[(0, 0)][0] == crossings // 2


def test_join_shapes_on_the_host():
    for name, (lines, polys, _) in JC.shape_cases(CELLS[0]).items():
        got = CC.as_dict(*host(lines, polys))
        assert got == {g: v[:2] for g, v in CC.join(lines, polys).items()}, name
        if name == "1200 groups":
            assert len(got) == 1200 and 0 < sum(1 for v in got.values() if v[0] > 0) < 1200
    inside = CC.as_dict(*host(*JC.shape_cases(CELLS[0])["inside"][:2]))[(0, 0)]
    assert len(CC.wkb_runs(inside[1])) == 1 and len(CC.wkb_runs(inside[1])[0]) == 200 and inside[0] > 0
    assert CC.as_dict(*host(*JC.shape_cases(CELLS[0])["around"][:2]))[(0, 0)] == (0.0, CC.EMPTY)


# ---- 5. the host driver under sanitizers ----
def test_host_driver_under_sanitizers(tmp_path):
    """The comb over the cut cap and a MULTILINESTRING with an empty member through the host driver in
    a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded."""
    exe = os.path.join(str(tmp_path), "line_clip_host_main")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                    "-ffp-contract=off", "-Wno-unknown-pragmas", "-pthread", "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "line_clip_host_main.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    rows = [ln.split() for ln in run.stdout.splitlines()]
    n = (ctypes.c_int64 * 6)()
    N.check(N.lib().mosaic_line_intersection_last(n, None))
    teeth = (int(n[5]) + 6) // 2
    assert rows == [["comb", "0", "1", str(teeth), "5", str(teeth), str(9 + teeth * 41)],
                    ["members", "0", "1", "13", "5", "2", str(9 + 2 * 41)]]
