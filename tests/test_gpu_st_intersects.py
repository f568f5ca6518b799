"""st_intersects on the GPU (mosaic_st_intersects, MosaicContext.st_intersects): k_isect_plan,
k_isect_small and k_isect_block of mosaic_amd/csrc/st_intersects.hip against (H), the sequential driver
compiled by g++ (tests/intersects_cases.py), value for value -- with the default dispatch and with every
pair on k_isect_block, with the default tile and with a tile of 4 segments that rings of 5 to 40 vertices
straddle -- and the reference's invariant: st_intersects_aggregate over a chip join equals st_intersects
of the whole geometries (ST_IntersectsBehaviors.scala:45-68), on every pair."""
import ctypes

import numpy as np
import pytest

from mosaic_amd import _native as N

from . import intersects_cases as C
from .intersects_cases import EXPLICIT, case_rows, host_intersects, kernel_cases, truth_table
from .test_st_distance import poly, pt
from .test_st_distance_lines import LCol, geom_wkb, line

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


@pytest.fixture(scope="module")
def case_tables(ctx):
    rows_l, rows_r, _ = case_rows()
    lt, rt = ctx.geometry_table(rows_l, lines=True), ctx.geometry_table(rows_r, lines=True)
    yield lt, rt
    lt.close()
    rt.close()


def last_split():
    a, b, c = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    N.check(N.lib().mosaic_st_intersects_last_split(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


@pytest.mark.parametrize("tile", (None, 4), ids=("tile default", "tile 4"))
@pytest.mark.parametrize("small_work", (None, 0), ids=("default dispatch", "all on k_isect_block"))
def test_cpu_cases(ctx, case_tables, small_work, tile):
    lt, rt = case_tables
    _, _, want = case_rows()
    assert lt.info()["n_row_path"] == 0 and rt.info()["n_row_path"] == 0
    try:
        if small_work is not None:
            ctx.set_option("dist_small_work", small_work)
        if tile is not None:
            ctx.set_option("dist_tile", tile)
        got = ctx.st_intersects(lt, rt)
        split = last_split()
    finally:
        ctx.set_option("dist_small_work", 512)
        ctx.set_option("dist_tile", 16)
    bad = np.flatnonzero(got != want)
    assert got.dtype == np.bool_ and len(bad) == 0, (small_work, tile, bad[:10].tolist())
    k = len(truth_table())
    assert got[:k].tolist() == [c[3] for c in truth_table()]
    assert got[k:k + len(EXPLICIT)].tolist() == [c[3] for c in EXPLICIT]
    # the plan kernel ends the empty and the box-disjoint pairs; both other kernels see pairs unless one is switched off
    ended, one_lane, workgroup = split
    assert ended + one_lane + workgroup == len(want) and ended >= 36 * 2
    if small_work == 0:
        assert one_lane == 0 and workgroup > 300
    else:
        assert one_lane > 300 and workgroup >= 8  # the 300-ring and the frame against 25 or more facets


def test_pair_lists_broadcasting_and_no_pairs(ctx, case_tables):
    import torch

    lt, rt = case_tables
    rows_l, rows_r, want = case_rows()
    n = len(want)
    rng = np.random.default_rng(5)
    li, ri = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    hl, hr = LCol.from_wkb(rows_l), LCol.from_wkb(rows_r)
    expect = host_intersects(hl, hr, li, ri)
    assert expect.any() and not expect.all()
    assert np.array_equal(ctx.st_intersects(lt, rt, pairs=(li, ri)), expect)  # a pair list on the host
    dl, dr = torch.from_numpy(li).cuda(), torch.from_numpy(ri).cuda()
    assert np.array_equal(ctx.st_intersects(lt, rt, pairs=(dl, dr)), expect)  # and on the device
    assert np.array_equal(ctx.st_intersects(rt, lt, pairs=(dr, dl)), host_intersects(hr, hl, ri, li))
    # n = 0
    got, st = ctx.st_intersects(lt, rt, pairs=(np.zeros(0, np.int64), np.zeros(0, np.int64)), return_status=True)
    assert got.shape == (0,) and st.shape == (0,) and last_split() == (0, 0, 0)
    from mosaic_amd.data import LineSet

    with ctx.geometry_table(LineSet.from_lines([])) as none:
        assert ctx.st_intersects(none, none).shape == (0,)
    # a single geometry against every row, on either side: the frame with its wide hole
    frame = next(c[1] for c in kernel_cases() if c[0].startswith("40-star in the frame"))
    one = LCol.from_geoms([frame] * n)
    assert np.array_equal(ctx.st_intersects(geom_wkb(frame), rt), host_intersects(one, hr))
    assert np.array_equal(ctx.st_intersects(lt, geom_wkb(frame)), host_intersects(hl, one))
    assert np.array_equal(ctx.st_intersects(lt, "POINT (800 0)"), host_intersects(hl, LCol.from_geoms([pt(800, 0)] * n)))


def same_groups(lk, rk, fl, li, ri, flat):
    """every group's flag equals the flat answer, and every pair absent from the groups is flat-false"""
    groups = {(int(a), int(b)): bool(f) for a, b, f in zip(lk, rk, fl)}
    flat_of = {(int(a), int(b)): bool(f) for a, b, f in zip(li, ri, flat)}
    assert len(flat_of) == len(li) and set(groups) <= set(flat_of)
    wrong = [k for k, f in groups.items() if flat_of[k] is not f]
    missing = [k for k, f in flat_of.items() if f and k not in groups]
    assert not wrong and not missing, (wrong[:5], missing[:5])
    return groups


def test_aggregate_over_the_chip_join_equals_flat_intersects(ctx):
    """intersectsBehaviour on the 35 NYC zones against their per-zone translated copy, all 35 x 35 pairs"""
    zones, moved, left, right, res = C.invariant_zones()
    lt = ctx.chip_table(left["is_core"], left["index_id"], left["wkb"], left["polygon_key"], res)
    rt = ctx.chip_table(right["is_core"], right["index_id"], right["wkb"], right["polygon_key"], res)
    try:
        lk, rk, fl = ctx.st_intersects_aggregate(lt, rt)
    finally:
        lt.close()
        rt.close()
    li, ri = C.all_pairs(len(zones), len(moved))
    with ctx.geometry_table(zones) as zt, ctx.geometry_table(moved) as mt:
        flat = ctx.st_intersects(zt, mt, pairs=(li, ri))
        flipped = ctx.st_intersects(mt, zt, pairs=(ri, li))
    assert np.array_equal(flat, flipped)
    assert np.array_equal(flat, host_intersects(LCol.from_polyset(zones), LCol.from_polyset(moved), li, ri))
    groups = same_groups(lk, rk, fl, li, ri, flat)
    assert 35 < int(flat.sum()) < len(groups) < len(flat)


def test_line_aggregate_over_the_chip_join_equals_flat_intersects(ctx):
    """the same for 60 walks against the 35 zones through a LineChipTable, in either order"""
    from mosaic_amd.data import LineSet
    from tests import line_join_cases as JC

    geoms, zones, lines, polys, res = JC.invariant_case("H3")
    lt = ctx.line_chip_table(lines["is_core"], lines["index_id"], lines["wkb"], lines["polygon_key"], res)
    pt_ = ctx.chip_table(polys["is_core"], polys["index_id"], polys["wkb"], polys["polygon_key"], res)
    try:
        lk, pk, fl = ctx.st_intersects_aggregate(lt, pt_)
        pk2, lk2, fl2 = ctx.st_intersects_aggregate(pt_, lt)
    finally:
        lt.close()
        pt_.close()
    ls = LineSet.from_lines(geoms)
    li, ri = C.all_pairs(len(geoms), len(zones))
    with ctx.geometry_table(ls) as tt, ctx.geometry_table(zones) as zt:
        flat = ctx.st_intersects(tt, zt, pairs=(li, ri))
        flipped = ctx.st_intersects(zt, tt, pairs=(ri, li))
    assert np.array_equal(flat, flipped)
    assert np.array_equal(flat, host_intersects(LCol.from_lineset(ls), LCol.from_polyset(zones), li, ri))
    groups = same_groups(lk, pk, fl, li, ri, flat)
    same_groups(pk2, lk2, fl2, ri, li, flipped)
    assert 20 < int(flat.sum()) < len(groups) < len(flat)


MIXED = ["LINESTRING (0 0, 0 9)", None, "LINESTRING EMPTY", "POINT (0 4)", "LINESTRING (3 3)", "GEOMETRYCOLLECTION EMPTY",
         "MULTILINESTRING ((50 0, 60 0), EMPTY, (0 0, 0 9))", "POLYGON ((0 0, 10 0, 10 10, 0 10, 0 0))", "POINT EMPTY",
         "LINESTRING (-1 0, 10 0, 10 10, -1 10, -1 0)"]


def test_status_in_a_mixed_column(ctx):
    from mosaic_amd import RowPathRequired

    ok, null, path = N.ROW_OK, N.ROW_NULL, N.ROW_PATH
    other = ctx.geometry_table((np.full(len(MIXED), 0.0), np.full(len(MIXED), 4.0)))
    with ctx.geometry_table(MIXED, lines=True) as table:
        got, st = ctx.st_intersects(table, other, return_status=True)
        assert st.tolist() == [ok, null, ok, ok, path, path, ok, ok, path, ok]
        # the empty line is served and false; the closed line around (0 4) does not hold it; the polygon's boundary does
        assert got.tolist() == [True, False, False, True, False, False, True, True, False, False]
        with pytest.raises(RowPathRequired) as e:
            ctx.st_intersects(other, table)
        assert e.value.rows.tolist() == [4, 5, 8]
    # a line row in a table built without lines=True stays a row for the row path
    with ctx.geometry_table(MIXED) as plain:
        got, st = ctx.st_intersects(plain, other, return_status=True)
        assert st.tolist() == [path, null, path, ok, path, path, path, ok, path, path]
        assert got.tolist() == [False, False, False, True, False, False, False, True, False, False]
    other.close()


def test_c_entry(ctx):
    import torch

    rows = [geom_wkb(g) for g in (poly([C.SQ, C.HOLE]), line([(20, 0), (30, 0)]), pt(5, 5), line([]))]
    probe = [geom_wkb(g) for g in (pt(1, 1), pt(25, 0), pt(5, 5), pt(1, 1))]
    lib = N.lib()
    with ctx.geometry_table(rows, lines=True) as lt, ctx.geometry_table(probe) as rt:
        # the status array is nullable
        out = np.full(4, 7, np.uint8)
        N.check(lib.mosaic_st_intersects(ctx.handle, lt.handle, rt.handle, None, None, 4, N.ptr(out), None))
        assert out.tolist() == [1, 1, 1, 0]
        # device pointers for the outputs and the rows
        d_out = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
        d_st = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        li, ri = torch.tensor([0, 0, 2, 3], device="cuda"), torch.tensor([2, 0, 0, 3], device="cuda")
        torch.cuda.synchronize()
        N.check(lib.mosaic_st_intersects(ctx.handle, lt.handle, rt.handle, N.ptr(li), N.ptr(ri), 4, N.ptr(d_out), N.ptr(d_st)))
        assert d_out.cpu().tolist() == [0, 1, 0, 0] and d_st.cpu().tolist() == [N.ROW_OK] * 4  # (5 5) lies in the hole
        # a bad index: the error code, and nothing is written
        for bad_l, bad_r in (([0, 4], [0, 0]), ([0, 0], [0, -1])):
            out, st = np.full(2, 7, np.uint8), np.full(2, -1, np.int32)
            bl, br = np.array(bad_l, np.int64), np.array(bad_r, np.int64)
            rc = lib.mosaic_st_intersects(ctx.handle, lt.handle, rt.handle, N.ptr(bl), N.ptr(br), 2, N.ptr(out), N.ptr(st))
            assert rc == N.MOSAIC_E_ARG and out.tolist() == [7, 7] and st.tolist() == [-1, -1]
            d_out.fill_(7)
            torch.cuda.synchronize()
            dl, dr = torch.from_numpy(bl).cuda(), torch.from_numpy(br).cuda()
            assert lib.mosaic_st_intersects(ctx.handle, lt.handle, rt.handle, N.ptr(dl), N.ptr(dr), 2, N.ptr(d_out), None) == N.MOSAIC_E_ARG
            assert d_out.cpu().tolist() == [7] * 4
        # one row array without the other, more row-wise pairs than rows
        one = np.zeros(1, np.int64)
        assert lib.mosaic_st_intersects(ctx.handle, lt.handle, rt.handle, N.ptr(one), None, 1, N.ptr(out), None) == N.MOSAIC_E_ARG
        assert lib.mosaic_st_intersects(ctx.handle, lt.handle, rt.handle, None, None, 5, N.ptr(out), None) == N.MOSAIC_E_ARG
