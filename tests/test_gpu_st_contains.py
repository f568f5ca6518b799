"""st_contains / st_within over geometry columns on the GPU (mosaic_st_contains_geoms,
MosaicContext.st_contains_geoms / st_within_geoms): k_cont_plan, k_cont_small and k_cont_block of
mosaic_amd/csrc/st_contains.hip against (H), the sequential driver compiled by g++
(tests/contains_cases.py), out and status bit for bit -- with the default dispatch, with every pair on one
lane, with every pair on a workgroup, and there with tiles of 1, 3 and 64 segments that rings of 5 to 40
vertices straddle or end on; the split counts against the counts derived from (H); POINT rows against the
point form ctx.st_contains; and the distance-within join feeding st_contains on the NYC zones."""
import numpy as np
import pytest

from mosaic_amd import _native as N
from mosaic_amd import wkb as W

from . import contains_cases as C
from .contains_cases import HAND, OK, UNDECIDED, case_rows, expected_split, host_contains
from .test_st_distance import HOLE, SQ, poly, pt
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
    rows_l, rows_r = case_rows()[:2]
    lt, rt = ctx.geometry_table(rows_l, lines=True), ctx.geometry_table(rows_r, lines=True)
    yield lt, rt
    lt.close()
    rt.close()


def last_split():
    five = np.full(5, -1, np.int64)
    N.check(N.lib().mosaic_st_contains_last_split(N.ptr(five)))
    return tuple(int(v) for v in five)


EVERYTHING = 1 << 40
DISPATCH = ((None, None), (EVERYTHING, None), (0, None), (0, 1), (0, 3), (0, 64))


@pytest.mark.parametrize("small_work,tile", DISPATCH,
                         ids=("default dispatch", "all on one lane", "all on a workgroup", "workgroup, tile 1", "workgroup, tile 3",
                              "workgroup, tile 64"))
def test_cpu_cases(ctx, case_tables, small_work, tile):
    lt, rt = case_tables
    _, _, want, want_st, how, work = case_rows()
    assert lt.info()["n_row_path"] == 0 and rt.info()["n_row_path"] == 0
    try:
        if small_work is not None:
            ctx.set_option("dist_small_work", small_work)
        if tile is not None:
            ctx.set_option("dist_tile", tile)
        got, st = ctx.st_contains_geoms(lt, rt, return_status=True)
        split = last_split()
    finally:
        ctx.set_option("dist_small_work", 512)
        ctx.set_option("dist_tile", 16)
    bad = np.flatnonzero((got != want) | (st != want_st))
    assert got.dtype == np.bool_ and st.dtype == np.int32 and len(bad) == 0, (small_work, tile, bad[:10].tolist())
    # the hand-made cases come first, (A, B) then (B, A): their pinned status and value
    k = len(HAND)
    assert st[:k].tolist() == [c[3] for c in HAND] and got[:k].tolist() == [bool(c[4]) for c in HAND]
    assert st[k:2 * k].tolist() == [c[6] for c in HAND]
    # the split counts are those derived from (H)
    expect = expected_split(want_st, how, work, 512 if small_work is None else small_work)
    assert split == expect, (split, expect)
    ended, out, clear, undecided, workgroup = split
    assert ended + out + clear + undecided == len(want) and undecided == int((want_st == UNDECIDED).sum()) > 20
    if small_work == 0:
        assert workgroup == out + clear + int((how == C.HOW_TOUCH).sum()) > 300
    elif small_work == EVERYTHING:
        assert workgroup == 0
    else:
        assert 10 <= workgroup < 40  # the 300-ring's pairs


def test_pair_lists_pointers_and_within(ctx, case_tables):
    import torch

    lt, rt = case_tables
    rows_l, rows_r, want, want_st, _, _ = case_rows()
    n = len(want)
    # the row-wise form equals the pair list (i, i), on the host and on the device
    idx = np.arange(n)
    got, st = ctx.st_contains_geoms(lt, rt, pairs=(idx, idx), return_status=True)
    assert np.array_equal(got, want) and np.array_equal(st, want_st)
    didx = torch.from_numpy(idx).cuda()
    got, st = ctx.st_contains_geoms(lt, rt, pairs=(didx, didx), return_status=True)
    assert np.array_equal(got, want) and np.array_equal(st, want_st)
    # random pairs across the lists, either orientation; st_within is st_contains with the sides swapped
    rng = np.random.default_rng(5)
    li, ri = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    hl, hr = LCol.from_wkb(rows_l), LCol.from_wkb(rows_r)
    expect, expect_st = host_contains(hl, hr, li, ri)
    assert expect.any() and set(expect_st.tolist()) == {OK, UNDECIDED}
    got, st = ctx.st_contains_geoms(lt, rt, pairs=(li, ri), return_status=True)
    assert np.array_equal(got, expect) and np.array_equal(st, expect_st)
    dl, dr = torch.from_numpy(li).cuda(), torch.from_numpy(ri).cuda()
    got, st = ctx.st_contains_geoms(lt, rt, pairs=(dl, dr), return_status=True)
    assert np.array_equal(got, expect) and np.array_equal(st, expect_st)
    got, st = ctx.st_within_geoms(rt, lt, pairs=(dr, dl), return_status=True)
    assert np.array_equal(got, expect) and np.array_equal(st, expect_st)
    back, back_st = host_contains(hr, hl, ri, li)
    got, st = ctx.st_within_geoms(lt, rt, pairs=(li, ri), return_status=True)
    assert np.array_equal(got, back) and np.array_equal(st, back_st)
    # n = 0
    got, st = ctx.st_contains_geoms(lt, rt, pairs=(np.zeros(0, np.int64), np.zeros(0, np.int64)), return_status=True)
    assert got.shape == (0,) and st.shape == (0,) and last_split() == (0, 0, 0, 0, 0)
    # a single geometry against every row, on either side
    zone = C.kernel_cases()[0][1]
    one = LCol.from_geoms([zone] * n)
    for a, b, ha, hb in ((geom_wkb(zone), rt, one, hr), (lt, geom_wkb(zone), hl, one)):
        got, st = ctx.st_contains_geoms(a, b, return_status=True)
        expect, expect_st = host_contains(ha, hb)
        assert np.array_equal(got, expect) and np.array_equal(st, expect_st)


def test_c_entry(ctx):
    import torch

    rows = [geom_wkb(g) for g in (poly([SQ, HOLE]), poly([SQ]), poly([SQ]), line([]))]
    probe = [geom_wkb(g) for g in (pt(1, 1), line([(5, 5), (10, 5)]), poly([[(2, 2), (4, 2), (4, 4), (2, 2)]]), pt(1, 1))]
    lib = N.lib()
    with ctx.geometry_table(rows, lines=True) as lt, ctx.geometry_table(probe, lines=True) as rt:
        # host pointers; the status array is nullable
        out = np.full(4, 7, np.uint8)
        N.check(lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, None, None, 4, N.ptr(out), None))
        assert out.tolist() == [1, 0, 1, 0]
        out, st = np.full(4, 7, np.uint8), np.full(4, -1, np.int32)
        N.check(lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, None, None, 4, N.ptr(out), N.ptr(st)))
        assert out.tolist() == [1, 0, 1, 0] and st.tolist() == [OK, UNDECIDED, OK, OK]
        # device pointers for the outputs and the rows: identical
        d_out = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
        d_st = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        li, ri = torch.tensor([0, 0, 2, 1], device="cuda"), torch.tensor([2, 0, 1, 1], device="cuda")
        torch.cuda.synchronize()
        N.check(lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, N.ptr(li), N.ptr(ri), 4, N.ptr(d_out), N.ptr(d_st)))
        assert d_out.cpu().tolist() == [0, 1, 0, 0] and d_st.cpu().tolist() == [OK, OK, UNDECIDED, UNDECIDED]  # the triangle crosses the hole
        h_out, h_st = np.full(4, 7, np.uint8), np.full(4, -1, np.int32)
        hl, hr = li.cpu().numpy(), ri.cpu().numpy()
        N.check(lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, N.ptr(hl), N.ptr(hr), 4, N.ptr(h_out), N.ptr(h_st)))
        assert h_out.tolist() == d_out.cpu().tolist() and h_st.tolist() == d_st.cpu().tolist()
        # a bad index: the error code, and nothing is written
        for bad_l, bad_r in (([0, 4], [0, 0]), ([0, 0], [0, -1])):
            out, st = np.full(2, 7, np.uint8), np.full(2, -1, np.int32)
            bl, br = np.array(bad_l, np.int64), np.array(bad_r, np.int64)
            rc = lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, N.ptr(bl), N.ptr(br), 2, N.ptr(out), N.ptr(st))
            assert rc == N.MOSAIC_E_ARG and out.tolist() == [7, 7] and st.tolist() == [-1, -1]
            d_out.fill_(7)
            d_st.fill_(-1)
            torch.cuda.synchronize()
            dl, dr = torch.from_numpy(bl).cuda(), torch.from_numpy(br).cuda()
            assert lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, N.ptr(dl), N.ptr(dr), 2, N.ptr(d_out), N.ptr(d_st)) == N.MOSAIC_E_ARG
            assert d_out.cpu().tolist() == [7] * 4 and d_st.cpu().tolist() == [-1] * 4
        # one row array without the other, more row-wise pairs than rows
        one = np.zeros(1, np.int64)
        assert lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, N.ptr(one), None, 1, N.ptr(out), None) == N.MOSAIC_E_ARG
        assert lib.mosaic_st_contains_geoms(ctx.handle, lt.handle, rt.handle, None, None, 5, N.ptr(out), None) == N.MOSAIC_E_ARG


MIXED = ["POLYGON ((0 0, 10 0, 10 10, 0 10, 0 0))", None, "LINESTRING EMPTY", "POINT (5 5)", "LINESTRING (3 3)", "GEOMETRYCOLLECTION EMPTY",
         "MULTILINESTRING ((50 0, 60 0), EMPTY, (0 0, 9 9))", "MULTIPOINT ((5 5), (0 4))", "POINT EMPTY",
         "LINESTRING (-1 0, 10 0, 10 10, -1 10, -1 0)"]


def test_status_in_a_mixed_column(ctx):
    from mosaic_amd import RowPathRequired

    ok, null, path = N.ROW_OK, N.ROW_NULL, N.ROW_PATH
    other = ctx.geometry_table((np.full(len(MIXED), 5.0), np.full(len(MIXED), 5.0)))
    with ctx.geometry_table(MIXED, lines=True) as table:
        got, st = ctx.st_contains_geoms(table, other, return_status=True)
        assert st.tolist() == [ok, null, ok, ok, path, path, UNDECIDED, ok, path, UNDECIDED]
        assert got.tolist() == [True, False, False, True, False, False, False, True, False, False]
        with pytest.raises(RowPathRequired) as e:
            ctx.st_contains_geoms(table, other)
        assert e.value.rows.tolist() == [4, 5, 6, 8, 9]
        # the point on the left: only the point row and the multipoint's box question remain
        got, st = ctx.st_within_geoms(table, other, return_status=True)
        assert st.tolist() == [ok, null, ok, ok, path, path, ok, ok, path, ok]
        assert got.tolist() == [False, False, False, True, False, False, False, False, False, False]
    # a line row in a table built without lines=True stays a row for the row path
    with ctx.geometry_table(MIXED) as plain:
        got, st = ctx.st_contains_geoms(plain, other, return_status=True)
        assert st.tolist() == [ok, null, path, ok, path, path, path, ok, path, path]
        assert got.tolist() == [True, False, False, True, False, False, False, True, False, False]
    other.close()


def test_point_rows_equal_the_point_form(ctx):
    """POINT rows on the right give exactly what ctx.st_contains(geoms, points) gives: the NYC zones against
    the golden pickups and two thousand generated points, each with a zone that holds it or a random one"""
    from mosaic_amd.data import PolygonSet, quickstart_points
    from .test_st_distance import pickups

    zones = PolygonSet.load("nyc_taxi_zones_35")
    qx, qy = quickstart_points(zones, 2000, seed=11)
    x, y = np.concatenate([pickups()[0], qx]), np.concatenate([pickups()[1], qy])
    n = len(x)
    zi, pi = C.all_pairs(len(zones), n)
    inside, _ = host_contains(LCol.from_polyset(zones), LCol.from_points(x, y), zi, pi)
    holder = np.full(n, -1)
    holder[pi[inside]] = zi[inside]
    rng = np.random.default_rng(7)
    row_zone = np.where((np.arange(n) % 2 == 0) & (holder >= 0), holder, rng.integers(0, len(zones), n))
    blobs = [W.geometry_wkb(zones.parts(g)) for g in range(len(zones))]
    want = ctx.st_contains([blobs[g] for g in row_zone], (x, y))
    with ctx.geometry_table(zones) as zt, ctx.geometry_table((x, y)) as pt_:
        got, st = ctx.st_contains_geoms(zt, pt_, pairs=(row_zone, np.arange(n)), return_status=True)
        allp, allp_st = ctx.st_contains_geoms(zt, pt_, pairs=(zi, pi), return_status=True)
    assert (st == OK).all() and np.array_equal(got, want) and 500 < int(got.sum()) < n - 500
    assert (allp_st == OK).all() and np.array_equal(allp, inside)


def test_join_then_contains_finds_every_building_zone(ctx):
    """end to end: st_dwithin_join(buildings, zones, 0.0) gives the candidate pairs, st_contains_geoms(zones,
    buildings, pairs) decides them; the zones found for every building are the oracle's, and no pair the join
    omits is contained"""
    zones, buildings, contained = C.zone_buildings()
    rows = [geom_wkb(b) for b in buildings]
    with ctx.geometry_table(rows) as bt, ctx.geometry_table(zones) as zt:
        bi, zi, d = ctx.st_dwithin_join(bt, zt, 0.0)
        got, st = ctx.st_contains_geoms(zt, bt, pairs=(zi, bi), return_status=True)
        within = ctx.st_within_geoms(bt, zt, pairs=(bi, zi))
    assert (st == OK).all() and (d == 0.0).all()  # clean: nothing undecided
    assert np.array_equal(within, got)
    found = {k: set() for k in range(len(buildings))}
    for b, z, g in zip(bi, zi, got):
        if g:
            found[int(b)].add(int(z))
    assert found == {k: set(c) for k, c in enumerate(contained)}
    joined = set(zip(bi.tolist(), zi.tolist()))
    assert all((k, z) in joined for k, c in enumerate(contained) for z in c)  # the join omits no contained pair
    n_in = sum(1 for c in contained if c)
    assert 30 <= n_in <= len(buildings) - 30 and len(joined) > n_in + 20  # overlapping pairs that are not contained
