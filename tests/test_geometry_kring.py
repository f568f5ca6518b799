"""grid_geometrykring / grid_geometrykloop (+explode): Mosaic.geometryKRing / geometryKLoop
(core/Mosaic.scala:111-144) over the chips of getChips(geometry, res, keepCoreGeom = false).

Expected values never come from the code under test: they are a brute force over the oracle's k-rings
(oracle.h3_kring_set, the sphere search, whose dict also gives the ring distances; oracle.bng_kring /
bng_kloop) of the chip rows the host producer tessellate(..., ctx=None) gives, by the reference's two
set formulas
    geometryKRing(k) = core + U_b kRing(b, k)
    geometryKLoop(k) = U_b kLoop(b, k) - (core + U_b kRing(b, k - 1))
with dist(c) = the smallest j such that c is in kLoop(b, j) for a border cell b.  The rows' order is
Scala 2.12 immutable HashSet iteration order (restated here in Python); no reference fixture pins it
("order unpinned").  The CPU tests run the header's sequential driver (mosaic_amd/csrc/geom_kring.h
compiled by g++, tests/native/geom_kring_host.cpp); the GPU tests run the kernels through
MosaicContext."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
from mosaic_amd import _native as N
from mosaic_amd.context import tessellate
from mosaic_amd.data import PolygonSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENTAGON_BASE_CELLS = (4, 14, 24, 38, 49, 58, 63, 72, 83, 97, 107, 117)
NEW_SYMBOLS = ("mosaic_chips_kring", "mosaic_geometry_kring", "mosaic_cell_lists_export_dist",
               "mosaic_geometry_kring_last_ms")
BNG_EDGE_POINTS = ((10.0, 10.0), (10.0, 650000.0), (699990.0, 1299990.0))


# ---- the brute force ----
@functools.lru_cache(maxsize=None)
def h3_ring(cell, k):
    return oracle.h3_kring_set(cell, k)


@functools.lru_cache(maxsize=None)
def bng_ring(cell, k):
    """{cell: smallest j with cell in kLoop(b, j)} for j <= k; its keys are oracle.bng_kring(b, k)"""
    d = {}
    for j in range(k, 0, -1):
        for c in oracle.bng_kloop(cell, j).tolist():
            d[c] = j
    d[cell] = 0
    assert set(d) == set(oracle.bng_kring(cell, k).tolist())
    return d


def brute(grid, is_core, ids, key, n_geoms, k):
    """per geometry: (kring set, {cell: dist} over it with -1 for unreached cores, kloop set or None)"""
    ring_of = h3_ring if grid == "H3" else bng_ring
    out = []
    for g in range(n_geoms):
        m = np.asarray(key) == g
        core = set(np.asarray(ids)[m & (np.asarray(is_core) != 0)].tolist())
        border = set(np.asarray(ids)[m & (np.asarray(is_core) == 0)].tolist())
        dist = {}
        for b in border:
            for c, d in ring_of(b, k).items():
                if d < dist.get(c, 1 << 30):
                    dist[c] = d
        kring = core | set(dist)
        full = {c: dist.get(c, -1) for c in kring}
        kloop = None
        if k >= 1:
            loop_cells = {c for b in border for c, d in ring_of(b, k).items() if d == k}
            if grid == "BNG":
                loop_cells = {c for b in border for c in oracle.bng_kloop(b, k).tolist()}
            inner = core | {c for b in border for c in ring_of(b, k - 1)}
            kloop = loop_cells - inner
        out.append((kring, full, kloop))
    return out


def order_key(v):
    """Scala 2.12 immutable.HashSet iteration order of a Long: the trie walks 5-bit groups of
    improve(v.##) from the lowest (scala.collection.immutable.HashSet.improve, Long.##)"""
    M = 0xffffffff
    u = v & ((1 << 64) - 1)
    lo = u & M
    iv = lo - (1 << 32) if lo >> 31 else lo
    h = lo if iv == v else (u ^ (u >> 32)) & M
    h = (h + (~(h << 9) & M)) & M
    h ^= h >> 14
    h = (h + (h << 4)) & M
    h ^= h >> 10
    key = 0
    for level in range(7):
        key = key << 5 | ((h >> (5 * level)) & 31)
    return key


def check_rows(grid, rows, dists, want, loop):
    """rows (lists of int cells) and their dists against brute()'s answer; the Scala set order"""
    assert len(rows) == len(want)
    for g, (kring, full, kloop) in enumerate(want):
        got = [int(c) for c in rows[g]]
        assert len(got) == len(set(got)), (g, "duplicates")
        assert set(got) == (kloop if loop else kring), (g, loop)
        keys = [(order_key(c), c) for c in got]
        assert keys == sorted(keys), (g, "order")
        if dists is not None:
            assert {c: int(d) for c, d in zip(got, dists[g])} == {c: full[c] for c in got}, (g, "dist")


# ---- fixtures (computed once, never modified) ----
def chips_of(grid, polys, res):
    t = tessellate(grid, polys, res, keep_core_geom=False, ctx=None)
    return (np.array(t["is_core"], np.uint8), np.array(t["index_id"], np.int64), np.array(t["polygon_key"], np.int32),
            len(polys))


@pytest.fixture(scope="module")
def nyc():
    return PolygonSet.load("nyc_taxi_zones_35")


@pytest.fixture(scope="module")
def london6():
    return PolygonSet.load("london_postcodes_bng").subset(range(6))


@pytest.fixture(scope="module")
def nyc9(nyc):
    chips = chips_of("H3", nyc, 9)
    return chips, {k: brute("H3", *chips, k) for k in (1, 2, 5)}


def pentagon_cell(bc, res):
    h = (1 << 59) | (res << 52) | (bc << 45)
    for r in range(res + 1, 16):
        h |= 7 << (3 * (15 - r))
    return h


@pytest.fixture(scope="module")
def pentagon_rows():
    """{res: cells}: the 12 pentagons and two neighbours of each, res 1-3"""
    rows = {}
    for res in (1, 2, 3):
        cells = []
        for bc in PENTAGON_BASE_CELLS:
            p = pentagon_cell(bc, res)
            cells += [p] + sorted(c for c in oracle.h3_kring_set(p, 1) if c != p)[:2]
        rows[res] = cells
    return rows


def bng_edge_cells(res):
    return [int(oracle.bng_point_to_index(e, n, res)) for e, n in BNG_EDGE_POINTS]


def point_chips(cells):
    n = len(cells)
    return np.zeros(n, np.uint8), np.array(cells, np.int64), np.arange(n, dtype=np.int32), n


# ---- CPU: the header's sequential driver ----
@pytest.fixture(scope="module")
def host_driver(tmp_path_factory):
    so = tmp_path_factory.mktemp("gk") / "libgk.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "mosaic_amd", "csrc"), "-o", str(so),
                    os.path.join(ROOT, "tests", "native", "geom_kring_host.cpp")], check=True)
    lib = ctypes.CDLL(str(so))
    vp = ctypes.c_void_p
    lib.geom_kring_host.restype = ctypes.c_int64
    lib.geom_kring_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, vp, vp, vp, ctypes.c_int64,
                                    ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int64]

    def run(grid, res, is_core, ids, key, n_geoms, k, loop):
        cap = 1 << 20
        offs = np.zeros(n_geoms + 1, np.int64)
        cells = np.zeros(cap, np.int64)
        dist = np.zeros(cap, np.int32)
        status = np.zeros(max(n_geoms, 1), np.int32)
        n = lib.geom_kring_host(1 if grid == "BNG" else 0, res, len(ids), N.ptr(is_core), N.ptr(ids), N.ptr(key),
                                n_geoms, k, loop, N.ptr(offs), N.ptr(cells), N.ptr(dist), N.ptr(status), cap)
        assert n >= 0 and offs[-1] == n
        rows = [cells[offs[g]:offs[g + 1]].tolist() for g in range(n_geoms)]
        dists = [dist[offs[g]:offs[g + 1]].tolist() for g in range(n_geoms)]
        return rows, dists, status[:n_geoms]
    return run


def host_check(host_driver, grid, res, chips, ks):
    for k in ks:
        want = brute(grid, *chips, k)
        for loop in (0, 1) if k >= 1 else (0,):
            rows, dists, status = host_driver(grid, res, *chips, k, loop)
            assert not status.any()
            check_rows(grid, rows, dists, want, loop)


def test_host_driver_h3_nyc_res8(host_driver, nyc):
    chips = chips_of("H3", nyc, 8)
    assert len(chips[1]) == 308 and int((chips[0] == 0).sum()) == 295
    host_check(host_driver, "H3", 8, chips, (0, 1, 3))


def test_host_driver_h3_pentagons(host_driver, pentagon_rows):
    for res, cells in pentagon_rows.items():
        host_check(host_driver, "H3", res, point_chips(cells), (1, 2, 3))


def test_host_driver_bng_london(host_driver, london6):
    host_check(host_driver, "BNG", 3, chips_of("BNG", london6, 3), (0, 1, 2, 3))
    host_check(host_driver, "BNG", 4, chips_of("BNG", london6, 4), (1, 2))


def test_host_driver_bng_grid_edge(host_driver):
    for res in (3, -3, 1):
        host_check(host_driver, "BNG", res, point_chips(bng_edge_cells(res)), (1, 2, 3))


def test_library_exports_new_symbols():
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in N.EXPORTS


def test_abi_version_unchanged():
    assert N.lib().mosaic_abi_version() == 4


# ---- GPU ----
@pytest.fixture(scope="module")
def h3ctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


@pytest.fixture(scope="module")
def bngctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("BNG", "JTS")
    yield c
    c.close()


@pytest.fixture(scope="module")
def nyc9_gpu_rows(h3ctx, nyc):
    """{(k, loop): (rows, dists)} of the geometry entry on the res 9 zones, default options"""
    out = {}
    for k in (1, 2, 5):
        out[k, 0] = h3ctx.grid_geometrykring(nyc, 9, k, return_distance=True)
        out[k, 1] = (h3ctx.grid_geometrykloop(nyc, 9, k), None)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 2, 5))
def test_gpu_h3_nyc_res9(nyc9, nyc9_gpu_rows, k):
    chips, want = nyc9
    assert len(chips[1]) == 1287 and int((chips[0] == 0).sum()) == 880
    rows, dists = nyc9_gpu_rows[k, 0]
    check_rows("H3", rows, dists, want[k], 0)
    check_rows("H3", nyc9_gpu_rows[k, 1][0], None, want[k], 1)


@pytest.mark.gpu
def test_gpu_h3_pentagon_point_rows(h3ctx, pentagon_rows):
    for res, cells in pentagon_rows.items():
        latlon = [oracle.h3_to_geo(c) for c in cells]
        lon = np.degrees([ll[1] for ll in latlon])
        lat = np.degrees([ll[0] for ll in latlon])
        assert h3ctx.grid_pointascellid((lon, lat), res, raw=True).tolist() == cells
        for k in (1, 2, 3):
            want = brute("H3", *point_chips(cells), k)
            rows, dists = h3ctx.grid_geometrykring((lon, lat), res, k, return_distance=True)
            check_rows("H3", rows, dists, want, 0)
            check_rows("H3", h3ctx.grid_geometrykloop((lon, lat), res, k), None, want, 1)


@pytest.mark.gpu
def test_gpu_bng_grid_edge_point_rows(bngctx):
    e = np.array([p[0] for p in BNG_EDGE_POINTS])
    n = np.array([p[1] for p in BNG_EDGE_POINTS])
    for res in (3, -3, 1):
        cells = bng_edge_cells(res)
        for k in (1, 2, 3):
            want = brute("BNG", *point_chips(cells), k)
            rows, dists = bngctx.grid_geometrykring((e, n), res, k, raw=True, return_distance=True)
            check_rows("BNG", rows, dists, want, 0)
            check_rows("BNG", bngctx.grid_geometrykloop((e, n), res, k, raw=True), None, want, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("res,ks", ((3, (0, 1, 2, 3)), (4, (1, 2))))
def test_gpu_bng_london(bngctx, london6, res, ks):
    chips = chips_of("BNG", london6, res)
    for k in ks:
        want = brute("BNG", *chips, k)
        rows, dists = bngctx.grid_geometrykring(london6, res, k, raw=True, return_distance=True)
        check_rows("BNG", rows, dists, want, 0)
        if k >= 1:
            check_rows("BNG", bngctx.grid_geometrykloop(london6, res, k, raw=True), None, want, 1)
    # formatted ids (the default) round-trip to the raw ones
    k = ks[-1]
    raw = bngctx.grid_geometrykring(london6, res, k, raw=True)
    fmt = bngctx.grid_geometrykring(london6, res, k)
    for r, f in zip(raw, fmt):
        assert all(isinstance(s, str) for s in f)
        assert [oracle.bng_parse(s) for s in f] == r.tolist()


@pytest.mark.gpu
def test_gpu_chips_entry_explode_duplicates_empty(h3ctx, nyc, nyc9_gpu_rows):
    k = 2
    rows = nyc9_gpu_rows[k, 0][0]
    loops = nyc9_gpu_rows[k, 1][0]
    chips = tessellate("H3", nyc, 9, keep_core_geom=False, ctx=h3ctx)
    by_chips = h3ctx.grid_geometrykring(dict(chips, n_geoms=len(nyc)), 9, k)
    assert [r.tolist() for r in by_chips] == [r.tolist() for r in rows]
    by_chips = h3ctx.grid_geometrykloop(chips, 9, k)  # n_geoms from the keys
    assert [r.tolist() for r in by_chips] == [r.tolist() for r in loops]
    for explode, lists in ((h3ctx.grid_geometrykringexplode, rows), (h3ctx.grid_geometrykloopexplode, loops)):
        idx, cells = explode(nyc, 9, k)
        assert idx.tolist() == [g for g, r in enumerate(lists) for _ in r]
        assert cells.tolist() == [int(c) for r in lists for c in r]
    # two identical geometries and an empty one in one batch
    one = nyc.subset([3, 3])
    ps = PolygonSet(one.xy, one.ring_offsets, one.part_rings, np.append(one.geom_parts, one.geom_parts[-1]))
    got, status = h3ctx.grid_geometrykring(ps, 9, k, return_status=True)
    assert len(got) == 3 and status.tolist() == [0, 0, 0]
    assert got[0].tolist() == got[1].tolist() == rows[3].tolist() and len(got[2]) == 0
    assert len(h3ctx.grid_geometrykloop(ps, 9, k)[2]) == 0


@pytest.mark.gpu
def test_gpu_rehash_path_and_batches(nyc, nyc9_gpu_rows):
    from mosaic_amd import MosaicContext

    ctx = MosaicContext.build("H3", "JTS")
    ctx.set_option("gk_table_log2", 4)
    for k in (1, 2, 5):
        got = ctx.grid_geometrykring(nyc, 9, k)
        assert [r.tolist() for r in got] == [r.tolist() for r in nyc9_gpu_rows[k, 0][0]]
        got = ctx.grid_geometrykloop(nyc, 9, k)
        assert [r.tolist() for r in got] == [r.tolist() for r in nyc9_gpu_rows[k, 1][0]]
    # 5,000 point rows: more than one batch of 4,094 geometries
    rng = np.random.default_rng(3)
    lon = rng.uniform(-74.25, -73.70, 5000)
    lat = rng.uniform(40.50, 40.91, 5000)
    cells = ctx.grid_pointascellid((lon, lat), 9, raw=True)
    rings = ctx.grid_cellkring(cells, 1)
    got = ctx.grid_geometrykring((lon, lat), 9, 1)
    assert len(got) == 5000
    for g in range(5000):
        assert len(got[g]) == 7 and set(got[g].tolist()) == set(rings[g].tolist()), g
    ctx.close()


@pytest.mark.gpu
def test_gpu_errors(nyc, nyc9):
    from mosaic_amd import MosaicContext, MosaicError

    ctx = MosaicContext.build("H3", "JTS")
    for k in (0, -1, 1001):
        with pytest.raises(MosaicError) as e:
            ctx.grid_geometrykloop(nyc, 9, k)
        assert e.value.code == N.MOSAIC_E_ARG
    for k in (-1, 1001):
        with pytest.raises(MosaicError) as e:
            ctx.grid_geometrykring(nyc, 9, k)
        assert e.value.code == N.MOSAIC_E_ARG
    # a chip of another resolution: its row is refused, its neighbours are answered
    (is_core, ids, key, _), want = nyc9
    m = key < 3
    ids3 = ids[m].copy()
    first_of_1 = int(np.flatnonzero(key[m] == 1)[0])
    ids3[first_of_1] = int(oracle.h3_point_to_index(np.array([-73.95]), np.array([40.7]), 8)[0])
    chips = dict(is_core=is_core[m], index_id=ids3, polygon_key=key[m], n_geoms=3)
    with pytest.raises(MosaicError, match="not a valid cell"):
        ctx.grid_geometrykring(chips, 9, 2)
    rows, status = ctx.grid_geometrykring(chips, 9, 2, return_status=True)
    assert status.tolist() == [0, -2, 0] and len(rows[1]) == 0
    for g in (0, 2):
        assert set(rows[g].tolist()) == want[2][g][0]
    # the table cap: the call returns MOSAIC_E_CAPACITY
    ctx.set_option("gk_max_cells", 64)
    with pytest.raises(MosaicError) as e:
        ctx.grid_geometrykring(nyc, 9, 1)
    assert e.value.code == N.MOSAIC_E_CAPACITY
    ctx.close()
