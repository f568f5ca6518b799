"""The mixed queue's two-word entries (row, tile << 16 | leaf code): every H3 stream kernel writes
them when k_join_leaf follows, and k_join_leaf answers its leaf-line rows from the entry instead of
walking the raster again.  NYC zones at res 9; counts and pairs of every case equal the oracle's and
the generic path's (option point_raster = 0).  Runs on the MI355X box only."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from mosaic_amd import MosaicContext
from mosaic_amd.context import tessellate
from mosaic_amd.data import PolygonSet

pytestmark = pytest.mark.gpu

RES = 9
SIZES = (1, 255, 256, 257, 1023, 1025, 100003)
N_BASE = max(SIZES) + 1  # the offset views start one element in


def _oracle(c, x, y):
    """(counts, sorted row * n_polygons + key) of the oracle"""
    want, _, orow, okey = oracle.pip_join(c.oc, oracle.GRID_H3, RES, x, y, c.npoly, pairs=True, threads=8)
    return want, np.sort(orow.astype(np.int64) * c.npoly + okey)


@pytest.fixture(scope="module")
def case():
    import torch

    zones = PolygonSet.load("nyc_taxi_zones")
    ctx = MosaicContext.build("H3", "JTS")
    chips = tessellate("H3", zones, RES)
    table = ctx.chip_table(chips["is_core"], chips["index_id"], chips["wkb"], chips["polygon_key"], RES,
                           n_polygons=len(zones))
    info = table.tiles()
    assert info["leaf_lines"] > 100_000 and info["stream"] == 1, info
    offs, data = chips["wkb"]
    c = SimpleNamespace(ctx=ctx, zones=zones, table=table, npoly=len(zones), torch=torch,
                        oc=dict(index_id=chips["index_id"], is_core=chips["is_core"], polygon_key=chips["polygon_key"],
                                wkb_offsets=offs, wkb=data))
    rng = np.random.default_rng(7)
    x0, y0, x1, y1 = zones.bbox()
    # uniform points: one oracle run, shared by every prefix and offset view
    c.ux, c.uy = rng.uniform(x0, x1, N_BASE), rng.uniform(y0, y1, N_BASE)
    _, _, orow, okey = oracle.pip_join(c.oc, oracle.GRID_H3, RES, c.ux, c.uy, c.npoly, pairs=True, threads=8)
    c.urow, c.ukey = orow.astype(np.int64), okey.astype(np.int64)
    c.uxd, c.uyd = torch.from_numpy(c.ux).cuda(), torch.from_numpy(c.uy).cuda()
    # 100k points within 1e-4 degrees of zone-boundary vertices: nearly every row is pending in the
    # stream kernel (more than 64 per group) and many are queued (pushes onto a stage that already
    # holds rows: the flush before a push that does not fit, k_join_stream_cpt's run-on into its buffer)
    v = zones.xy[rng.integers(0, len(zones.xy), 100_000)]
    c.jx = v[:, 0] + rng.uniform(-1e-4, 1e-4, len(v))
    c.jy = v[:, 1] + rng.uniform(-1e-4, 1e-4, len(v))
    c.jwant = _oracle(c, c.jx, c.jy)
    c.jxd, c.jyd = torch.from_numpy(c.jx).cuda(), torch.from_numpy(c.jy).cuda()
    yield c
    table.close()
    ctx.close()


def _join(c, xd, yd):
    counts = c.ctx.pip_join_count(c.table, xd, yd)
    kernel = c.ctx.last_kernel()
    counts = counts.cpu().numpy() if hasattr(counts, "cpu") else counts
    rows, keys = c.ctx.pip_join_pairs(c.table, xd, yd)
    return counts, rows.astype(np.int64) * c.npoly + keys, kernel


def _check(c, xd, yd, want, kernel=None, what=None):
    """counts and pairs of the point-raster path (stream kernel -> k_join_leaf -> k_join_mixed) and of
    the generic path against the oracle's"""
    wcounts, wpairs = want
    try:
        for praster in (1, 0):
            c.ctx.set_option("point_raster", praster)
            counts, pairs, k = _join(c, xd, yd)
            if praster and kernel:
                assert k == kernel, (k, kernel, what)
            assert np.array_equal(counts, wcounts), (praster, what)
            assert np.array_equal(pairs, wpairs), (praster, what)
    finally:
        c.ctx.set_option("point_raster", 1)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_alignment(case, n, off):
    """Uniform points: the partial-group tail and, for fewer than 256 rows or columns that start 8
    bytes past a 16-byte boundary (off = 1), the non-vector kernel k_join_stream as the producer."""
    c = case
    m = (c.urow >= off) & (c.urow < off + n)
    want = (np.bincount(c.ukey[m], minlength=c.npoly), np.sort((c.urow[m] - off) * c.npoly + c.ukey[m]))
    kernel = "k_join_stream_cpt" if off == 0 and n >= 256 else "k_join_stream"
    _check(c, c.uxd[off:off + n], c.uyd[off:off + n], want, kernel, (n, off))


def test_every_producer(case):
    """Options stream_pipe = 0, 1, 2: k_join_stream, k_join_stream_pipe and k_join_stream_cpt queue the
    same entries -- identical counts and pairs, the oracle's -- on uniform and boundary points."""
    c = case
    x, y = np.concatenate([c.ux, c.jx]), np.concatenate([c.uy, c.jy])
    want = _oracle(c, x, y)
    xd, yd = c.torch.from_numpy(x).cuda(), c.torch.from_numpy(y).cuda()
    names = {0: "k_join_stream", 1: "k_join_stream_pipe", 2: "k_join_stream_cpt"}
    try:
        for pipe in (0, 1, 2):
            c.ctx.set_option("stream_pipe", pipe)
            counts, pairs, k = _join(c, xd, yd)
            assert k == names[pipe], (pipe, k)
            assert np.array_equal(counts, want[0]), pipe
            assert np.array_equal(pairs, want[1]), pipe
    finally:
        c.ctx.set_option("stream_pipe", 2)


def test_boundary_points_full_stages(case):
    """100k points jittered around zone-boundary vertices: many queued rows in every group."""
    c = case
    _check(c, c.jxd, c.jyd, c.jwant, "k_join_stream_cpt", "jitter")
    # the same rows through the non-vector producer
    want = _oracle(c, c.jx[1:], c.jy[1:])
    _check(c, c.jxd[1:], c.jyd[1:], want, "k_join_stream", "jitter, offset view")


def test_non_finite_rows(case):
    """NaN and +-inf rows mixed into uniform and boundary points, pairs and counts: they join nothing
    and raise nothing (H3: the reference's geoToH3 gives no cell), on every producer."""
    c = case
    x = np.concatenate([c.ux[:20_000], c.jx[:20_000]])
    y = np.concatenate([c.uy[:20_000], c.jy[:20_000]])
    x[::7] = np.nan
    y[3::11] = np.inf
    x[5::13] = -np.inf
    y[::91] = np.nan
    bad = ~(np.isfinite(x) & np.isfinite(y))
    want = _oracle(c, x, y)
    assert not bad[want[1] // c.npoly].any() and want[0].sum() > 5_000
    xd, yd = c.torch.from_numpy(x).cuda(), c.torch.from_numpy(y).cuda()
    try:
        for pipe in (2, 1, 0):
            c.ctx.set_option("stream_pipe", pipe)
            _check(c, xd, yd, want, None, ("non-finite", pipe))
    finally:
        c.ctx.set_option("stream_pipe", 2)


def test_leaf_join_off_same_counts(case):
    """Option leaf_join = 0 (one-word queue straight to k_join_mixed) and 1 give the same counts; with
    k_join_leaf the leaf-line rows do not reach the chip loop."""
    c = case
    tests = {}
    try:
        for lj in (0, 1):
            c.ctx.set_option("leaf_join", lj)
            counts, pairs, _ = _join(c, c.jxd, c.jyd)
            assert np.array_equal(counts, c.jwant[0]), lj
            assert np.array_equal(pairs, c.jwant[1]), lj
            c.ctx.pip_join_count(c.table, c.jxd, c.jyd)
            tests[lj] = c.ctx.last_stats()["contains_tests"]
    finally:
        c.ctx.set_option("leaf_join", 1)
    assert tests[1] < tests[0], tests
