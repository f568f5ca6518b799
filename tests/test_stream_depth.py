"""The stream kernels of the chip join (mosaic_amd/csrc/join_stream.hip) at every pipeline depth,
residue and overflow.  They are software pipelines: a wave takes T full 256-row groups through two
(H3) or three (BNG) sets of pending rows, a group with more than 64 pending rows takes an overflow
set and one with more than 128 a second, and a drain and an unpipelined partial group follow.
Option stream_grid = 1 with stream_block = 64 makes the stream kernel one wave, so T = n // 256 and
the partial group has n % 256 rows: depth and residue are functions of n alone.

Small tables (35 NYC taxi zones at H3 res 9, 36 London postcode zones at BNG res 4) and base arrays
of 14 groups + 255 rows made of four row classes:

  R  resolved: uniform over the zones' bbox widened by 20 %
  P  pending, answered from the raster: zone vertices jittered (+-1e-4 degrees, +-half a BNG cell)
  M  pending and queued: points exactly on a zone's exterior ring (a vertex, or the exactly
     representable midpoint of an edge) at which the oracle's keys differ a small step to either
     side.  The point's raster cell cannot carry one pure code (it would be wrong on one side, which
     tests/test_tiles_selfcheck.py rules out), so the stream kernel has to queue the row
  N  H3: NaN / +-inf rows (join nothing, raise nothing); BNG: coordinates <= -1 or >= 1e7 (outside
     the one-to-one range: queued by the first stage without becoming pending).  Two BNG rows with
     a coordinate in (-1, 0) ride along (Z): the reference's toInt gives 0, inside the range, so the
     first stage answers them and does not queue them

Every case is a prefix or offset view of a base array; its expected counts and sorted
row * n_polygons + key pairs are the oracle's pairs of that base array, masked.  Every comparison
is exact equality.  Runs on the MI355X box only."""
from contextlib import contextmanager
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from mosaic_amd import MosaicContext
from mosaic_amd._native import IllegalStateException
from mosaic_amd.context import tessellate
from mosaic_amd.data import PolygonSet

pytestmark = pytest.mark.gpu

R_, P_, M_, N_, Z_ = 0, 1, 2, 3, 4
GROUPS = 14
N_BASE = GROUPS * 256 + 255
# (M rows, where, N rows) of each 256-row group, filled up with P and R.  Every M count around the
# set sizes (64, 128, 192); M rows as the group's first rows, its last rows, in row slot 3 alone
# (row - group base >= 128 and odd: the slot's compaction offsets start past zero), in the odd slots
# first, or anywhere; a run of three groups (6-8) and one of four (10-13) with >= 129 M rows each
RECIPES = [(0, "first", 0), (1, "first", 3), (63, "last", 0), (64, "slot3", 0), (65, "first", 0), (127, "last", 0),
           (129, "last", 0), (191, "first", 0), (192, "last", 0), (128, "first", 0), (193, "first", 0),
           (256, "first", 0), (160, "odd", 5), (255, "spread", 0)]
G193 = 10  # the group of recipe "193 M"
TAIL = (70, "spread", 2)  # the 255 rows after the groups
DEFAULTS = dict(stream_grid=0, stream_block=1024, stream_pipe=2, leaf_join=1, bng_cpt=1)
DEPTH_SIZES = sorted({min(256 * t + r, N_BASE) for t in range(1, GROUPS + 1) for r in (0, 1, 255)})
H3_KERNELS = {0: "k_join_stream", 1: "k_join_stream_pipe", 2: "k_join_stream_cpt"}
BNG_KERNELS = {0: "k_join_stream_bng", 1: "k_join_stream_bng_cpt"}
# 3 workgroups of 16 waves: three sweeps of 3 * 4096 rows, one more full group and one row
N_TILED = 3 * 4096 * 3 + 257


@contextmanager
def _options(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


def _positions(rng, m, where, n):
    if where == "first":
        return np.arange(m)
    if where == "last":
        return np.arange(n - m, n)
    if where == "slot3":  # rows wb + 128 + 2 lane + 1
        return 129 + 2 * np.arange(m)
    if where == "odd":  # slots 3 and 1 full, the rest in the even rows
        return np.concatenate([np.arange(129, 256, 2), np.arange(1, 128, 2), np.arange(0, 256, 2)])[:m]
    return rng.choice(n, m, replace=False)


def _key_sets(rows, keys, n):
    out = [set() for _ in range(n)]
    for r, k in zip(rows.tolist(), keys.tolist()):
        out[r].add(k)
    return out


def _m_rows(g, rng, step, want):
    """Points exactly on an exterior ring whose oracle keys differ `step` to either side of the edge
    (asserted): vertices and exactly representable edge midpoints, `want` of them (repeats when the
    zones have fewer)."""
    px, py, nx, ny = [], [], [], []
    for z in range(len(g.zones)):
        for rings in g.zones.parts(z):
            ring = rings[0]
            for i in range(len(ring) - 1):
                (ax, ay), (bx, by) = ring[i], ring[i + 1]
                d = float(np.hypot(bx - ax, by - ay))
                if d == 0.0:
                    continue
                cand = [(ax, ay)]
                mx, my = 0.5 * (ax + bx), 0.5 * (ay + by)
                if Fraction(mx) * 2 == Fraction(ax) + Fraction(bx) and Fraction(my) * 2 == Fraction(ay) + Fraction(by):
                    cand.append((mx, my))
                for x, y in cand:
                    px.append(x), py.append(y), nx.append(-(by - ay) / d), ny.append((bx - ax) / d)
    px, py, nx, ny = (np.array(v) for v in (px, py, nx, ny))
    if len(px) > 4 * want:  # enough candidates: test a sample
        pick = rng.choice(len(px), 4 * want, replace=False)
        px, py, nx, ny = px[pick], py[pick], nx[pick], ny[pick]
    n = len(px)
    sx = np.concatenate([px + step * nx, px - step * nx])
    sy = np.concatenate([py + step * ny, py - step * ny])
    _, _, orow, okey = oracle.pip_join(g.oc, g.grid, g.res, sx, sy, g.npoly, pairs=True)
    sets = _key_sets(orow, okey, 2 * n)
    keep = np.array([sets[i] != sets[n + i] for i in range(n)])
    assert keep.sum() >= 200, (int(keep.sum()), n)
    kept = np.nonzero(keep)[0]
    pick = rng.choice(kept, want, replace=len(kept) < want)
    assert all(sets[i] != sets[n + i] for i in pick)
    return px[pick], py[pick]


def _n_rows(g, rng, want):
    x0, y0, x1, y1 = g.zones.bbox()
    x, y = rng.uniform(x0, x1, want), rng.uniform(y0, y1, want)
    cls = np.full(want, N_)
    if g.grid == oracle.GRID_H3:
        k = np.arange(want) % 6
        for j, v in enumerate((np.nan, np.inf, -np.inf)):
            x[k == j] = v
            y[k == 3 + j] = v
    else:
        k = np.arange(want) % 8
        for j, v in enumerate((-1.0, -150000.0, 1e7, 2.5e9)):
            x[k == j] = v
        for j, v in enumerate((-1.5, 1.2e7)):
            y[k == 4 + j] = v
        # a coordinate in (-1, 0) is inside the range (the reference's toInt gives 0): answered by the
        # first stage, not queued, so not an N row
        x[k == 6] = -0.5
        y[k == 7] = -0.25
        cls[k >= 6] = Z_
    return x, y, cls


def _base_arrays(g, rng, jitter, step):
    """g.base["fwd"] / ["rev"]: the recipes' groups in order and reversed, then the tail; one oracle
    run each.  g.tiled: the forward array repeated to N_TILED rows (its groups drift by one row per
    repeat), one more oracle run."""
    x0, y0, x1, y1 = g.zones.bbox()
    wx, wy = 0.1 * (x1 - x0), 0.1 * (y1 - y0)
    parts = RECIPES + [TAIL]
    n_m = sum(p[0] for p in parts)
    mx, my = _m_rows(g, rng, step, n_m)
    bx, by, bcls = _n_rows(g, rng, sum(p[2] for p in parts))
    m_at = b_at = 0
    groups = []
    for k, (m, where, bad) in enumerate(parts):
        n = 256 if k < GROUPS else 255
        cls = np.where(rng.random(n) < 0.5, R_, P_)
        mpos = _positions(rng, m, where, n)
        cls[mpos] = M_
        rest = np.nonzero(cls != M_)[0]
        if bad:
            cls[rng.choice(rest, bad, replace=False)] = N_
        x, y = rng.uniform(x0 - wx, x1 + wx, n), rng.uniform(y0 - wy, y1 + wy, n)
        p = cls == P_
        v = g.zones.xy[rng.integers(0, len(g.zones.xy), int(p.sum()))]
        x[p] = v[:, 0] + rng.uniform(-jitter, jitter, len(v))
        y[p] = v[:, 1] + rng.uniform(-jitter, jitter, len(v))
        x[mpos], y[mpos] = mx[m_at:m_at + m], my[m_at:m_at + m]
        m_at += m
        b = cls == N_
        x[b], y[b], cls[b] = bx[b_at:b_at + bad], by[b_at:b_at + bad], bcls[b_at:b_at + bad]
        b_at += bad
        groups.append((x, y, cls))
    g.base = {}
    for name, order in (("fwd", list(range(GROUPS))), ("rev", list(range(GROUPS))[::-1])):
        gs = [groups[k] for k in order] + [groups[GROUPS]]
        g.base[name] = _array(g, *(np.concatenate([q[j] for q in gs]) for j in range(3)))
        g.base[name].group_at = {k: 256 * i for i, k in enumerate(order)}
    f = g.base["fwd"]
    reps = -(-N_TILED // N_BASE)
    g.tiled = _array(g, *(np.tile(v, reps)[:N_TILED] for v in (f.x, f.y, f.cls)))


def _array(g, x, y, cls):
    _, _, orow, okey = oracle.pip_join(g.oc, g.grid, g.res, x, y, g.npoly, pairs=True)
    b = SimpleNamespace(x=x, y=y, cls=cls, row=orow.astype(np.int64), key=okey.astype(np.int64),
                        xd=g.torch.from_numpy(x).cuda(), yd=g.torch.from_numpy(y).cuda(),
                        queued=np.concatenate([[0], np.cumsum((cls == M_) | (cls == N_))]))
    if g.grid == oracle.GRID_H3:
        assert not (cls[b.row] == N_).any()  # non-finite rows join nothing
    return b


def _want(b, off, n, npoly, kmul=1):
    m = (b.row >= off) & (b.row < off + n)
    key = b.key[m] * kmul
    return np.bincount(key, minlength=npoly), np.sort((b.row[m] - off) * npoly + key)


def _grid_case(system, zones, res, jitter, step, seed):
    import torch

    ctx = MosaicContext.build(system, "JTS")
    chips = tessellate(system, zones, res)
    offs, data = chips["wkb"]
    g = SimpleNamespace(ctx=ctx, zones=zones, res=res, chips=chips, npoly=len(zones), torch=torch,
                        grid=oracle.GRID_H3 if system == "H3" else oracle.GRID_BNG,
                        oc=dict(index_id=chips["index_id"], is_core=chips["is_core"], polygon_key=chips["polygon_key"],
                                wkb_offsets=offs, wkb=data))
    g.table = _table(g)
    _base_arrays(g, np.random.default_rng(seed), jitter, step)
    return g


def _table(g, kmul=1):
    c = g.chips
    return g.ctx.chip_table(c["is_core"], c["index_id"], c["wkb"], c["polygon_key"] * kmul, g.res,
                            n_polygons=g.npoly * kmul)


@pytest.fixture(scope="module")
def h3():
    g = _grid_case("H3", PolygonSet.load("nyc_taxi_zones_35"), 9, 1e-4, 1e-7, 11)
    info = g.table.tiles()
    assert info["stream"] == 1 and info["leaf_lines"] > 0, info
    yield g
    g.table.close()
    g.ctx.close()


@pytest.fixture(scope="module")
def bng():
    zones = PolygonSet.load("london_postcodes_bng")
    g = _grid_case("BNG", zones.subset(list(range(0, len(zones), 5))), 4, 50.0, 1e-2, 12)
    info = g.table.tiles()
    assert info["built"] == 1 and info["records"] > 0, info  # records: the LDS cell level's bytes
    yield g
    g.table.close()
    g.ctx.close()


@pytest.fixture(scope="module")
def h3_wide(h3):
    """The H3 table with polygon keys * 300: more than 8192 polygons, so count calls add to the
    counts in memory (LDS_COUNTS = false) instead of LDS."""
    t = _table(h3, 300)
    assert t.tiles()["stream"] == 1
    yield t
    t.close()


def _check(g, b, off, n, kernel, what, table=None, kmul=1, queue=False):
    """counts and sorted pairs of rows [off, off + n) of a base array against the oracle's, bit for
    bit, and the stream kernel that ran; queue: the queue readout's bounds (see test_queue_readout)"""
    table = table or g.table
    npoly = g.npoly * kmul
    wcounts, wpairs = _want(b, off, n, npoly, kmul)
    xd, yd = b.xd[off:off + n], b.yd[off:off + n]
    counts = g.ctx.pip_join_count(table, xd, yd).cpu().numpy()
    assert g.ctx.last_kernel() == kernel, (g.ctx.last_kernel(), kernel, what, off, n)
    q = g.ctx.last_queue()
    rows, keys = g.ctx.pip_join_pairs(table, xd, yd)
    assert g.ctx.last_kernel() == kernel, (g.ctx.last_kernel(), kernel, what, off, n)
    assert np.array_equal(counts, wcounts), (what, off, n)
    assert np.array_equal(rows.astype(np.int64) * npoly + keys, wpairs), (what, off, n)
    if queue:
        least = int(b.queued[off + n] - b.queued[off])
        assert q["stream_queued"] >= least, (q, least, what, off, n)
        assert q["leaf_forwarded"] <= q["stream_queued"], (q, what, off, n)
        assert g.ctx.last_queue()["stream_queued"] >= least, (what, off, n)  # the pairs call's
    return q


# ---- 1. one wave, every depth ----

@pytest.mark.parametrize("name", ["fwd", "rev"])
@pytest.mark.parametrize("leaf", [1, 0])
@pytest.mark.parametrize("pipe", [2, 1, 0])
def test_h3_one_wave_every_depth(h3, pipe, leaf, name):
    """T = 1 .. 14 full groups and a partial group of 0, 1 or 255 rows through one wave of each H3
    producer, with and without k_join_leaf's two-word queue: T mod 2 and every position of a dense
    group relative to the pipeline's end."""
    with _options(h3.ctx, stream_grid=1, stream_block=64, stream_pipe=pipe, leaf_join=leaf):
        for n in DEPTH_SIZES:
            _check(h3, h3.base[name], 0, n, H3_KERNELS[pipe], (pipe, leaf, name))


@pytest.mark.parametrize("name", ["fwd", "rev"])
@pytest.mark.parametrize("cpt", [1, 0])
def test_bng_one_wave_every_depth(bng, cpt, name):
    """The same depths through one wave of each BNG producer: T mod 6 of k_join_stream_bng_cpt's
    unrolled loop and every link of its tail chain."""
    with _options(bng.ctx, stream_grid=1, stream_block=64, bng_cpt=cpt):
        for n in DEPTH_SIZES:
            _check(bng, bng.base[name], 0, n, BNG_KERNELS[cpt], (cpt, name))


# ---- 2. non-vector producers at depth ----

SMALL = (1, 64, 255)


@pytest.mark.parametrize("name", ["fwd", "rev"])
@pytest.mark.parametrize("leaf", [1, 0])
def test_h3_non_vector_at_depth(h3, leaf, name):
    """Device views that start one element in (8 bytes past a 16-byte boundary), and fewer than 256
    rows: k_join_stream with VEC = false, one wave."""
    with _options(h3.ctx, stream_grid=1, stream_block=64, leaf_join=leaf):
        for n in sorted({min(n, N_BASE - 1) for n in DEPTH_SIZES} | set(SMALL)):
            _check(h3, h3.base[name], 1, n, "k_join_stream", (leaf, name))
        for n in SMALL:
            _check(h3, h3.base[name], 0, n, "k_join_stream", (leaf, name))
            _check(h3, h3.base[name], 256 * 7, n, "k_join_stream", (leaf, name))  # dense rows


@pytest.mark.parametrize("name", ["fwd", "rev"])
def test_bng_non_vector_at_depth(bng, name):
    """k_join_stream_bng with VEC = false: offset views, fewer than 256 rows, odd row counts."""
    with _options(bng.ctx, stream_grid=1, stream_block=64):
        for n in sorted({min(n, N_BASE - 1) for n in DEPTH_SIZES} | set(SMALL)):
            _check(bng, bng.base[name], 1, n, "k_join_stream_bng", name)
        for n in SMALL:
            _check(bng, bng.base[name], 0, n, "k_join_stream_bng", name)
            _check(bng, bng.base[name], 256 * 7, n, "k_join_stream_bng", name)


# ---- 3. waves that disagree about T ----

def _four_wave_sizes():
    # two workgroups of two waves, wave w takes groups w, w + 4, ...: 4 T - 2 full groups and a
    # partial one give waves 0 and 1 T groups, wave 2 T - 1 and the partial group, wave 3 T - 1
    return [256 * (4 * t - 2) + 100 for t in (3, 6, 7)]


@pytest.mark.parametrize("pipe", [2, 1, 0])
def test_h3_waves_disagree(h3, pipe):
    with _options(h3.ctx, stream_grid=2, stream_block=128, stream_pipe=pipe):
        for n in _four_wave_sizes():
            _check(h3, h3.tiled, 0, n, H3_KERNELS[pipe], ("4 waves", pipe))
    with _options(h3.ctx, stream_grid=3, stream_pipe=pipe):  # 48 waves of the default workgroup size
        _check(h3, h3.tiled, 0, N_TILED, H3_KERNELS[pipe], ("48 waves", pipe))


@pytest.mark.parametrize("cpt", [1, 0])
def test_bng_waves_disagree(bng, cpt):
    with _options(bng.ctx, stream_grid=2, stream_block=128, bng_cpt=cpt):
        for n in _four_wave_sizes():
            _check(bng, bng.tiled, 0, n, BNG_KERNELS[cpt], ("4 waves", cpt))
    with _options(bng.ctx, stream_grid=3, bng_cpt=cpt):
        _check(bng, bng.tiled, 0, N_TILED, BNG_KERNELS[cpt], ("48 waves", cpt))


# ---- 4. count paths ----

@pytest.mark.parametrize("name", ["fwd", "rev"])
@pytest.mark.parametrize("leaf", [1, 0])
def test_h3_counts_in_memory(h3, h3_wide, leaf, name):
    """More than 8192 polygons: k_join_stream_cpt<false, false> adds its counts with global atomics."""
    with _options(h3.ctx, stream_grid=1, stream_block=64, leaf_join=leaf):
        for n in DEPTH_SIZES:
            _check(h3, h3.base[name], 0, n, "k_join_stream_cpt", ("wide", leaf, name), table=h3_wide, kmul=300)


# ---- 5. proof the paths ran ----

@pytest.mark.parametrize("leaf", [1, 0])
def test_h3_queue_readout(h3, leaf):
    """The stream kernel queued at least the M and non-finite rows of every prefix (a condition on
    the inputs: no M row's cell can carry a pure code); k_join_leaf passes on no more than it got, and
    nothing without it.  The one group of 193 M rows alone: four sets of pending rows."""
    with _options(h3.ctx, stream_grid=1, stream_block=64, leaf_join=leaf):
        for pipe in (2, 1, 0):
            h3.ctx.set_option("stream_pipe", pipe)
            for name in ("fwd", "rev"):
                b = h3.base[name]
                for n in DEPTH_SIZES:
                    q = _check(h3, b, 0, n, H3_KERNELS[pipe], (pipe, leaf, name), queue=True)
                    if not leaf:
                        assert q["leaf_forwarded"] == 0, q
                q = _check(h3, b, b.group_at[G193], 256, H3_KERNELS[pipe], ("193 M", pipe, leaf), queue=True)
                assert q["stream_queued"] >= 193, q
    # a call that runs no stream kernel
    h3.ctx.set_option("point_raster", 0)
    try:
        h3.ctx.pip_join_count(h3.table, h3.base["fwd"].xd, h3.base["fwd"].yd)
        assert h3.ctx.last_kernel() not in H3_KERNELS.values()
        assert h3.ctx.last_queue() == {"stream_queued": 0, "leaf_forwarded": 0}
    finally:
        h3.ctx.set_option("point_raster", 1)


def test_bng_queue_readout(bng):
    with _options(bng.ctx, stream_grid=1, stream_block=64):
        for cpt in (1, 0):
            bng.ctx.set_option("bng_cpt", cpt)
            for name in ("fwd", "rev"):
                b = bng.base[name]
                for n in DEPTH_SIZES:
                    q = _check(bng, b, 0, n, BNG_KERNELS[cpt], (cpt, name), queue=True)
                    assert q["leaf_forwarded"] == 0, q
                q = _check(bng, b, b.group_at[G193], 256, BNG_KERNELS[cpt], ("193 M", cpt), queue=True)
                assert q["stream_queued"] >= 193, q


def test_stream_grid_option(h3):
    for bad in (-1, 65537):
        with pytest.raises(Exception, match="stream_grid"):
            h3.ctx.set_option("stream_grid", bad)
    for ok in (65536, 1, 0):
        h3.ctx.set_option("stream_grid", ok)


# ---- 6. BNG NaN at depth ----

@pytest.mark.parametrize("cpt", [1, 0])
@pytest.mark.parametrize("group", [7, 0])
def test_bng_nan_at_depth(bng, cpt, group):
    """A NaN row in group 7 of a T = 9 single-wave run, and in group 0 (which the drain steps load
    again): the call raises, and the next call on the clean array is the oracle's, bit for bit."""
    b = bng.base["fwd"]
    n = 9 * 256
    for col in (0, 1):
        xd, yd = b.xd[:n].clone(), b.yd[:n].clone()
        (xd, yd)[col][256 * group + 5] = float("nan")
        with _options(bng.ctx, stream_grid=1, stream_block=64, bng_cpt=cpt):
            with pytest.raises(IllegalStateException, match="NaN coordinates are not supported."):
                bng.ctx.pip_join_count(bng.table, xd, yd)
            assert bng.ctx.last_kernel() == BNG_KERNELS[cpt]
            with pytest.raises(IllegalStateException, match="NaN coordinates are not supported."):
                bng.ctx.pip_join_pairs(bng.table, xd, yd)
            _check(bng, b, 0, n, BNG_KERNELS[cpt], ("after NaN", cpt, group))


# ---- 7. layouts no other test builds ----

def _lds_left(npoly):
    # the table build's LDS budget for the quad level and tile bases: the LDS of a CU less the stages
    # of 16 waves, 1 KiB and the counts
    return 160 * 1024 - 16 * 128 * 4 - 1024 - (npoly + 64) * 4


def _h3_kernel(info, npoly, pipe, tb_option):
    """The H3 producer for >= 256 aligned rows: k_join_stream_cpt carries cell + 12 fraction + quad
    bits in 24, k_join_stream_pipe reads tile bases from LDS only."""
    tbytes = info["nx"] * info["ny"] * 4
    tb_lds = {0: False, 1: tbytes <= _lds_left(npoly) // 3, 2: tbytes <= _lds_left(npoly) // 16}[tb_option]
    cs = info["raster_cell"].bit_length() - 1
    mode = pipe
    if mode == 2 and cs + 12 + info["quad_shift"] > 24:
        mode = 1
    if mode == 1 and not tb_lds:
        mode = 0
    return H3_KERNELS[mode]


H3_LAYOUTS = [("raster_tb_lds", 0, 1), ("raster_tb_lds", 2, 1), ("raster_quad_records", 0, 1), ("raster_quad", 64, 1),
              ("raster_quad", 1024, 1), ("raster_quad", 2048, 1), ("raster_quad", 8192, 1), ("raster_quad", 0, 1),
              ("exact_defer", 1, 0)]
# tiles()["stream"] of the table: without a quad level (0), or with a budget that 64 x 64 sub-blocks per
# quad entry do not meet (64, 1024: this table has 2048 x 2496 sub-blocks, 1248 entries at the
# largest quad; the builder drops the level), no stream kernel applies and the tile-directory kernel
# runs.  Budgets 2048 and 8192 give quads of 64 and 32 sub-blocks a side (the default: 16)
H3_NO_STREAM = {("raster_quad", 0), ("raster_quad", 64), ("raster_quad", 1024)}
H3_QUAD_SHIFT = {2048: 6, 8192: 5}


@pytest.mark.parametrize("option,value,default", H3_LAYOUTS)
def test_h3_layouts(h3, option, value, default):
    """Tables built with an option no other GPU test sets, at T = 7 and a partial group of 255 rows:
    one wave and the default grid, every producer."""
    g = h3
    b = g.base["fwd"]
    n = 7 * 256 + 255
    g.ctx.set_option(option, value)
    try:
        table = _table(g)
        if option != "exact_defer":  # (a join option: it stays set for the joins)
            g.ctx.set_option(option, default)
        info = table.tiles()
        assert info["stream"] == (0 if (option, value) in H3_NO_STREAM else 1), info
        if option == "raster_quad" and value in H3_QUAD_SHIFT:
            assert info["quad_shift"] == H3_QUAD_SHIFT[value], info
        tb_option = value if option == "raster_tb_lds" else 1
        for grid, block in ((1, 64), (0, 1024)):
            for pipe in (2, 1, 0):
                # without the quad level no stream kernel applies: the tile-directory kernel
                kernel = _h3_kernel(info, g.npoly, pipe, tb_option) if info["stream"] else "k_join_tiled"
                if option == "raster_tb_lds" and value == 0:
                    assert kernel == {2: "k_join_stream_cpt", 1: "k_join_stream", 0: "k_join_stream"}[pipe]
                with _options(g.ctx, stream_grid=grid, stream_block=block, stream_pipe=pipe):
                    q = _check(g, b, 0, n, kernel, (option, value, grid, pipe), table=table, queue=bool(info["stream"]))
                if not info["stream"]:
                    assert q == {"stream_queued": 0, "leaf_forwarded": 0}
        table.close()
    finally:
        g.ctx.set_option(option, default)


@pytest.mark.parametrize("option", ["bng_group_lines", "bng_wedges"])
def test_bng_layouts(bng, option):
    g = bng
    b = g.base["fwd"]
    n = 7 * 256 + 255
    g.ctx.set_option(option, 0)
    try:
        table = _table(g)
    finally:
        g.ctx.set_option(option, 1)
    info = table.tiles()
    assert info["built"] == 1 and info["records"] > 0, info
    for grid, block in ((1, 64), (0, 1024)):
        for cpt in (1, 0):
            with _options(g.ctx, stream_grid=grid, stream_block=block, bng_cpt=cpt):
                _check(g, b, 0, n, BNG_KERNELS[cpt], (option, grid, cpt), table=table, queue=True)
    table.close()
