"""GPU: Mosaic.lineFill on the device (mosaic_tessellate_lines_gpu: k_line_spans, k_line_walk,
k_line_clip) against the host producer, row for row and byte for byte, on H3 resolution 9 and BNG
resolution 4 -- the smallest shapes at which the kernels can go wrong: one lane's work, a segment of
hundreds of spans, groups of thousands of segments whose chips exceed the lane's workspace, enough
lines for multi-block scans and the sort, empty inputs; polar segments whose spans go to the host's
walk, BNG spans that walk twice, more work than the kernels have lanes, batches that fail.  The host
producer itself is checked against the Python restatement in tests/test_line_fill.py."""
import ctypes
import os
import struct
import threading

import numpy as np
import pytest

from mosaic_amd import MosaicError
from mosaic_amd import _native as N
from mosaic_amd.context import tessellate
from mosaic_amd.data import LineSet
from tests import line_cases as LC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [("H3", LC.H3, 9), ("BNG", LC.BNG, 4)]
K_ITEMS = 8  # lineclip::kItems, the lane's workspace


@pytest.fixture(scope="module")
def ctxs():
    from mosaic_amd import MosaicContext

    c = {"H3": MosaicContext.build("H3", "JTS"), "BNG": MosaicContext.build("BNG", "JTS")}
    yield c
    for v in c.values():
        v.close()


def last():
    out, ms = (ctypes.c_int64 * 4)(), (ctypes.c_double * 3)()
    N.check(N.lib().mosaic_tess_lines_last(out, ms))
    return dict(segments=out[0], groups=out[1], handed=out[2], pairs=out[3], ms=list(ms))


def last_walk():
    out = (ctypes.c_int64 * 3)()
    N.check(N.lib().mosaic_tess_lines_last_walk(out))
    return dict(spans=out[0], spans_handed=out[1], pairs_added=out[2])


def both_columns(ctxs, name, geoms, res, **kw):
    """The device producer's columns after asserting that they are the host producer's; the counters
    (mosaic_tess_lines_last and, under "walk", mosaic_tess_lines_last_walk)."""
    ls = LineSet.from_lines(geoms)
    host = tessellate(name, ls, res, **kw)
    dev = tessellate(name, ls, res, ctx=ctxs[name], **kw)
    st = last()
    st["walk"] = last_walk()
    for col in ("is_core", "index_id", "polygon_key"):
        assert np.array_equal(host[col], dev[col]), col
    assert np.array_equal(host["wkb"][0], dev["wkb"][0])
    n = int(host["wkb"][0][-1])
    assert np.array_equal(np.asarray(host["wkb"][1])[:n], np.asarray(dev["wkb"][1])[:n])
    return dev, st


def both(ctxs, name, geoms, res, **kw):
    """both_columns with the columns as rows."""
    dev, st = both_columns(ctxs, name, geoms, res, **kw)
    return LC.rows_of(dev), st


@pytest.fixture(scope="module")
def caps(tmp_path_factory):
    """tests/native/linewalk_caps_host.cpp, compiled once: caps(grid, res, geoms) = (constants, per segment
    (K, spans)) -- the source of every expected walk count below."""
    d = tmp_path_factory.mktemp("linewalk")
    exe = LC.build_linewalk_caps(ROOT, d)
    return lambda grid, res, geoms: LC.walk_counts(exe, d, grid, res, LC.segments_of(geoms))


def n_cu_of(ctx):
    dev, jdk, n_cu, stream = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_void_p()
    N.check(N.lib().mosaic_ctx_exec(ctx.handle, ctypes.byref(dev), ctypes.byref(stream), ctypes.byref(jdk), ctypes.byref(n_cu)))
    return n_cu.value


def wkb_type(blob):
    return struct.unpack(">I", blob[1:5])[0]


def inside_one_cell(grid):
    return [(-73.98, 40.75), (-73.9801, 40.7501)] if grid == LC.H3 else [(400010.0, 300010.0), (400090.0, 300080.0)]


def long_segment(grid):
    return [(-74.6, 40.31), (-73.3, 41.02)] if grid == LC.H3 else [(380013.0, 290007.0), (415021.0, 309013.0)]


def zigzag(grid, res, n=5000):
    """n vertices alternating between the first and the third of three cells in a row."""
    if grid == LC.BNG:
        xs = np.linspace(400010.0, 400090.0, n)
        return [(float(x), 300150.0 if i % 2 else 299950.0) for i, x in enumerate(xs)]
    C = np.asarray(LC.cell_poly(grid, LC.point_cell(grid, res, (-73.98, 40.75))))
    c = C.mean(axis=0)
    d = (C[0] + C[1]) / 2 - c  # to the middle of a side: 2 d is the neighbour's centre, 4 d the next one's
    side = (C[1] - C[0]) * 0.1
    ts = np.linspace(-1.0, 1.0, n)
    return [tuple((c + (4 * d if i % 2 else 0) + side * t).tolist()) for i, t in enumerate(ts)]


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_one_short_line(ctxs, name, grid, res):
    rows, st = both(ctxs, name, [[inside_one_cell(grid)]], res)
    assert len(rows) == 1 and st["handed"] == 0 and st["segments"] == 1 and st["groups"] == 1


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_one_segment_across_hundreds_of_cells(ctxs, name, grid, res):
    rows, st = both(ctxs, name, [[long_segment(grid)]], res)
    assert len(rows) > 300 and st["groups"] == len(rows)
    assert st["handed"] == 0 and st["segments"] == 1 and st["pairs"] >= len(rows)


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_zigzag_hands_its_chips_to_the_host(ctxs, name, grid, res):
    """Groups of thousands of segments; every chip has more pieces than the lane's workspace holds.  The
    hand-off count is the number of chips with more than lineclip::kItems items: the rule that
    tests/native/lineclip_caps_host.cpp checks the builder's "needs more" against."""
    rows, st = both(ctxs, name, [[zigzag(grid, res)], [inside_one_cell(grid)]], res)
    big = [r for r in rows if r[0] == 0]
    assert len(big) == 3 and min(LC.item_count(r[2]) for r in big) >= 2000
    assert st["handed"] == sum(LC.item_count(r[2]) > K_ITEMS for r in rows) == 3
    assert st["segments"] == 5000


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_two_thousand_lines(ctxs, name, grid, res):
    rows, st = both(ctxs, name, LC.short_lines(grid, res, 2000, 11), res)
    assert len(rows) > 4000 and st["handed"] == 0 and st["groups"] == len(rows)


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_empty_inputs(ctxs, name, grid, res):
    rows, st = both(ctxs, name, [], res)
    assert rows == [] and st["handed"] == 0
    ln = inside_one_cell(grid)
    rows, st = both(ctxs, name, [[[], ln, []], [[]], [], [ln]], res)
    assert [r[0] for r in rows] == [0, 3] and st["handed"] == 0


def test_bng_degenerates(ctxs):
    rows, st = both(ctxs, "BNG", LC.bng_degenerates(), 3)
    assert rows == LC.line_fill(LC.BNG, 3, LC.bng_degenerates())
    both(ctxs, "BNG", LC.bng_degenerates(), 4)


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_cells_only(ctxs, name, grid, res):
    geoms = LC.short_lines(grid, res, 200, 12) + [[long_segment(grid)]]
    full, _ = both(ctxs, name, geoms, res)
    bare, _ = both(ctxs, name, geoms, res, cells_only=True)
    assert [r[:2] for r in bare] == [r[:2] for r in full] and all(r[2] == b"" for r in bare)


@pytest.mark.parametrize("name,grid,res", GRIDS, ids=lambda v: str(v))
def test_geometry_kring_of_lines(ctxs, name, grid, res):
    ctx = ctxs[name]
    geoms = LC.short_lines(grid, res, 40, 13) + [[]]
    ls = LineSet.from_lines(geoms)
    chips = tessellate(name, ls, res)
    cells = [sorted({int(c) for c, k in zip(chips["index_id"], chips["polygon_key"]) if k == g}) for g in range(len(ls))]

    def check():
        for k in (0, 1, 3):
            got = ctx.grid_geometrykring(ls, res, k, raw=True)
            assert len(got) == len(ls)
            for g, row in enumerate(got):
                want = set(cells[g])
                if k and cells[g]:
                    want = {int(c) for r in ctx.grid_cellkring(np.asarray(cells[g], np.int64), k, raw=True) for c in r}
                assert len(row) == len(set(row.tolist())) and set(row.tolist()) == want, (k, g)

    check()
    errors = []

    def worker():
        try:
            check()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert not errors, errors


# ---- the walk's hand-off, the second walk, more work than lanes, the error order ----
# Every expected count comes from tests/native/linewalk_caps_host.cpp (the fixture `caps`), not from the
# device.  The wall times in the docstrings are the whole test's, measured on an MI355X host with 16 threads.
def handed_by_the_helper(caps, grid, res, geoms):
    """(spans, spans the helper says need more than kWalkCap cells, the cells those emit); no bad cell."""
    _, segs = caps(grid, res, geoms)
    assert all(k > 0 and not any(sp[0] == 2 or sp[2] for sp in spans) for k, spans in segs)
    return LC.walk_totals(segs)


@pytest.mark.parametrize("res", [8, 9, 10])
def test_polar_spans_are_walked_by_the_host_routine(ctxs, caps, res):
    """Spans whose walk tries more than lineclip::kWalkCap cells (H3 in degrees near a pole): the host
    routine's pairs are appended and sorted in by segment.  The helper's counts for the batches at resolution
    8 / 9 / 10: 126 / 904 / 3979 spans, 2 / 15 / 29 of them handed, which add 52 / 344 / 784 pairs.
    0.1 s, 1.1 s, 2.9 s (the helper's and the host producer's share of the last: a segment of 3146 spans)."""
    geoms = LC.polar_batch(res)
    spans, more, cells = handed_by_the_helper(caps, LC.H3, res, geoms)
    assert more > 0 and cells > more
    rows, st = both(ctxs, "H3", geoms, res)
    assert st["walk"] == dict(spans=spans, spans_handed=more, pairs_added=cells)
    assert st["handed"] == 0 and st["groups"] == len(rows)
    assert {r[0] for r in rows} == set(range(len(geoms)))
    if res == 9:
        bare, st = both(ctxs, "H3", geoms, res, cells_only=True)
        assert st["walk"] == dict(spans=spans, spans_handed=more, pairs_added=cells) and st["handed"] == 0
        assert [r[:2] for r in bare] == [r[:2] for r in rows] and all(r[2] == b"" for r in bare)


def test_spans_and_groups_handed_in_one_call(ctxs, caps):
    """Both hand-offs share counters[1]: neither count may leak into the other.  0.7 s."""
    geoms = LC.polar_batch(9) + [[zigzag(LC.H3, 9)], [inside_one_cell(LC.H3)]]
    spans, more, cells = handed_by_the_helper(caps, LC.H3, 9, geoms)
    assert more > 0
    rows, st = both(ctxs, "H3", geoms, 9)
    assert st["walk"] == dict(spans=spans, spans_handed=more, pairs_added=cells)
    assert st["handed"] == sum(LC.item_count(r[2]) > K_ITEMS for r in rows) == 3


def test_bng_spans_of_more_than_a_slot_walk_twice(ctxs, caps):
    """A BNG line through the lattice corners touches two diagonal cells at every corner: every span
    emits more than lineclip::kSlot cells and walks again in k_line_walk<true>.  Under 0.1 s."""
    geoms = LC.bng_corner_lines()
    consts, segs = caps(LC.BNG, 4, geoms)
    assert all(k > 0 and all(sp == (0, sp[1], 0) and sp[1] > consts["slot"] for sp in spans) for k, spans in segs[:4])
    assert all(sp[0] == 0 and not sp[2] for sp in segs[4][1])
    rows, st = both(ctxs, "BNG", geoms, 4)
    assert st["walk"] == dict(spans=sum(k for k, _ in segs), spans_handed=0, pairs_added=0) and st["handed"] == 0
    for g in range(4):  # 100 cells on the diagonal, two touched at each of the 99 corners between them and one at either end
        kinds = [wkb_type(r[2]) for r in rows if r[0] == g]
        assert kinds.count(2) == 100 and kinds.count(1) == 2 * 99 + 2 * 3 and len(kinds) == 304
    kinds = [wkb_type(r[2]) for r in rows if r[0] == 4]  # no corner: a piece in every cell but the two its ends touch
    assert kinds.count(2) == 200 and kinds.count(1) == 2 and len(kinds) == 202


def test_more_work_than_lanes(ctxs, caps):
    """Every grid-stride loop takes a second iteration and every lane reuses its scratch: more segments,
    spans and groups than the walking kernels have lanes (n_cu * 1024), more pairs than the light ones
    (n_cu * 2048).  BNG: Batch.g is a runtime field, so the loops are the same code for both grids.
    At 256 CUs: 1491 copies, 0.8 million rows, 37 MB of WKB; 3.7 s."""
    lanes = n_cu_of(ctxs["BNG"]) * 1024
    a, b = long_segment(LC.BNG)
    _, segs = caps(LC.BNG, 4, [[[a, b]]])
    copies = lanes // segs[0][0] + 2
    geoms = [[[(a[0] + dx, a[1] + dy), (b[0] + dx, b[1] + dy)]]
             for dx, dy in ((i % 40 * 1000.0 + i // 40 * 3.0, i // 40 * 2000.0 + i % 40 * 7.0) for i in range(copies))]
    i = np.arange(lanes + 2)
    jitter = np.stack([400010.0 + (i % 797) * 0.1, 300010.0 + (i % 601) * 0.13], axis=1)  # inside one 100 m cell
    geoms.append([jitter.tolist()])
    dev, st = both_columns(ctxs, "BNG", geoms, 4)
    assert st["segments"] == copies + lanes + 1 > lanes  # k_line_spans
    assert st["walk"]["spans"] == copies * segs[0][0] + lanes + 1 and st["walk"]["spans"] - (lanes + 1) > lanes  # k_line_walk
    assert st["walk"]["spans_handed"] == 0 and st["handed"] == 0
    assert st["groups"] == len(dev["index_id"]) > lanes  # k_line_clip
    assert st["pairs"] > 2 * lanes  # k_line_flags, k_line_fill
    assert int(dev["polygon_key"][-1]) == copies and int((dev["polygon_key"] == copies).sum()) == 1


@pytest.mark.parametrize("batch", [0, 1], ids=["walk-then-spans", "spans-then-walk"])
def test_a_failed_call_names_the_geometry_the_host_names(ctxs, batch):
    """The first bad geometry of the batch, whichever stage finds it: by the walk (a cell over the pole) in
    one batch, by span_count in the other, and a later geometry is bad for the other stage.  Under 0.1 s."""
    ls = LineSet.from_lines(LC.error_batches()[batch])
    with pytest.raises(MosaicError) as host:
        tessellate("H3", ls, 5)
    assert "geometry 1:" in str(host.value)
    with pytest.raises(MosaicError) as dev:
        tessellate("H3", ls, 5, ctx=ctxs["H3"])
    assert type(dev.value) is type(host.value) and dev.value.code == host.value.code == N.MOSAIC_E_ARG
    assert str(dev.value) == str(host.value)
    h = ctypes.c_void_p(1)
    rc = N.lib().mosaic_tessellate_lines_gpu(ctxs["H3"].handle, N.GRID_H3, 5, len(ls), N.ptr(ls.geom_lines), N.ptr(ls.line_offsets),
                                             N.ptr(ls.xy), 0, ctypes.byref(h))
    assert rc == N.MOSAIC_E_ARG and h.value is None
    assert N.lib().mosaic_last_error().decode() == str(host.value)
