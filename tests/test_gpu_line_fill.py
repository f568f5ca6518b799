"""GPU: Mosaic.lineFill on the device (mosaic_tessellate_lines_gpu: k_line_spans, k_line_walk,
k_line_clip) against the host producer, row for row and byte for byte, on H3 resolution 9 and BNG
resolution 4 -- the smallest shapes at which the kernels can go wrong: one lane's work, a segment of
hundreds of spans, groups of thousands of segments whose chips exceed the lane's workspace, enough
lines for multi-block scans and the sort, empty inputs.  The host producer itself is checked against
the Python restatement in tests/test_line_fill.py."""
import ctypes
import threading

import numpy as np
import pytest

from mosaic_amd import _native as N
from mosaic_amd.context import tessellate
from mosaic_amd.data import LineSet
from tests import line_cases as LC

pytestmark = pytest.mark.gpu

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


def both(ctxs, name, geoms, res, **kw):
    """The device producer's rows after asserting that they are the host producer's; the counters."""
    ls = LineSet.from_lines(geoms)
    host = tessellate(name, ls, res, **kw)
    dev = tessellate(name, ls, res, ctx=ctxs[name], **kw)
    st = last()
    for col in ("is_core", "index_id", "polygon_key"):
        assert np.array_equal(host[col], dev[col]), col
    assert np.array_equal(host["wkb"][0], dev["wkb"][0])
    n = int(host["wkb"][0][-1])
    assert np.array_equal(np.asarray(host["wkb"][1])[:n], np.asarray(dev["wkb"][1])[:n])
    return LC.rows_of(dev), st


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
