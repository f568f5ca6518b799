"""The GPU border clip (k_tess_clip_ll, mosaic_amd/csrc/tess_clip.hip) hands a candidate back to the
host producer when the lane's workspace is too small, when the cell is no planar polygon, or when the
shared output buffer is full.  Byte equality with the host producer alone cannot tell which side made
a chip, so every test here also reads tessellate_counters() right before and after the GPU call: the
first counter's growth is the number of border chips the host clipped (host redos), the second's the
cells that fell back to the face-plane clip.  Expected redo counts come from the host helper
(tests/native/llclip_caps_host.cpp: llclip::clip with the device's workspace), not from the device.
"""
import struct
import time

import numpy as np
import pytest

import oracle
from mosaic_amd import MosaicContext
from mosaic_amd.context import tessellate, tessellate_counters
from mosaic_amd.data import synthetic_buildings

from . import clip_cases as cc
from .test_tessellate_gpu import _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


@pytest.fixture(scope="module")
def caps_exe(tmp_path_factory):
    return cc.build_caps_helper(tmp_path_factory.mktemp("caps"))


def _gpu(grid, polys, res, ctx, **kw):
    """The GPU producer's chips, the host redos and the fallbacks of that call alone."""
    before = tessellate_counters()
    t0 = time.perf_counter()
    chips = tessellate(grid, polys, res, ctx=ctx, **kw)
    dt = time.perf_counter() - t0
    after = tessellate_counters()
    redos, fallbacks = after[0] - before[0], after[1] - before[1]
    print(f"{grid} res {res} {kw}: {len(chips['index_id'])} chips, gpu path {dt:.3f} s, host redos {redos}, "
          f"fallbacks {fallbacks}")
    return chips, redos, fallbacks


def _border_vertices(chips, keys):
    """Ring vertices (closed rings) in the border chips of the geometries `keys`: what the lanes that
    clip them write into the shared output buffer."""
    offs, data = chips["wkb"]
    total = 0
    for i in np.nonzero(np.isin(chips["polygon_key"], keys) & (np.asarray(chips["is_core"]) == 0))[0]:
        buf, pos = data[offs[i]:offs[i + 1]].tobytes(), 0
        n_polys = 1
        if struct.unpack_from(">I", buf, 1)[0] == 6:
            n_polys, pos = struct.unpack_from(">I", buf, 5)[0], 9
        for _ in range(n_polys):
            n_rings = struct.unpack_from(">I", buf, pos + 5)[0]
            pos += 9
            for _ in range(n_rings):
                n = struct.unpack_from(">I", buf, pos)[0]
                total += n
                pos += 4 + 16 * n
        assert pos == len(buf)
    return total


def test_workspace_handoff_h3_combs(ctx, caps_exe, tmp_path):
    # three combs in one launch: most cells of the 1e-4 comb need more than 12 result rings, the 4e-4
    # comb's fullest cell needs exactly 12, the 8e-4 comb fits easily
    polys = cc.one_ring_each([cc.comb(1e-4), cc.comb(4e-4), cc.comb(8e-4)])
    host = tessellate("H3", polys, 9)
    verdict = cc.h3_border_verdicts(caps_exe, tmp_path, polys, host)
    want = int((verdict[:, 0] != 0).sum())
    assert 0 < want < len(verdict) and int(verdict[verdict[:, 0] == 0][:, 2].max()) == 12
    gpu, redos, fallbacks = _gpu("H3", polys, 9, ctx)
    _same(host, gpu)
    assert (redos, fallbacks) == (want, 0)


def test_workspace_limit_exactly_reached_stays_on_device(ctx):
    polys = cc.one_ring_each([cc.comb(4e-4)])
    host = tessellate("H3", polys, 9)
    gpu, redos, fallbacks = _gpu("H3", polys, 9, ctx)
    _same(host, gpu)
    assert (host["is_core"] == 0).sum() == 50 and (redos, fallbacks) == (0, 0)


def test_workspace_handoff_bng_comb(ctx, caps_exe, tmp_path):
    # mode 1 (tessclip::clip_ll, explicit squares): 4 m teeth in 100 m cells, 25 teeth per cell
    polys = cc.one_ring_each([cc.comb(4.0, x0=530010.0, y0=180010.0, width=400.0, base=20.0, top=400.0)])
    host = tessellate("BNG", polys, 4)
    verdict = cc.lane_verdicts(caps_exe, tmp_path, polys, cc.bng_squares(polys, 100.0), False)
    # (a square the lane refuses holds teeth, so the host's clip of it is a chip and is counted)
    want = int((verdict[:, 0] != 0).sum())
    fit = int(((verdict[:, 0] == 0) & (verdict[:, 4] > 0)).sum())
    assert want > 0 and fit > 0 and want + fit == len(host["index_id"])
    gpu, redos, fallbacks = _gpu("BNG", polys, 4, ctx)
    _same(host, gpu)
    assert (redos, fallbacks) == (want, 0)


def test_output_overflow_h3(ctx):
    # 20 border cells, all within the lane workspace (tests/test_clip_caps.py), 1,500,084 result
    # vertices against out_cap = 20 * 96 + 2^20: the first lane to reserve fits, at least 6 cannot
    polys = cc.wavy_circles(6, 250_000)
    host = tessellate("H3", polys, 7)
    n_border = int((host["is_core"] == 0).sum())
    assert n_border == len(host["index_id"]) == 20
    assert _border_vertices(host, np.arange(6)) > 1.15 * (n_border * 96 + (1 << 20))
    gpu, redos, fallbacks = _gpu("H3", polys, 7, ctx)
    _same(host, gpu)
    assert 1 <= redos <= n_border - 1 and fallbacks == 0


def test_output_overflow_bng(ctx):
    # the same circles in metres, 1 km cells: each spans a 3 x 3 block or less
    polys = cc.wavy_circles(6, 250_000, cx=530300.0, cy=180200.0, step=3000.0, radius=600.0, ky=1.0)
    host = tessellate("BNG", polys, 3)
    n_border = int((host["is_core"] == 0).sum())
    assert 6 * 4 <= n_border <= 6 * 9
    assert _border_vertices(host, np.arange(6)) > 1.15 * (n_border * 96 + (1 << 20))
    gpu, redos, fallbacks = _gpu("BNG", polys, 3, ctx)
    _same(host, gpu)
    assert 1 <= redos <= n_border - 1 and fallbacks == 0


def test_more_than_one_chunk(ctx):
    # at densify 64 the H3 session takes 10,922 candidates per chunk; every chip comes from one
    # candidate, so more chips than that means at least two chunks (buffers reused, chunk-local
    # candidate indices, ids offset by the chunk's start)
    bld = synthetic_buildings(6000)
    host = tessellate("H3", bld, 11, densify=64)
    assert len(host["index_id"]) > cc.CHUNK_D64
    gpu, redos, fallbacks = _gpu("H3", bld, 11, ctx, densify=64)
    _same(host, gpu)
    assert (redos, fallbacks) == (0, 0)


def test_output_overflow_in_a_later_chunk(ctx):
    # buildings first: more chips than one chunk's candidates, so the first chunk is full of ordinary
    # border tasks whose records stay in the session's buffers; the circles, last in the batch, then
    # overflow the last chunk's output.  That chunk has at most min(10,922, border chips) tasks, which
    # bounds its out_cap from above.  (Each circle lies around the centre of its own res-7 cell, well
    # inside it: that cell is its only candidate, so the host producer's classification of densified
    # hexagons against 250,000 vertices -- all of them, for a candidate it drops -- stays cheap.)
    n_bld, n_circ, res = 12_000, 9, 7
    ids = oracle.h3_point_to_index(-73.9 + 0.05 * np.arange(n_circ), np.full(n_circ, 40.7), res)
    assert len(set(ids.tolist())) == n_circ
    centres = [tuple(np.mean(np.array(cc.h3_cell_degrees(i)), axis=0)) for i in ids]
    polys = cc.concat(synthetic_buildings(n_bld), cc.wavy_circles(n_circ, 250_000, radius=0.002, centres=centres))
    host = tessellate("H3", polys, res, densify=64)
    n_border = int((host["is_core"] == 0).sum())
    assert int((host["polygon_key"] < n_bld).sum()) > cc.CHUNK_D64
    cap_max = 96 * min(cc.CHUNK_D64, n_border) + (1 << 20)
    circle_vertices = _border_vertices(host, np.arange(n_bld, n_bld + n_circ))
    print(f"last chunk: out_cap <= {cap_max}, circles' output >= {circle_vertices} vertices")
    assert circle_vertices > cap_max
    gpu, redos, fallbacks = _gpu("H3", polys, res, ctx, densify=64)
    _same(host, gpu)
    assert redos > 0 and fallbacks == 0


@pytest.mark.parametrize("res,n_chips,n_fallbacks", [(5, 10, 4), (6, 40, 8), (7, 192, 16)])
def test_cells_over_the_antimeridian_go_to_the_face_plane_clip(ctx, res, n_chips, n_fallbacks):
    # cells over the antimeridian are no planar lon / lat polygons: the lane's cell_ok refuses them
    # (status 1) and the host clips them in the face plane, as the host producer does
    def sq(x0, x1):
        return np.array([(x0, -17.0), (x1, -17.0), (x1, -16.85), (x0, -16.85), (x0, -17.0)], np.float64)

    polys = cc.one_ring_each([sq(179.80, 179.9995), sq(-179.9995, -179.80)])
    before = tessellate_counters()
    host = tessellate("H3", polys, res)
    host_fallbacks = tessellate_counters()[1] - before[1]
    assert (len(host["index_id"]), host_fallbacks) == (n_chips, n_fallbacks)
    gpu, _, fallbacks = _gpu("H3", polys, res, ctx)
    _same(host, gpu)
    assert fallbacks == host_fallbacks > 0
