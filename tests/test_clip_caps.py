"""CPU-only: which border candidates the GPU clip's lane can take (kLLChains = 24 chains, kLLOut = 12
result rings per lane, mosaic_amd/csrc/tess_gpu.h), from llclip::clip on the host with that workspace
(tests/native/llclip_caps_host.cpp).  llclip.h is the code both sides compile, so these are the counts
the GPU tests (tests/test_gpu_clip_handoff.py) expect of the device: no NYC zone cell at res 8 / 9
goes to the host for workspace; a comb of period 1e-4 overflows 45 of its 50 cells at res 9, one of
period 4e-4 fits at exactly 12 rings."""
import numpy as np
import pytest

from mosaic_amd.context import tessellate
from mosaic_amd.data import PolygonSet

from . import clip_cases as cc


@pytest.fixture(scope="module")
def caps_exe(tmp_path_factory):
    return cc.build_caps_helper(tmp_path_factory.mktemp("caps"))


def _table_row(exe, tmp, polys, res):
    chips = tessellate("H3", polys, res)
    rows = cc.h3_border_verdicts(exe, tmp, polys, chips)
    ok = rows[rows[:, 0] == 0]
    assert set(rows[:, 0].tolist()) <= {0, 1}  # workspace overflow is the only refusal here
    return len(rows), int((rows[:, 0] != 0).sum()), (int(ok[:, 1].max()), int(ok[:, 2].max())) if len(ok) else None, chips, rows


@pytest.mark.parametrize("res,n_border,peak", [(8, 2639, (8, 8)), (9, 7947, (14, 10))])
def test_nyc_zone_cells_fit_the_lane_workspace(caps_exe, tmp_path, res, n_border, peak):
    n, exceed, mx, _, _ = _table_row(caps_exe, tmp_path, PolygonSet.load("nyc_taxi_zones"), res)
    assert (n, exceed, mx) == (n_border, 0, peak)


@pytest.mark.parametrize("period,n_vertices,exceed,peak", [(1e-4, 803, 45, None), (4e-4, 203, 0, (22, 12)),
                                                          (8e-4, 103, 0, (11, 6))])
def test_comb_cells_against_the_lane_workspace(caps_exe, tmp_path, period, n_vertices, exceed, peak):
    ring = cc.comb(period)
    assert len(ring) == n_vertices
    n, ex, mx, _, _ = _table_row(caps_exe, tmp_path, cc.one_ring_each([ring]), 9)
    assert (n, ex) == (50, exceed)
    if peak is not None:
        assert mx == peak


def test_wavy_circle_cells_fit_the_workspace_but_not_the_output(caps_exe, tmp_path):
    polys = cc.wavy_circles(6, 250_000)
    n, exceed, mx, chips, rows = _table_row(caps_exe, tmp_path, polys, 7)
    assert (n, exceed, mx) == (20, 0, (1, 1))
    assert int(np.asarray(chips["is_core"]).sum()) == 0
    # the lanes' output against the shared buffer (mosaic_hip.hip run_clip_ll: 96 per task + 2^20)
    assert int(rows[:, 3].sum()) == 1_500_084 > 20 * 96 + (1 << 20)
