"""st_area / st_length / st_centroid / st_numpoints / bounds on the GPU (mosaic_st_measures,
MosaicContext.st_measures): k_meas_plan, k_meas_lane and k_meas_wave of mosaic_amd/csrc/st_measures.hip
against (H), the sequential definition compiled by g++ (tests/measures_cases.py), bit for bit -- under the
default options, with every row on the wave kernel, with every row on the lane kernel and with a tile of 4
segments that rings of 5 to 40 vertices straddle -- and the resolution analyzer through the engine's own calls."""
import numpy as np
import pytest

from mosaic_amd import _native as N

from . import measures_cases as C
from .measures_cases import CASES, case_rows, host_measures, ring_size_rows
from .test_st_distance_lines import LCol

pytestmark = pytest.mark.gpu

DEFAULT_WAVE_MIN = 128
WHAT = ("area", "length", "centroid", "numpoints", "xmin", "ymin", "xmax", "ymax")
DEFAULTS = dict(meas_wave_min=DEFAULT_WAVE_MIN, meas_tile=256)
ALL_WAVE, ALL_LANE = 0, 1 << 40


@pytest.fixture(scope="module")
def ctx():
    from mosaic_amd import MosaicContext

    c = MosaicContext.build("H3", "JTS")
    yield c
    c.close()


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same(got, want, what=""):
    """a dict of MosaicContext.st_measures against a dict of host_measures, on the bits"""
    pairs = [("area", got.get("area")), ("length", got.get("length")), ("numpoints", got.get("numpoints")),
             ("xmin", got.get("xmin")), ("ymin", got.get("ymin")), ("xmax", got.get("xmax")), ("ymax", got.get("ymax")),
             ("status", got.get("status"))]
    if "centroid" in got:
        pairs += [("cx", got["centroid"][0]), ("cy", got["centroid"][1])]
    seen = 0
    for name, g in pairs:
        if g is None:
            continue
        w = want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        same = u64(g) == u64(w) if g.dtype == np.float64 else g == w
        bad = np.flatnonzero(~same)
        assert len(bad) == 0, (what, name, len(bad), bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
        seen += 1
    assert seen


def with_options(ctx, options, call):
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        return call(), ctx.st_measures_last_split()
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


WAYS = {
    "default options": {},
    "every row on the wave kernel": dict(meas_wave_min=ALL_WAVE),
    "every row on the lane kernel": dict(meas_wave_min=ALL_LANE),
    "wave kernel, a tile of 4": dict(meas_wave_min=ALL_WAVE, meas_tile=4),
    "wave kernel, a tile of 1": dict(meas_wave_min=ALL_WAVE, meas_tile=1),
}


@pytest.fixture(scope="module")
def case_table(ctx):
    rows, _ = case_rows()
    t = ctx.geometry_table(rows, lines=True)
    yield t
    t.close()


@pytest.mark.parametrize("way", list(WAYS))
def test_case_table(ctx, case_table, way):
    _, want = case_rows()
    assert case_table.info()["n_row_path"] == 0
    got, (one_lane, wave) = with_options(ctx, WAYS[way], lambda: ctx.st_measures(case_table, WHAT, return_status=True))
    assert_same(got, want, way)
    n, n_empty = len(want["status"]), int((want["numpoints"] == 0).sum())
    assert one_lane + wave == n and n_empty >= 4
    if WAYS[way].get("meas_wave_min") == ALL_WAVE:
        assert (one_lane, wave) == (n_empty, n - n_empty)  # a row without a vertex has nothing for a wave to do
    elif WAYS[way].get("meas_wave_min") == ALL_LANE:
        assert (one_lane, wave) == (n, 0)
    else:
        assert wave == int((want["numpoints"] >= DEFAULT_WAVE_MIN).sum())
    # the docs polygon, first row
    d = C.DOCS
    assert got["area"][0] == d["area"] and got["numpoints"][0] == d["numpoints"] and got["xmax"][0] == d["xmax"]


@pytest.fixture(scope="module")
def ring_table(ctx):
    rows, _ = ring_size_rows()
    t = ctx.geometry_table(rows)
    yield t
    t.close()


@pytest.mark.parametrize("options", ({}, dict(meas_wave_min=64), dict(meas_wave_min=65), dict(meas_wave_min=65, meas_tile=64),
                                     dict(meas_wave_min=ALL_WAVE, meas_tile=63), dict(meas_wave_min=ALL_LANE)),
                         ids=("default", "wave from 64", "wave from 65", "wave from 65, tile 64", "all wave, tile 63",
                              "all lane"))
def test_ring_sizes(ctx, ring_table, options):
    rows, want = ring_size_rows()
    got, (one_lane, wave) = with_options(ctx, options, lambda: ctx.st_measures(ring_table, WHAT, return_status=True))
    assert_same(got, want, str(options))
    st = want["status"]
    assert st[0] == st[-1] == N.ROW_OK and {N.ROW_NULL, N.ROW_PATH} <= set(st.tolist()) and (want["numpoints"][st == N.ROW_OK] == 0).any()
    assert want["numpoints"].max() >= 3001 + 64
    thr = options.get("meas_wave_min", DEFAULTS["meas_wave_min"])
    expect_wave = int(((st == N.ROW_OK) & (want["numpoints"] > 0) & (want["numpoints"] >= thr)).sum())
    assert (one_lane, wave) == (len(st) - expect_wave, expect_wave)
    if thr in (64, 65):  # the row of 64 stored vertices changes sides between the two
        assert (want["numpoints"] == 64).sum() == 1 and 0 < wave < len(st)


def test_single_measures_and_what(ctx, ring_table):
    rows, want = ring_size_rows()
    path = np.flatnonzero(want["status"] == N.ROW_PATH)
    from mosaic_amd import RowPathRequired

    with pytest.raises(RowPathRequired) as e:
        ctx.st_area(ring_table)
    assert e.value.rows.tolist() == path.tolist()
    for name, fn in (("area", ctx.st_area), ("length", ctx.st_length), ("length", ctx.st_perimeter), ("numpoints", ctx.st_numpoints),
                     ("xmin", ctx.st_xmin), ("xmax", ctx.st_xmax), ("ymin", ctx.st_ymin), ("ymax", ctx.st_ymax)):
        got, st = fn(ring_table, return_status=True)
        assert_same({name: got, "status": st}, want, name)
    (cx, cy), st = ctx.st_centroid(ring_table, return_status=True)
    assert_same({"centroid": (cx, cy), "status": st}, want, "centroid")
    # only what is asked for: area and length do not need isCCW, the centroid alone does not need the area terms
    for what in (("area",), ("length", "area"), ("centroid",), ("xmin", "numpoints")):
        for opt in ({}, dict(meas_wave_min=ALL_WAVE, meas_tile=16)):
            got, _ = with_options(ctx, opt, lambda: ctx.st_measures(ring_table, what, return_status=True))
            assert set(got) == set(what) | {"status"}
            assert_same(got, want, str(what))
    # geometries given directly: the table is built and closed inside the call
    assert ctx.st_area("POLYGON ((30 10, 40 40, 20 40, 10 20, 30 10))").tolist() == [550.0]
    assert ctx.st_length(["LINESTRING (0 0, 3 4)", "POINT (1 1)"], lines=True).tolist() == [5.0, 0.0]
    got, st = ctx.st_length(["LINESTRING (0 0, 3 4)"], return_status=True)  # without lines=True: a row for the row path
    assert st.tolist() == [N.ROW_PATH] and np.isnan(got).all()


def test_row_lists(ctx, ring_table):
    import torch

    rows, want = ring_size_rows()
    n = len(rows)
    col = LCol.from_wkb(rows, flags=0)
    assert_same(ctx.st_measures(ring_table, WHAT, rows=np.arange(n), return_status=True), want, "arange")
    rng = np.random.default_rng(3)
    for name, pick in (("reversed", np.arange(n)[::-1].copy()), ("duplicates", rng.integers(0, n, 500)),
                       ("one row many times", np.full(700, n - 2))):
        expect = host_measures(col, pick)
        assert_same(ctx.st_measures(ring_table, WHAT, rows=pick, return_status=True), expect, name)
        dev = torch.from_numpy(pick).cuda()
        assert_same(ctx.st_measures(ring_table, WHAT, rows=dev, return_status=True), expect, name + ", on the device")
    got = ctx.st_measures(ring_table, WHAT, rows=np.zeros(0, np.int64), return_status=True)
    assert got["area"].shape == (0,) and got["status"].shape == (0,) and ctx.st_measures_last_split() == (0, 0)


def test_c_entry(ctx, ring_table):
    """device pointers for outputs and rows; a bad index writes nothing; nullable everything"""
    import torch

    rows, want = ring_size_rows()
    n = len(rows)
    lib = N.lib()
    pick = np.array([n - 2, 0, 5, n - 1], np.int64)
    expect = host_measures(LCol.from_wkb(rows, flags=0), pick)
    d = {k: torch.full((4,), -7.0, dtype=torch.float64, device="cuda") for k in ("area", "length", "cx", "cy", "xmin", "ymin", "xmax", "ymax")}
    d_np = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    d_st = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    d_rows = torch.from_numpy(pick).cuda()
    torch.cuda.synchronize()

    def call(rows_ptr, k):
        return lib.mosaic_st_measures(ctx.handle, ring_table.handle, rows_ptr, k, N.ptr(d["area"]), N.ptr(d["length"]), N.ptr(d["cx"]),
                                      N.ptr(d["cy"]), N.ptr(d_np), N.ptr(d["xmin"]), N.ptr(d["ymin"]), N.ptr(d["xmax"]),
                                      N.ptr(d["ymax"]), N.ptr(d_st))

    N.check(call(N.ptr(d_rows), 4))
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got["centroid"] = (got.pop("cx"), got.pop("cy"))
    got["numpoints"], got["status"] = d_np.cpu().numpy(), d_st.cpu().numpy()
    assert_same(got, expect, "device pointers")
    # mixed: a host output next to device outputs, everything else null
    h_len = np.full(4, -7.0)
    N.check(lib.mosaic_st_measures(ctx.handle, ring_table.handle, N.ptr(pick), 4, N.ptr(d["area"]), N.ptr(h_len), None, None, None,
                                   None, None, None, None, None))
    assert np.array_equal(u64(h_len), u64(expect["length"])) and np.array_equal(u64(d["area"].cpu().numpy()), u64(expect["area"]))
    # an index out of range: the error code, and nothing is written, on the host or the device
    for bad in ([0, n], [-1, 0]):
        for v in d.values():
            v.fill_(-7.0)
        d_st.fill_(-1)
        torch.cuda.synchronize()
        b = np.array(bad, np.int64)
        assert call(N.ptr(torch.from_numpy(b).cuda()), 2) == N.MOSAIC_E_ARG
        assert all((v.cpu().numpy() == -7.0).all() for v in d.values()) and (d_st.cpu().numpy() == -1).all()
        h = np.full(2, -7.0)
        rc = lib.mosaic_st_measures(ctx.handle, ring_table.handle, N.ptr(b), 2, N.ptr(h), None, None, None, None, None, None, None,
                                    None, None)
        assert rc == N.MOSAIC_E_ARG and h.tolist() == [-7.0, -7.0]
    # more rows than the column has, without a row list
    h = np.full(n + 1, -7.0)
    assert lib.mosaic_st_measures(ctx.handle, ring_table.handle, None, n + 1, N.ptr(h), None, None, None, None, None, None, None, None,
                                  None) == N.MOSAIC_E_ARG
    # option ranges
    for key, bad in (("meas_tile", 0), ("meas_tile", 257), ("meas_wave_min", -1)):
        with pytest.raises(N.MosaicError):
            ctx.set_option(key, bad)


def test_fixture_columns(ctx):
    """the 35 zones, the 99 pickups as a point column and 64 seeded trips, under both kernels"""
    from mosaic_amd.data import PolygonSet

    from .test_st_distance import pickups
    from .test_st_distance_lines import trips

    zones = PolygonSet.load("nyc_taxi_zones_35")
    x, y = pickups()
    walks = trips(64)
    for name, src, col in (("zones", zones, LCol.from_polyset(zones)), ("pickups", (x, y), LCol.from_points(x, y)),
                           ("trips", walks, LCol.from_lineset(walks))):
        want = host_measures(col)
        with ctx.geometry_table(src) as t:
            for opt in ({}, dict(meas_wave_min=ALL_WAVE), dict(meas_wave_min=ALL_LANE)):
                got, _ = with_options(ctx, opt, lambda: ctx.st_measures(t, WHAT, return_status=True))
                assert_same(got, want, f"{name} {opt}")
    assert len(x) == 99


def test_analyzer_h3_on_263_zones(ctx):
    """get_optimal_resolution() == 9, the reference's pinned answer; every ratio within relative 1e-6 of the
    oracle composition: cell vertices here may differ from the oracle's by 1-2 ulp of ~74 degrees (3e-14); at
    resolution 15 a cell is ~1e-5 degrees wide, so its area moves by ~1e-9 relative -- far below 1e-6, which is
    far below the factor of ~7 between consecutive resolutions"""
    from mosaic_amd import MosaicAnalyzer
    from mosaic_amd import analyzer as A
    from mosaic_amd.data import PolygonSet

    areas, cell_areas = C.nyc_oracle_inputs()
    with MosaicAnalyzer(ctx, PolygonSet.load("nyc_taxi_zones")) as an:
        assert an.get_optimal_resolution() == 9
        assert an.get_optimal_resolution(sample_fraction=1.0) == 9
        for lo, hi in ((1, 100), (5, 500)):
            got = an.get_resolution_metrics(lower_limit=lo, upper_limit=hi)
            want = A.resolution_metrics(areas, cell_areas, lo, hi)
            assert got["resolution"] == want["resolution"]
            for c in A.COLUMNS[1:]:
                assert np.allclose(got[c], want[c], rtol=1e-6, atol=0), (c, got[c], want[c])
        t = an.get_resolution_metrics(lower_limit=1, upper_limit=100)
        assert [r for _, r in sorted(zip(t["percentile_50_geometry_area"], t["resolution"]))] == [8, 9, 10]
        first = an.get_resolution_metrics(sample_rows=50)
        sub_areas, sub_cells = areas[:50], [(r, c[:50]) for r, c in cell_areas]
        want = A.resolution_metrics(sub_areas, sub_cells)
        assert first["resolution"] == want["resolution"]
        assert np.allclose(first["percentile_50_geometry_area"], want["percentile_50_geometry_area"], rtol=1e-6, atol=0)


def test_analyzer_bng_on_london_postcodes():
    from mosaic_amd import MosaicAnalyzer, MosaicContext, NotEnoughGeometries
    from mosaic_amd import analyzer as A
    from mosaic_amd.data import PolygonSet

    zones = PolygonSet.load("london_postcodes_bng").subset(np.arange(6))
    areas = host_measures(LCol.from_polyset(zones), fields=("area",))["area"]
    cell_areas = [(r, np.full(6, float(C.BNG_EDGE[r]) ** 2)) for r in A.BNG_RESOLUTIONS]
    bng = MosaicContext.build("BNG", "JTS")
    try:
        with MosaicAnalyzer(bng, zones) as an:
            got = an.get_resolution_metrics()
            want = A.resolution_metrics(areas, cell_areas)
            assert got["resolution"] == want["resolution"] and want["resolution"]
            for c in A.COLUMNS[1:]:
                assert np.allclose(got[c], want[c], rtol=1e-6, atol=0), c
            assert an.get_optimal_resolution() == A.optimal_resolution(areas, cell_areas)
        # null, row-path and empty rows are left out; none left raises
        with MosaicAnalyzer(bng, [None, "GEOMETRYCOLLECTION EMPTY", "POLYGON EMPTY"]) as an:
            with pytest.raises(NotEnoughGeometries):
                an.get_optimal_resolution()
    finally:
        bng.close()
