"""MosaicAnalyzer (sql/MosaicAnalyzer.scala:28-129): the resolution at which a geometry column is worth
tessellating, from the ratio of the geometries' areas to the area of the grid cell under each
geometry's centroid.

The reference computes, per resolution of the index system, mean(st_area(grid_boundaryaswkb(
grid_longlatascellid(st_centroid(geom), res)))) and divides the mean and the 25th / 50th / 75th
percentile of st_area(geom) by it; ``get_optimal_resolution`` keeps the resolutions where one of the
four ratios lies strictly between 1 and 100, sorts them by the p50 ratio and returns the one at index
(len - 1) // 2.  The arithmetic is in two pure functions (``resolution_metrics``,
``optimal_resolution``: arrays in, table out); ``MosaicAnalyzer`` feeds them through the engine's own
calls.

Where Spark leaves a choice the engine's rule is:
  * all rows by default (the reference samples 1 %: the GPU makes that unnecessary); ``sample_rows=k``
    takes the first k rows (the reference's limit(k)), ``sample_fraction=f < 1`` a seeded Bernoulli
    subset (the reference's sample(f) is unseeded);
  * a percentile p over n values is the value of 1-based rank ceil(p n) in sorted order: what
    percentile_approx(col, p, 10000) returns while n <= 10,000, where its summary is exact;
  * a mean is the in-order sum divided by n;
  * null rows, rows for the row path and empty geometries are left out; no row left raises
    ``NotEnoughGeometries`` (the reference's NotEnoughGeometriesException).
"""
import math

import numpy as np

H3_RESOLUTIONS = tuple(range(16))
BNG_RESOLUTIONS = (-1, 1, -2, 2, -3, 3, -4, 4, -5, 5, -6, 6)  # coarse to fine (BNGIndexSystem.resolutionMap)
COLUMNS = ("resolution", "mean_index_area", "mean_geometry_area", "percentile_25_geometry_area",
           "percentile_50_geometry_area", "percentile_75_geometry_area")


class NotEnoughGeometries(ValueError):
    """MosaicSQLExceptions.NotEnoughGeometriesException: no geometry to take statistics of."""


def mean_in_order(values):
    values = np.ascontiguousarray(values, np.float64)
    return float(np.cumsum(values)[-1]) / len(values)  # cumsum adds in order


def percentile_by_rank(sorted_values, p):
    """the value of 1-based rank ceil(p n)"""
    n = len(sorted_values)
    return float(sorted_values[max(1, math.ceil(p * n)) - 1])


def resolution_metrics(areas, cell_areas, lower_limit=5, upper_limit=500):
    """The reference's metrics table as a dict of columns (COLUMNS), one row per surviving resolution in
    the order given.  ``areas``: st_area of each kept geometry; ``cell_areas``: (resolution, the area
    of the cell under each geometry's centroid) per resolution.  The last four columns are the mean /
    p25 / p50 / p75 of ``areas`` divided by that resolution's mean cell area; a row survives if one of
    the four lies strictly between the limits (MosaicAnalyzer.scala:92-98)."""
    areas = np.ascontiguousarray(areas, np.float64)
    if len(areas) == 0:
        raise NotEnoughGeometries("no geometry to take statistics of")
    ordered = np.sort(areas)
    stats = (mean_in_order(areas), percentile_by_rank(ordered, 0.25), percentile_by_rank(ordered, 0.5),
             percentile_by_rank(ordered, 0.75))
    table = {c: [] for c in COLUMNS}
    for res, cells in cell_areas:
        if len(cells) != len(areas):
            raise ValueError(f"resolution {res}: {len(cells)} cell areas for {len(areas)} geometries")
        index_area = mean_in_order(cells)
        ratios = [s / index_area for s in stats]
        if any(lower_limit < r < upper_limit for r in ratios):
            for c, v in zip(COLUMNS, (int(res), index_area, *ratios)):
                table[c].append(v)
    return table


def optimal_resolution(areas, cell_areas):
    """getOptimalResolution (MosaicAnalyzer.scala:28-39): limits 1 and 100, the surviving rows sorted by
    the p50 ratio, the resolution at index (len - 1) // 2"""
    table = resolution_metrics(areas, cell_areas, 1, 100)
    rows = sorted(zip(table["percentile_50_geometry_area"], table["resolution"]), key=lambda r: r[0])  # stable, like sortBy
    if not rows:
        raise NotEnoughGeometries("no resolution has a ratio between 1 and 100")
    return rows[(len(rows) - 1) // 2][1]


class MosaicAnalyzer:
    """``MosaicAnalyzer(ctx, geoms)``: ``geoms`` is a ``GeometryTable`` or anything
    ``ctx.geometry_table`` accepts (the table is then built here, with ``lines``, and closed by
    ``close()`` or the ``with`` block)."""

    def __init__(self, ctx, geoms, lines=False, seed=0):
        from .context import GeometryTable

        self.ctx = ctx
        self.seed = seed
        self._own = not isinstance(geoms, GeometryTable)
        self.table = ctx.geometry_table(geoms, lines=lines) if self._own else geoms

    def close(self):
        if self._own and self.table is not None:
            self.table.close()
        self.table = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def resolutions(self):
        return H3_RESOLUTIONS if self.ctx.index_system.name == "H3" else BNG_RESOLUTIONS

    def _sample(self, sample_fraction, sample_rows):
        n = len(self.table)
        if sample_fraction is not None and sample_rows is not None:
            raise ValueError("sample_fraction and sample_rows are alternatives")
        if sample_rows is not None:
            if sample_rows < 0:
                raise ValueError("sample_rows must be >= 0")
            return np.arange(min(int(sample_rows), n), dtype=np.int64)
        if sample_fraction is not None:
            if not 0.0 < sample_fraction <= 1.0:
                raise ValueError("sample_fraction must be in (0, 1]")
            if sample_fraction < 1.0:
                return np.flatnonzero(np.random.default_rng(self.seed).random(n) < sample_fraction).astype(np.int64)
        return None

    def measured(self, sample_fraction=None, sample_rows=None):
        """(areas, [(resolution, cell areas)]) of the kept rows, through the engine's calls"""
        from . import _native as N

        ctx = self.ctx
        m = ctx.st_measures(self.table, ("area", "centroid", "numpoints"), rows=self._sample(sample_fraction, sample_rows),
                            return_status=True)
        keep = (m["status"] == N.ROW_OK) & (m["numpoints"] > 0)
        areas = m["area"][keep]
        cx, cy = m["centroid"][0][keep], m["centroid"][1][keep]
        if len(areas) == 0:
            raise NotEnoughGeometries("no geometry to take statistics of")
        cell_areas = []
        for res in self.resolutions():
            cells = ctx.grid_longlatascellid(cx, cy, res, raw=True)
            cell_areas.append((res, ctx.st_area(ctx.grid_boundaryaswkb(cells))))
        return areas, cell_areas

    def get_resolution_metrics(self, sample_fraction=None, sample_rows=None, lower_limit=5, upper_limit=500):
        areas, cell_areas = self.measured(sample_fraction, sample_rows)
        return resolution_metrics(areas, cell_areas, lower_limit, upper_limit)

    def get_optimal_resolution(self, sample_fraction=None, sample_rows=None):
        areas, cell_areas = self.measured(sample_fraction, sample_rows)
        return optimal_resolution(areas, cell_areas)
