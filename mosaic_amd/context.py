"""Host-side mirror of the reference's function surface for the PIP chip-join path.

Mirrors (bransonf/mosaic 0.3.9, src/main/scala/com/databricks/labs/mosaic/):
  * ``MosaicContext.build(indexSystem, geometryAPI)``       functions/MosaicContext.scala:796-800
  * ``functions.grid_pointascellid / grid_longlatascellid``  MosaicContext.scala:655-668
  * ``functions.st_contains``                                MosaicContext.scala (st_contains) ->
                                                             expressions/geometry/ST_Contains.scala:21-64
  * ``H3IndexSystem / BNGIndexSystem.getResolution``         core/index/H3IndexSystem.scala:39-54,
                                                             core/index/BNGIndexSystem.scala:342-353
  * the chip join of the Quickstart                         notebooks/examples/python/QuickstartNotebook.py:205-219,
                                                             sql/join/PointInPolygonJoin.scala:68-84
Everything computes on the GPU through libmosaic_hip.so; inputs are columnar (numpy arrays or torch
tensors, host or device), the Spark row wrappers are not reproduced.  Errors follow the reference:
bad resolutions and NaN BNG coordinates raise ``IllegalStateException`` with the reference's message.
"""
import ctypes
import threading

import numpy as np

from . import _native as N
from . import wkb as W


class IndexSystem:
    name = None
    grid = None
    cell_id_type = "long"

    def get_resolution(self, res):
        raise NotImplementedError


class H3IndexSystem(IndexSystem):
    """core/index/H3IndexSystem.scala; cell ids are LongType."""

    name = "H3"
    grid = N.GRID_H3
    cell_id_type = "long"

    def get_resolution(self, res):
        out = ctypes.c_int(0)
        if isinstance(res, (bool,)):
            raise ValueError("Resolution must be an Int or String.")
        if isinstance(res, (int, np.integer)):
            N.check(N.lib().mosaic_resolution(self.grid, int(res), ctypes.byref(out)))
        elif isinstance(res, str):
            N.check(N.lib().mosaic_resolution_str(self.grid, res.encode(), ctypes.byref(out)))
        else:
            raise ValueError("Resolution must be an Int or String.")
        return out.value

    def format(self, cell_id):
        return format(int(cell_id), "x")

    def parse(self, s):
        return int(s, 16)


class BNGIndexSystem(IndexSystem):
    """core/index/BNGIndexSystem.scala; cell ids default to StringType (MosaicContext.scala:41-48)."""

    name = "BNG"
    grid = N.GRID_BNG
    cell_id_type = "string"

    def get_resolution(self, res):
        out = ctypes.c_int(0)
        if isinstance(res, (int, np.integer)) and not isinstance(res, bool):
            N.check(N.lib().mosaic_resolution(self.grid, int(res), ctypes.byref(out)))
        elif isinstance(res, str):
            N.check(N.lib().mosaic_resolution_str(self.grid, res.encode(), ctypes.byref(out)))
        else:
            raise N.IllegalStateException(N.MOSAIC_E_RES, f"BNG resolution not supported; found {res}")
        return out.value

    def format(self, cell_id):
        buf = ctypes.create_string_buffer(64)
        rc = N.lib().mosaic_bng_format(int(cell_id), buf, 64)
        if rc < 0 or rc > 64:
            N.check(rc if rc > 0 else N.MOSAIC_E_ARG)
        return buf.value.decode()

    def parse(self, s):
        out = ctypes.c_int64(0)
        N.check(N.lib().mosaic_bng_parse(s.encode(), ctypes.byref(out)))
        return out.value


INDEX_SYSTEMS = {"H3": H3IndexSystem, "BNG": BNGIndexSystem}


def _f64(a):
    """Contiguous float64 buffer (numpy or torch, host or device) kept alive by the caller."""
    if hasattr(a, "data_ptr"):
        import torch

        if a.dtype != torch.float64:
            a = a.to(torch.float64)
        return a.contiguous()
    return np.ascontiguousarray(a, dtype=np.float64)


def _is_torch(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


class RowPathRequired(RuntimeError):
    """Rows the engine leaves to the reference's row-wise expression (MOSAIC_ROW_PATH): geometry
    types other than Point (the reference indexes their centroid), POINT EMPTY and malformed rows
    (on which the reference throws).  ``rows`` holds their indices.  The columnar exec of
    INTEGRATION.md evaluates them with PointIndexGeom.nullSafeEval; this mirror reports them."""

    def __init__(self, rows):
        super().__init__(f"{len(rows)} row(s) need the reference row path (first: row {int(rows[0])})")
        self.rows = rows


def geometry_column(geoms):
    """A sequence of WKB (bytes) / WKT (str) / hex-WKB (str with format="hex") rows, None = null,
    as an Arrow-layout column: (format, int64 offsets[n+1], uint8 values, uint8 validity or None)."""
    geoms = list(geoms)
    kinds = {type(g) for g in geoms if g is not None}
    if kinds <= {bytes, bytearray, memoryview}:
        fmt = N.GEOM_WKB
        rows = [bytes(g) if g is not None else b"" for g in geoms]
    elif kinds <= {str}:
        fmt = N.GEOM_WKT
        rows = [g.encode("utf-8") if g is not None else b"" for g in geoms]
    else:
        raise TypeError("a geometry column holds WKB bytes or WKT strings")
    lens = np.fromiter((len(r) for r in rows), np.int64, len(rows))
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer(b"".join(rows), np.uint8) if offsets[-1] else np.zeros(1, np.uint8)
    valid = None
    if any(g is None for g in geoms):
        valid = np.fromiter((g is not None for g in geoms), np.uint8, len(geoms))
    return fmt, offsets, data, valid


class CoordsColumn:
    """The COORDS geometry form (InternalGeometryType: struct<typeId, srid, boundaries:
    array<array<array<double>>>, holes: array<array<array<array<double>>>>>,
    core/types/model/InternalGeometry.scala) as Arrow columns: type_id int32[n], srid int32[n],
    boundary_offsets int32[n + 1] (row -> boundaries), coord_offsets int32 (boundary -> coordinates),
    value_offsets int32 (coordinate -> values), values float64, validity uint8 or None.  The holes
    column is not kept (no point has one)."""

    def __init__(self, type_id, srid, boundary_offsets, coord_offsets, value_offsets, values, valid=None):
        self.type_id = np.ascontiguousarray(type_id, np.int32)
        self.srid = np.ascontiguousarray(srid, np.int32)
        self.boundary_offsets = np.ascontiguousarray(boundary_offsets, np.int32)
        self.coord_offsets = np.ascontiguousarray(coord_offsets, np.int32)
        self.value_offsets = np.ascontiguousarray(value_offsets, np.int32)
        self.values = np.ascontiguousarray(values, np.float64)
        self.valid = None if valid is None else np.ascontiguousarray(valid, np.uint8)

    def __len__(self):
        return len(self.type_id)

    @classmethod
    def from_rows(cls, rows):
        """rows: (type_id, srid, boundaries, holes) tuples -- boundaries a list of coordinate lists,
        a coordinate a list of 2 or 3 floats -- or None for a null row."""
        tid, srid, bo, co, vo, vals, valid = [], [], [0], [0], [0], [], []
        for r in rows:
            valid.append(r is not None)
            t, sr, bnds = (r[0], r[1], r[2]) if r is not None else (0, 0, [])
            tid.append(t)
            srid.append(sr)
            for b in bnds:
                for c in b:
                    vals.extend(float(v) for v in c)
                    vo.append(len(vals))
                co.append(len(vo) - 1)
            bo.append(len(co) - 1)
        return cls(tid, srid, bo, co, vo, vals, np.array(valid, np.uint8))


def st_point(x, y):
    """ST_Point (expressions/constructors/ST_Point.scala:27-32): InternalGeometry(POINT, 0,
    [[[x, y]]], [[]]) per row, as a CoordsColumn."""
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    n = len(x)
    vals = np.empty(2 * n, np.float64)
    vals[0::2] = x
    vals[1::2] = y
    ar = np.arange(n + 1, dtype=np.int32)
    return CoordsColumn(np.ones(n, np.int32), np.zeros(n, np.int32), ar, ar, 2 * ar, vals)


def _is_arrow_utf8(v):
    """An Arrow utf8 column given explicitly as (offsets int32 / int64 array, chars bytes / uint8 array)."""
    if not (isinstance(v, tuple) and len(v) == 2):
        return False
    offs, chars = v
    return (isinstance(offs, np.ndarray) and offs.dtype in (np.int32, np.int64) and
            (isinstance(chars, (bytes, bytearray)) or (isinstance(chars, np.ndarray) and chars.dtype == np.uint8)))


def _points_xy(points):
    """Accepts (x, y) arrays or an (n, 2) array (host or device)."""
    if isinstance(points, tuple) and len(points) == 2:
        return _f64(points[0]), _f64(points[1])
    if isinstance(points, np.ndarray) and points.ndim == 2 and points.shape[1] == 2:
        return _f64(points[:, 0]), _f64(points[:, 1])
    if _is_torch(points) and points.dim() == 2:
        return _f64(points[:, 0]), _f64(points[:, 1])
    return None


def _chip_columns(ctx, is_core, index_id, wkb_list, key):
    """Chip columns as the contiguous arrays the library reads: (is_core uint8, index_id int64,
    key int32, wkb offsets int32 / int64, wkb data uint8).  wkb_list: an Arrow (offsets, data) pair or
    a list of bytes / None."""
    is_core = np.ascontiguousarray(is_core, dtype=np.uint8)
    strings = not _is_arrow_utf8(index_id) and len(index_id) and isinstance(index_id[0], str)
    if ctx.index_system.cell_id_type == "string" and (_is_arrow_utf8(index_id) or strings):
        # StringType ids (the BNG default, BNGIndexSystem.scala:28): parsed on the GPU
        index_id = ctx.bng_parse_column(index_id)
    elif strings:
        # string ids of a LongType index system (H3 hex strings, H3IndexSystem.parse)
        index_id = [ctx.index_system.parse(v) for v in index_id]
    elif _is_arrow_utf8(index_id):
        raise ValueError(f"an Arrow utf8 id column needs a StringType index system, not {ctx.index_system.name}")
    index_id = np.ascontiguousarray(index_id, dtype=np.int64)
    key = np.ascontiguousarray(key, dtype=np.int32)
    if isinstance(wkb_list, tuple) and len(wkb_list) == 2:
        # Arrow binary (int32 offsets) or large_binary (int64)
        offsets = np.ascontiguousarray(wkb_list[0])
        if offsets.dtype != np.int32:
            offsets = offsets.astype(np.int64, copy=False)
        data = np.ascontiguousarray(wkb_list[1], dtype=np.uint8)
    else:
        lens = np.array([0 if w is None else len(w) for w in wkb_list], dtype=np.int64)
        offsets = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=offsets[1:])
        data = np.frombuffer(b"".join(b"" if w is None else bytes(w) for w in wkb_list), dtype=np.uint8)
        data = np.ascontiguousarray(data) if len(data) else np.zeros(1, np.uint8)
    n = len(index_id)
    if not (len(is_core) == n == len(key) == len(offsets) - 1):
        raise ValueError("chip columns have different lengths")
    return is_core, index_id, key, offsets, data


class ChipTable:
    """Device-resident build side of the chip join: rows of ChipType(is_core, index_id, wkb) plus the
    key of the polygon each chip belongs to (core/types/ChipType.scala:17-28)."""

    def __init__(self, ctx, is_core, index_id, wkb_list, polygon_key, n_polygons=None):
        self.ctx = ctx
        is_core, index_id, polygon_key, offsets, data = _chip_columns(ctx, is_core, index_id, wkb_list, polygon_key)
        n = len(index_id)
        if n_polygons is None:
            n_polygons = int(polygon_key.max()) + 1 if n else 0
        self.n_polygons = int(n_polygons)
        self.n_chips = n
        h = ctypes.c_void_p()
        N.check(N.lib().mosaic_chip_table_create_arrow(
            ctx.handle, ctx.index_system.grid, ctx.resolution_of_table, n, N.ptr(is_core), N.ptr(index_id),
            N.ptr(offsets), 1 if offsets.dtype == np.int32 else 0, N.ptr(data), N.ptr(polygon_key), self.n_polygons,
            ctypes.byref(h)))
        self.handle = h

    @classmethod
    def from_arrays(cls, ctx, chip_offsets, is_core, index_id, wkb_list):
        """The array form of the build side (PointInPolygonJoin.joinArrayRows,
        sql/join/PointInPolygonJoin.scala:39-66): polygon row p's chip array (grid_tessellate output)
        is rows [chip_offsets[p], chip_offsets[p + 1]) of the flattened chip columns; a point joins a
        row at most once, through the row's first chip with the point's cell."""
        self = cls.__new__(cls)
        self.ctx = ctx
        chip_offsets = np.ascontiguousarray(chip_offsets, dtype=np.int64)
        is_core = np.ascontiguousarray(is_core, dtype=np.uint8)
        index_id = np.ascontiguousarray(index_id, dtype=np.int64)
        lens = np.array([0 if w is None else len(w) for w in wkb_list], dtype=np.int64)
        offsets = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=offsets[1:])
        data = np.frombuffer(b"".join(b"" if w is None else bytes(w) for w in wkb_list), dtype=np.uint8)
        data = np.ascontiguousarray(data) if len(data) else np.zeros(1, np.uint8)
        self.n_polygons = len(chip_offsets) - 1
        self.n_chips = len(index_id)
        h = ctypes.c_void_p()
        N.check(N.lib().mosaic_chip_table_create_arrays(
            ctx.handle, ctx.index_system.grid, ctx.resolution_of_table, self.n_polygons, N.ptr(chip_offsets),
            N.ptr(is_core), N.ptr(index_id), N.ptr(offsets), N.ptr(data), ctypes.byref(h)))
        self.handle = h
        return self

    def info(self):
        out = np.zeros(8, np.int64)
        N.check(N.lib().mosaic_chip_table_info(self.handle, N.ptr(out)))
        keys = ["n_chips", "n_cells", "n_border", "n_vertices", "n_rings", "device_bytes", "hash_capacity",
                "n_polygons"]
        return dict(zip(keys, (int(v) for v in out)))

    def tiles(self):
        """The H3 tile directory of this table (tiles.h): whether it was built, and its size."""
        out = np.zeros(13, np.int64)
        N.check(N.lib().mosaic_chip_table_tiles(self.handle, N.ptr(out)))
        keys = ["built", "nx", "ny", "records", "entries", "full_tiles", "rings", "raster", "raster_sub",
                "raster_cell", "pure_sub_blocks", "mixed_sub_blocks", "mixed_cells"]
        d = dict(zip(keys, (int(v) for v in out)))
        g = np.zeros(4, np.float64)
        N.check(N.lib().mosaic_chip_table_tile_grid(self.handle, N.ptr(g)))
        d.update(x0=float(g[0]), y0=float(g[1]), sx=float(g[2]), sy=float(g[3]))
        r = np.zeros(9, np.int64)
        N.check(N.lib().mosaic_chip_table_raster(self.handle, N.ptr(r)))
        d.update(line_sub_blocks=int(r[0]), quad_entries=int(r[1]), quad_shift=int(r[2]), raster_bytes=int(r[3]),
                 stream=int(r[4]), image_records=int(r[5]), image_bytes=int(r[6]), image_max_bytes=int(r[7]),
                 leaf_lines=int(r[8]))
        return d

    def build_info(self):
        """Build cost of this table in ms (chip core, tile directory, point-raster classification,
        point-raster assembly) and the point raster's FNV-1a digest (0: no raster)."""
        ms = np.zeros(4, np.float64)
        dig = np.zeros(1, np.uint64)
        N.check(N.lib().mosaic_chip_table_build_info(self.handle, N.ptr(ms), N.ptr(dig)))
        return dict(core_ms=float(ms[0]), directory_ms=float(ms[1]), raster_classify_ms=float(ms[2]),
                    raster_assemble_ms=float(ms[3]), raster_digest=int(dig[0]))

    def close(self):
        if self.handle:
            N.lib().mosaic_chip_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LineChipTable:
    """Device-resident line chips (grid_tessellateexplode over a LineSet, Mosaic.lineFill): rows of
    ChipType(is_core, index_id, wkb) holding LINESTRING / MULTILINESTRING pieces or POINT / MULTIPOINT
    contacts, plus the key of the line each chip belongs to.  The line side of
    MosaicContext.st_intersects_aggregate.  wkb: an Arrow (offsets, data) pair or a list of bytes / None."""

    def __init__(self, ctx, is_core, index_id, wkb, key, resolution):
        self.ctx = ctx
        is_core, index_id, key, offsets, data = _chip_columns(ctx, is_core, index_id, wkb, key)
        self.n_chips = len(index_id)
        h = ctypes.c_void_p()
        N.check(N.lib().mosaic_line_chips_create(
            ctx.handle, ctx.index_system.grid, ctx.index_system.get_resolution(resolution), self.n_chips,
            N.ptr(is_core), N.ptr(index_id), N.ptr(key), N.ptr(offsets), 1 if offsets.dtype == np.int32 else 0,
            N.ptr(data), ctypes.byref(h)))
        self.handle = h

    def info(self):
        out = np.zeros(4, np.int64)
        N.check(N.lib().mosaic_line_chips_info(self.handle, N.ptr(out)))
        return dict(zip(["n_chips", "n_pieces", "n_vertices", "device_bytes"], (int(v) for v in out)))

    def close(self):
        if self.handle:
            N.lib().mosaic_line_chips_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def line_intersects_aggregate_host(index_system, line_chips, polygon_chips, resolution):
    """st_intersects_aggregate over the join of line chips with polygon chips on the host
    (mosaic_line_intersects_aggregate_host: no context, no GPU): the two chip dicts `tessellate`
    returns -> (line_key int32, polygon_key int32, flag bool), sorted by (line key, polygon key)."""
    if isinstance(index_system, str):
        index_system = INDEX_SYSTEMS[index_system]()
    res = index_system.get_resolution(resolution)

    def cols(c):
        off = np.ascontiguousarray(c["wkb"][0], dtype=np.int64)
        data = np.ascontiguousarray(c["wkb"][1], dtype=np.uint8)
        return (len(c["index_id"]), np.ascontiguousarray(c["is_core"], dtype=np.uint8),
                np.ascontiguousarray(c["index_id"], dtype=np.int64), np.ascontiguousarray(c["polygon_key"], dtype=np.int32),
                off if len(off) else np.zeros(1, np.int64), data if len(data) else np.zeros(1, np.uint8))

    L, P = cols(line_chips), cols(polygon_chips)
    cap = 1024
    while True:
        lk = np.empty(cap, np.int32)
        pk = np.empty(cap, np.int32)
        fl = np.empty(cap, np.uint8)
        n_out = ctypes.c_int64(0)
        rc = N.lib().mosaic_line_intersects_aggregate_host(
            index_system.grid, res, L[0], *[N.ptr(a) for a in L[1:]], P[0], *[N.ptr(a) for a in P[1:]],
            N.ptr(lk), N.ptr(pk), N.ptr(fl), cap, ctypes.byref(n_out))
        if rc == N.MOSAIC_E_CAPACITY and n_out.value > cap:
            cap = int(n_out.value)
            continue
        N.check(rc)
        k = int(n_out.value)
        return lk[:k], pk[:k], fl[:k].astype(bool)


def _export_isect_geoms(h):
    """A mosaic_isect_geoms handle -> (left_key, right_key, area or length, status, wkb list); releases it."""
    try:
        n, nb = ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(N.lib().mosaic_isect_geoms_info(h, ctypes.byref(n), ctypes.byref(nb)))
        k = int(n.value)
        lk = np.empty(k, np.int32)
        rk = np.empty(k, np.int32)
        ar = np.empty(k, np.float64)
        st = np.empty(k, np.uint8)
        off = np.empty(k + 1, np.int64)
        data = np.empty(max(int(nb.value), 1), np.uint8)
        N.check(N.lib().mosaic_isect_geoms_export(h, N.ptr(lk), N.ptr(rk), N.ptr(ar), N.ptr(st), N.ptr(off), N.ptr(data)))
    finally:
        N.lib().mosaic_isect_geoms_destroy(h)
    wkb = [None if st[i] else bytes(data[off[i]:off[i + 1]]) for i in range(k)]
    return lk, rk, ar, st, wkb


def line_intersection_aggregate_host(index_system, line_chips, polygon_chips, resolution):
    """st_intersection_aggregate over the join of line chips with polygon chips on the host
    (mosaic_line_intersection_aggregate_host: no context, no GPU): the two chip dicts `tessellate`
    returns -> (line_key int32, polygon_key int32, length float64, status uint8 (all 0), wkb list of
    bytes), sorted by (line key, polygon key).  What MosaicContext.st_intersection_aggregate returns
    for a LineChipTable and a ChipTable, bit for bit."""
    if isinstance(index_system, str):
        index_system = INDEX_SYSTEMS[index_system]()
    res = index_system.get_resolution(resolution)

    def cols(c):
        off = np.ascontiguousarray(c["wkb"][0], dtype=np.int64)
        data = np.ascontiguousarray(c["wkb"][1], dtype=np.uint8)
        return (len(c["index_id"]), np.ascontiguousarray(c["is_core"], dtype=np.uint8),
                np.ascontiguousarray(c["index_id"], dtype=np.int64), np.ascontiguousarray(c["polygon_key"], dtype=np.int32),
                off if len(off) else np.zeros(1, np.int64), data if len(data) else np.zeros(1, np.uint8))

    L, P = cols(line_chips), cols(polygon_chips)
    h = ctypes.c_void_p()
    N.check(N.lib().mosaic_line_intersection_aggregate_host(
        index_system.grid, res, L[0], *[N.ptr(a) for a in L[1:]], P[0], *[N.ptr(a) for a in P[1:]], ctypes.byref(h)))
    return _export_isect_geoms(h)


_WKB_ROW_PATH = b"\x00\x00\x00\x00\x02\x00\x00\x00\x00"  # LINESTRING EMPTY: stands for a row the engine does not serve


_WKB_ROW_PATH_LINES = b"\x00\x00\x00\x00\x07\x00\x00\x00\x00"  # GEOMETRYCOLLECTION EMPTY: the same, in a column that serves lines


def _wkt_row_wkb(text, lines=False):
    """A WKT row as the WKB the geometry column decodes; what wkb.read_wkt does not read
    (collections, malformed text; line geometries unless ``lines``) becomes a row for the row path.
    With ``lines`` LINESTRING / MULTILINESTRING text is converted too, and the row-path marker is
    GEOMETRYCOLLECTION EMPTY: LINESTRING EMPTY is a served row there."""
    row_path = _WKB_ROW_PATH_LINES if lines else _WKB_ROW_PATH
    kinds = ("POINT", "MULTIPOINT", "POLYGON", "MULTIPOLYGON") + (("LINESTRING", "MULTILINESTRING") if lines else ())
    head = text.split("(", 1)[0].split()
    if not head or head[0].upper() not in kinds:
        return row_path
    try:
        kind, g = W.read_wkt(text)
    except (ValueError, IndexError):
        return row_path
    if kind == "point":
        return W.point_wkb(*(g if g is not None else (float("nan"), float("nan"))))
    if kind == "multipoint":
        return W.multipoint_wkb(g)
    if kind == "linestring":
        if not g and not text.rstrip().upper().endswith("EMPTY"):  # no component was read from text that is not EMPTY
            return row_path
        return W.multilinestring_wkb(g) if len(g) > 1 else W.linestring_wkb(g[0] if g else [])
    return W.geometry_wkb(g) if len(g) != 1 else W.polygon_wkb(g[0])


class GeometryTable:
    """A device-resident geometry column (mosaic_geoms): Point, MultiPoint, LineString,
    MultiLineString, Polygon and MultiPolygon rows in the flat ring layout, immutable after creation
    and usable from any thread, for ``MosaicContext.st_distance``.  Line rows are served by a table
    built from a LineSet or with ``lines=True``; in a table of WKB / WKT rows built without it they
    stay rows for the row path.  The KNN iteration evaluates distances against the same candidate
    column on every round (models/knn/GridRingNeighbours.scala:76-99), so the column outlives a call.
    Built by ``MosaicContext.geometry_table``; ``close()`` frees the device memory."""

    def __init__(self, ctx, geoms, lines=False):
        self.ctx = ctx
        h = ctypes.c_void_p()
        lib = N.lib()
        if hasattr(geoms, "geom_lines"):  # a LineSet
            N.check(lib.mosaic_geoms_create_lines(ctx.handle, len(geoms), N.ptr(geoms.geom_lines), N.ptr(geoms.line_offsets),
                                                  N.ptr(geoms.xy), ctypes.byref(h)))
            self.handle = h
            self.n_geoms = self.info()["n_geoms"]
            return
        rows_given = isinstance(geoms, (list, tuple)) and any(g is None or isinstance(g, (str, bytes, bytearray, memoryview))
                                                            for g in geoms)
        xy = None if hasattr(geoms, "geom_parts") or rows_given else _points_xy(geoms)
        if hasattr(geoms, "geom_parts"):  # a PolygonSet
            N.check(lib.mosaic_geoms_create_arrays(ctx.handle, len(geoms), N.ptr(geoms.geom_parts), N.ptr(geoms.part_rings),
                                                   N.ptr(geoms.ring_offsets), N.ptr(geoms.xy), ctypes.byref(h)))
        elif xy is not None:
            x, y = xy
            if len(x) != len(y):
                raise ValueError("x and y have different lengths")
            ctx._order(x, y)
            N.check(lib.mosaic_geoms_create_points(ctx.handle, N.ptr(x), N.ptr(y), len(x), ctypes.byref(h)))
        else:
            if isinstance(geoms, (str, bytes, bytearray)):
                geoms = [geoms]
            rows = [_wkt_row_wkb(g, lines) if isinstance(g, str) else g for g in geoms]
            _, offsets, data, valid = geometry_column(rows)
            if lines:
                N.check(lib.mosaic_geoms_create_wkb_ex(ctx.handle, len(rows), N.ptr(offsets), N.ptr(data), N.ptr(valid),
                                                       N.GEOMS_LINES, ctypes.byref(h)))
            else:
                N.check(lib.mosaic_geoms_create_wkb(ctx.handle, len(rows), N.ptr(offsets), N.ptr(data), N.ptr(valid),
                                                    ctypes.byref(h)))
        self.handle = h
        info = self.info()
        self.n_geoms = info["n_geoms"]

    def __len__(self):
        return self.n_geoms

    def info(self):
        n, v, p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(N.lib().mosaic_geoms_info(self.handle, ctypes.byref(n), ctypes.byref(v), ctypes.byref(p)))
        return dict(n_geoms=n.value, n_vertices=v.value, n_row_path=p.value)

    def close(self):
        if self.handle:
            N.lib().mosaic_geoms_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MosaicContext:
    """``MosaicContext.build(indexSystem, geometryAPI)``; geometry API is JTS semantics only."""

    def __init__(self, index_system="H3", geometry_api="JTS", device=0, jdk=8):
        if geometry_api.upper() != "JTS":
            raise ValueError("only JTS semantics are implemented (BASELINE north_star)")
        if index_system not in INDEX_SYSTEMS:
            raise ValueError(f"unsupported index system {index_system} (H3, BNG)")
        self.index_system = INDEX_SYSTEMS[index_system]()
        self.geometry_api = "JTS"
        h = ctypes.c_void_p()
        N.check(N.lib().mosaic_init(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = device
        self.set_option("jdk", jdk)
        self.resolution_of_table = None
        self._bound = threading.local()  # per calling thread: the stream set with set_stream

    @classmethod
    def build(cls, index_system="H3", geometry_api="JTS", device=0, jdk=8):
        return cls(index_system, geometry_api, device, jdk)

    def set_option(self, key, value):
        N.check(N.lib().mosaic_set_option(self.handle, key.encode(), int(value)))

    def stream(self):
        s = ctypes.c_void_p()
        N.check(N.lib().mosaic_get_stream(self.handle, ctypes.byref(s)))
        return s.value

    def set_stream(self, stream_handle):
        N.check(N.lib().mosaic_set_stream(self.handle, stream_handle))
        # a null handle binds no caller stream of ours to order against (HIP's null stream)
        self._bound.stream = stream_handle or None

    def wait_event(self, event_handle):
        """Order this thread's later calls after a recorded hipEvent_t (mosaic_stream_wait_event)."""
        N.check(N.lib().mosaic_stream_wait_event(self.handle, event_handle))

    def _order(self, *arrays):
        """Device columns written on torch's current stream are complete before the engine's own
        (non-blocking) stream reads them: without a stream bound with set_stream, an event recorded
        on torch's current stream is waited for on the engine's stream (no host block); a bound
        stream orders the work itself."""
        if getattr(self._bound, "stream", None) is not None:
            return
        for a in arrays:
            if _is_torch(a) and a.is_cuda:
                import torch

                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(a.device))
                self.wait_event(ev.cuda_event)
                self._bound.last_event = ev  # kept alive until the next ordered call
                return

    def sync(self):
        N.check(N.lib().mosaic_sync(self.handle))

    def last_kernel(self):
        """name of the dominant kernel of this thread's last join call (mosaic_last_kernel)"""
        return N.lib().mosaic_last_kernel(self.handle).decode()

    def kernel_times(self, cap=4096):
        """Elapsed ms of each fused join kernel since option "timing" was set (HIP events)."""
        out = np.zeros(cap, np.float64)
        n = ctypes.c_int64(0)
        N.check(N.lib().mosaic_kernel_times(self.handle, N.ptr(out), cap, ctypes.byref(n)))
        return out[:min(n.value, cap)]

    def thread_release(self):
        """Free the calling thread's execution state on this context (its stream, scratch, events);
        a later call from the thread creates a fresh one (mosaic_thread_release)."""
        N.check(N.lib().mosaic_thread_release(self.handle))
        # the released state's stream binding is gone: later calls run on a fresh context stream
        self._bound.stream = None

    def thread_states(self):
        """(live per-thread states, scratch bytes they hold) (mosaic_thread_count)."""
        n, b = ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(N.lib().mosaic_thread_count(self.handle, ctypes.byref(n), ctypes.byref(b)))
        return n.value, b.value

    def last_binned_rows(self):
        """Rows the last join on this thread sorted on its binned path (0: another path)."""
        out = np.zeros(1, np.int64)
        N.check(N.lib().mosaic_last_binned_rows(self.handle, N.ptr(out)))
        return int(out[0])

    def last_queue(self):
        """Queue counts of this thread's last join call: rows its stream kernel queued, and rows
        k_join_leaf passed on to k_join_mixed; both 0 when no stream kernel ran (mosaic_last_queue)."""
        out = np.zeros(2, np.int64)
        N.check(N.lib().mosaic_last_queue(self.handle, N.ptr(out)))
        return {"stream_queued": int(out[0]), "leaf_forwarded": int(out[1])}

    def last_stats(self):
        out = np.zeros(3, np.int64)
        N.check(N.lib().mosaic_last_stats(self.handle, N.ptr(out)))
        return {"exact_path_rows": int(out[0]), "contains_tests": int(out[1]), "pairs": int(out[2])}

    def close(self):
        if getattr(self, "handle", None):
            N.lib().mosaic_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- grid functions ----
    def _cells(self, x, y, resolution, valid=None):
        res = self.index_system.get_resolution(resolution)
        x, y = _f64(x), _f64(y)
        self._order(x, y, valid)
        n = int(x.shape[0])
        if _is_torch(x):
            import torch

            out = torch.empty(n, dtype=torch.int64, device=x.device)
        else:
            out = np.empty(n, np.int64)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        ov = None if v is None else np.empty(n, np.uint8)
        N.check(N.lib().mosaic_point_to_cell(self.handle, self.index_system.grid, res, N.ptr(x), N.ptr(y), N.ptr(v), n,
                                             N.ptr(out), N.ptr(ov)))
        return (out, ov) if v is not None else out

    def _serialize(self, cells):
        """IndexSystem.serializeCellId: Long for H3, String for BNG (IndexSystem.scala:37-46)."""
        if self.index_system.cell_id_type == "string":
            offs, chars = self.bng_format_column(cells)
            return [chars[offs[i]:offs[i + 1]].decode() for i in range(len(offs) - 1)]
        return cells

    def bng_format_column(self, cells, valid=None):
        """BNG ids -> Arrow utf8 column (int64 offsets[n + 1], bytes), formatted on the GPU
        (BNGIndexSystem.format, BNGIndexSystem.scala:114-129)."""
        ids = cells.contiguous() if _is_torch(cells) else np.ascontiguousarray(cells, np.int64)
        self._order(ids, valid)
        n = int(ids.shape[0])
        offs = np.zeros(n + 1, np.int64)
        need = ctypes.c_int64(0)
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        cap = 16 * n
        chars = np.zeros(max(cap, 1), np.uint8)
        N.check(N.lib().mosaic_bng_format_column(self.handle, N.ptr(ids), None if v is None else N.ptr(v), n,
                                                 N.ptr(offs), N.ptr(chars), cap, ctypes.byref(need)))
        return offs, chars[:need.value].tobytes()

    def bng_parse_column(self, strings, valid=None):
        """BNG string ids -> long ids, parsed on the GPU (BNGIndexSystem.parse,
        BNGIndexSystem.scala:391-413).  ``strings``: a sequence of str (None = null) or an Arrow utf8
        tuple (offsets int32 / int64, chars)."""
        if _is_arrow_utf8(strings):
            offs, chars = strings
            offs = np.ascontiguousarray(offs)
            chars = np.frombuffer(chars, np.uint8) if isinstance(chars, (bytes, bytearray)) else np.ascontiguousarray(chars, np.uint8)
        else:
            enc = [b"" if v is None else v.encode() for v in strings]
            if valid is None and any(v is None for v in strings):
                valid = np.array([v is not None for v in strings], np.uint8)
            offs = np.zeros(len(enc) + 1, np.int32)
            np.cumsum([len(e) for e in enc], out=offs[1:])
            chars = np.frombuffer(b"".join(enc) or b"\0", np.uint8)
        o32 = 1 if offs.dtype == np.int32 else 0
        if not o32:
            offs = offs.astype(np.int64, copy=False)
        n = len(offs) - 1
        out = np.zeros(max(n, 1), np.int64)
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        N.check(N.lib().mosaic_bng_parse_column(self.handle, o32, N.ptr(offs), N.ptr(chars), N.ptr(v), n, N.ptr(out)))
        return out[:n]

    def grid_longlatascellid(self, lon, lat, resolution, raw=False):
        """PointIndexLonLat (expressions/index/PointIndexLonLat.scala:44-51)."""
        cells = self._cells(lon, lat, resolution)
        return cells if raw else self._serialize(cells)

    def grid_pointascellid(self, points, resolution, raw=False, fmt=None, return_status=False):
        """PointIndexGeom (expressions/index/PointIndexGeom.scala:32-40).  ``points``: (x, y)
        arrays / an (n, 2) array, or a geometry column -- a sequence of WKB bytes / WKT strings
        (None = null) or an Arrow-layout tuple (offsets, values, validity) with ``fmt`` one of
        "wkb" / "wkt" / "hex" -- decoded on the device (mosaic_point_geom_to_cell).  Rows the
        engine leaves to the reference row path raise RowPathRequired unless return_status, which
        returns (cells, row_status) with row_status 0 null / 1 ok / 2 row path."""
        xy = _points_xy(points)
        if xy is not None:
            cells = self._cells(xy[0], xy[1], resolution)
            return cells if raw else self._serialize(cells)
        res = self.index_system.get_resolution(resolution)
        if isinstance(points, CoordsColumn):
            n = len(points)
            out = np.empty(n, np.int64)
            status = np.empty(n, np.uint8)
            n_rp = ctypes.c_int64(0)
            N.check(N.lib().mosaic_point_coords_to_cell(
                self.handle, self.index_system.grid, res, N.ptr(points.type_id), N.ptr(points.boundary_offsets),
                N.ptr(points.coord_offsets), N.ptr(points.value_offsets),
                N.ptr(points.values) if len(points.values) else None, N.ptr(points.valid), n, N.ptr(out),
                N.ptr(status), ctypes.byref(n_rp)))
            if n_rp.value and not return_status:
                raise RowPathRequired(np.flatnonzero(status == N.ROW_PATH))
            cells = out if raw else self._serialize(out)
            return (cells, status) if return_status else cells
        if isinstance(points, tuple) and len(points) == 3:
            offsets, data, valid = points
            f = {"wkb": N.GEOM_WKB, "wkt": N.GEOM_WKT, "hex": N.GEOM_HEX}[fmt or "wkb"]
        else:
            f, offsets, data, valid = geometry_column(points)
            if fmt == "hex":
                f = N.GEOM_HEX
        if not _is_torch(offsets):
            offsets = np.ascontiguousarray(offsets)
            if offsets.dtype == np.int32:
                f |= N.GEOM_OFFSETS32
            else:
                offsets = offsets.astype(np.int64, copy=False)
        elif str(offsets.dtype) == "torch.int32":
            f |= N.GEOM_OFFSETS32
        if valid is not None and not _is_torch(valid):
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
        n = int(offsets.shape[0]) - 1
        self._order(offsets, data, valid)
        if _is_torch(offsets):
            import torch

            out = torch.empty(n, dtype=torch.int64, device=offsets.device)
            status = torch.empty(n, dtype=torch.uint8, device=offsets.device)
        else:
            out = np.empty(n, np.int64)
            status = np.empty(n, np.uint8)
        n_rp = ctypes.c_int64(0)
        N.check(N.lib().mosaic_point_geom_to_cell(self.handle, self.index_system.grid, res, f, N.ptr(offsets),
                                                  N.ptr(data), N.ptr(valid), n, N.ptr(out), N.ptr(status),
                                                  ctypes.byref(n_rp)))
        if n_rp.value and not return_status:
            st = status.cpu().numpy() if _is_torch(status) else status
            raise RowPathRequired(np.flatnonzero(st == N.ROW_PATH))
        cells = out if raw else self._serialize(out)
        return (cells, status) if return_status else cells

    def decode_points(self, points, fmt=None):
        """Point geometry column (as in grid_pointascellid) -> (x, y) on the device decoder
        (mosaic_point_geom_decode); raises RowPathRequired for rows it does not decode."""
        if isinstance(points, tuple) and len(points) == 3:
            offsets, data, valid = points
            f = {"wkb": N.GEOM_WKB, "wkt": N.GEOM_WKT, "hex": N.GEOM_HEX}[fmt or "wkb"]
        else:
            f, offsets, data, valid = geometry_column(points)
            if fmt == "hex":
                f = N.GEOM_HEX
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype == np.int32:
            f |= N.GEOM_OFFSETS32
        else:
            offsets = offsets.astype(np.int64, copy=False)
        n = len(offsets) - 1
        x, y, status = np.empty(n), np.empty(n), np.empty(n, np.uint8)
        n_rp = ctypes.c_int64(0)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        N.check(N.lib().mosaic_point_geom_decode(self.handle, f, N.ptr(offsets), N.ptr(data), N.ptr(v), n, N.ptr(x),
                                                 N.ptr(y), N.ptr(status), ctypes.byref(n_rp)))
        if n_rp.value or (status == N.ROW_NULL).any():
            raise RowPathRequired(np.flatnonzero(status != N.ROW_OK))
        return x, y

    # ---- st_contains ----
    def st_contains(self, geoms, points):
        """Row-wise st_contains(geom, point): geoms are WKB bytes or WKT strings (one per row, or one
        for all rows); points as in grid_pointascellid (a point geometry column is decoded on the
        device; rows it leaves to the row path raise RowPathRequired)."""
        xy = _points_xy(points)
        if xy is None:
            xy = self.decode_points(points)
        x, y = xy
        if _is_torch(x):
            x, y = x.cpu(), y.cpu()
        x, y = np.asarray(x), np.asarray(y)
        n = len(x)
        if isinstance(geoms, (str, bytes, bytearray)):
            geoms = [geoms]
            index = np.zeros(n, np.int32)
        else:
            geoms = list(geoms)
            if len(geoms) != n:
                raise ValueError("one geometry per point row expected")
            index = np.arange(n, dtype=np.int32)
        blobs = []
        for g in geoms:
            if isinstance(g, str):
                kind, parts = W.read_wkt(g)
                if kind != "polygon":
                    raise ValueError("st_contains left side must be polygonal in this engine")
                blobs.append(W.geometry_wkb(parts) if parts else b"")
            else:
                blobs.append(bytes(g))
        lens = np.array([len(b) for b in blobs], np.int64)
        offs = np.zeros(len(blobs) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        data = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8).copy()
        out = np.zeros(n, np.uint8)
        N.check(N.lib().mosaic_st_contains(self.handle, len(blobs), N.ptr(offs), N.ptr(data), N.ptr(index),
                                           N.ptr(np.ascontiguousarray(x)), N.ptr(np.ascontiguousarray(y)), n,
                                           N.ptr(out)))
        return out.astype(bool)

    # ---- st_distance ----
    def geometry_table(self, geoms, lines=False):
        """A ``GeometryTable``: ``geoms`` as a device-resident geometry column.  Accepts a PolygonSet;
        a LineSet (LineString / MultiLineString rows; a component of one vertex makes its row a row
        for the row path); a sequence of WKB (bytes) or WKT (str) rows of POINT / MULTIPOINT /
        POLYGON / MULTIPOLYGON, None = null (one row may be given bare); or points as an ``(x, y)``
        pair or an ``[n, 2]`` array or tensor, on the host or the device.  Collections, POINT EMPTY
        and undecodable rows are kept as rows for the reference's row path.  So are LINESTRING /
        MULTILINESTRING rows among WKB / WKT rows, unless ``lines=True``: then they are served like
        the rows of a LineSet (LINESTRING EMPTY is a served row at distance 0.0).  ``lines`` changes
        nothing for a PolygonSet, a LineSet or points."""
        return GeometryTable(self, geoms, lines)

    def st_distance(self, left, right, pairs=None, return_status=False):
        """st_distance(left, right) (functions/MosaicContext.scala:146 ST_Distance ->
        expressions/geometry/ST_Distance.scala:34-36 -> core/geometry/MosaicGeometryJTS.distance ->
        JTS 1.19 Geometry.distance / DistanceOp.distance; docs/source/api/spatial-functions.rst:416-471),
        and step 3 of the KNN iteration (models/knn/GridRingNeighbours.scala:153-156), on this
        context's GPU (mosaic_st_distance): 0.0 when either geometry is empty or a polygon of one
        contains a component of the other (a line contains nothing, closed or not), otherwise the
        smallest JTS segment / point distance over all pairs of facets -- the bits of the sequential
        definition in mosaic_amd/csrc/st_distance.h.  Point, MultiPoint, LineString, MultiLineString,
        Polygon and MultiPolygon rows are served on either side.

        ``left`` / ``right``: ``GeometryTable``s, or anything ``geometry_table`` accepts, a LineSet
        included (the table is then built and closed inside the call; WKB / WKT line rows need a
        table built with ``lines=True``).  ``pairs=None`` is row-wise: the lengths match, or
        one side is a single geometry that every row of the other is measured against (as in
        ``st_contains``).  ``pairs=(left_idx, right_idx)`` evaluates exactly those (left row, right
        row) pairs; the index arrays may live on the device.  Returns a float64 array with NaN on
        null rows.  Rows either side leaves to the row path raise ``RowPathRequired`` with the pair
        indices, unless return_status, which adds the pairs' status array (ROW_OK / ROW_NULL /
        ROW_PATH; NaN on the row-path pairs too)."""
        return self._pair_call("st_distance", N.lib().mosaic_st_distance, np.float64, left, right, pairs, return_status)

    def _pair_call(self, name, entry, dtype, left, right, pairs, return_status):
        """The argument handling that the pair functions over geometry columns share (st_distance,
        st_intersects): the two sides as tables (built and closed here unless given as tables), the
        row-wise form with a single geometry broadcast, or the pair list on the host or the device;
        then ``entry(ctx, left, right, left_row, right_row, n, out, status)`` with a zeroed ``out`` of
        ``dtype``.  Returns out (and status): row-path pairs raise unless return_status."""
        own = []
        try:
            tabs = []
            for side in (left, right):
                if not isinstance(side, GeometryTable):
                    side = self.geometry_table(side)
                    own.append(side)
                tabs.append(side)
            lt, rt = tabs
            if pairs is None:
                nl, nr = len(lt), len(rt)
                if nl == nr:
                    n, li, ri = nl, None, None
                elif nl == 1 or nr == 1:
                    n = max(nl, nr)
                    li = np.zeros(n, np.int64) if nl == 1 else np.arange(n, dtype=np.int64)
                    ri = np.zeros(n, np.int64) if nr == 1 else np.arange(n, dtype=np.int64)
                else:
                    raise ValueError(f"row-wise {name} of {nl} and {nr} rows: the lengths must match "
                                     "(or one side is a single geometry)")
            else:
                li, ri = pairs
                if _is_torch(li) or _is_torch(ri):
                    import torch

                    li = li.to(torch.int64).contiguous()
                    ri = ri.to(torch.int64).contiguous()
                    self._order(li, ri)
                else:
                    li = np.ascontiguousarray(li, np.int64)
                    ri = np.ascontiguousarray(ri, np.int64)
                if len(li) != len(ri):
                    raise ValueError("pairs: the two index arrays have different lengths")
                n = len(li)
            out = np.zeros(n, dtype)
            status = np.zeros(n, np.int32)
            N.check(entry(self.handle, lt.handle, rt.handle, N.ptr(li), N.ptr(ri), n, N.ptr(out), N.ptr(status)))
        finally:
            for t in own:
                t.close()
        if return_status:
            return out, status
        path = np.flatnonzero(status == N.ROW_PATH)
        if len(path):
            raise RowPathRequired(path)
        return out

    def st_intersects(self, left, right, pairs=None, return_status=False):
        """st_intersects(left, right) (functions/MosaicContext.scala ST_Intersects ->
        expressions/geometry/ST_Intersects.scala -> core/geometry/MosaicGeometryJTS.intersects -> JTS
        1.19 Geometry.intersects; python/mosaic/api/predicates.py) on this context's GPU
        (mosaic_st_intersects): the two closed point sets share a point -- two facets meet
        (RobustLineIntersector on CGAlgorithmsDD orientation signs), or a polygon part of one side holds
        a component of the other (a line holds nothing, closed or not); the value of the sequential
        definition in mosaic_amd/csrc/st_intersects.h.  An empty geometry intersects nothing (where
        ``st_distance`` gives 0.0).  Point, MultiPoint, LineString, MultiLineString, Polygon and
        MultiPolygon rows are served on either side.  It is the flat side of the reference's check of
        ``st_intersects_aggregate`` (ST_IntersectsBehaviors.scala:45-68).

        Arguments as for ``st_distance``: ``GeometryTable``s or anything ``geometry_table`` accepts;
        ``pairs=None`` is row-wise, with a single geometry on one side broadcast;
        ``pairs=(left_idx, right_idx)`` on the host or the device.  Returns a bool array, False on null
        rows.  Rows either side leaves to the row path raise ``RowPathRequired`` with the pair
        indices, unless return_status, which adds the pairs' status array (False on those pairs too)."""
        res = self._pair_call("st_intersects", N.lib().mosaic_st_intersects, np.uint8, left, right, pairs, return_status)
        return (res[0].astype(bool), res[1]) if return_status else res.astype(bool)

    def st_contains_geoms(self, left, right, pairs=None, return_status=False):
        """st_contains(left, right) over any two geometries (expressions/geometry/ST_Contains.scala ->
        core/geometry/MosaicGeometryJTS.contains -> JTS 1.19 Geometry.contains, DE-9IM T*****FF*) on this
        context's GPU (mosaic_st_contains_geoms): no point of the right geometry lies in the exterior of
        the left one, and the interiors share a point -- value and status of the sequential definition
        in mosaic_amd/csrc/st_contains.h, which decides on exact predicates only.  Point, MultiPoint,
        LineString, MultiLineString, Polygon and MultiPolygon rows are served on either side.
        ``st_contains(geoms, points)`` is the older form for polygons from WKB against point columns.

        Arguments as for ``st_intersects``.  Returns a bool array, False on null rows.  A pair the
        engine does not decide has the status ``PAIR_UNDECIDED`` (the boundaries touch without
        crossing and no vertex is outside, or the left side is not polygonal and the right side is
        not points only): both rows are served, but this pair goes to the reference's row-wise
        expression.  Such pairs, and rows either side leaves to the row path, raise
        ``RowPathRequired`` with the pair indices, unless return_status, which adds the pairs' status
        array (ROW_OK / ROW_NULL / ROW_PATH / PAIR_UNDECIDED; False wherever it is not ROW_OK)."""
        out, status = self._pair_call("st_contains", N.lib().mosaic_st_contains_geoms, np.uint8, left, right, pairs, True)
        if return_status:
            return out.astype(bool), status
        rest = np.flatnonzero((status == N.ROW_PATH) | (status == N.PAIR_UNDECIDED))
        if len(rest):
            raise RowPathRequired(rest)
        return out.astype(bool)

    def st_within_geoms(self, left, right, pairs=None, return_status=False):
        """st_within(left, right) = st_contains(right, left) (JTS Geometry.within): ``st_contains_geoms``
        with the sides swapped; ``pairs=(left_idx, right_idx)`` name (left row, right row) as given."""
        return self.st_contains_geoms(right, left, None if pairs is None else (pairs[1], pairs[0]), return_status)

    # ---- one geometry per row: area, length, centroid, numpoints, bounds ----
    MEASURES = ("area", "length", "centroid", "numpoints", "xmin", "ymin", "xmax", "ymax")

    @classmethod
    def _measure_names(cls, what):
        """``what`` as a tuple of distinct names of MEASURES ("perimeter" is "length"); ValueError otherwise"""
        if isinstance(what, str):
            what = (what,)
        names = []
        for w in what:
            if not isinstance(w, str):
                raise ValueError(f"st_measures: what holds {w!r}, not a name")
            w = "length" if w == "perimeter" else w
            if w not in cls.MEASURES:
                raise ValueError(f"st_measures: unknown measure {w!r} (one of {', '.join(cls.MEASURES)}, perimeter)")
            if w not in names:
                names.append(w)
        if not names:
            raise ValueError("st_measures: what is empty")
        return tuple(names)

    def st_measures(self, geoms, what=MEASURES, rows=None, return_status=False, lines=False):
        """Several measures of one geometry per row in one call (mosaic_st_measures): ``what`` names
        any of "area", "length" (or "perimeter"), "centroid", "numpoints", "xmin", "ymin", "xmax",
        "ymax"; only those are computed.  Returns a dict from the name to a float64 array (int64 for
        numpoints; "centroid": the pair ``(x, y)``) -- the bits of the sequential definition in
        mosaic_amd/csrc/st_measures.h (JTS 1.19 getArea / getLength / getCentroid / getNumPoints and
        the envelope).  An empty geometry has area 0.0, length 0.0, numpoints 0 and NaN centroid and
        bounds; null rows give NaN (numpoints 0).

        ``geoms``: a ``GeometryTable``, or anything ``geometry_table`` accepts (the table is then
        built with ``lines`` and closed inside the call).  LineString / MultiLineString rows are served
        by a LineSet or a table built with ``lines=True``, as for ``st_distance``.  ``rows``: the rows
        to measure, in that order (host array or device tensor); None = every row.  Rows left to the
        row path raise ``RowPathRequired`` unless return_status, which adds the "status" array
        (ROW_OK / ROW_NULL / ROW_PATH; NaN on row-path rows too)."""
        names = self._measure_names(what)
        own = None
        try:
            table = geoms
            if not isinstance(geoms, GeometryTable):
                table = own = self.geometry_table(geoms, lines=lines)
            if rows is None:
                n = len(table)
            else:
                if _is_torch(rows):
                    import torch

                    rows = rows.to(torch.int64).contiguous()
                    self._order(rows)
                else:
                    rows = np.ascontiguousarray(rows, np.int64)
                n = len(rows)
            size = max(n, 1)
            bufs = {w: np.zeros(size) for w in names if w not in ("centroid", "numpoints")}
            if "centroid" in names:
                bufs["cx"], bufs["cy"] = np.zeros(size), np.zeros(size)
            if "numpoints" in names:
                bufs["numpoints"] = np.zeros(size, np.int64)
            status = np.zeros(size, np.int32)
            order = ("area", "length", "cx", "cy", "numpoints", "xmin", "ymin", "xmax", "ymax")
            N.check(N.lib().mosaic_st_measures(self.handle, table.handle, N.ptr(rows), n, *[N.ptr(bufs.get(k)) for k in order],
                                               N.ptr(status)))
        finally:
            if own is not None:
                own.close()
        status = status[:n]
        out = {w: (bufs["cx"][:n], bufs["cy"][:n]) if w == "centroid" else bufs[w][:n] for w in names}
        if return_status:
            out["status"] = status
            return out
        path = np.flatnonzero(status == N.ROW_PATH)
        if len(path):
            raise RowPathRequired(path)
        return out

    def _measure(self, name, geoms, return_status, lines):
        out = self.st_measures(geoms, (name,), return_status=return_status, lines=lines)
        return (out[name], out["status"]) if return_status else out[name]

    def st_area(self, geoms, return_status=False, lines=False):
        """st_area(geom) (ST_Area.scala -> MosaicGeometryJTS.getArea -> JTS Geometry.getArea): per
        polygon part |shell| minus its |holes| by Area.ofRingSigned, summed over the parts; 0.0 for
        lines, points and empty geometries.  Arguments and row handling as for ``st_measures``."""
        return self._measure("area", geoms, return_status, lines)

    def st_length(self, geoms, return_status=False, lines=False):
        """st_length(geom) (ST_Length.scala -> JTS Geometry.getLength): the length of every component
        line and of every polygon ring, holes included (the perimeter); 0.0 for points."""
        return self._measure("length", geoms, return_status, lines)

    def st_perimeter(self, geoms, return_status=False, lines=False):
        """st_perimeter(geom): the reference registers ST_Length under this name too (MosaicContext.scala:488)."""
        return self._measure("length", geoms, return_status, lines)

    def st_centroid(self, geoms, return_status=False, lines=False):
        """st_centroid(geom) / st_centroid2D (ST_Centroid.scala -> JTS Geometry.getCentroid) as ``(x, y)``:
        JTS Centroid's area part; without area its line part; without length the mean of the points;
        (NaN, NaN) for an empty geometry."""
        return self._measure("centroid", geoms, return_status, lines)

    def st_numpoints(self, geoms, return_status=False, lines=False):
        """st_numpoints(geom) (JTS Geometry.getNumPoints): a closed ring counts its closing vertex."""
        return self._measure("numpoints", geoms, return_status, lines)

    def st_xmin(self, geoms, return_status=False, lines=False):
        """st_xmin(geom): the envelope's smallest x; NaN for an empty geometry (the reference throws)."""
        return self._measure("xmin", geoms, return_status, lines)

    def st_xmax(self, geoms, return_status=False, lines=False):
        """st_xmax(geom); see ``st_xmin``."""
        return self._measure("xmax", geoms, return_status, lines)

    def st_ymin(self, geoms, return_status=False, lines=False):
        """st_ymin(geom); see ``st_xmin``."""
        return self._measure("ymin", geoms, return_status, lines)

    def st_ymax(self, geoms, return_status=False, lines=False):
        """st_ymax(geom); see ``st_xmin``."""
        return self._measure("ymax", geoms, return_status, lines)

    def st_measures_last_split(self):
        """(rows served by one lane, rows served by a wave) of this thread's last ``st_measures``"""
        a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        N.check(N.lib().mosaic_st_measures_last_split(ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- the KNN model (mosaic_amd/knn.py) ----
    def cell_index(self, chips):
        """A ``CellIndex``: the candidates' chips as a device-resident map from a cell to its candidate
        rows, built once and probed by every ``grid_ring_neighbours`` call (see ``knn.CellIndex``)."""
        from .knn import CellIndex

        return CellIndex(self, chips)

    def grid_ring_neighbours(self, landmarks, candidates, cell_index, rows, cells, keep_self=False):
        """One iteration of the reference's KNN model (models/knn/GridRingNeighbours.scala:121-160):
        ``(landmark_row, candidate_row, distance, unmatched)``; see ``knn.grid_ring_neighbours``."""
        from .knn import grid_ring_neighbours

        return grid_ring_neighbours(self, landmarks, candidates, cell_index, rows, cells, keep_self)

    def st_dwithin_join(self, left, right, radius, rows=None, keep_self=True):
        """The distance-within join: ``(left_row, right_row, distance)`` of all pairs with
        ``st_distance(left[l], right[c]) <= radius`` -- one radius for all rows or one per requested row,
        ``rows`` the left rows asked for (strictly ascending; None: all) -- ordered by (left row,
        distance, right row).  With radius 0 it is the pair list of the geometries that touch or
        overlap.  See ``knn.within_neighbours``."""
        from .knn import within_neighbours

        return within_neighbours(self, left, right, radius, rows, keep_self)

    def st_dwithin_candidates(self, left, right, radius, rows=None):
        """Per requested row, the number of candidate pairs ``st_dwithin_join``'s envelope filter finds
        (int64, at least the row's pairs): what a caller sizes its calls by.  See
        ``knn.within_candidates``."""
        from .knn import within_candidates

        return within_candidates(self, left, right, radius, rows)

    # ---- the chip join ----
    def grid_tessellateexplode(self, polygons, resolution, keep_core_geom=True, densify=1, cells_only=False):
        """grid_tessellateexplode(geom, res, keepCoreGeom) (MosaicContext.scala functions ->
        MosaicExplode.scala:70-79 -> Mosaic.getChips core/Mosaic.scala:21-87) over a PolygonSet:
        chip columns (is_core, index_id, polygon_key, wkb) with the cell classification on this
        context's GPU (mosaic_tessellate_gpu).

        H3 geometries spanning icosahedron faces are cut into per-face pieces; only a
        geometry with a vertex more than ~78 degrees from the centre of a face it meets (no gnomonic
        face plane holds it) raises MosaicError (MOSAIC_E_ARG).

        A LineSet (LineString / MultiLineString rows) takes Mosaic.lineFill on this context's GPU
        (mosaic_tessellate_lines_gpu): LINESTRING / MULTILINESTRING chips of the pieces of each
        component line inside a cell, POINT / MULTIPOINT chips where it only touches one; a line that
        comes to a cell over the antimeridian or a pole raises MosaicError (MOSAIC_E_ARG)."""
        return tessellate(self.index_system, polygons, resolution, keep_core_geom, densify, ctx=self, cells_only=cells_only)

    def chip_table(self, is_core, index_id, wkb_list, polygon_key, resolution, n_polygons=None):
        """Build side: rows of grid_tessellateexplode output (MosaicExplode.scala:70-79)."""
        self.resolution_of_table = self.index_system.get_resolution(resolution)
        return ChipTable(self, is_core, index_id, wkb_list, polygon_key, n_polygons)

    def line_chip_table(self, is_core, index_id, wkb_list, key, resolution):
        """The line side of st_intersects_aggregate: rows of grid_tessellateexplode over a LineSet."""
        return LineChipTable(self, is_core, index_id, wkb_list, key, resolution)

    def chip_table_arrays(self, chip_offsets, is_core, index_id, wkb_list, resolution):
        """Build side from grid_tessellate chip arrays, one array per polygon row (the array form of
        PointInPolygonJoin, sql/join/PointInPolygonJoin.scala:39-66); see ChipTable.from_arrays."""
        self.resolution_of_table = self.index_system.get_resolution(resolution)
        return ChipTable.from_arrays(self, chip_offsets, is_core, index_id, wkb_list)

    def pip_join_count(self, chips, x, y, out=None):
        """Quickstart join + filter + groupBy(polygon).count(): int64 count per polygon key.
        ``out`` (optional, >= n_polygons int64, host or device) receives the counts."""
        x, y = _f64(x), _f64(y)
        n = int(x.shape[0])
        if out is not None:
            counts = out
        elif _is_torch(x):
            import torch

            counts = torch.zeros(max(chips.n_polygons, 1), dtype=torch.int64, device=x.device)
        else:
            counts = np.zeros(max(chips.n_polygons, 1), np.int64)
        # after the allocation: torch fills `counts` on its own stream, and that fill has to be ordered
        # before the join like the inputs (a late fill would clear what the join counted)
        self._order(x, y, counts)
        N.check(N.lib().mosaic_pip_join_count(self.handle, chips.handle, N.ptr(x), N.ptr(y), n, N.ptr(counts)))
        return counts[:chips.n_polygons]

    def pip_join_pairs(self, chips, x, y, capacity=None):
        """Quickstart join + filter: (row, polygon_key) pairs sorted by (row, key)."""
        x, y = _f64(x), _f64(y)
        self._order(x, y)
        n = int(x.shape[0])
        cap = capacity if capacity is not None else max(2 * n, 1024)
        while True:
            rows = np.empty(max(cap, 1), np.int64)
            keys = np.empty(max(cap, 1), np.int32)
            n_out = ctypes.c_int64(0)
            rc = N.lib().mosaic_pip_join_pairs(self.handle, chips.handle, N.ptr(x), N.ptr(y), n, N.ptr(rows),
                                               N.ptr(keys), cap, ctypes.byref(n_out))
            if rc == N.MOSAIC_E_CAPACITY:
                cap = int(n_out.value)
                continue
            N.check(rc)
            k = int(n_out.value)
            order = np.lexsort((keys[:k], rows[:k]))
            return rows[:k][order], keys[:k][order]


    def _kring(self, cells, k, loop, raw):
        strings = len(cells) and isinstance(cells[0], str)
        ids = np.array([self.index_system.parse(c) for c in cells] if strings else cells, np.int64)
        valid = None
        n = len(ids)
        if self.index_system.grid == N.GRID_H3:
            stride = max(6 * k, 1) if loop else 1 + 3 * k * (k + 1)
        else:
            stride = 8 * k if loop else 1 + 4 * k * (k + 1)
        out = np.zeros(max(n * stride, 1), np.int64)
        cnt = np.zeros(max(n, 1), np.int32)
        N.check(N.lib().mosaic_cell_kring(self.handle, self.index_system.grid, N.ptr(ids), valid, n, int(k),
                                          int(loop), N.ptr(out), N.ptr(cnt)))
        bad = np.nonzero(cnt[:n] == -2)[0]
        if len(bad):
            raise N.MosaicError(
                N.MOSAIC_E_ARG, f"grid_cellkring / grid_cellkloop: row {int(bad[0])} (cell {int(ids[bad[0]])}) is not a valid "
                "H3 cell id")
        rows = [out[i * stride:i * stride + cnt[i]] for i in range(n)]
        if raw or self.index_system.cell_id_type != "string":
            return rows
        return [[self.index_system.format(c) for c in r] for r in rows]

    def grid_cellkring(self, cells, k, raw=False):
        """grid_cellkring(cellId, k) (MosaicContext.scala:692-693 -> CellKRing.nullSafeEval ->
        IndexSystem.kRing; BNG: BNGIndexSystem.scala:216-222, the cell and its loops 1..k; H3:
        H3IndexSystem.scala:154-160, h3.kRing: hexRange order, or H3's hash-table order where the ring
        meets a pentagon)."""
        return self._kring(cells, k, False, raw)

    def grid_cellkloop(self, cells, k, raw=False):
        """grid_cellkloop(cellId, k) (MosaicContext.scala:696-697 -> CellKLoop -> IndexSystem.kLoop;
        BNG: BNGIndexSystem.scala:234-246, the valid cells at distance k; H3: H3IndexSystem.scala:
        171-177, h3.hexRing order, or the reference's kRing set-difference fallback (Scala HashSet
        order) where the ring meets a pentagon)."""
        return self._kring(cells, k, True, raw)

    def grid_cellkringexplode(self, cells, k):
        """grid_cellkringexplode (MosaicContext.scala:694-695, CellKRingExplode): one output row per
        (input row, ring cell) -- (row index array, cell array), in the reference's order."""
        return self._explode(self.grid_cellkring(cells, k, raw=True))

    def grid_cellkloopexplode(self, cells, k):
        """grid_cellkloopexplode (CellKLoopExplode): one output row per (input row, loop cell)."""
        return self._explode(self.grid_cellkloop(cells, k, raw=True))

    def _explode(self, rows):
        lens = np.array([len(r) for r in rows], np.int64)
        idx = np.repeat(np.arange(len(rows), dtype=np.int64), lens)
        cells = np.concatenate(rows) if len(rows) else np.zeros(0, np.int64)
        if self.index_system.cell_id_type == "string":
            return idx, self._serialize(cells)
        return idx, cells

    def _geometry_kring(self, geoms, resolution, k, loop, raw, return_distance=False, return_status=False):
        res = self.index_system.get_resolution(resolution)
        grid = self.index_system.grid
        h = ctypes.c_void_p()
        if hasattr(geoms, "geom_parts"):  # a PolygonSet
            N.check(N.lib().mosaic_geometry_kring(self.handle, grid, res, len(geoms), N.ptr(geoms.geom_parts),
                                                  N.ptr(geoms.part_rings), N.ptr(geoms.ring_offsets),
                                                  N.ptr(geoms.xy), int(k), int(loop), ctypes.byref(h)))
        else:
            if hasattr(geoms, "geom_lines"):  # a LineSet: its line chips' cells, all border chips
                chips = tessellate(self.index_system, geoms, resolution, ctx=self, cells_only=True)
                geoms = dict(is_core=chips["is_core"], index_id=chips["index_id"], polygon_key=chips["polygon_key"],
                             n_geoms=len(geoms))
            if isinstance(geoms, dict):  # chip columns
                is_core = np.ascontiguousarray(geoms["is_core"], np.uint8)
                ids = np.ascontiguousarray(geoms["index_id"], np.int64)
                key = np.ascontiguousarray(geoms["polygon_key"], np.int32)
                n_geoms = geoms.get("n_geoms")
                if n_geoms is None:
                    n_geoms = int(key.max()) + 1 if len(key) else 0
            else:  # a point column: Mosaic.pointChip, one non-core chip at each point's cell
                ids = self.grid_pointascellid(geoms, res, raw=True)
                if _is_torch(ids):
                    ids = ids.cpu().numpy()
                ids = np.ascontiguousarray(ids, np.int64)
                is_core = np.zeros(len(ids), np.uint8)
                key = np.arange(len(ids), dtype=np.int32)
                n_geoms = len(ids)
            N.check(N.lib().mosaic_chips_kring(self.handle, grid, res, len(ids), N.ptr(is_core), N.ptr(ids),
                                               N.ptr(key), int(n_geoms), int(k), int(loop), ctypes.byref(h)))
        try:
            n_rows, n_cells = ctypes.c_int64(0), ctypes.c_int64(0)
            N.check(N.lib().mosaic_cell_lists_info(h, ctypes.byref(n_rows), ctypes.byref(n_cells)))
            n = n_rows.value
            offs = np.zeros(n + 1, np.int64)
            cells = np.zeros(max(n_cells.value, 1), np.int64)
            dist = np.zeros(max(n_cells.value, 1), np.int32)
            status = np.zeros(max(n, 1), np.int32)
            N.check(N.lib().mosaic_cell_lists_export(h, N.ptr(offs), N.ptr(cells), N.ptr(status)))
            N.check(N.lib().mosaic_cell_lists_export_dist(h, N.ptr(dist)))
        finally:
            N.lib().mosaic_cell_lists_destroy(h)
        status = status[:n]
        bad = np.nonzero(status != 0)[0]
        if len(bad) and not return_status:
            raise N.MosaicError(N.MOSAIC_E_ARG, f"grid_geometrykring / grid_geometrykloop: rows {bad[:8].tolist()} hold a "
                                                f"chip id that is not a valid cell of resolution {res}")
        rows = [cells[offs[g]:offs[g + 1]].copy() for g in range(n)]
        if not raw and self.index_system.cell_id_type == "string":
            rows = [list(self._serialize(r)) if len(r) else [] for r in rows]
        out = (rows,)
        if return_distance:
            out += ([dist[offs[g]:offs[g + 1]].copy() for g in range(n)],)
        if return_status:
            out += (status,)
        return out[0] if len(out) == 1 else out

    def grid_geometrykring(self, geoms, resolution, k, raw=False, return_distance=False, return_status=False):
        """grid_geometrykring(geom, res, k) (python/mosaic/api/functions.py:1184-1207 ->
        expressions/index/GeometryKRing.scala -> Mosaic.geometryKRing, core/Mosaic.scala:111-116): per
        geometry, the core cells of its tessellation and the k-rings of its border cells, 0 <= k <=
        1000, found on this context's GPU as one multi-source search from the border cells
        (mosaic_geometry_kring / mosaic_chips_kring).

        ``geoms``: a PolygonSet; the chip columns ``tessellate`` / ``grid_tessellateexplode`` return
        (a dict, optionally with ``n_geoms``; MultiPoint rows are chips sharing a key, one non-core
        chip per point); or a point column in any form ``grid_pointascellid`` accepts (each row's cell
        is one border chip, Mosaic.pointChip); or a LineSet, whose line chips (Mosaic.lineFill on the
        GPU, cells only) are all border chips.  A line row inside a point column still raises
        RowPathRequired.

        Returns one array of cells per geometry -- BNG ids as the reference's strings unless raw --
        in Scala 2.12 immutable HashSet iteration order (the reference returns a Set[Long]; equal
        hashes by ascending id).  Sets of <= 4 cells iterate in insertion order in Scala, which is
        not restated, and no reference fixture pins these orders ("order unpinned").
        return_distance adds, per cell, the smallest loop distance from a border cell (-1: a core
        cell not reached within k).  A row with a chip id that is not a valid cell of the resolution
        raises MosaicError, unless return_status, which adds the rows' status array (0 ok, -2 such a
        row, left empty)."""
        return self._geometry_kring(geoms, resolution, k, False, raw, return_distance, return_status)

    def grid_geometrykloop(self, geoms, resolution, k, raw=False, return_status=False):
        """grid_geometrykloop(geom, res, k) (python/mosaic/api/functions.py:1209-1232 ->
        expressions/index/GeometryKLoop.scala -> Mosaic.geometryKLoop, core/Mosaic.scala:130-144): the
        cells at loop distance exactly k (1 <= k <= 1000) from the geometry's border cells that are
        neither core cells nor in the (k - 1)-ring.  Arguments, order and errors as
        grid_geometrykring; the same search gives every loop 1..k, which is what the KNN iteration
        (models/knn/GridRingNeighbours.scala:76-99) asks for."""
        return self._geometry_kring(geoms, resolution, k, True, raw, False, return_status)

    def grid_geometrykringexplode(self, geoms, resolution, k):
        """grid_geometrykringexplode (python/mosaic/api/functions.py:1234-1257,
        expressions/index/GeometryKRingExplode.scala): one output row per (geometry, ring cell) --
        (row index array, cell array), as grid_cellkringexplode."""
        return self._explode(self.grid_geometrykring(geoms, resolution, k, raw=True))

    def grid_geometrykloopexplode(self, geoms, resolution, k):
        """grid_geometrykloopexplode (python/mosaic/api/functions.py:1259-1281,
        expressions/index/GeometryKLoopExplode.scala): one output row per (geometry, loop cell)."""
        return self._explode(self.grid_geometrykloop(geoms, resolution, k, raw=True))

    def _h3_geometry(self, cells, mode):
        ids = np.ascontiguousarray(cells, np.int64)
        n = len(ids)
        width = (2, 20, 189)[mode]
        out = np.zeros(max(n * width, 1), np.uint8 if mode == 2 else np.float64)
        cnt = np.zeros(max(n, 1), np.int32)
        N.check(N.lib().mosaic_h3_cell_geometry(self.handle, mode, N.ptr(ids), None, n, N.ptr(out), N.ptr(cnt)))
        return out, cnt[:n], width

    def grid_cellcenter(self, cells):
        """H3 h3ToGeo over a cell column (the cell centres polyfill tests, H3IndexSystem.scala:113-126):
        array [n, 2] of (lng, lat) degrees."""
        out, _, _ = self._h3_geometry(cells, 0)
        return out[:2 * len(cells)].reshape(-1, 2)

    def grid_boundary(self, cells):
        """H3IndexSystem.indexToGeometry's vertices (h3.h3ToGeoBoundary, H3IndexSystem.scala:93-100):
        per row an array [k, 2] of (lng, lat) degrees, k = 5..10 (the ring is not closed)."""
        out, cnt, w = self._h3_geometry(cells, 1)
        return [out[w * i:w * i + 2 * cnt[i]].reshape(-1, 2) for i in range(len(cells))]

    def grid_boundaryaswkb(self, cells):
        """grid_boundaryaswkb(cellId) (IndexGeometry.scala:65-75 -> IndexSystem.indexToGeometry ->
        toWKB): per row the cell polygon as JTS big-endian WKB -- BNG: the cell square (93 bytes);
        H3: the h3ToGeoBoundary ring closed with its first vertex."""
        if self.index_system.grid == N.GRID_H3:
            out, cnt, w = self._h3_geometry(cells, 2)
            return [out[w * i:w * i + cnt[i]].tobytes() for i in range(len(cells))]
        strings = len(cells) and isinstance(cells[0], str)
        ids = np.array([self.index_system.parse(c) for c in cells] if strings else cells, np.int64)
        out = np.zeros(max(93 * len(ids), 1), np.uint8)
        N.check(N.lib().mosaic_cell_boundary_wkb(self.handle, self.index_system.grid, N.ptr(ids), None, len(ids),
                                                 N.ptr(out)))
        return [out[93 * i:93 * (i + 1)].tobytes() for i in range(len(ids))]

    def grid_polyfill(self, polygons, resolution, raw=False):
        """grid_polyfill(geometry, res) (expressions/index/Polyfill.scala nullSafeEval ->
        IndexSystem.polyfill: H3IndexSystem.scala:113-126, BNGIndexSystem.scala:185-204) over a
        PolygonSet, on this context's GPU (mosaic_polyfill).  Returns one list per geometry: int64
        cells (H3), or BNG ids formatted as the reference's StringType ids unless raw=True.  A row the
        engine does not answer (an H3 search meeting a pentagon, a non-finite vertex, a BNG geometry
        without area) raises MosaicError."""
        res = self.index_system.get_resolution(resolution)
        h = ctypes.c_void_p()
        N.check(N.lib().mosaic_polyfill(self.handle, self.index_system.grid, res, len(polygons),
                                        N.ptr(polygons.geom_parts), N.ptr(polygons.part_rings),
                                        N.ptr(polygons.ring_offsets), N.ptr(polygons.xy), ctypes.byref(h)))
        try:
            n_rows, n_cells = ctypes.c_int64(0), ctypes.c_int64(0)
            N.check(N.lib().mosaic_cell_lists_info(h, ctypes.byref(n_rows), ctypes.byref(n_cells)))
            offs = np.zeros(n_rows.value + 1, np.int64)
            cells = np.zeros(max(n_cells.value, 1), np.int64)
            status = np.zeros(max(n_rows.value, 1), np.int32)
            N.check(N.lib().mosaic_cell_lists_export(h, N.ptr(offs), N.ptr(cells), N.ptr(status)))
        finally:
            N.lib().mosaic_cell_lists_destroy(h)
        bad = np.nonzero(status[:n_rows.value] != 0)[0]
        if len(bad):
            raise N.MosaicError(N.MOSAIC_E_ARG, f"grid_polyfill: rows {bad[:8].tolist()} are not supported by this "
                                                "engine (H3 search meeting a pentagon, non-finite vertex, or a "
                                                "BNG geometry without area)")
        out = [cells[offs[g]:offs[g + 1]].copy() for g in range(n_rows.value)]
        if raw or self.index_system.grid == N.GRID_H3:
            return out
        return [list(self._serialize(c)) for c in out]

    def buffer_radius(self, polygons, resolution):
        """IndexSystem.getBufferRadius(geometry, res) per geometry of a PolygonSet (the radius
        Mosaic.mosaicFill buffers by, core/Mosaic.scala:68; H3IndexSystem.scala:73-80,
        BNGIndexSystem.scala:146-149), computed on this context's GPU (H3).  float64[n]."""
        res = self.index_system.get_resolution(resolution)
        out = np.zeros(max(len(polygons), 1), np.float64)
        N.check(N.lib().mosaic_buffer_radius(self.handle, self.index_system.grid, res, len(polygons),
                                             N.ptr(polygons.geom_parts), N.ptr(polygons.part_rings),
                                             N.ptr(polygons.ring_offsets), N.ptr(polygons.xy), N.ptr(out)))
        return out[:len(polygons)]

    def st_intersects_aggregate(self, left, right):
        """left.join(right, left_index.index_id == right_index.index_id).groupBy(left_key, right_key)
        .agg(st_intersects_aggregate(left_index, right_index)) over two chip tables
        (ST_IntersectsAggregate.scala:28-39, ST_IntersectsBehaviors.scala:34-47): arrays
        (left_key int32, right_key int32, flag bool) sorted by (left_key, right_key), one row per key
        pair that shares a cell id.

        One side may be a LineChipTable (the chips of grid_tessellateexplode over a LineSet): "which
        trips cross which zones" (mosaic_line_intersects_aggregate).  With the line table on the right
        the columns come back swapped and sorted by (left key, right key) all the same.  Two line
        tables raise ValueError."""
        lines = (isinstance(left, LineChipTable), isinstance(right, LineChipTable))
        if all(lines):
            raise ValueError("st_intersects_aggregate: a line x line join is not served")
        if lines[1]:
            rk, lk, fl = self.st_intersects_aggregate(right, left)
            order = np.lexsort((rk, lk))
            return lk[order], rk[order], fl[order]
        fn = N.lib().mosaic_line_intersects_aggregate if lines[0] else N.lib().mosaic_intersects_aggregate
        cap = 1024
        while True:
            lk = np.empty(cap, np.int32)
            rk = np.empty(cap, np.int32)
            fl = np.empty(cap, np.uint8)
            n_out = ctypes.c_int64(0)
            rc = fn(self.handle, left.handle, right.handle, N.ptr(lk), N.ptr(rk), N.ptr(fl), cap, ctypes.byref(n_out))
            if rc == N.MOSAIC_E_CAPACITY and n_out.value > cap:
                cap = int(n_out.value)
                continue
            N.check(rc)
            k = int(n_out.value)
            return lk[:k], rk[:k], fl[:k].astype(bool)

    def st_intersection_aggregate(self, left, right):
        """st_intersection_aggregate(left_index, right_index) grouped by (left_key, right_key) over the
        chip join (MosaicContext st_intersection_aggregate -> ST_IntersectionAggregate.scala:40-72):
        (left_key int32, right_key int32, area float64, status uint8, wkb list of bytes) sorted by key
        pair.  The WKB is the union's polygonal part as JTS writes it (big-endian; POLYGON EMPTY when
        the pieces have no area); status 1 = not answered (wkb None, area NaN): the row path.

        One side may be a LineChipTable: "how much of each trip lies in each zone"
        (mosaic_line_intersection_aggregate_geometry).  The same 5-tuple with the length of the line
        inside the polygon in place of the area, the pieces as LINESTRING / MULTILINESTRING (LINESTRING
        EMPTY for none) and status 0 throughout.  With the line table on the right the key columns
        come back swapped and sorted by (left key, right key) all the same.  Two line tables raise
        ValueError."""
        lines = (isinstance(left, LineChipTable), isinstance(right, LineChipTable))
        if all(lines):
            raise ValueError("st_intersection_aggregate: a line x line join is not served")
        if lines[1]:
            rk, lk, ln, st, wkb = self.st_intersection_aggregate(right, left)
            order = np.lexsort((rk, lk))
            return lk[order], rk[order], ln[order], st[order], [wkb[i] for i in order]
        fn = N.lib().mosaic_line_intersection_aggregate_geometry if lines[0] else N.lib().mosaic_intersection_aggregate_geometry
        h = ctypes.c_void_p()
        N.check(fn(self.handle, left.handle, right.handle, ctypes.byref(h)))
        return _export_isect_geoms(h)

    def st_intersection_aggregate_length(self, left, right):
        """st_length(st_intersection_aggregate(left_index, right_index)) per (left_key, right_key) group
        of the join of a LineChipTable with a ChipTable (mosaic_line_intersection_aggregate): arrays
        (left_key int32, right_key int32, length float64) sorted by key pair; the length column of
        st_intersection_aggregate bit for bit, without the geometry.  With the line table on the right
        the key columns come back swapped and sorted all the same."""
        lines = (isinstance(left, LineChipTable), isinstance(right, LineChipTable))
        if all(lines):
            raise ValueError("st_intersection_aggregate_length: a line x line join is not served")
        if not any(lines):
            raise ValueError("st_intersection_aggregate_length: one side has to be a LineChipTable; two polygon "
                             "tables have an area: st_intersection_aggregate_area")
        if lines[1]:
            rk, lk, ln = self.st_intersection_aggregate_length(right, left)
            order = np.lexsort((rk, lk))
            return lk[order], rk[order], ln[order]
        cap = 1 << 16  # (a call that finds more groups reports the count and is repeated once)
        while True:
            lk = np.empty(cap, np.int32)
            rk = np.empty(cap, np.int32)
            ln = np.empty(cap, np.float64)
            n_out = ctypes.c_int64(0)
            rc = N.lib().mosaic_line_intersection_aggregate(self.handle, left.handle, right.handle, N.ptr(lk), N.ptr(rk),
                                                            N.ptr(ln), cap, ctypes.byref(n_out))
            if rc == N.MOSAIC_E_CAPACITY and n_out.value > cap:
                cap = int(n_out.value)
                continue
            N.check(rc)
            k = int(n_out.value)
            return lk[:k], rk[:k], ln[:k]

    def st_intersection_aggregate_area(self, left, right):
        """st_area(st_intersection_aggregate(left_index, right_index)) per (left_key, right_key) group of
        the chip join (ST_IntersectionAggregate.scala; the quantity ST_IntersectionBehaviors.scala:22-135
        checks): arrays (left_key, right_key, area float64, status uint8) sorted by key pair; status 1
        marks groups the engine does not answer (a core chip without geometry, an overlay capacity
        exceeded)."""
        if isinstance(left, LineChipTable) or isinstance(right, LineChipTable):
            raise ValueError("st_intersection_aggregate_area: a line has no area; st_intersection_aggregate_length "
                             "serves a LineChipTable")
        cap = 1 << 16  # (a call that finds more groups reports the count and is repeated once)
        while True:
            lk = np.empty(cap, np.int32)
            rk = np.empty(cap, np.int32)
            ar = np.empty(cap, np.float64)
            st = np.empty(cap, np.uint8)
            n_out = ctypes.c_int64(0)
            rc = N.lib().mosaic_intersection_aggregate(self.handle, left.handle, right.handle, N.ptr(lk), N.ptr(rk),
                                                       N.ptr(ar), N.ptr(st), cap, ctypes.byref(n_out))
            if rc == N.MOSAIC_E_CAPACITY and n_out.value > cap:
                cap = int(n_out.value)
                continue
            N.check(rc)
            k = int(n_out.value)
            return lk[:k], rk[:k], ar[:k], st[:k]


def tessellate(index_system, polygons, resolution, keep_core_geom=True, densify=1, ctx=None, cells_only=False):
    """grid_tessellateexplode over a PolygonSet or a LineSet (mosaic_amd.data).

    ctx=None: the host producer (mosaic_tessellate).  ctx=MosaicContext: the cell classification
    runs on the context's GPU (mosaic_tessellate_gpu), same chip set row for row.
    A LineSet takes Mosaic.lineFill (mosaic_tessellate_lines / mosaic_tessellate_lines_gpu): one
    non-core chip per (component line, cell the line meets), rows in line order; keep_core_geom and
    densify do not apply, and cells_only=True leaves the wkb column empty.

    Returns chip columns: dict(is_core uint8, index_id int64, polygon_key int32 (geometry index),
    wkb=(offsets int64[n+1], data uint8[...])).  MosaicExplode.scala:70-79 / Mosaic.scala:21-87.
    """
    if isinstance(index_system, str):
        index_system = INDEX_SYSTEMS[index_system]()
    res = index_system.get_resolution(resolution)
    h = ctypes.c_void_p()
    if hasattr(polygons, "geom_lines"):  # a LineSet: Mosaic.lineFill (keep_core_geom does not exist there)
        args = (index_system.grid, res, len(polygons), N.ptr(polygons.geom_lines), N.ptr(polygons.line_offsets),
                N.ptr(polygons.xy), int(bool(cells_only)), ctypes.byref(h))
        if ctx is not None:
            N.check(N.lib().mosaic_tessellate_lines_gpu(ctx.handle, *args))
        else:
            N.check(N.lib().mosaic_tessellate_lines(*args))
    elif ctx is not None:
        N.check(N.lib().mosaic_tessellate_gpu(ctx.handle, index_system.grid, res, len(polygons),
                                              N.ptr(polygons.geom_parts), N.ptr(polygons.part_rings),
                                              N.ptr(polygons.ring_offsets), N.ptr(polygons.xy),
                                              int(bool(keep_core_geom)), int(densify), ctypes.byref(h)))
    else:
        N.check(N.lib().mosaic_tessellate(index_system.grid, res, len(polygons), N.ptr(polygons.geom_parts),
                                          N.ptr(polygons.part_rings), N.ptr(polygons.ring_offsets),
                                          N.ptr(polygons.xy), int(bool(keep_core_geom)), int(densify),
                                          ctypes.byref(h)))
    # zero-copy: the arrays view the chip set's own columns, which live until the last of them is
    # collected (_ChipSetOwner destroys the set)
    owner = _ChipSetOwner(h)
    n = ctypes.c_int64(0)
    nb = ctypes.c_int64(0)
    N.check(N.lib().mosaic_chip_set_info(h, ctypes.byref(n), ctypes.byref(nb)))
    n, nb = n.value, nb.value
    p = [ctypes.c_void_p() for _ in range(5)]
    N.check(N.lib().mosaic_chip_set_columns(h, *[ctypes.byref(q) for q in p]))
    is_core = owner.view(p[0], n, ctypes.c_uint8, np.uint8)
    index_id = owner.view(p[1], n, ctypes.c_int64, np.int64)
    key = owner.view(p[2], n, ctypes.c_int32, np.int32)
    offs = owner.view(p[3], n + 1, ctypes.c_int64, np.int64)
    data = owner.view(p[4], nb, ctypes.c_uint8, np.uint8) if nb else np.zeros(1, np.uint8)
    return dict(is_core=is_core, index_id=index_id, polygon_key=key, wkb=(offs, data))


def tessellate_counters():
    """(border chips clipped by the reference-style planar clip on the host, cells that fell back to
    the face-plane clip): process-wide counters of the chip producers (mosaic_tess_counters)."""
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    N.check(N.lib().mosaic_tess_counters(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


class _ChipSetOwner:
    """Holds a mosaic_chip_set whose columns numpy arrays view; destroyed with the last of them."""

    def __init__(self, h):
        self.h = h

    def view(self, ptr, n, ctype, dtype):
        if n == 0 or not ptr.value:
            return np.zeros(0, dtype)
        buf = (ctype * n).from_address(ptr.value)
        buf._owner = self  # the arrays' base keeps the set alive
        return np.frombuffer(buf, dtype=dtype)

    def __del__(self):
        if self.h:
            N.lib().mosaic_chip_set_destroy(self.h)
            self.h = None
