"""The reference's KNN model on this engine: ``GridRingNeighbours`` (models/knn/GridRingNeighbours.scala)
as one GPU primitive, and ``SpatialKNN`` (models/knn/SpatialKNN.scala, models/core/IterativeTransformer.scala)
in its ``approximate = true`` form on top of it.

One iteration (``grid_ring_neighbours``; mosaic_amd/csrc/ring_neighbours.h defines the rows) joins the
landmarks' ring cells with the candidates' chip cells, keeps one row per (landmark, candidate), drops
self matches, measures st_distance and orders each landmark's candidates by (distance, candidate row).
The iteration's bookkeeping (``knn_iterate`` / ``knn_result``) runs in numpy on the exported rows.

``within_neighbours`` is the distance-within join (all pairs with st_distance <= a per-landmark radius)
as a second GPU primitive, and ``SpatialKNN.transform_exact`` ranks its rows into every landmark's true
k nearest (``knn_exact_radius`` / ``knn_exact_batches`` / ``knn_exact_result``, numpy)."""
import ctypes
import sys

import numpy as np

from . import _native as N
from .context import GeometryTable, _is_torch, tessellate

__all__ = ["CellIndex", "SpatialKNN", "grid_ring_neighbours", "knn_iterate", "knn_result", "within_candidates",
           "within_neighbours", "knn_exact_radius", "knn_exact_batches", "knn_exact_result"]


class CellIndex:
    """The candidates' chips as a device-resident map from a cell to its candidate rows
    (mosaic_cell_index): built once per chip set, immutable afterwards, usable from any thread.
    ``chips``: the chip columns ``tessellate`` / ``grid_tessellateexplode`` return (a dict with
    ``index_id`` and ``polygon_key``), a ``(cells, candidate rows)`` pair, or one array of cells -- one
    chip per point row (Mosaic.pointChip).  Cells are raw int64 ids.  The chips are host arrays: a
    device tensor is copied to the host first (the index is built once, from the few chips of a
    tessellation).  Built by ``MosaicContext.cell_index``; ``close()`` frees the device memory."""

    def __init__(self, ctx, chips):
        self.ctx = ctx
        if isinstance(chips, dict):
            cells, keys = chips["index_id"], chips["polygon_key"]
        elif isinstance(chips, tuple) and len(chips) == 2:
            cells, keys = chips
        else:
            cells, keys = chips, None
        if _is_torch(cells):
            cells = cells.cpu().numpy()
        if _is_torch(keys):
            keys = keys.cpu().numpy()
        cells = np.ascontiguousarray(cells, np.int64)
        keys = np.arange(len(cells), dtype=np.int32) if keys is None else np.ascontiguousarray(keys, np.int32)
        if cells.ndim != 1 or keys.shape != cells.shape:
            raise ValueError("cell index: cells and candidate rows are two 1-d arrays of one length")
        h = ctypes.c_void_p()
        N.check(N.lib().mosaic_cell_index_create(ctx.handle, len(cells), N.ptr(cells), N.ptr(keys), ctypes.byref(h)))
        self.handle = h

    def info(self):
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(N.lib().mosaic_cell_index_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return dict(n_cells=a.value, n_entries=b.value, max_per_cell=c.value)

    def close(self):
        if self.handle:
            N.lib().mosaic_cell_index_destroy(self.handle)
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


def _index_array(a):
    if _is_torch(a):
        import torch

        return a.to(torch.int64).contiguous()
    return np.ascontiguousarray(a, np.int64)


def grid_ring_neighbours(ctx, landmarks, candidates, cell_index, rows, cells, keep_self=False):
    """GridRingNeighbours.transform (models/knn/GridRingNeighbours.scala:121-160) for one iteration, on
    the context's GPU (mosaic_ring_neighbours).  ``landmarks`` / ``candidates``: ``GeometryTable``s or
    anything ``geometry_table`` accepts (a PolygonSet, a LineSet, points, WKB / WKT rows);
    ``cell_index``: the candidates' ``CellIndex``; ``rows`` /
    ``cells``: one (landmark row, raw cell id) per row -- grid_geometrykringexplode(l, res, 1) in the
    first iteration, grid_geometrykloopexplode(l, res, i) in iteration i -- on the host or the device,
    duplicates allowed.

    Returns ``(landmark_row, candidate_row, distance, unmatched)``: one row per (landmark, candidate)
    such that a given cell of the landmark is the cell of a chip of the candidate, ordered by
    (landmark row, distance, candidate row); ``unmatched[l]`` is True iff a given cell of landmark l is
    no chip's cell (the left-outer join's null row).  A self match -- both rows are ROW_OK and have
    identical parts, rings and bitwise-equal vertices, an exact comparison where the reference compares
    hashes -- is dropped unless ``keep_self``; a pair with a null or row-path side is kept, with
    distance NaN, after the landmark's numbers.  The reference's st_intersects_aggregate filter is
    always true in this join and is not evaluated.  Ties in distance are broken by the candidate row,
    the engine's own rule (Spark's row_number leaves them undefined)."""
    rows, cells = _index_array(rows), _index_array(cells)
    if len(rows) != len(cells):
        raise ValueError("grid_ring_neighbours: rows and cells have different lengths")
    own = []
    h = ctypes.c_void_p()
    lib = N.lib()
    try:
        tabs = []
        for side in (landmarks, candidates):
            if not isinstance(side, GeometryTable):
                side = ctx.geometry_table(side)
                own.append(side)
            tabs.append(side)
        ctx._order(rows, cells)
        N.check(lib.mosaic_ring_neighbours(ctx.handle, cell_index.handle, tabs[0].handle, tabs[1].handle, N.ptr(rows),
                                           N.ptr(cells), len(rows), int(bool(keep_self)), ctypes.byref(h)))
        n_pairs, n_left = ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(lib.mosaic_neighbours_info(h, ctypes.byref(n_pairs), ctypes.byref(n_left)))
        l = np.zeros(n_pairs.value, np.int64)
        c = np.zeros(n_pairs.value, np.int64)
        d = np.zeros(n_pairs.value, np.float64)
        un = np.zeros(n_left.value, np.uint8)
        N.check(lib.mosaic_neighbours_export(h, N.ptr(l), N.ptr(c), N.ptr(d), N.ptr(un)))
    finally:
        if h:
            lib.mosaic_neighbours_destroy(h)
        for t in own:
            t.close()
    return l, c, d, un.astype(bool)


def ring_neighbours_last_ms():
    """(probe + de-duplication + self-match filter, distance, order): device ms of the calling thread's
    last grid_ring_neighbours (HIP events)."""
    split = np.zeros(3, np.float64)
    N.lib().mosaic_ring_neighbours_last_ms(N.ptr(split))
    return tuple(float(v) for v in split)


def _within_args(ctx, landmarks, candidates, radius, rows, own):
    """the two sides as tables (those built here are appended to ``own``), the rows (or None) and one
    radius per requested row, on the host or the device"""
    tabs = []
    for side in (landmarks, candidates):
        if not isinstance(side, GeometryTable):
            side = ctx.geometry_table(side)
            own.append(side)
        tabs.append(side)
    if rows is not None:
        rows = _index_array(rows)
        if rows.ndim != 1:
            raise ValueError("st_dwithin: rows is a 1-d array of landmark rows")
    n = len(tabs[0]) if rows is None else len(rows)
    if _is_torch(radius):
        import torch

        radius = radius.to(torch.float64).contiguous()
        if radius.dim() == 0:
            radius = radius.expand(n).contiguous()
    else:
        radius = np.asarray(radius, np.float64)
        radius = np.full(n, float(radius)) if radius.ndim == 0 else np.ascontiguousarray(radius)
    if radius.ndim != 1 or len(radius) != n:
        raise ValueError(f"st_dwithin: {len(radius) if radius.ndim == 1 else radius.shape} radii for {n} rows")
    ctx._order(rows, radius)
    return tabs, rows, radius, n


def within_candidates(ctx, landmarks, candidates, radius, rows=None):
    """The envelope filter's own count per requested row (mosaic_within_candidates): the candidates that
    are ROW_OK with at least one facet and whose box bound ``dist::box_lower_bound`` is <= the row's
    radius; 0 for a landmark that is not such a row and for a NaN or negative radius.  It is at least
    the number of pairs ``within_neighbours`` returns for the row, and what a caller sizes its calls by.
    Arguments as for ``within_neighbours``.  Returns int64 counts."""
    own = []
    try:
        tabs, rows, radius, n = _within_args(ctx, landmarks, candidates, radius, rows, own)
        counts = np.zeros(n, np.int64)
        N.check(N.lib().mosaic_within_candidates(ctx.handle, tabs[0].handle, tabs[1].handle, N.ptr(rows), N.ptr(radius), n,
                                                 N.ptr(counts)))
    finally:
        for t in own:
            t.close()
    return counts


def within_neighbours(ctx, landmarks, candidates, radius, rows=None, keep_self=True):
    """The distance-within join on the context's GPU (mosaic_within_neighbours): all (landmark,
    candidate) pairs with ``st_distance <= radius`` of the landmark's row.  ``landmarks`` /
    ``candidates``: ``GeometryTable``s or anything ``geometry_table`` accepts; ``radius``: one number
    for all rows or one per requested row; ``rows``: the landmark rows asked for, strictly ascending
    (None: all of them); radius and rows on the host or the device.

    Returns ``(landmark_row, candidate_row, distance)`` ordered by (landmark row, distance, candidate
    row).  Both rows of a pair are ROW_OK and have at least one facet: an empty geometry is within
    distance of nothing, null and row-path rows never pair.  A NaN or negative radius gives its row no
    pairs; ``inf`` accepts every such candidate.  A self match (``grid_ring_neighbours``' exact
    comparison) is dropped unless ``keep_self``.  The rows are those of the sequential definition over
    all pairs in mosaic_amd/csrc/ring_neighbours.h (rn::within): the envelope filter that finds the
    candidates drops none."""
    own = []
    h = ctypes.c_void_p()
    lib = N.lib()
    try:
        tabs, rows, radius, n = _within_args(ctx, landmarks, candidates, radius, rows, own)
        N.check(lib.mosaic_within_neighbours(ctx.handle, tabs[0].handle, tabs[1].handle, N.ptr(rows), N.ptr(radius), n,
                                             int(bool(keep_self)), ctypes.byref(h)))
        n_pairs = ctypes.c_int64(0)
        N.check(lib.mosaic_neighbours_info(h, ctypes.byref(n_pairs), None))
        l = np.zeros(n_pairs.value, np.int64)
        c = np.zeros(n_pairs.value, np.int64)
        d = np.zeros(n_pairs.value, np.float64)
        N.check(lib.mosaic_neighbours_export(h, N.ptr(l), N.ptr(c), N.ptr(d), None))
    finally:
        if h:
            lib.mosaic_neighbours_destroy(h)
        for t in own:
            t.close()
    return l, c, d


def within_neighbours_last_ms():
    """(envelope filter + self-match filter, distance + radius select, order): device ms of the calling
    thread's last within_neighbours (HIP events)."""
    split = np.zeros(3, np.float64)
    N.lib().mosaic_within_neighbours_last_ms(N.ptr(split))
    return tuple(float(v) for v in split)


def _bits(d):
    return np.ascontiguousarray(d, np.float64).view(np.uint64)


def knn_iterate(n_landmarks, step, k_neighbours, max_iterations, early_stop_iterations, distance_threshold):
    """SpatialKNN's iteration (SpatialKNN.scala:109-164, IterativeTransformer.scala:49-84), literally.
    ``step(active, iteration)`` is one GridRingNeighbours pass over the active landmarks: it returns
    ``(landmark_row, candidate_row, distance, unmatched)`` with ``unmatched`` a bool array over all
    landmarks.  Returns the match list M as ``(landmark_row, candidate_row, distance, iteration)``
    arrays -- a list, not a set: a candidate matched in two iterations has two rows, as the reference's
    matchesCheckpoint.append leaves it -- and the active sets of every iteration run."""
    n = int(n_landmarks)
    m_l, m_c, m_d, m_it = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float64)], [np.zeros(0, np.int32)]
    null = np.zeros(n, bool)
    active = np.arange(n, dtype=np.int64)
    actives = []
    stop_count, prev_cond, prev_distinct = 0, False, 0
    for it in range(1, int(max_iterations) + 1):
        actives.append(active)
        l, c, d, unmatched = step(active, it)
        m_l.append(np.asarray(l, np.int64))
        m_c.append(np.asarray(c, np.int64))
        m_d.append(np.asarray(d, np.float64))
        m_it.append(np.full(len(l), it, np.int32))
        null |= np.asarray(unmatched, bool)
        all_l, all_c, all_d = np.concatenate(m_l), np.concatenate(m_c), np.concatenate(m_d)
        with np.errstate(invalid="ignore"):
            within = all_d <= distance_threshold
        count = np.bincount(all_l[within], minlength=n)
        # a row within the threshold or a null row, and match_count - 1 < k (the null row counts for nothing)
        nxt = np.flatnonzero(((count > 0) | null) & (count <= k_neighbours)).astype(np.int64)
        distinct = len(np.unique(all_l << 32 | all_c))
        cond = len(active) == len(nxt) and distinct == prev_distinct and distinct > 0
        prev_distinct = distinct
        stop_count = 0 if cond != prev_cond else stop_count + 1
        prev_cond = cond
        active = nxt
        if (cond and stop_count == early_stop_iterations) or len(active) == 0:
            break
    return (np.concatenate(m_l), np.concatenate(m_c), np.concatenate(m_d), np.concatenate(m_it)), actives


def knn_result(matches, k_neighbours, distance_threshold):
    """SpatialKNN.transform's last step (SpatialKNN.scala:224-231): each landmark's rows ordered by
    (distance, candidate row, iteration), neighbour_number the 1-based rank, neighbour_number <=
    k_neighbours kept, then distance <= distance_threshold."""
    l, c, d, it = matches
    order = np.lexsort((it, c, _bits(d), l))
    l, c, d, it = l[order], c[order], d[order], it[order]
    first = np.flatnonzero(np.r_[True, l[1:] != l[:-1]]) if len(l) else np.zeros(0, np.int64)
    sizes = np.diff(np.r_[first, len(l)])
    number = (np.arange(len(l)) - np.repeat(first, sizes) + 1).astype(np.int32)
    keep = number <= k_neighbours
    with np.errstate(invalid="ignore"):
        keep &= d <= distance_threshold
    return dict(landmark_row=l[keep], candidate_row=c[keep], distance=d[keep], iteration=it[keep],
                neighbour_number=number[keep])


def knn_exact_radius(matches, n_landmarks, k_neighbours, distance_threshold):
    """The radius ``transform_exact`` asks the distance-within join for, per landmark: over the distinct
    candidates of the match list whose distance is a number <= ``distance_threshold``, the
    ``k_neighbours``-th smallest distance when there are that many, else ``distance_threshold``.
    With k candidates within r, a landmark's true k nearest all lie within r.  Returns ``(radius,
    from_ring)``; ``from_ring[l]`` says that the radius is a k-th ring distance."""
    l, c, d, _ = matches
    n = int(n_landmarks)
    radius = np.full(n, float(distance_threshold), np.float64)
    from_ring = np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        ok = np.asarray(d, np.float64) <= distance_threshold  # False for NaN
    l, c, d = np.asarray(l, np.int64)[ok], np.asarray(c, np.int64)[ok], np.asarray(d, np.float64)[ok]
    if len(l) == 0:
        return radius, from_ring
    _, first = np.unique(l << 32 | c, return_index=True)  # a pair's distance is the same in every iteration
    l, d = l[first], d[first]
    order = np.lexsort((_bits(d), l))
    l, d = l[order], d[order]
    start = np.flatnonzero(np.r_[True, l[1:] != l[:-1]])
    size = np.diff(np.r_[start, len(l)])
    full = size >= k_neighbours
    radius[l[start[full]]] = d[start[full] + k_neighbours - 1]
    from_ring[l[start[full]]] = True
    return radius, from_ring


def knn_exact_batches(counts, pair_budget):
    """Consecutive landmarks grouped while their summed candidate counts stay <= ``pair_budget``; a
    landmark over the budget is a batch of its own.  Returns ``[(first, stop), ...]`` covering
    ``range(len(counts))``."""
    batches, first, total = [], 0, 0
    for i, k in enumerate(np.asarray(counts, np.int64).tolist()):
        if i > first and total + k > pair_budget:
            batches.append((first, i))
            first, total = i, 0
        total += k
    if len(counts) > first:
        batches.append((first, len(counts)))
    return batches


def knn_exact_result(within, matches, active_sets, n_landmarks, k_neighbours):
    """``transform_exact``'s result from the distance-within rows ``within = (landmark_row,
    candidate_row, distance)``, ordered by (landmark row, distance bits, candidate row) with each pair
    once: neighbour_number is the rank in that order and the first ``k_neighbours`` stay.
    ``iteration`` is the first iteration of the match list that holds the pair, else the landmark's
    last active iteration + 1 (what the reference's last pass writes)."""
    l, c, d = (np.asarray(within[0], np.int64), np.asarray(within[1], np.int64), np.asarray(within[2], np.float64))
    first = np.flatnonzero(np.r_[True, l[1:] != l[:-1]]) if len(l) else np.zeros(0, np.int64)
    sizes = np.diff(np.r_[first, len(l)])
    number = (np.arange(len(l)) - np.repeat(first, sizes) + 1).astype(np.int32)
    keep = number <= k_neighbours
    l, c, d, number = l[keep], c[keep], d[keep], number[keep]
    last_active = np.zeros(int(n_landmarks), np.int32)
    for it, active in enumerate(active_sets, 1):
        last_active[np.asarray(active, np.int64)] = it
    iteration = last_active[l] + 1
    m_l, m_c, _, m_it = matches
    if len(m_l) and len(l):
        key = np.asarray(m_l, np.int64) << 32 | np.asarray(m_c, np.int64)
        order = np.lexsort((m_it, key))
        key, its = key[order], np.asarray(m_it, np.int32)[order]
        head = np.r_[True, key[1:] != key[:-1]]
        key, its = key[head], its[head]  # the first iteration of every matched pair
        mine = l << 32 | c
        at = np.minimum(np.searchsorted(key, mine), len(key) - 1)
        hit = key[at] == mine
        iteration = np.where(hit, its[at], iteration)
    return dict(landmark_row=l, candidate_row=c, distance=d, iteration=iteration.astype(np.int32), neighbour_number=number)


def _side_kind(geoms, what):
    if hasattr(geoms, "geom_parts"):
        return "polygons"
    if hasattr(geoms, "geom_lines"):
        return "lines"
    arrays = (np.ndarray, list)
    if isinstance(geoms, tuple) and len(geoms) == 2 and all(isinstance(a, arrays) or _is_torch(a) for a in geoms):
        return "points"
    if isinstance(geoms, np.ndarray) and geoms.ndim == 2 and geoms.shape[1] == 2:
        return "points"
    if _is_torch(geoms) and geoms.dim() == 2 and geoms.shape[1] == 2:
        return "points"
    raise TypeError(f"SpatialKNN: {what} are a PolygonSet, a LineSet or a point column ((x, y) arrays or an "
                    f"[n, 2] array), not {type(geoms).__name__}")


class _Side:
    """One side of the model on the device: its geometry column and its chips at the index resolution
    (grid_tessellateexplode(keepCoreGeometries = false); a LineSet's line chips, all non-core; or one
    chip per point), both produced once."""

    def __init__(self, ctx, geoms, res):
        self.table = ctx.geometry_table(geoms)
        self.n = len(self.table)
        if hasattr(geoms, "geom_parts"):
            chips = tessellate(ctx.index_system, geoms, res, keep_core_geom=False, ctx=ctx)
            self.is_core = np.array(chips["is_core"], np.uint8)
            self.index_id = np.array(chips["index_id"], np.int64)
            self.key = np.array(chips["polygon_key"], np.int32)
        elif hasattr(geoms, "geom_lines"):
            chips = tessellate(ctx.index_system, geoms, res, ctx=ctx, cells_only=True)
            self.is_core = np.array(chips["is_core"], np.uint8)
            self.index_id = np.array(chips["index_id"], np.int64)
            self.key = np.array(chips["polygon_key"], np.int32)
        else:
            ids = ctx.grid_pointascellid(geoms, res, raw=True)
            if _is_torch(ids):
                ids = ids.cpu().numpy()
            self.index_id = np.ascontiguousarray(ids, np.int64)
            self.is_core = np.zeros(self.n, np.uint8)
            self.key = np.arange(self.n, dtype=np.int32)

    def chips_of(self, rows):
        """the kept chips of the given (ascending) rows, keyed by their position in ``rows``"""
        lut = np.full(self.n, -1, np.int32)
        lut[rows] = np.arange(len(rows), dtype=np.int32)
        key = lut[self.key]
        m = key >= 0
        return dict(is_core=self.is_core[m], index_id=self.index_id[m], polygon_key=key[m], n_geoms=len(rows))

    def close(self):
        self.table.close()


class SpatialKNN:
    """SpatialKNN (models/knn/SpatialKNN.scala) with ``approximate = true``: for every landmark, up to
    ``k_neighbours`` candidates found by growing grid rings, nearest first.

    ``candidates`` / ``transform(landmarks)``: a PolygonSet, a LineSet or a point column (``(x, y)``
    arrays or an ``[n, 2]`` array); anything else raises TypeError.  A LineSet side is indexed by its
    line chips (Mosaic.lineFill); a line whose cells cross the antimeridian or a pole raises
    MosaicError there, and the error is passed on.  The keywords are the reference's parameters
    (kNeighbours, indexResolution, maxIterations, earlyStopIterations, distanceThreshold, approximate).
    The candidates are tessellated and indexed once, at the first ``transform``; a landmark column's
    chips are produced once per ``transform`` and every iteration asks the k-ring (iteration 1) or the
    k-loop (iteration i) of the active landmarks' kept chips only.

    As in the reference, the match list is a list: a candidate with chips both in a landmark's ring 1
    and in its loop 2 is matched in both iterations, both rows count towards k_neighbours and both stay
    in the result.  ``approximate=False`` -- the exact last pass over st_buffer(geometry, k-th distance)
    -- raises NotImplementedError: the engine has no st_buffer.  ``transform_exact`` is the engine's own
    exact answer -- every landmark's true k nearest, from the distance-within join -- and says why it
    is not that pass."""

    def __init__(self, ctx, candidates, k_neighbours=5, index_resolution=None, max_iterations=10, early_stop_iterations=3,
                 distance_threshold=sys.float_info.max, approximate=True):
        if not approximate:
            raise NotImplementedError("SpatialKNN(approximate=False): the exact last pass tessellates "
                                      "st_buffer(geometry, k-th neighbour distance), and the engine has no st_buffer")
        _side_kind(candidates, "the candidates")
        if index_resolution is None:
            raise ValueError("SpatialKNN: index_resolution is required")
        if k_neighbours < 1 or max_iterations < 1 or early_stop_iterations < 0:
            raise ValueError("SpatialKNN: k_neighbours >= 1, max_iterations >= 1 and early_stop_iterations >= 0")
        self.ctx = ctx
        self.candidates = candidates
        self.k_neighbours = int(k_neighbours)
        self.index_resolution = index_resolution
        self.max_iterations = int(max_iterations)
        self.early_stop_iterations = int(early_stop_iterations)
        self.distance_threshold = float(distance_threshold)
        self.approximate = True
        self._right = None
        self._index = None
        self._matches = None
        self.active_sets = None
        self.exact_stats = None  # of the last transform_exact
        self.exact_radius = None  # the radius it asked for, per landmark

    def _prepare(self):
        if self._right is None:
            self._right = _Side(self.ctx, self.candidates, self.index_resolution)
            self._index = CellIndex(self.ctx, (self._right.index_id, self._right.key))

    def _iterate(self, left):
        """the model's iterations over the landmark side: the match list and the active sets"""
        ctx = self.ctx
        res = self.index_resolution

        def step(active, it):
            rings = ctx._geometry_kring(left.chips_of(active), res, it, it > 1, True)
            lens = np.fromiter((len(r) for r in rings), np.int64, len(rings))
            rows = np.repeat(active, lens)
            cells = np.concatenate(rings) if len(rings) else np.zeros(0, np.int64)
            return grid_ring_neighbours(ctx, left.table, self._right.table, self._index, rows, cells)

        return knn_iterate(left.n, step, self.k_neighbours, self.max_iterations, self.early_stop_iterations,
                           self.distance_threshold)

    def transform(self, landmarks):
        """The matches as columns ``landmark_row``, ``candidate_row``, ``distance``, ``iteration`` and
        ``neighbour_number`` (a dict of arrays), ordered by (landmark row, neighbour number)."""
        _side_kind(landmarks, "the landmarks")
        self._prepare()
        left = _Side(self.ctx, landmarks, self.index_resolution)
        try:
            matches, self.active_sets = self._iterate(left)
        finally:
            left.close()
        self._matches = knn_result(matches, self.k_neighbours, self.distance_threshold)
        return self._matches

    def transform_exact(self, landmarks, pair_budget=1 << 24):
        """Every landmark's true ``k_neighbours`` nearest candidates within ``distance_threshold``, by
        (distance, candidate row), self matches excluded: the columns of ``transform``, each (landmark,
        candidate) once, what a brute force over all pairs returns.

        The iterations of ``transform`` run first.  A landmark whose match list holds k distinct
        candidates within the threshold gets their k-th distance as its radius (``knn_exact_radius``),
        any other landmark the threshold; the distance-within join (``within_neighbours``,
        ``keep_self=False``) over those radii returns a superset of the k nearest, which is ranked.
        The join runs in batches of consecutive landmarks whose candidate pairs
        (``within_candidates``) sum to at most ``pair_budget``; a landmark over the budget is a batch
        of its own.  ``iteration`` is the first iteration that matched the pair, else the landmark's
        last active iteration + 1.  ``exact_stats`` reports landmarks with a ring radius and with the
        threshold radius, batches, candidate pairs and pairs within; ``metrics()`` serves the result.

        This is the engine's own exact answer, not the reference's ``approximate = false`` pass: that
        pass tessellates st_buffer(geometry, k-th distance), revisits only the landmarks still active
        after the last iteration and appends to the match list, so it is neither de-duplicated nor
        exact for the others.  Here every landmark is revisited, the result is de-duplicated, and no
        buffer polygon is involved."""
        _side_kind(landmarks, "the landmarks")
        self._prepare()
        ctx = self.ctx
        left = _Side(ctx, landmarks, self.index_resolution)
        try:
            matches, self.active_sets = self._iterate(left)
            radius, from_ring = knn_exact_radius(matches, left.n, self.k_neighbours, self.distance_threshold)
            counts = within_candidates(ctx, left.table, self._right.table, radius)
            batches = knn_exact_batches(counts, pair_budget)
            parts = [within_neighbours(ctx, left.table, self._right.table, radius[a:b], rows=np.arange(a, b, dtype=np.int64),
                                       keep_self=False) for a, b in batches]
        finally:
            left.close()
        within = tuple(np.concatenate([p[i] for p in parts]) if parts else np.zeros(0, t)
                       for i, t in enumerate((np.int64, np.int64, np.float64)))
        self.exact_radius = radius
        self.exact_stats = dict(ring_radius=int(from_ring.sum()), threshold_radius=int((~from_ring).sum()), batches=len(batches),
                                candidate_pairs=int(counts.sum()), pairs_within=len(within[0]))
        self._matches = knn_exact_result(within, matches, self.active_sets, left.n, self.k_neighbours)
        return self._matches

    def metrics(self):
        """getMetrics (SpatialKNN.scala:280-318) over the last transform's matches."""
        m = self._matches
        if m is None:
            raise RuntimeError("SpatialKNN.metrics: call transform first")
        some = len(m["distance"]) > 0
        return dict(match_count=float(len(m["distance"])),
                    max_neighbours=float(m["neighbour_number"].max()) if some else float("nan"),
                    max_radius=float(m["distance"].max()) if some else float("nan"),
                    min_radius=float(m["distance"].min()) if some else float("nan"),
                    convergence_iteration=float(m["iteration"].max()) if some else float("nan"))

    def close(self):
        if self._index is not None:
            self._index.close()
            self._index = None
        if self._right is not None:
            self._right.close()
            self._right = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
