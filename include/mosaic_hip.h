/*
 * libmosaic_hip.so -- C ABI of the MI355X engine for Mosaic's point-in-polygon chip-join hot path.
 *
 * Plain C: pointers, sizes and status codes; no exceptions cross the boundary; no torch types.
 * Every entry point is callable from a JNI shim (the Catalyst columnar exec sketched in
 * INTEGRATION.md) or from Python ctypes (mosaic_amd/_native.py).
 *
 * Reference interfaces replaced (bransonf/mosaic @ 0.3.9, paths under
 * src/main/scala/com/databricks/labs/mosaic/):
 *   mosaic_point_to_cell      grid_pointascellid / grid_longlatascellid per row:
 *                             expressions/index/PointIndexGeom.scala:32-40,
 *                             expressions/index/PointIndexLonLat.scala:44-51 ->
 *                             core/index/H3IndexSystem.scala:140-142 (pointToIndex) and
 *                             core/index/BNGIndexSystem.scala:277-291 (pointToIndex)
 *   mosaic_point_geom_to_cell grid_pointascellid over a geometry column (WKB / WKT / hex rows):
 *   mosaic_point_geom_decode    PointIndexGeom.scala:32-40 -> GeometryAPI.geometry (GeometryAPI.scala:64-72)
 *                             -> MosaicGeometryJTS.fromWKB / fromWKT / fromHEX (MosaicGeometryJTS.scala:164,
 *                             195-200) -> getCentroid (:49-53) -> getX / getY (point/MosaicPointJTS.scala:23-25)
 *   mosaic_resolution         H3IndexSystem.getResolution (H3IndexSystem.scala:39-54),
 *                             BNGIndexSystem.getResolution (BNGIndexSystem.scala:342-353)
 *   mosaic_bng_format/_parse  BNGIndexSystem.format / parse (BNGIndexSystem.scala:114-129, 391-413)
 *   mosaic_chip_table_create  the build side of the chip join: rows of ChipType
 *                             struct<is_core, index_id, wkb> (core/types/ChipType.scala:17-28,
 *                             core/types/model/MosaicChip.scala:20-74) produced by
 *                             grid_tessellateexplode (expressions/index/MosaicExplode.scala:70-79)
 *   mosaic_pip_join_count     the Quickstart join + filter + groupBy(zone).count():
 *   mosaic_pip_join_pairs       point_cell == chip.index_id && (chip.is_core || st_contains(chip.wkb, point))
 *                             (notebooks/examples/python/QuickstartNotebook.py:205-219;
 *                             sql/join/PointInPolygonJoin.scala:68-84)
 *   mosaic_st_contains        st_contains(geom, point) per row: expressions/geometry/ST_Contains.scala:34-42
 *                             -> core/geometry/MosaicGeometryJTS.scala:101 (JTS Geometry.contains)
 *
 * Conventions
 *   - Return value: MOSAIC_OK (0) or a mosaic_status code; mosaic_last_error() (thread-local)
 *     holds the message.  MOSAIC_E_RES / MOSAIC_E_NAN carry the reference's exception messages
 *     ("H3 resolution has to be between 0 and 15; found N", "BNG resolution not supported; found N",
 *     "NaN coordinates are not supported.") so a JNI shim can rethrow IllegalStateException.
 *   - Input arrays are borrowed for the duration of the call and may live in host memory or in
 *     device memory of the context's GPU (detected per pointer).  Host inputs are staged over PCIe.
 *     Device inputs must be complete when the call's work starts: the context's own streams are
 *     non-blocking (no implicit order with the null stream), so a caller producing columns on another
 *     stream binds that stream with mosaic_set_stream, records an event on it and passes it to
 *     mosaic_stream_wait_event before the call, or synchronises it first.
 *   - Calls are synchronous unless the context option "async" is 1, in which case device-pointer
 *     calls only enqueue work on the calling thread's stream (mosaic_sync() waits and reports
 *     deferred errors).  Exception: a binned join (option "bin_points", tables without a usable point
 *     raster) reads its kept-row count back once per sort chunk, so it blocks the calling thread
 *     until each chunk's cover pass has run; its results are still reported through mosaic_sync.
 *   - Threads: a context is bound to one GPU and every entry point is thread-safe (SURVEY.md §8(b),
 *     the executor's task threads sharing one context; the reference's index systems are JVM
 *     singletons, H3IndexSystem.scala:22-27).  Each calling thread gets its own HIP stream (created
 *     on first use; mosaic_set_stream / mosaic_get_stream act on the calling thread's), scratch
 *     buffers, counters (mosaic_last_stats) and timing events, so concurrent calls never share
 *     state.  Options are shared by the context and copied once at the start of every call.  Chip
 *     tables are immutable once created and may be joined from any thread.
 */
#ifndef MOSAIC_HIP_H
#define MOSAIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: mosaic_chip_table_raster writes 8 values (was 5); option "exact_cap"; the aggregate geometry.
 * 3: mosaic_chip_table_raster writes 9 values (out9[8] = leaf_lines; callers must pass 9 slots);
 *    mosaic_intersection_aggregate_geometry; mosaic_cell_kring count -4 for rows with k > 128 near a
 *    pentagon (now answered, see 4).
 * 4: border chips are the reference's planar clip against indexToGeometry (mosaic_tessellate);
 *    mosaic_tess_counters; mosaic_cell_kring answers every row (no -4). */
#define MOSAIC_ABI_VERSION 4

typedef enum {
    MOSAIC_OK = 0,
    MOSAIC_E_ARG = 1,      /* invalid argument (null pointer, bad size, bad option) */
    MOSAIC_E_RES = 2,      /* unsupported resolution (IllegalStateException in the reference) */
    MOSAIC_E_NAN = 3,      /* NaN coordinate with BNG (IllegalStateException in the reference) */
    MOSAIC_E_HIP = 4,      /* HIP runtime error / no device */
    MOSAIC_E_WKB = 5,      /* undecodable or unsupported chip WKB */
    MOSAIC_E_CAPACITY = 6, /* output buffer too small (pairs) or deferred queue overflow (async) */
    MOSAIC_E_NOMEM = 7     /* allocation failure */
} mosaic_status;

typedef enum { MOSAIC_GRID_H3 = 0, MOSAIC_GRID_BNG = 1 } mosaic_grid;

typedef struct mosaic_ctx mosaic_ctx;
typedef struct mosaic_chips mosaic_chips;

int mosaic_abi_version(void);
const char* mosaic_last_error(void);

/* ---- context ---- */
/* Bind a context to HIP device `device` (ordinal as seen by this process). */
int mosaic_init(int device, mosaic_ctx** out);
int mosaic_destroy(mosaic_ctx* ctx);
/* Options: "jdk" (8: Math.toRadians = deg / 180 * PI, the JDK 8 runtime of the reference's CI;
 * 9+: deg * DEGREES_TO_RADIANS), "async" (0/1), "block" (threads per block of the row kernels,
 * multiple of 64), "blocks_per_cu" (grid sizing), "timing" (0/1: HIP events around each join's main
 * kernel; 2: the point-raster join's mixed-cell kernel is timed as a second entry), "raster" (ray-parity
 * raster cells per border chip side, 1..64, for tables built afterwards), "raster_adaptive" (0/1: rings
 * with few segments get 2 ceil(sqrt(segments)) cells a side instead, at most "raster"; default 1),
 * "raster_min_segments" (rings with fewer segments get no raster: their contains test walks the
 * segments; default 0, and at least 16 for H3 tables with more polygons than point-raster codes,
 * whose joins test chips from tile images instead),
 * "lane_edges" (raster cell lists up to this long are evaluated by the owning lane), "tiles" (0/1: H3
 * tile directory for tables built afterwards, and its use by joins), "point_raster" (0/1: the point
 * raster over the tile directory, likewise), "raster_sub" / "raster_cell" (its sub-blocks per tile
 * side and leaf cells per sub-block side, powers of two, for tables built afterwards; default 64 /
 * 16), "raster_lines" (0/1: sub-blocks crossed by one straight chip edge store a line record instead
 * of a leaf block; default 1), "raster_leaf_lines" (0/1: leaf cells of the other mixed sub-blocks
 * crossed by one straight chip edge store a line record too, answered by k_join_leaf before
 * k_join_mixed; default 1 since round 6: the reference's chord-edged border chips leave ~1.6x more
 * mixed leaf rows than face-plane chips did), "leaf_join" (0/1: joins run k_join_leaf on the mixed queue; default 1),
 * "raster_build" (1: the point raster is classified on the GPU, the
 * default; 0: on host threads -- identical bytes), "raster_quad" (its LDS level: 0 off, 1 default budget of 32768
 * entries, or an entry budget <= 65536), "stream_block" (k_join_stream workgroup size, a multiple of
 * 64 up to 1024, default 1024), "stream_grid" (0, the default: the stream kernels' persistent grid;
 * k in [1, 65536]: at most k workgroups -- a test knob that fixes how many 256-row groups each wave
 * pipelines; nothing but the two stream launches follows it), "host_chunk" (rows per chunk when mosaic_pip_join_count gets
 * host-resident coordinates: the next chunk's copy overlaps the current chunk's join; 0 = stage the
 * whole batch; default 2^25), "mixed_rows" (1/2/4, default 1), "mixed_blocks_per_cu" (default 16), "cell_blocks_per_cu" (k_cell_h3 grid, default 256; 0 = one lane per row pair), "stream_pipe"
 * (0: k_join_stream; 1: the software-pipelined H3 stream kernel; 2: it with the gathering rows
 * compacted, k_join_stream_cpt, the default -- each where it applies), "bng_cpt" (0/1: the compacted
 * BNG stream kernel where it applies; default 1), "bng_lds" (0/1: BNG tables
 * built afterwards carry an LDS cell level for the BNG stream kernel; default 1), "bng_cell" (sub-cells
 * per BNG border cell side in those tables, a power of two <= 64; default 32), "bng_group_lines" (0/1:
 * those tables' sub-block levels name a line record wherever one decides a whole 4 x 4 group; default
 * 1), "bng_wedges" (0/1: those tables carry wedge records for sub-cells split at a chip vertex,
 * answered by the BNG mixed-row kernel before its chip loop; default 1), "scratch_limit" (see
 * the per-thread state below), "bin_points" (0/1: H3 joins on a tile directory without a usable point
 * raster sort the points by tile before the chip loop -- the border-chip-heavy C4 shape; default 1),
 * "bin_min_rows" (smallest batch that is binned; default 2^18), "bin_chunk" (rows per sort chunk;
 * default 2^28), "tile_images" (0: none; 1: tables built without a point raster carry per-tile chip
 * images the binned join copies into LDS, the default; 2: every tile-directory table carries them),
 * "bin_spin_cap" (the binned join's look-back poll limit; < 0 forces its uncompacted fallback -- a test
 * knob), "exact_cap" (rows of the exact-H3 queue; 0 = the default max(n / 8, 2^20) capped at n; an overflow
 * reruns the batch on the exact path, or is reported as MOSAIC_E_CAPACITY by mosaic_sync after an
 * async call). */
int mosaic_set_option(mosaic_ctx* ctx, const char* key, int64_t value);
/* Per-thread state.  Each calling thread gets its own execution state on a context (HIP stream,
 * copy stream, timing events, scratch queues and staging sized by its largest call).  It is freed
 * by mosaic_thread_release (the calling thread's state), by mosaic_destroy (all), or when a thread
 * other than the process's main thread exits (a thread_local guard), so an executor whose worker
 * pool retires and creates threads does not accumulate streams or scratch.  States are keyed by a
 * per-thread serial number, never by pthread ids (which the runtime reuses).  Option
 * "scratch_limit" (bytes, 0 = keep; default 0) frees a thread's scratch when a call returns holding
 * more than that.  mosaic_thread_count reports the live states and the scratch they hold.
 * (Replaces no reference interface: the JVM side's H3Core / index-system singletons hold no device
 * state, H3IndexSystem.scala:22-27; this is the multiplexing SURVEY.md §8(b) asks of the ABI.) */
int mosaic_thread_release(mosaic_ctx* ctx);
int mosaic_thread_count(mosaic_ctx* ctx, int64_t* n_threads, int64_t* scratch_bytes);
/* The calling thread's hipStream_t (created by the context unless set by this thread). */
int mosaic_get_stream(mosaic_ctx* ctx, void** stream);
int mosaic_set_stream(mosaic_ctx* ctx, void* stream);
/* Orders the calling thread's later work after a caller event: enqueues hipStreamWaitEvent(stream,
 * (hipEvent_t)event) on the thread's stream, so device columns produced on another stream (a cuDF /
 * Arrow producer, torch) are complete before the next call reads them, without binding that stream
 * or blocking the host.  The event must have been recorded (hipEventRecord) before this call. */
int mosaic_stream_wait_event(mosaic_ctx* ctx, void* event);
/* Wait for enqueued work; reports deferred errors of async calls. */
int mosaic_sync(mosaic_ctx* ctx);
/* Counters of the calling thread's last join/index call: [0] rows that needed the exact H3 path,
 * [1] (point, border chip) contains tests, [2] matched pairs (pairs calls only).
 * Filled only by sync calls. */
int mosaic_last_stats(mosaic_ctx* ctx, int64_t* out3);
/* Rows the calling thread's last join sorted on its binned path (the points some chip may hold:
 * k_bin_cover's keep count), 0 when the join took another path. */
int mosaic_last_binned_rows(mosaic_ctx* ctx, int64_t* out);
/* Queue counts of the calling thread's last join call (of its last chunk of < 2^32 rows): out2[0] rows
 * the stream kernel queued for the kernels after it (rows its raster could not answer, and rows
 * outside the raster's range), out2[1] rows k_join_leaf passed on to k_join_mixed (0 without
 * k_join_leaf: option "leaf_join" = 0, BNG, tables without leaf lines).  Both 0 when the call ran no
 * stream kernel.  Filled only by sync calls.  For tests that must know a queue path ran. */
int mosaic_last_queue(mosaic_ctx* ctx, int64_t* out2);
/* With option "timing" = 1, every join call brackets its fused kernel with HIP events on the
 * context stream.  Waits for the stream, writes up to cap elapsed times (ms) in call order, reports
 * how many calls were timed in *n_out, and resets the list. */
int mosaic_kernel_times(mosaic_ctx* ctx, double* out_ms, int64_t cap, int64_t* n_out);
/* Name of the dominant kernel of the calling thread's last join call ("k_join_stream_cpt",
 * "k_join_stream_pipe", "k_join_stream_bng", ...; "" before any): what a profile of that call
 * should be filtered on.  Static storage; never freed. */
const char* mosaic_last_kernel(mosaic_ctx* ctx);

/* ---- grid systems ---- */
/* getResolution for an Int resolution; validates the range of the grid system. */
int mosaic_resolution(int grid, int res, int* out);
/* getResolution for a String resolution ("9" for H3; "100m", "500m", ... or "4" for BNG). */
int mosaic_resolution_str(int grid, const char* res, int* out);
/* grid_pointascellid / grid_longlatascellid: x = lon (H3) or easting (BNG), y = lat or northing.
 * valid (nullable): 1 = row present; null rows give out_valid 0 and cell 0 (NullIntolerant). */
int mosaic_point_to_cell(mosaic_ctx* ctx, int grid, int res, const double* x, const double* y,
                         const uint8_t* valid, int64_t n, int64_t* out_cell, uint8_t* out_valid);
/* H3 cells from the exact path alone (h3_exact: the line-by-line H3 C v3.7 restatement with the
 * glibc 2.35 libm restatement glibc_math.h) for every row, skipping the certified fast path;
 * x = lon, y = lat (degrees).  Same answer as mosaic_point_to_cell; exists so the exact path can be
 * checked against the reference on arbitrarily many rows. */
int mosaic_point_to_cell_exact(mosaic_ctx* ctx, int res, const double* x, const double* y, int64_t n,
                               int64_t* out_cell);
/* Diagnostics: out[i] = the device's glibc restatement of fn(a[i]) / atan2(a[i], b[i]);
 * fn 0 = sin, 1 = cos (both via sincos), 2 = tan, 3 = acos, 4 = atan2. */
int mosaic_diag_libm(mosaic_ctx* ctx, int fn, const double* a, const double* b, int64_t n, double* out);
/* grid_pointascellid over a point geometry column in Arrow binary / utf8 layout: row i is
 * data[offsets[i] .. offsets[i+1]); format = MOSAIC_GEOM_WKB / _WKT / _HEX, | MOSAIC_GEOM_OFFSETS32
 * for 32-bit offsets (default 64-bit).  Every row JTS 1.19 certainly reads as a non-empty Point is
 * decoded on the device (Double.parseDouble-exact numbers; either WKB byte order; EWKB / ISO Z, M,
 * SRID) and indexed: row_status MOSAIC_ROW_OK.  Null rows: MOSAIC_ROW_NULL, cell 0.  Every other
 * row (other geometry types, whose centroid the reference indexes; POINT EMPTY and malformed rows,
 * on which the reference throws) gets MOSAIC_ROW_PATH and cell 0: the caller evaluates those rows
 * with the reference's row-wise expression.  *n_rowpath (nullable) = their number. */
#define MOSAIC_GEOM_WKB 0
#define MOSAIC_GEOM_WKT 1
#define MOSAIC_GEOM_HEX 2
#define MOSAIC_GEOM_OFFSETS32 0x100
#define MOSAIC_ROW_NULL 0
#define MOSAIC_ROW_OK 1
#define MOSAIC_ROW_PATH 2
int mosaic_point_geom_to_cell(mosaic_ctx* ctx, int grid, int res, int format, const void* offsets,
                              const uint8_t* data, const uint8_t* valid, int64_t n, int64_t* out_cell,
                              uint8_t* row_status, int64_t* n_rowpath);
/* The decode alone: x / y of MOSAIC_ROW_OK rows (0 elsewhere), row_status as above. */
int mosaic_point_geom_decode(mosaic_ctx* ctx, int format, const void* offsets, const uint8_t* data,
                             const uint8_t* valid, int64_t n, double* x, double* y, uint8_t* row_status,
                             int64_t* n_rowpath);
/* grid_pointascellid over the COORDS form of points: InternalGeometryType rows
 * struct<typeId: int, srid: int, boundaries: array<array<array<double>>>, holes: ...>
 * (core/types/model/InternalGeometry.scala; st_point's output, expressions/constructors/ST_Point.scala:27-32)
 * as Arrow columns: type_id[n]; boundary_offsets[n + 1] (row -> boundaries), coord_offsets
 * (boundary -> coordinates), value_offsets (coordinate -> values), all int32 (Arrow list); values
 * (float64).  Rows with type_id 1 (POINT) whose first boundary's first coordinate has 2 values, or
 * 3 or more (z ignored), are decoded as MosaicPointJTS.fromInternal does
 * (core/geometry/point/MosaicPointJTS.scala:82-89) and indexed: MOSAIC_ROW_OK.  Null rows:
 * MOSAIC_ROW_NULL.  Other types (the reference indexes their centroid) and rows the reference throws
 * on (no boundary, no coordinate, a 1-value coordinate): MOSAIC_ROW_PATH.  Child arrays must not
 * hold nulls.  The holes column is not read (a Point has none). */
int mosaic_point_coords_to_cell(mosaic_ctx* ctx, int grid, int res, const int32_t* type_id,
                                const int32_t* boundary_offsets, const int32_t* coord_offsets,
                                const int32_t* value_offsets, const double* values, const uint8_t* valid, int64_t n,
                                int64_t* out_cell, uint8_t* row_status, int64_t* n_rowpath);
/* The decode alone: x / y of MOSAIC_ROW_OK rows (0 elsewhere), row_status as above. */
int mosaic_point_coords_decode(mosaic_ctx* ctx, const int32_t* type_id, const int32_t* boundary_offsets,
                               const int32_t* coord_offsets, const int32_t* value_offsets, const double* values,
                               const uint8_t* valid, int64_t n, double* x, double* y, uint8_t* row_status,
                               int64_t* n_rowpath);
/* BNG id <-> string (BNGIndexSystem.format / parse).  format returns the string length. */
int mosaic_bng_format(int64_t id, char* buf, size_t cap);
int mosaic_bng_parse(const char* s, int64_t* out);
/* serializeCellId over a BNG cell column (IndexSystem.scala:37-46 -> BNGIndexSystem.format
 * :114-129), computed on the GPU, in Arrow utf8 layout: offsets[n + 1] (int64) and the characters.
 * Null rows (valid[i] == 0; valid may be null) are empty strings.  If the characters exceed
 * chars_cap, returns MOSAIC_E_CAPACITY with *chars_needed set (offsets are written either way);
 * an id the reference cannot format gives MOSAIC_E_ARG. */
int mosaic_bng_format_column(mosaic_ctx* ctx, const int64_t* ids, const uint8_t* valid, int64_t n, int64_t* offsets,
                             char* chars, int64_t chars_cap, int64_t* chars_needed);

/* BNGIndexSystem.parse (BNGIndexSystem.scala:391-413) over a string column on the GPU: the
 * StringType cell ids of BNG chips (BNGIndexSystem.scala:28, serializeCellId IndexSystem.scala:37-46)
 * back to the long ids mosaic_chip_table_create takes.  Arrow utf8 (offsets32 = 1: int32 offsets) or
 * large_utf8 (int64 offsets) layout, offsets[n + 1] + chars; null rows (valid[i] == 0) give 0.
 * A row the reference cannot parse (its letterMap lookup or Integer.parseInt throws) gives
 * MOSAIC_E_ARG naming the first such row. */
int mosaic_bng_parse_column(mosaic_ctx* ctx, int offsets32, const void* offsets, const uint8_t* chars,
                            const uint8_t* valid, int64_t n, int64_t* out_ids);

/* ---- chip table (build side) ---- */
/* n_chips rows of ChipType: is_core[i], index_id[i] (int64 cell id), wkb bytes
 * wkb[wkb_offsets[i] .. wkb_offsets[i+1]) (Polygon / MultiPolygon, either byte order; empty or
 * zero-length = no geometry), polygon_key[i] in [0, n_polygons) (the row's zone / group key).
 * The table is copied to device memory; the caller may free its buffers after the call. */
int mosaic_chip_table_create(mosaic_ctx* ctx, int grid, int res, int64_t n_chips, const uint8_t* is_core,
                             const int64_t* index_id, const int64_t* wkb_offsets, const uint8_t* wkb,
                             const int32_t* polygon_key, int32_t n_polygons, mosaic_chips** out);
/* The same over Arrow columns as a JNI shim hands them over: wkb_offsets are int32 (Arrow binary)
 * when wkb_offsets32 != 0, else int64 (large_binary).  BNG StringType ids: parse them first with
 * mosaic_bng_parse_column. */
int mosaic_chip_table_create_arrow(mosaic_ctx* ctx, int grid, int res, int64_t n_chips, const uint8_t* is_core,
                                   const int64_t* index_id, const void* wkb_offsets, int wkb_offsets32,
                                   const uint8_t* wkb, const int32_t* polygon_key, int32_t n_polygons,
                                   mosaic_chips** out);
/* The array form (PointInPolygonJoin.joinArrayRows, sql/join/PointInPolygonJoin.scala:39-66): polygon
 * row p's chip array (grid_tessellate's chips) is rows [chip_offsets[p], chip_offsets[p + 1]) of the
 * flattened columns is_core / index_id / wkb (wkb_offsets indexed from chip_offsets[0], n + 1 entries);
 * joins then count at most one pair per (point, polygon row), from the first chip of the row with
 * the point's cell (array_position + element_at), as the reference does. */
int mosaic_chip_table_create_arrays(mosaic_ctx* ctx, int grid, int res, int32_t n_polygons, const int64_t* chip_offsets,
                                    const uint8_t* is_core, const int64_t* index_id, const int64_t* wkb_offsets,
                                    const uint8_t* wkb, mosaic_chips** out);
int mosaic_chip_table_destroy(mosaic_chips* chips);
/* out8: n_chips, n_cells, n_border, n_vertices, n_rings, device_bytes, hash_capacity, n_polygons */
int mosaic_chip_table_info(const mosaic_chips* chips, int64_t* out8);

/* H3 tile directory of the table (built when option "tiles" = 1, the default): out13 = built (0/1),
 * tiles along lon, tiles along lat, tile records, window entries, tiles on the generic path, rings;
 * point raster (option "point_raster" = 1, the default) built (0/1), sub-blocks per tile side,
 * cells per sub-block side, pure sub-blocks, mixed sub-blocks, mixed cells.  BNG tables report their
 * dense cell table instead in the first five: built (0/1), cells along e, cells along n, bytes of the
 * LDS cell level (option "bng_lds"), its block shift, mixed border-cell sub-cells, line-record sub-cells. */
int mosaic_chip_table_tiles(const mosaic_chips* chips, int64_t* out13);
/* out4 = lon, lat of the tile grid origin and tiles per degree along lon, lat (tile i covers
 * [x0 + i / sx, x0 + (i + 1) / sx)). */
int mosaic_chip_table_tile_grid(const mosaic_chips* chips, double* out4);
/* Point raster detail: out5 = sub-blocks stored as line records (option "raster_lines"), LDS quad
 * level entries (0: none), quad shift (sub-blocks per quad side = 1 << shift), raster bytes on the
 * device, 1 if joins run the stream kernel on it (quad level with compact copies, edges clamp-safe);
 * then the binned join's per-tile LDS chip images (option "tile_images"): records with an image,
 * image bytes on the device, bytes of the largest image; leaf cells stored as line records (option
 * "raster_leaf_lines"). */
int mosaic_chip_table_raster(const mosaic_chips* chips, int64_t* out9);
/* Build cost of the table in ms (ms4): chip hash + geometry + chip rasters, tile directory (host),
 * point-raster classification (GPU with option "raster_build" = 1, the default; host threads with
 * 0), point-raster assembly (host); *digest = FNV-1a 64 of the point raster's arrays (0: no raster),
 * equal for both classification builds. */
int mosaic_chip_table_build_info(const mosaic_chips* chips, double* ms4, uint64_t* digest);

/* ---- the join ---- */
/* counts[p] = number of (point, chip) pairs with chip polygon_key p (overwritten). */
int mosaic_pip_join_count(mosaic_ctx* ctx, const mosaic_chips* chips, const double* x, const double* y,
                          int64_t n, int64_t* counts);
/* Emits every matching (row, polygon_key) pair (unordered).  If more than `cap` pairs match,
 * returns MOSAIC_E_CAPACITY with *n_out = required size. */
int mosaic_pip_join_pairs(mosaic_ctx* ctx, const mosaic_chips* chips, const double* x, const double* y,
                          int64_t n, int64_t* out_row, int32_t* out_key, int64_t cap, int64_t* n_out);

/* ---- chip production (host; build side of the join, not the hot path) ---- */
/* grid_tessellateexplode(geometry, res, keep_core_geom) over n_geoms polygonal geometries given as
 * flat rings: geometry g = parts [geom_parts[g], geom_parts[g+1]); part p = rings
 * [part_rings[p], part_rings[p+1]); ring r = vertices xy[2*ring_offsets[r] ..] (x, y interleaved,
 * lon/lat for H3, BNG metres for BNG).  Chip rows carry the geometry index as their key.
 * Cells are enumerated and classified (core / border / none) in the plane where they are exact
 * (H3: the icosahedron face's gnomonic plane; BNG: metres).  A border chip is the reference's
 * `geometry.intersection(indexToGeometry(cell))` (IndexSystem.getBorderChips): the geometry clipped
 * in its own coordinates against the cell polygon -- H3: the h3ToGeoBoundary ring in degrees (JDK 8
 * Math.toDegrees) with straight sides, face-edge vertices included; BNG: the square -- with JTS
 * 1.19's crossing arithmetic (RobustLineIntersector / Intersection.intersection), every ring written
 * from its lowest vertex, shells counter-clockwise, holes clockwise, polygons by lowest vertex (the
 * order of the reference's rendered chips); a border chip equal to its cell is a core chip
 * (`intersect.equals(indexGeom)`).  A core chip's geometry is indexToGeometry(cell) (densify > 1: H3
 * core outlines follow the cell's arcs with `densify` points a side instead).
 * Divergence from the reference: a cell the planar clip cannot take -- its h3ToGeoBoundary ring lies
 * over the antimeridian (a side spanning more than 180 degrees of longitude) or a pole, so it is no
 * polygon in the lon / lat plane -- gets the face-plane chip, not `geometry n indexToGeometry`: the
 * geometry clipped against the cell's hexagon in the icosahedron face's gnomonic plane, computed
 * vertices mapped back to lon / lat.  The reference intersects with the wrapped lon / lat ring there
 * (a polygon spanning the globe's width), which is not restated.  mosaic_tess_counters counts these
 * cells.  MOSAIC_E_ARG for a geometry with a vertex more than ~78 degrees
 * from the centre of a face it meets.
 * Reference: expressions/index/MosaicExplode.scala:70-79, core/Mosaic.scala:21-87,
 * core/index/IndexSystem.scala:152-186, core/index/H3IndexSystem.scala:93-100. */
typedef struct mosaic_chip_set mosaic_chip_set;
int mosaic_tessellate(int grid, int res, int64_t n_geoms, const int64_t* geom_parts, const int64_t* part_rings,
                      const int64_t* ring_offsets, const double* xy, int keep_core_geom, int densify,
                      mosaic_chip_set** out);
int mosaic_chip_set_info(const mosaic_chip_set* cs, int64_t* n_chips, int64_t* wkb_bytes);
/* Copies the chip rows out: is_core[n], index_id[n], key[n], wkb_offsets[n+1], wkb[wkb_bytes]. */
/* Zero-copy view of the same columns: pointers into the chip set, valid until mosaic_chip_set_destroy
 * (what mosaic_chip_set_export copies; the Python binding wraps them and destroys the set with the
 * last array). */
int mosaic_chip_set_columns(const mosaic_chip_set* cs, const uint8_t** is_core, const int64_t** index_id,
                            const int32_t** key, const int64_t** wkb_offsets, const uint8_t** wkb);
int mosaic_chip_set_export(const mosaic_chip_set* cs, uint8_t* is_core, int64_t* index_id, int32_t* key,
                           int64_t* wkb_offsets, uint8_t* wkb);
int mosaic_chip_set_destroy(mosaic_chip_set* cs);
/* grid_tessellateexplode with the cell classification on the GPU: the same chip set as
 * mosaic_tessellate, row for row and byte for byte.  Each candidate cell of a geometry's envelope is
 * classified on the GPU (border: a ring segment within eps of the cell; core: cell centre inside
 * the part, even-odd; else dropped), replacing the per-cell JTS buffer / intersects of
 * IndexSystem.getBorderChips / getCoreChips (core/index/IndexSystem.scala:152-186, via
 * Mosaic.mosaicFill core/Mosaic.scala:60-87).  BNG: k_bng_tess_classify on the cell squares; H3:
 * k_tess_classify_poly on the (densify-subdivided) hexagons in the icosahedron face plane.  Border
 * cells are clipped on the GPU as well (k_tess_clip_ll, one lane per cell, the host routine's
 * arithmetic); candidate enumeration, the per-face pieces of H3 geometries spanning faces and the
 * chip WKB assembly are host code.  A border cell the lane cannot take is clipped by
 * mosaic_tessellate's host routine, with the same bytes: one needing more than the lane's workspace
 * (24 ring chains, 12 result rings), one whose result does not fit the shared output buffer, and one
 * that is no planar lon / lat polygon (over the antimeridian or a pole) -- the last gets the
 * face-plane chip, mosaic_tessellate's divergence from the reference above, and is counted by
 * mosaic_tess_counters in the same way.  Errors as mosaic_tessellate. */
int mosaic_tessellate_gpu(mosaic_ctx* ctx, int grid, int res, int64_t n_geoms, const int64_t* geom_parts,
                          const int64_t* part_rings, const int64_t* ring_offsets, const double* xy,
                          int keep_core_geom, int densify, mosaic_chip_set** out);
/* Duration (HIP events on the context stream) of the last classification launch, ms. */
double mosaic_tess_last_classify_ms(const mosaic_ctx* ctx);
/* Process-wide counters of the chip producers' host clip: border chips clipped (ll_chips) and cells
 * that fell back to the face-plane clip (ll_fallbacks). */
int mosaic_tess_counters(int64_t* ll_chips, int64_t* ll_fallbacks);

/* ---- grid_tessellateexplode for LineString / MultiLineString (Mosaic.lineFill) ---- */
/* Chips of line geometries (core/Mosaic.scala:89-97, 146-194): geometry g is the component lines
 * [geom_lines[g], geom_lines[g + 1]) and line l the vertices xy[2 line_offsets[l] .. 2 line_offsets[l + 1])
 * (host arrays; x = lon, y = lat for H3, BNG metres).  Each component is decomposed on its own (the
 * reference flattens a MultiLineString), so a cell two components meet gives two rows.  Consecutive
 * repeated vertices are removed first; a component without vertices gives no chips, one of a single
 * distinct vertex MOSAIC_E_ARG, a NaN coordinate MOSAIC_E_NAN.
 * One row per (component, cell whose closed indexToGeometry polygon the line meets) -- the cells the
 * reference's lineDecompose traversal reaches -- with is_core = 0, key = g and the WKB (JTS WKBWriter,
 * big-endian 2D) of line n cell after JTS's overlay of a line with an area: the line cut where it meets
 * the cell's boundary (the polygon producer's crossing arithmetic: llclip.h), the pieces inside or on the
 * cell kept, each a LineString in the line's direction with original vertices copied; one piece:
 * LINESTRING, several: MULTILINESTRING in line order; a cell the line only touches: POINT / MULTIPOINT
 * of the distinct contact points in line order.  A piece along a cell side belongs to both cells.
 * Rows are ordered by geometry, component, then the position along the line where the chip begins (ties
 * by cell id): the reference's breadth-first order is a Spark row order and is not restated.  The piece
 * order and direction are derived from JTS's algorithm; no JTS output pins them.
 * Divergences from the reference: (a) a cell holding both pieces and isolated contact points gives the
 * pieces (the reference's GeometryCollection collapses to POLYGON EMPTY: it drops the chip and stops
 * expanding there, which can lose the rest of the line); (b) the line is not noded at its own crossings
 * (the same point set in fewer, longer pieces); (c) a cell the walk comes to that is no planar lon / lat
 * polygon (over the antimeridian or a pole), or a vertex outside the grid: MOSAIC_E_ARG naming the
 * geometry.  keep_core_geom does not exist for lines (the reference ignores it).
 * cells_only = 1: the same rows with an empty WKB column (what the k-rings need). */
int mosaic_tessellate_lines(int grid, int res, int64_t n_geoms, const int64_t* geom_lines, const int64_t* line_offsets,
                            const double* xy, int cells_only, mosaic_chip_set** out);
/* The same chip set, row for row and byte for byte, produced on the GPU: k_line_spans splits every
 * segment into spans of about two cells; k_line_walk (one lane per span, count then write) emits the
 * (cell, segment) pairs of exact walks; a radix sort groups them by (cell, line); k_line_clip (one lane
 * per group, count then write) builds each chip's pieces into space taken by a prefix sum; the host
 * orders the rows and writes the WKB.  A span trying more than 64 cells and a chip of more than 8 pieces
 * are handed to the host routine (same bytes). */
int mosaic_tessellate_lines_gpu(mosaic_ctx* ctx, int grid, int res, int64_t n_geoms, const int64_t* geom_lines,
                                const int64_t* line_offsets, const double* xy, int cells_only, mosaic_chip_set** out);
/* The calling thread's last mosaic_tessellate_lines_gpu: out = segments walked, (line, cell) groups,
 * groups handed to the host, (cell, segment) pairs emitted; ms = device time (HIP events) of the walk
 * (spans included), the sort (grouping included) and the clip. */
int mosaic_tess_lines_last(int64_t out[4], double ms[3]);
/* The walk of the calling thread's last mosaic_tessellate_lines_gpu, read-only: out = spans walked (the
 * sum of the segments' span counts), spans whose walk tried more than 64 cells and went to the host
 * routine, (cell, segment) pairs those spans added (counted in mosaic_tess_lines_last's pairs, before
 * equal pairs of overlapping spans are dropped).  All zero after a call without vertices; not specified
 * after a call that failed.  The groups handed to the host are mosaic_tess_lines_last's out[2]:
 * neither count includes the other. */
int mosaic_tess_lines_last_walk(int64_t out[3]);

/* ---- st_contains per row ---- */
/* out[i] = JTS contains(geometry[geom_index[i]], POINT(px[i] py[i])); geometries given as WKB. */
int mosaic_st_contains(mosaic_ctx* ctx, int64_t n_geoms, const int64_t* wkb_offsets, const uint8_t* wkb,
                       const int32_t* geom_index, const double* px, const double* py, int64_t n, uint8_t* out);

/* ---- st_intersects_aggregate over the chip join of two chip tables ---- */
/* For every (left polygon_key, right polygon_key) pair whose chip sets share at least one cell id,
 * flag = OR over the chip pairs of the shared cells of (left.is_core || right.is_core ||
 * JTS 1.19 intersects(left.wkb, right.wkb)).  Groups are written sorted by (left key, right key);
 * if more than `cap` groups exist, returns MOSAIC_E_CAPACITY with *n_out = the required size.
 * Both tables must use the same grid and resolution.  Replaces the equi-join + groupBy +
 * st_intersects_aggregate pattern: ST_IntersectsAggregate.update
 * (expressions/geometry/ST_IntersectsAggregate.scala:28-39) as used in
 * ST_IntersectsBehaviors.scala:34-47 / MosaicContext.scala st_intersects_aggregate. */
int mosaic_intersects_aggregate(mosaic_ctx* ctx, const mosaic_chips* left, const mosaic_chips* right,
                                int32_t* out_left_key, int32_t* out_right_key, uint8_t* out_flag, int64_t cap,
                                int64_t* n_out);

/* ---- st_intersects_aggregate over the join of line chips with polygon chips ---- */
/* The reason lines are tessellated: "which trips cross which zones" is the equi-join of two
 * grid_tessellateexplode outputs on index_id, grouped by (line row, polygon row) and folded with
 * st_intersects_aggregate.  getChips sends LINESTRING / MULTILINESTRING to lineFill
 * (core/Mosaic.scala:21-35) and ST_IntersectsAggregate.update decodes whatever WKB a chip holds
 * (expressions/geometry/ST_IntersectsAggregate.scala:28-39).
 * Semantics: one group per (line key, polygon key) whose chip sets share a cell id (the group exists
 * even when its flag is false); flag = OR over the group's chip pairs of l.is_core || p.is_core ||
 * intersects(l.wkb, p.wkb).  lineFill's chips are never core, but the column is honoured literally.
 * intersects is JTS Geometry.intersects (the closed point sets share a point), restated in
 * mosaic_amd/csrc/line_isect.h on exact predicates: (1) a side without a coordinate: false; (2) the
 * chips' envelopes do not meet: false; (3) a segment of a piece meets a ring segment of the polygon
 * chip, holes included: true; (4) the first vertex of some piece -- every POINT / MULTIPOINT item is a
 * piece -- is inside or on the boundary of some polygon part: true; (5) false.  Host and GPU answers
 * are equal, not close.
 * A line chip set is the chip columns of mosaic_tessellate_lines: WKB types 1 POINT (NaN ordinates:
 * an empty chip), 4 MULTIPOINT, 2 LINESTRING (no points: an empty chip), 5 MULTILINESTRING, either byte
 * order, ISO Z/M and EWKB flags; a zero-length row is an empty chip.
 * Errors: MOSAIC_E_WKB naming the row for any other type, a truncated buffer, a member of another type
 * inside a multi-geometry, a LineString of exactly one point; MOSAIC_E_NAN for a NaN inside a line;
 * MOSAIC_E_ARG for a negative key, decreasing offsets, or tables of different grid / resolution;
 * MOSAIC_E_CAPACITY at 2^31 chips or 2^32 - 1 vertices, and -- with *n_out = the required size -- when
 * more than `cap` groups exist.  Groups are written sorted by (line key, polygon key). */
typedef struct mosaic_line_chips mosaic_line_chips;
/* The device-resident line chip table (immutable after creation).  wkb_offsets: n_chips + 1 offsets
 * into wkb, int32 when offsets32 != 0, else int64 (Arrow binary / large_binary). */
int mosaic_line_chips_create(mosaic_ctx* ctx, int grid, int res, int64_t n_chips, const uint8_t* is_core,
                             const int64_t* index_id, const int32_t* key, const void* wkb_offsets, int offsets32,
                             const uint8_t* wkb, mosaic_line_chips** out);
/* out4 = chips, pieces (a piece of one vertex is a point), vertices, device bytes. */
int mosaic_line_chips_info(const mosaic_line_chips* lines, int64_t* out4);
int mosaic_line_chips_destroy(mosaic_line_chips* lines);
/* The join on the GPU: k_lj_probe (one lane per line chip; probes the polygon table's cell hash, finds
 * or inserts every chip pair's group, lists the pairs that need the geometry test) and k_lj_test (one
 * team of lanes per listed pair); k_lj_groups then packs the groups for the copy back.  The output
 * protocol is mosaic_intersects_aggregate's. */
int mosaic_line_intersects_aggregate(mosaic_ctx* ctx, const mosaic_line_chips* lines, const mosaic_chips* polygons,
                                     int32_t* out_line_key, int32_t* out_polygon_key, uint8_t* out_flag, int64_t cap,
                                     int64_t* n_out);
/* The calling thread's last mosaic_line_intersects_aggregate: out = line chips whose cell the polygon
 * table holds, chip pairs, pairs geometry-tested, groups; ms = device time (HIP events) of k_lj_probe
 * (both passes) and of k_lj_test. */
int mosaic_line_join_last(int64_t out[4], double ms[2]);
/* Lanes per pair of k_lj_test for the process's later calls: 64 (one wave per pair) or 16 (four pairs
 * per wave); another value changes nothing.  Returns the previous width.  The answers do not depend on
 * it; it exists to measure the two forms. */
int mosaic_line_join_team(int lanes);
/* The same join on the host, on at most 16 threads: no context, no GPU.  Polygon chips are decoded as
 * mosaic_chip_table_create decodes them (Polygon / MultiPolygon), line chips as above; offsets are
 * int64. */
int mosaic_line_intersects_aggregate_host(int grid, int res, int64_t n_l, const uint8_t* l_core, const int64_t* l_cell,
                                          const int32_t* l_key, const int64_t* l_off, const uint8_t* l_wkb, int64_t n_p,
                                          const uint8_t* p_core, const int64_t* p_cell, const int32_t* p_key,
                                          const int64_t* p_off, const uint8_t* p_wkb, int32_t* out_line_key,
                                          int32_t* out_polygon_key, uint8_t* out_flag, int64_t cap, int64_t* n_out);

/* ---- st_intersection_aggregate over the chip join of two chip tables ---- */
/* For every (left polygon_key, right polygon_key) pair whose chip sets share a cell id: the union
 * ST_IntersectionAggregate.update / merge (expressions/geometry/ST_IntersectionAggregate.scala:40-72)
 * builds from, per joined chip pair, the cell (both core: indexToGeometry), the other chip (one core)
 * or the two chips' intersection.  Per cell that union is (the group's left chips there, or the
 * cell when one is core) n (its right chips, likewise); a cell with one pair is the pair's piece.
 * mosaic_intersection_aggregate returns its area per group -- st_area(st_intersection_aggregate(..)),
 * the quantity the reference's tests check (ST_IntersectionBehaviors.scala:22-135, 1e-8): per cell the
 * area of that piece from the cell overlay (overlay.h, one GPU lane per (group, cell)).  out_status 1
 * marks groups the engine does not answer (an overlay capacity exceeded, a cell without geometry):
 * evaluate those on the row path.  Sorted by key pair;
 * MOSAIC_E_CAPACITY with *n_out set when more than cap groups exist.  Each (group, cell) piece is one
 * record and a group's area is summed on the host in cell-slot order, so repeated calls return the
 * same bits. */
int mosaic_intersection_aggregate(mosaic_ctx* ctx, const mosaic_chips* left, const mosaic_chips* right,
                                  int32_t* out_left_key, int32_t* out_right_key, double* out_area, uint8_t* out_status,
                                  int64_t cap, int64_t* n_out);
/* The aggregate's geometry: per group the union as the WKB JTS writes (big-endian 2D Polygon, or
 * MultiPolygon for several polygons; POLYGON EMPTY when the pieces have no area), dissolved across
 * cells (pieces of adjacent cells form one polygon; shells clockwise, holes counter-clockwise).  The
 * per-cell boundaries come from the GPU (overlay.h, one lane per (group, cell)); the host joins them
 * (isect_geom.cpp).  Lower-dimensional parts of the reference's result (chips that only touch, whose
 * JTS intersection is a line or a point) are not emitted: the polygonal part is.  Vertex order and
 * ring starts are not JTS's (the reference's own depend on Spark's aggregation order).  area = the
 * sum of the cells' piece areas (cell-slot order); status 1 = not answered (area NaN, no WKB). */
typedef struct mosaic_isect_geoms mosaic_isect_geoms;
int mosaic_intersection_aggregate_geometry(mosaic_ctx* ctx, const mosaic_chips* left, const mosaic_chips* right,
                                           mosaic_isect_geoms** out);
int mosaic_isect_geoms_info(const mosaic_isect_geoms* g, int64_t* n_groups, int64_t* wkb_bytes);
/* left_key[n], right_key[n], area[n], status[n], wkb_offsets[n + 1], wkb[wkb_bytes] (any may be null) */
int mosaic_isect_geoms_export(const mosaic_isect_geoms* g, int32_t* left_key, int32_t* right_key, double* area,
                              uint8_t* status, int64_t* wkb_offsets, uint8_t* wkb);
int mosaic_isect_geoms_destroy(mosaic_isect_geoms* g);

/* ---- st_intersection_aggregate over the join of line chips with polygon chips ---- */
/* "How much of each trip lies in each zone": one row per (line key, polygon key) whose chip sets share
 * a cell id (the groups of mosaic_line_intersects_aggregate; a group exists even when its length is
 * 0), sorted by key pair, with the length of the line inside the polygon -- and, from the geometry
 * call, the pieces themselves (ST_IntersectionAggregate.scala:40-72 over a lineFill table).
 * Increment per joined chip pair (csrc/line_clip.h is the definition):
 *   polygon chip core   the whole line chip: every piece of at least 2 vertices (POINT / MULTIPOINT
 *                       items contribute nothing); the polygon chip's geometry is not read, so a table
 *                       built without core geometry serves
 *   neither side core   clip(line chip, polygon chip): every segment is cut where llclip::meet finds
 *                       it meeting a ring segment; an interval between consecutive cuts is kept iff
 *                       its midpoint is not exterior to the polygon chip (the boundary counts: a
 *                       stretch along a polygon edge is in the closed intersection, as in JTS) and
 *                       contributes sqrt(dx * dx + dy * dy); maximal chains of kept intervals within a
 *                       piece are the runs
 *   line chip core      MOSAIC_E_ARG naming the first such chip that joins: lineFill never makes one,
 *                       and the reference would union the polygon chip in, which is not a line result
 * A group's length is the sum of its pairs' lengths in (cell id, line chip row, polygon chip row)
 * order, each pair's in (piece, segment, interval) order: GPU, host and repeated calls agree bit for
 * bit.  Its geometry is its runs in that order as JTS writes them (big-endian 2D): LINESTRING for one
 * run, MULTILINESTRING for several, LINESTRING EMPTY (type 2, zero points) for none; a run is its first
 * cut point, the original vertices in between (copied), its last cut point.
 * Divergences from the reference (JTS intersection, then union): isolated touch points are not emitted
 * (the union would carry a POINT); runs are not noded at ring vertices they pass, nor merged across
 * cells (JTS's union does not line-merge either; no JTS output pins piece order or direction); a
 * segment lying exactly along a side shared by two cells is in both cells' chips and is counted twice.
 * On the GPU: k_lx_probe lists every chip pair with its cell (count, then fill: no guessed capacity),
 * k_lx_chip_len the whole-chip lengths, k_lx_clip one wave per pair to clip.  A pair with a segment of
 * more than kCutCap meet points is finished by the host driver (the same code and bits): no group is
 * refused, the status column is 0 throughout.
 * Errors as mosaic_line_intersects_aggregate: MOSAIC_E_ARG for tables of different grid / resolution or
 * another device, MOSAIC_E_CAPACITY at 2^31 chip pairs and -- with *n_out = the required size -- when
 * more than `cap` groups exist. */
int mosaic_line_intersection_aggregate(mosaic_ctx* ctx, const mosaic_line_chips* lines, const mosaic_chips* polygons,
                                       int32_t* out_line_key, int32_t* out_polygon_key, double* out_length, int64_t cap,
                                       int64_t* n_out);
/* The same with the geometry: read with mosaic_isect_geoms_info / _export (the area column holds the
 * length, left key = line key, right key = polygon key), release with mosaic_isect_geoms_destroy. */
int mosaic_line_intersection_aggregate_geometry(mosaic_ctx* ctx, const mosaic_line_chips* lines,
                                                const mosaic_chips* polygons, mosaic_isect_geoms** out);
/* The calling thread's last call of either: out = chip pairs, pairs clipped (no core side), pairs
 * finished on the host (over the cut cap), run records of the clipped pairs, groups, kCutCap; ms =
 * device time (HIP events) of k_lx_probe (both passes), of k_lx_chip_len + k_lx_clip (lengths and run
 * counts) and of k_lx_clip's run fill pass (the geometry call). */
int mosaic_line_intersection_last(int64_t out[6], double ms[3]);
/* The same aggregate on the host, on at most 16 threads: no context, no GPU; the columns of
 * mosaic_line_intersects_aggregate_host.  The GPU calls are tested against it bit for bit. */
int mosaic_line_intersection_aggregate_host(int grid, int res, int64_t n_l, const uint8_t* l_core, const int64_t* l_cell,
                                            const int32_t* l_key, const int64_t* l_off, const uint8_t* l_wkb, int64_t n_p,
                                            const uint8_t* p_core, const int64_t* p_cell, const int32_t* p_key,
                                            const int64_t* p_off, const uint8_t* p_wkb, mosaic_isect_geoms** out);

/* ---- grid_cellkring / grid_cellkloop over a cell column (BNG, H3) ---- */
/* loop = 0: kRing(cell, k); loop = 1: kLoop(cell, k).  Row i's cells go to out[i * stride ..] and
 * out_count[i] = their number (-1 for null rows, valid[i] == 0).  0 <= k <= 1000.
 * BNG: stride = 8k (loop) or 1 + 4k(k + 1) (ring), the cell then the loops 1..k, in the reference's
 * order (bottom, right, top, left; cells failing isValid dropped).  Reference: BNGIndexSystem.kRing /
 * kLoop / isValid (core/index/BNGIndexSystem.scala:216-263).
 * H3: stride = max(6k, 1) (loop) or 1 + 3k(k + 1) (ring), in H3 v3.7's hexRange / hexRing order
 * (reference H3IndexSystem.kRing / kLoop, core/index/H3IndexSystem.scala:154-177); where the walk
 * meets a pentagon, kRing is H3's _kRingInternal hash table read in slot order (as h3-java returns
 * it) and kLoop the reference's own fallback, kRing(k).toSet diff kRing(k - 1).toSet in Scala
 * HashSet order (:169-176).  That search makes ~5 k^3 dependent steps per row: it runs on the GPU for
 * k <= 128 and on host threads beyond (the same code), so every row is answered.  A row whose id is
 * not a valid cell gets out_count[i] = -2 (no cells written). */
int mosaic_cell_kring(mosaic_ctx* ctx, int grid, const int64_t* cells, const uint8_t* valid, int64_t n, int k,
                      int loop, int64_t* out, int32_t* out_count);

/* ---- H3 cell geometry over a cell column ---- */
/* H3 C v3.7 h3ToGeo / h3ToGeoBoundary bit for bit (x87 long-double steps and glibc libm restated),
 * in degrees through java.lang.Math.toDegrees (option "jdk"), x = lng, y = lat.
 * mode 0 (h3ToGeo): out = double[2 n], the cell centre (x, y); out_count[i] = 1.
 * mode 1 (h3ToGeoBoundary): out = double[20 n], row i's vertices from out + 20 i as (x, y) pairs;
 *   out_count[i] = their number (5..10: Class III cells crossing an icosahedron edge and pentagons
 *   carry extra edge vertices).
 * mode 2 (grid_boundaryaswkb: IndexGeometry -> H3IndexSystem.indexToGeometry -> toWKB): out =
 *   uint8[189 n], row i's JTS big-endian 2D WKB polygon (the boundary closed with its first vertex)
 *   from out + 189 i; out_count[i] = its byte length (13 + 16 (vertices + 1)).
 * Null rows (valid[i] == 0): out_count[i] = -1.  An id that is not a valid H3 cell: MOSAIC_E_ARG.
 * Reference: H3IndexSystem.indexToGeometry / getBufferRadius / polyfill
 * (core/index/H3IndexSystem.scala:73-126), expressions/index/IndexGeometry.scala:65-75. */
int mosaic_h3_cell_geometry(mosaic_ctx* ctx, int mode, const int64_t* cells, const uint8_t* valid, int64_t n,
                            void* out, int32_t* out_count);

/* ---- grid_polyfill ---- */
/* grid_polyfill(geometry, res) over n_geoms polygonal geometries in the flat-ring layout of
 * mosaic_tessellate (x = lon, y = lat for H3; BNG metres), on the GPU.  Row g's cells are
 * cells[offsets[g] .. offsets[g + 1]) of the result (mosaic_cell_lists_export).
 * H3: per polygon part, H3 C v3.7 polyfill(shell, holes, res) as h3-java 3.7.0 is called by
 * H3IndexSystem.polyfill (core/index/H3IndexSystem.scala:113-126): the cells whose h3ToGeo centre
 * H3's pointInsidePolygon accepts, reached from the cells of the sampled ring edges; the parts' lists
 * concatenated, each in the order h3-java returns (H3's output-table slot order).  Vertices through
 * Math.toRadians (option "jdk").
 * BNG: BNGIndexSystem.polyfill (core/index/BNGIndexSystem.scala:185-204): the cells reached from
 * the vertex and centroid cells whose square's centroid the geometry contains (JTS), ordered as
 * the reference's Scala immutable HashSet iterates them.
 * status[g]: MOSAIC_POLYFILL_OK, or MOSAIC_POLYFILL_UNSUPPORTED (no cells written) for an H3 row
 * holding a non-finite vertex, or a BNG row without area (searches through the 12 pentagon base
 * cells follow H3's _kRingInternal fallback, as h3-java does).  An empty
 * geometry gives no cells.  Errors: MOSAIC_E_RES, MOSAIC_E_NAN (BNG NaN vertex), MOSAIC_E_CAPACITY. */
#define MOSAIC_POLYFILL_OK 0
#define MOSAIC_POLYFILL_UNSUPPORTED (-2)
typedef struct mosaic_cell_lists mosaic_cell_lists;
int mosaic_polyfill(mosaic_ctx* ctx, int grid, int res, int64_t n_geoms, const int64_t* geom_parts,
                    const int64_t* part_rings, const int64_t* ring_offsets, const double* xy, mosaic_cell_lists** out);
int mosaic_cell_lists_info(const mosaic_cell_lists* lists, int64_t* n_rows, int64_t* n_cells);
/* offsets[n_rows + 1], cells[n_cells], status[n_rows] (any may be null) */
int mosaic_cell_lists_export(const mosaic_cell_lists* lists, int64_t* offsets, int64_t* cells, int32_t* status);
int mosaic_cell_lists_destroy(mosaic_cell_lists* lists);
/* Device time (HIP events on the calling thread's stream) of the calling thread's last mosaic_polyfill, ms. */
double mosaic_polyfill_last_ms(void);

/* ---- grid_geometrykring / grid_geometrykloop ---- */
/* The k-ring (loop = 0) or k-loop (loop = 1) of each geometry's chips (Mosaic.geometryKRing /
 * geometryKLoop, core/Mosaic.scala:111-144, 211-223; expressions/index/GeometryKRing*.scala,
 * GeometryKLoop*.scala), on the GPU.  With core = the cells of a geometry's is_core chips, border =
 * the cells of its other chips and dist(c) = the smallest j with c in kLoop(b, j) for a border cell
 * b (0 for the border cells):
 *   k-ring(k) = core + {c : dist(c) <= k}, 0 <= k <= 1000;
 *   k-loop(k) = {c : dist(c) == k} - core, 1 <= k <= 1000;  any other k: MOSAIC_E_ARG.
 * H3: a breadth-first search under kRing(., 1); BNG: every border cell's loops 1..k by the
 * reference's arithmetic (exact at the grid's edge, where a neighbour walk is not).  Row g's cells are
 * cells[offsets[g] .. offsets[g + 1]) of the result, in Scala 2.12 immutable HashSet iteration order
 * (equal 32-bit hashes by ascending id); sets of <= 4 cells iterate in insertion order in Scala,
 * which is not restated, and no reference fixture pins these orders ("order unpinned").
 * mosaic_chips_kring takes chip columns (the rows of grid_tessellateexplode, or one non-core chip per
 * point: Mosaic.pointChip): key[i] in [0, n_geoms) names the chip's geometry, duplicate rows are
 * allowed, a cell given both as core and as border counts as both.  mosaic_geometry_kring is
 * mosaic_tessellate_gpu(keep_core_geom = 0) followed by it; for line geometries
 * the binding runs mosaic_tessellate_lines_gpu(cells_only = 1) and passes its rows, all border chips,
 * to mosaic_chips_kring.  status[g]: MOSAIC_POLYFILL_UNSUPPORTED (no cells) for a geometry with a
 * chip id that is not a valid cell of res; a geometry without chips gives an empty row.
 * Options: "gk_table_log2" (log2 of the search table's first slot count, 4..30, default 16; the
 * table grows by rehashing), "gk_max_cells" (slot count past which the call returns
 * MOSAIC_E_CAPACITY, default 2^27: a safety cap, not a measured one). */
int mosaic_chips_kring(mosaic_ctx* ctx, int grid, int res, int64_t n_chips, const uint8_t* is_core,
                       const int64_t* index_id, const int32_t* key, int64_t n_geoms, int k, int loop,
                       mosaic_cell_lists** out);
int mosaic_geometry_kring(mosaic_ctx* ctx, int grid, int res, int64_t n_geoms, const int64_t* geom_parts,
                          const int64_t* part_rings, const int64_t* ring_offsets, const double* xy, int k, int loop,
                          mosaic_cell_lists** out);
/* dist[n_cells] of a geometry k-ring result, cell for cell: -1 for a core cell the search did not
 * reach within k.  MOSAIC_E_ARG for the lists of mosaic_polyfill, which carry none. */
int mosaic_cell_lists_export_dist(const mosaic_cell_lists* lists, int32_t* dist);
/* Device time (HIP events on the calling thread's stream) of the search, sort and offsets of the calling
 * thread's last mosaic_chips_kring (for mosaic_geometry_kring: without the tessellation), ms. */
double mosaic_geometry_kring_last_ms(void);

/* ---- st_distance over geometry columns (functions/MosaicContext.scala:146 ST_Distance ->
 * expressions/geometry/ST_Distance.scala:34-36 -> JTS Geometry.distance; step 3 of the KNN iteration,
 * models/knn/GridRingNeighbours.scala:153-156) ---- */
/* A device-resident geometry column: immutable after creation, usable from any thread (like a chip
 * table), freed with mosaic_geoms_destroy.  Rows are Point, MultiPoint, LineString, MultiLineString,
 * Polygon or MultiPolygon; line rows are served by the columns that ask for them (below).
 * _wkb: row i is wkb[offsets[i] .. offsets[i + 1]) (either byte order, ISO Z/M and EWKB variants);
 *   valid[i] == 0 is a null row (MOSAIC_ROW_NULL); LineString, MultiLineString, GeometryCollection,
 *   POINT EMPTY and undecodable rows are MOSAIC_ROW_PATH (the convention of
 *   mosaic_point_geom_to_cell), not an error of the call.
 * _wkb_ex: _wkb with flags.  MOSAIC_GEOMS_LINES: LineString and MultiLineString rows are decoded
 *   (through the same reader) into line parts -- each component line an open run of n >= 2 vertices
 *   with n - 1 segments, never closed and never a container -- and are MOSAIC_ROW_OK; LINESTRING
 *   EMPTY / MULTILINESTRING EMPTY are MOSAIC_ROW_OK rows at distance 0.0 from everything, an empty
 *   member adds nothing, a component of exactly one vertex makes the row MOSAIC_ROW_PATH.  flags 0 is
 *   _wkb: a column built without the flag keeps line rows as MOSAIC_ROW_PATH, on purpose, so callers
 *   that send such rows to the row path see no change.  An unknown flag: MOSAIC_E_ARG.
 * _arrays: polygonal geometries in the flat-ring layout of mosaic_polyfill (host pointers).
 * _lines: line geometries in the layout of mosaic_tessellate_lines (host pointers): geometry g is the
 *   component lines [geom_lines[g], geom_lines[g + 1]), line l the vertices [line_offsets[l],
 *   line_offsets[l + 1]) of xy (interleaved).  Rows as under MOSAIC_GEOMS_LINES; inconsistent offsets:
 *   MOSAIC_E_ARG.
 * _points: row i is POINT (x[i] y[i]); host or device pointers; a NaN coordinate is MOSAIC_ROW_PATH. */
typedef struct mosaic_geoms mosaic_geoms;
#define MOSAIC_GEOMS_LINES 1u
int mosaic_geoms_create_wkb(mosaic_ctx* ctx, int64_t n, const int64_t* offsets, const uint8_t* wkb,
                            const uint8_t* valid /*nullable*/, mosaic_geoms** out);
int mosaic_geoms_create_wkb_ex(mosaic_ctx* ctx, int64_t n, const int64_t* offsets, const uint8_t* wkb,
                               const uint8_t* valid /*nullable*/, uint32_t flags, mosaic_geoms** out);
int mosaic_geoms_create_lines(mosaic_ctx* ctx, int64_t n, const int64_t* geom_lines, const int64_t* line_offsets,
                              const double* xy, mosaic_geoms** out);
int mosaic_geoms_create_arrays(mosaic_ctx* ctx, int64_t n, const int64_t* geom_parts, const int64_t* part_rings,
                               const int64_t* ring_offsets, const double* xy, mosaic_geoms** out);
int mosaic_geoms_create_points(mosaic_ctx* ctx, const double* x, const double* y, int64_t n, mosaic_geoms** out);
int mosaic_geoms_info(const mosaic_geoms* geoms, int64_t* n_geoms, int64_t* n_vertices, int64_t* n_row_path);
int mosaic_geoms_destroy(mosaic_geoms* geoms);
/* out[i] = st_distance(left[left_row[i]], right[right_row[i]]); left_row == right_row == NULL: row i
 * with row i (n_pairs rows of both columns).  The value is that of the sequential definition in
 * mosaic_amd/csrc/st_distance.h, bit for bit: 0.0 when either geometry is empty or one holds a
 * component of the other (only polygons hold; a line never does, closed or not), otherwise the
 * smallest JTS segment / point distance over all facet pairs.
 * status[i] (nullable): MOSAIC_ROW_OK; MOSAIC_ROW_NULL (either side null, out NaN); MOSAIC_ROW_PATH
 * (either side a row-path row, out NaN).  A row index out of range: MOSAIC_E_ARG, nothing written.
 * out / status / the row arrays: host or device pointers.  Options: "dist_tile" (segments per LDS
 * tile, [1, 1024]), "dist_small_work" (facet pairs up to which one lane serves a pair) and
 * "dist_prune" (0: no pruning, same result). */
int mosaic_st_distance(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                       const int64_t* right_row, int64_t n_pairs, double* out, int32_t* status);
/* out[i] = st_intersects(left[left_row[i]], right[right_row[i]]) as 1 or 0 (ST_Intersects.scala ->
 * MosaicGeometryJTS.intersects -> JTS Geometry.intersects: the closed point sets share a point);
 * left_row == right_row == NULL: row i with row i.  The value is that of the sequential definition in
 * mosaic_amd/csrc/st_intersects.h: 0 when either geometry is empty (where mosaic_st_distance gives
 * 0.0) or the geometry boxes do not meet, 1 when two facets meet or a polygon part of one side holds
 * the first vertex of a component of the other (a line never holds anything), else 0.  The same
 * row kinds are served as by mosaic_st_distance.
 * status[i] (nullable): MOSAIC_ROW_OK; MOSAIC_ROW_NULL / MOSAIC_ROW_PATH as for mosaic_st_distance,
 * out 0 on both.  A row index out of range: MOSAIC_E_ARG, nothing written.  out / status / the row
 * arrays: host or device pointers.  Options: "dist_tile" and "dist_small_work" as for
 * mosaic_st_distance (the same two decisions; no option of its own was measured to be needed);
 * "dist_prune" does not apply: the blocks skipped here are skipped exactly. */
int mosaic_st_intersects(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                         const int64_t* right_row, int64_t n_pairs, uint8_t* out, int32_t* status);
/* the calling thread's last mosaic_st_intersects: pairs ended in the plan kernel (null, row-path, empty
 * or box-disjoint), pairs served by one lane, pairs served by a workgroup (any may be null) */
int mosaic_st_intersects_last_split(int64_t* ended_in_plan, int64_t* one_lane, int64_t* workgroup);
/* out[i] = st_contains(left[left_row[i]], right[right_row[i]]) as 1 or 0 (ST_Contains.scala ->
 * MosaicGeometryJTS.contains -> JTS Geometry.contains, DE-9IM T*****FF*: no point of the right geometry
 * lies in the exterior of the left one and the interiors share a point), for any two of the row kinds
 * mosaic_st_distance serves; left_row == right_row == NULL: row i with row i.  st_within(b, a) is the
 * same call with the sides swapped.  Value and status are those of the sequential definition in
 * mosaic_amd/csrc/st_contains.h, which decides on exact predicates only and constructs no point:
 * 0 when either geometry is empty or the right box is not inside the left box; points against a
 * polygonal or a points-only left side are located one by one; a line or polygon against a polygonal
 * left side is 0 on a proper crossing or an exterior vertex, and decided by first vertices when no
 * facets meet.
 * status[i] (nullable): MOSAIC_ROW_OK: out is the answer.  MOSAIC_ROW_NULL / MOSAIC_ROW_PATH as for
 * mosaic_st_distance, out 0.  MOSAIC_PAIR_UNDECIDED, out 0: both rows are served, but this pair is left
 * to the caller's row-wise expression -- the boundaries touch without crossing and no vertex is
 * outside, or the left side has line parts, or it is points only and the right side is not.  It is a
 * property of the pair, where MOSAIC_ROW_PATH is one of a row.
 * A row index out of range: MOSAIC_E_ARG, nothing written.  out / status / the row arrays: host or
 * device pointers.  Options: "dist_tile" and "dist_small_work" as for mosaic_st_intersects.
 * mosaic_st_contains (polygon contains POINT (x y) from WKB) is untouched. */
#define MOSAIC_PAIR_UNDECIDED 3
int mosaic_st_contains_geoms(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                             const int64_t* right_row, int64_t n_pairs, uint8_t* out, int32_t* status);
/* the calling thread's last mosaic_st_contains_geoms, five counts that add up to its pairs except the
 * last: [0] ended in the plan kernel with a status other than MOSAIC_PAIR_UNDECIDED (null, row-path,
 * empty, box-rejected, or points decided there); [1] served by a later kernel and decided by a proper
 * crossing, an exterior vertex or an exterior point; [2] served by a later kernel and decided without
 * contact, or points all located; [3] MOSAIC_PAIR_UNDECIDED; [4] of all these, served by a workgroup */
int mosaic_st_contains_last_split(int64_t out5[5]);
/* The measures of one geometry per row (ST_Area, ST_Length = ST_Perimeter, ST_Centroid, ST_NumPoints,
 * ST_XMin .. ST_YMax -> MosaicGeometryJTS -> JTS 1.19 getArea / getLength / getCentroid /
 * getNumPoints): output row i describes geoms[rows[i]], rows == NULL: row i (n <= the column's rows).
 * Every output pointer is nullable and only the non-null ones are computed; each may be a host or a
 * device pointer, as may rows.  The values are those of the sequential definition in
 * mosaic_amd/csrc/st_measures.h, bit for bit: area = sum over polygon parts of |shell| - |holes|
 * (lines and points 0.0); length = every ring's and component line's length (a polygon's perimeter;
 * points 0.0); centroid = JTS Centroid (area part, else line part, else the mean of the points);
 * numpoints = the stored vertex count (a closed ring counts its closing vertex); the bounds = the
 * geometry's envelope.  A geometry without a vertex: area 0.0, length 0.0, numpoints 0, centroid and
 * bounds NaN (the reference throws on the bounds).  status[i]: MOSAIC_ROW_OK; MOSAIC_ROW_NULL and
 * MOSAIC_ROW_PATH rows give NaN and numpoints 0.  Line rows are served in a column built with
 * MOSAIC_GEOMS_LINES.  A row index out of range: MOSAIC_E_ARG, nothing written; so is a column whose
 * sizes pass the store's 32-bit offsets.  Options: "meas_wave_min" (stored vertices from which a row
 * takes a wave instead of one lane, default 128) and "meas_tile" (segments per LDS tile of the wave
 * kernel, [1, 256], default 256); neither changes a bit of the result. */
int mosaic_st_measures(mosaic_ctx* ctx, const mosaic_geoms* geoms, const int64_t* rows /*nullable*/, int64_t n,
                       double* area, double* length, double* centroid_x, double* centroid_y, int64_t* numpoints,
                       double* xmin, double* ymin, double* xmax, double* ymax, int32_t* status);
/* the calling thread's last mosaic_st_measures: rows served by one lane, rows served by a wave (either may be null) */
int mosaic_st_measures_last_split(int64_t* one_lane, int64_t* wave);

/* ---- GridRingNeighbours: one iteration of the KNN model (models/knn/GridRingNeighbours.scala:121-160) ---- */
/* The candidates' chips as a map from a cell to its sorted, distinct candidate rows: built once per chip
 * set on the GPU, immutable afterwards and usable from any thread, freed with
 * mosaic_cell_index_destroy.  Chip i is (index_id[i], key[i] = its candidate row >= 0): the rows of
 * grid_tessellateexplode(keepCoreGeometries = false), or one chip per point (Mosaic.pointChip).
 * index_id / key: host or device pointers; at most 2^31 - 1 chips.  A negative key: MOSAIC_E_ARG. */
typedef struct mosaic_cell_index mosaic_cell_index;
int mosaic_cell_index_create(mosaic_ctx* ctx, int64_t n_chips, const int64_t* index_id, const int32_t* key,
                             mosaic_cell_index** out);
/* distinct cells, distinct (cell, candidate) entries, the largest number of candidates in one cell (any may be null) */
int mosaic_cell_index_info(const mosaic_cell_index* index, int64_t* n_cells, int64_t* n_entries, int64_t* max_per_cell);
int mosaic_cell_index_destroy(mosaic_cell_index* index);
/* Row i says that cell[i] belongs to landmark left_row[i] (grid_geometrykringexplode(l, res, 1) in the
 * model's first iteration, grid_geometrykloopexplode(l, res, it) afterwards; duplicate rows allowed;
 * host or device pointers).  The result holds
 *   the pairs: the set of (l, c) such that a given cell of l is the cell of a chip of c, without self
 *     matches unless keep_self -- (l, c) is a self match iff both rows are MOSAIC_ROW_OK and have
 *     identical flat content (the same parts, part kinds and rings, bitwise-equal vertices: an exact
 *     comparison where the reference compares hashes) -- each with distance =
 *     mosaic_st_distance(left[l], right[c]) (NaN where either row is not MOSAIC_ROW_OK: such a pair is
 *     never a self match and sorts after the landmark's numbers), ordered by (l, distance bits, c):
 *     ties by candidate row;
 *   unmatched[l] = 1 iff a given cell of l is the cell of no chip (the left-outer join's null row).
 * The reference's st_intersects_aggregate filter is always true in this join (the left chips are core
 * chips) and is not evaluated.  The rows are those of the sequential definition in
 * mosaic_amd/csrc/ring_neighbours.h.  Every size comes from a count pass: nothing is truncated.
 * Errors, with nothing written: MOSAIC_E_ARG for a landmark row outside `left`, an index naming a row
 * outside `right`, or 2^31 or more rows; MOSAIC_E_CAPACITY for 2^31 or more (landmark, candidate) hits
 * before de-duplication in one call. */
typedef struct mosaic_neighbours mosaic_neighbours;
int mosaic_ring_neighbours(mosaic_ctx* ctx, const mosaic_cell_index* index, const mosaic_geoms* left,
                           const mosaic_geoms* right, const int64_t* left_row, const int64_t* cell, int64_t n,
                           int keep_self, mosaic_neighbours** out);
int mosaic_neighbours_info(const mosaic_neighbours* nb, int64_t* n_pairs, int64_t* n_left);
/* left_row[n_pairs], right_row[n_pairs], distance[n_pairs], unmatched[n_left] (any may be null; host or device) */
int mosaic_neighbours_export(const mosaic_neighbours* nb, int64_t* left_row, int64_t* right_row, double* distance,
                             uint8_t* unmatched);
int mosaic_neighbours_destroy(mosaic_neighbours* nb);
/* Device time (HIP events on the calling thread's stream) of the calling thread's last
 * mosaic_ring_neighbours, ms; split3 (nullable): probe + de-duplication + self-match filter, distance, order. */
double mosaic_ring_neighbours_last_ms(double* split3);

/* ---- the distance-within join: all (landmark, candidate) pairs with st_distance <= radius ---- */
/* Row i asks for landmark left_row[i] with radius[i]; left_row == NULL: rows 0 .. n - 1 of `left`,
 * otherwise strictly ascending rows of `left`.  (l, c) is a pair iff both rows are MOSAIC_ROW_OK, both
 * have at least one facet, radius >= 0 and the bits of mosaic_st_distance(left[l], right[c]) are <=
 * the radius' bits.  An empty geometry is within distance of nothing (mosaic_st_distance's 0.0 for
 * it does not count, as in mosaic_st_intersects); null and row-path rows never pair.  A NaN or
 * negative radius gives its row no pairs; +inf and DBL_MAX accept every eligible candidate; -0.0 is 0.
 * Self matches (as in mosaic_ring_neighbours) are dropped unless keep_self.  The result is a
 * mosaic_neighbours ordered by (l, distance bits, c) whose unmatched[] is all zero:
 * mosaic_neighbours_info / _export / _destroy serve it.  The rows are those of the sequential
 * definition rn::within in mosaic_amd/csrc/ring_neighbours.h, which looks at all pairs.
 * The candidates are found by an envelope filter over all (requested row, candidate row) pairs
 * (k_wn_count / k_wn_emit) that can drop no pair; mosaic_within_candidates returns that filter's own
 * count per requested row -- the eligible candidates c with dist::box_lower_bound(box(l), box(c)) <=
 * radius[i], rn::within_candidates -- so that a caller can size its calls.  left_row / radius /
 * counts: host or device pointers.  Options: "within_tile" (candidate boxes per LDS tile, [1, 1024],
 * default 256) and "within_slices" (slices of the candidate rows, a second grid dimension; 0 =
 * enough to fill the device); neither changes a row.
 * Errors, with nothing written: MOSAIC_E_ARG for a null context (before any device work), for a row
 * outside `left` or rows that are not strictly ascending, for columns of another device, or 2^31 or
 * more rows; MOSAIC_E_CAPACITY for 2^31 or more candidate pairs in one call. */
int mosaic_within_candidates(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right,
                             const int64_t* left_row /*nullable*/, const double* radius, int64_t n, int64_t* counts);
int mosaic_within_neighbours(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right,
                             const int64_t* left_row /*nullable*/, const double* radius, int64_t n, int keep_self,
                             mosaic_neighbours** out);
/* Device time of the calling thread's last mosaic_within_neighbours, ms; split3 (nullable): filter +
 * self-match filter, distance + radius select, order. */
double mosaic_within_neighbours_last_ms(double* split3);

/* getBufferRadius(geometry, res) per geometry (the radius mosaicFill buffers by, core/Mosaic.scala:68):
 * H3 (H3IndexSystem.scala:73-80): the largest distance (degrees) from the centroid of the cell
 * holding the geometry's JTS centroid (its indexToGeometry polygon's JTS centroid) to that polygon's
 * ring points; NaN for a geometry without area.  BNG (BNGIndexSystem.scala:146-149): edge * sqrt(2) / 2.
 * Geometries in the flat-ring layout of mosaic_polyfill; out[n_geoms]. */
int mosaic_buffer_radius(mosaic_ctx* ctx, int grid, int res, int64_t n_geoms, const int64_t* geom_parts,
                         const int64_t* part_rings, const int64_t* ring_offsets, const double* xy, double* out);

/* Execution state of the calling thread on ctx (its device, stream, the "jdk" option and the
 * device's CU count), for the library's own translation units. */
int mosaic_ctx_exec(mosaic_ctx* ctx, int* device, void** stream, int* jdk, int* n_cu);

/* ---- grid_boundaryaswkb over a cell column (BNG) ---- */
/* out[93 i .. 93 i + 92] = the WKB JTS writes for BNGIndexSystem.indexToGeometry(ids[i])
 * (core/index/BNGIndexSystem.scala indexToGeometry; functions/MosaicContext.scala
 * grid_boundaryaswkb -> expressions/index/IndexGeometry.scala:65-75): big-endian 2D Polygon of the
 * cell square, 5 points.  Null rows (valid[i] == 0) are left zero.  H3 cells are served by
 * mosaic_h3_cell_geometry mode 2 (variable-length rings); with grid H3 this entry returns
 * MOSAIC_E_ARG. */
int mosaic_cell_boundary_wkb(mosaic_ctx* ctx, int grid, const int64_t* ids, const uint8_t* valid, int64_t n,
                             uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif
