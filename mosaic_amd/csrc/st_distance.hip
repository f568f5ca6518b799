// st_distance over device-resident geometry columns (mosaic_geoms_*, mosaic_st_distance): JTS
// Geometry.distance for Point / MultiPoint / LineString / MultiLineString / Polygon / MultiPolygon
// rows, on (left row, right row)
// pairs -- step 3 of the reference's KNN iteration (models/knn/GridRingNeighbours.scala:153-156) and
// the public ST_Distance (expressions/geometry/ST_Distance.scala:34-36).  st_distance.h holds the
// semantics, the arithmetic and the sequential driver whose bits these kernels return.
//
// A column is the GeomStore layout of pip_device.h in HBM plus a kind per part (point / polygon /
// line), a facet count per geometry and a status per row; it is immutable after creation.  A line
// part is one open ring: dist::ring_facets gives it n - 1 segments, a tile stages the vertices of its
// own segments only (the index is clamped to the ring's last vertex), so no kernel forms a closing
// segment, and only polygon parts are containers.
//
// Per call:
//   k_dist_plan    one lane per pair: row range check and row status (pairs::plan_status), work =
//                  facets(left) x facets(right); pair ids with work <= dist_small_work are appended to the
//                  front of one list, the others to its back (pairs::plan_append: one atomicAdd per wave
//                  and list)
//   k_dist_fill    status[] of every pair, NaN for the null / row-path ones (only after the host has
//                  seen that no row index was out of range: such a call writes nothing)
//   k_dist_small   one lane per pair: the sequential driver dist::distance (with the part kinds)
//   k_dist_block   one workgroup per pair.  Containment first, one lane per (polygon part, component)
//                  and direction; a component is a point, a line part or a polygon's shell, located
//                  by its first vertex.  Then the side with fewer facets is staged in LDS, a tile of
//                  dist_tile segments at a time (pairs::stage_tile, pairs::tile_box), and the other side's
//                  segments are streamed across the lanes, each lane keeping a running minimum (its own
//                  loop: pairs::sweep_tiles prunes by boxes meeting).  The workgroup's current minimum lives
//                  in LDS as the bit pattern of a non-negative double (integer atomicMin); a
//                  (tile, streamed geometry), (tile, streamed ring) or (tile, streamed segment) block is
//                  skipped only when dist::box_lower_bound of it is strictly greater than that minimum,
//                  and a minimum of 0 ends the pair.  The lanes' minima are reduced within each wave by
//                  shuffles, then across the waves through LDS.
#include <memory>

#include "geoms_build.h"
#include "geoms_device.h"
#include "pair_call.h"
#include "st_distance.h"

using namespace mosaic;

namespace {

using dev::blocks_for;
using dev::Buf;
using pairs::kBlock;
using pairs::kMaxTile;

// a point column built on the device: row i is the point part (x[i], y[i]); a NaN coordinate is POINT EMPTY
__global__ void __launch_bounds__(kBlock) k_points_col(const double* x, const double* y, int64_t n, pip::Vec2* verts,
                                                       uint32_t* ring_start, pip::Box* ring_bbox, uint32_t* part_ring,
                                                       uint8_t* part_kind, uint32_t* geom_part, pip::Box* geom_bbox,
                                                       uint32_t* facets, int32_t* status, unsigned long long* n_path) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 <= n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool path = false;
        if (i <= n) {
            ring_start[i] = (uint32_t)i;
            part_ring[i] = (uint32_t)i;
            geom_part[i] = (uint32_t)i;
        }
        if (i < n) {
            const double px = x[i], py = y[i];
            path = px != px || py != py;
            verts[i] = pip::Vec2{px, py};
            ring_bbox[i] = pip::Box{px, py, px, py};
            geom_bbox[i] = pip::Box{px, py, px, py};
            part_kind[i] = kPartPoint;
            facets[i] = 1;
            status[i] = path ? MOSAIC_ROW_PATH : MOSAIC_ROW_OK;
        }
        const unsigned long long m = __ballot(path);
        if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(n_path, (unsigned long long)__popcll(m));
    }
}

__global__ void __launch_bounds__(kBlock) k_dist_plan(pairs::PlanArgs a) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool small = false, block = false;
        if (i < a.n) {
            int64_t g, h;
            const int32_t st = pairs::plan_status(a, i, g, h);
            a.plan[i] = st;
            if (st == MOSAIC_ROW_OK) {
                const unsigned long long work = (unsigned long long)a.L.facets[g] * a.R.facets[h];
                small = work <= a.small_work;
                block = !small;
            }
        }
        pairs::plan_append(a, i, small, block);
    }
}

__global__ void __launch_bounds__(kBlock) k_dist_fill(const int32_t* plan, int64_t n, double* out, int32_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t st = plan[i];
        if (status) status[i] = st;
        if (st != MOSAIC_ROW_OK) out[i] = __longlong_as_double(0x7ff8000000000000LL);
    }
}

struct DistArgs : pairs::ListArgs {
    double* out;
    int tile;
    int prune;
};

__global__ void __launch_bounds__(kBlock) k_dist_small(DistArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n_list; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = a.list[k];
        uint32_t g, h;
        pairs::pair_rows(a, i, g, h);
        a.out[i] = dist::distance(a.L.s, a.L.part_kind, g, a.R.s, a.R.part_kind, h);
    }
}

__device__ inline double lds_min(const unsigned long long* p) {
    return __longlong_as_double((long long)*(const volatile unsigned long long*)p);
}

__global__ void __launch_bounds__(kBlock) k_dist_block(DistArgs a) {
    __shared__ pip::Vec2 s_v[kMaxTile + 1];
    __shared__ pip::Box s_box;
    __shared__ unsigned long long s_min, s_snap;
    __shared__ int s_hit;
    __shared__ double s_wave[kBlock / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t T = (uint32_t)a.tile;
    for (int64_t k = blockIdx.x; k < a.n_list; k += gridDim.x) {
        const int64_t i = a.list[k];
        uint32_t g, h;
        pairs::pair_rows(a, i, g, h);
        // S: the staged side (fewer facets), W: the streamed side; flip: S is the right geometry
        const bool flip = a.L.facets[g] > a.R.facets[h];
        const pairs::Col& CS = flip ? a.R : a.L;
        const pairs::Col& CW = flip ? a.L : a.R;
        const pip::GeomStore& S = CS.s;
        const pip::GeomStore& W = CW.s;
        const uint32_t gs = flip ? h : g, gw = flip ? g : h;
        __syncthreads();  // the previous pair's readers of s_hit / s_wave are done
        if (tid == 0) {
            s_hit = 0;
            s_min = (unsigned long long)__double_as_longlong(INFINITY);
        }
        __syncthreads();
        // ---- containment: (polygon part p of one side, component q of the other), both directions ----
        {
            const uint32_t ps0 = S.geom_part[gs], nps = S.geom_part[gs + 1] - ps0;
            const uint32_t pw0 = W.geom_part[gw], npw = W.geom_part[gw + 1] - pw0;
            const uint64_t tasks = 2ull * nps * npw;
            for (uint64_t t = tid; t < tasks; t += kBlock) {
                if (*(volatile int*)&s_hit) break;
                const uint64_t u = t >> 1;
                const uint32_t p = ps0 + (uint32_t)(u / npw), q = pw0 + (uint32_t)(u % npw);
                bool hit;
                if (t & 1)
                    hit = CW.part_kind[q] == kPartPolygon && dist::component_in_part(W, q, S, p);
                else
                    hit = CS.part_kind[p] == kPartPolygon && dist::component_in_part(S, p, W, q);
                if (hit) s_hit = 1;
            }
        }
        __syncthreads();
        if (s_hit) {  // uniform
            if (tid == 0) a.out[i] = 0.0;
            continue;
        }
        // ---- facets ----
        uint32_t rs0, rs1, rw0, rw1;
        dist::geom_rings(S, gs, rs0, rs1);
        dist::geom_rings(W, gw, rw0, rw1);
        const pip::Box wbox = W.geom_bbox[gw];
        double m = INFINITY;
        bool done = false;
        for (uint32_t rs = rs0; rs < rs1 && !done; rs++) {
            const uint32_t v0 = S.ring_start[rs], n = S.ring_start[rs + 1] - v0;
            const uint32_t nf = dist::ring_facets(n);
            for (uint32_t f0 = 0; f0 < nf; f0 += T) {
                const uint32_t cnt = nf - f0 < T ? nf - f0 : T;
                __syncthreads();  // the previous tile's readers of s_v / s_box are done
                pairs::stage_tile(s_v, S.verts + v0, n, f0, cnt);
                if (tid == 0) s_snap = s_min;
                __syncthreads();
                if (s_snap == 0) {  // uniform: a zero ends the pair
                    done = true;
                    break;
                }
                pairs::tile_box(s_v, cnt, &s_box);
                __syncthreads();
                const pip::Box tb = s_box;
                if (a.prune && dist::box_lower_bound(tb, wbox) > __longlong_as_double((long long)s_snap)) continue;  // uniform
                for (uint32_t rw = rw0; rw < rw1; rw++) {
                    const uint32_t w0 = W.ring_start[rw], nw = W.ring_start[rw + 1] - w0;
                    const uint32_t nfw = dist::ring_facets(nw);
                    if (a.prune && dist::box_lower_bound(tb, W.ring_bbox[rw]) > lds_min(&s_min)) continue;
                    for (uint32_t j = tid; j < nfw; j += kBlock) {
                        pip::Vec2 C, D;
                        dist::ring_facet(W.verts + w0, nw, j, C, D);
                        const double cur = lds_min(&s_min);
                        if (cur == 0) break;
                        if (a.prune && dist::box_lower_bound(tb, dist::facet_box(C, D)) > cur) continue;
                        double mm = m;
                        if (flip) {
                            for (uint32_t t = 0; t < cnt; t++) mm = dist::min2(mm, dist::segment_segment(C, D, s_v[t], s_v[t + 1]));
                        } else {
                            for (uint32_t t = 0; t < cnt; t++) mm = dist::min2(mm, dist::segment_segment(s_v[t], s_v[t + 1], C, D));
                        }
                        if (mm < m) {
                            m = mm;
                            atomicMin(&s_min, (unsigned long long)__double_as_longlong(m));
                        }
                    }
                }
            }
        }
        // ---- the lanes' minima: within the wave by shuffles, across the waves through LDS ----
        for (int off = 32; off; off >>= 1) m = dist::min2(m, __shfl_xor(m, off, 64));
        if ((tid & 63) == 0) s_wave[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            double r = s_wave[0];
            for (int w = 1; w < kBlock / 64; w++) r = dist::min2(r, s_wave[w]);
            a.out[i] = r;
        }
    }
}

template <class T>
int upload(T** dst, const std::vector<T>& src) {
    MOSAIC_HIP(hipMalloc((void**)dst, std::max<size_t>(src.size() * sizeof(T), 16)));
    if (!src.empty()) MOSAIC_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return MOSAIC_OK;
}

int upload_column(int device, const GeomColumn& c, mosaic_geoms** out) {
    if (c.too_large()) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry column: 2^32 - 1 vertices or rows at the most");
    std::unique_ptr<mosaic_geoms> g(new mosaic_geoms());
    g->device = device;
    g->n_geoms = c.size();
    g->n_vertices = (int64_t)c.b.verts.size();
    g->n_row_path = c.n_row_path;
    MOSAIC_RC(upload(&g->verts, c.b.verts));
    MOSAIC_RC(upload(&g->ring_start, c.b.ring_start));
    MOSAIC_RC(upload(&g->ring_bbox, c.b.ring_bbox));
    MOSAIC_RC(upload(&g->part_ring, c.b.part_ring));
    MOSAIC_RC(upload(&g->part_kind, c.part_kind));
    MOSAIC_RC(upload(&g->geom_part, c.b.geom_part));
    MOSAIC_RC(upload(&g->geom_bbox, c.b.geom_bbox));
    MOSAIC_RC(upload(&g->geom_facets, c.geom_facets));
    MOSAIC_RC(upload(&g->row_status, c.row_status));
    *out = g.release();
    return MOSAIC_OK;
}

}  // namespace

extern "C" {

uint64_t mosaic_layout_st_distance(void) { return dist::layout_fingerprint(); }

int mosaic_geoms_create_wkb_ex(mosaic_ctx* ctx, int64_t n, const int64_t* offsets, const uint8_t* wkb, const uint8_t* valid,
                               uint32_t flags, mosaic_geoms** out) {
    if (!ctx || !out || n < 0 || (n > 0 && (!offsets || !wkb))) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (flags & ~(uint32_t)MOSAIC_GEOMS_LINES) return mosaic_tess_fail(MOSAIC_E_ARG, "geometry column: unknown flag");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    GeomColumn c;
    c.lines = (flags & MOSAIC_GEOMS_LINES) != 0;
    for (int64_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return mosaic_tess_fail(MOSAIC_E_ARG, "geometry column: offsets decrease");
        if (valid && !valid[i])
            c.add_empty(kRowNull);
        else
            c.add_wkb(wkb + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    }
    return upload_column(ex.device, c, out);
}

int mosaic_geoms_create_wkb(mosaic_ctx* ctx, int64_t n, const int64_t* offsets, const uint8_t* wkb, const uint8_t* valid,
                            mosaic_geoms** out) {
    return mosaic_geoms_create_wkb_ex(ctx, n, offsets, wkb, valid, 0, out);
}

int mosaic_geoms_create_lines(mosaic_ctx* ctx, int64_t n, const int64_t* geom_lines, const int64_t* line_offsets,
                              const double* xy, mosaic_geoms** out) {
    if (!ctx || !out || n < 0 || !geom_lines || (n > 0 && !line_offsets)) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (geom_lines[0] != 0) return mosaic_tess_fail(MOSAIC_E_ARG, "geometry column: inconsistent offsets");
    for (int64_t g = 0; g < n; g++)
        if (geom_lines[g + 1] < geom_lines[g]) return mosaic_tess_fail(MOSAIC_E_ARG, "geometry column: inconsistent offsets");
    if (geom_lines[n] > 0 && !xy) return mosaic_tess_fail(MOSAIC_E_ARG, "geometry column: inconsistent offsets");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    GeomColumn c;
    c.lines = true;
    if (!c.add_lines(n, geom_lines, line_offsets, xy)) return mosaic_tess_fail(MOSAIC_E_ARG, "geometry column: inconsistent offsets");
    return upload_column(ex.device, c, out);
}

int mosaic_geoms_create_arrays(mosaic_ctx* ctx, int64_t n, const int64_t* geom_parts, const int64_t* part_rings,
                               const int64_t* ring_offsets, const double* xy, mosaic_geoms** out) {
    if (!ctx || !out || n < 0 || !geom_parts || (n > 0 && (!part_rings || !ring_offsets)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    GeomColumn c;
    if (geom_parts[0] != 0 || !c.add_arrays(n, geom_parts, part_rings, ring_offsets, xy))
        return mosaic_tess_fail(MOSAIC_E_ARG, "geometry column: inconsistent offsets");
    return upload_column(ex.device, c, out);
}

int mosaic_geoms_create_points(mosaic_ctx* ctx, const double* x, const double* y, int64_t n, mosaic_geoms** out) {
    if (!ctx || !out || n < 0 || (n > 0 && (!x || !y))) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (n >= 0xffffffffLL) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry column: 2^32 - 1 vertices or rows at the most");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    hipStream_t stream = ex.stream;
    std::unique_ptr<mosaic_geoms> g(new mosaic_geoms());
    g->device = ex.device;
    g->n_geoms = n;
    g->n_vertices = n;
    const size_t n1 = (size_t)n + 1;
    MOSAIC_HIP(hipMalloc((void**)&g->verts, n1 * sizeof(pip::Vec2)));
    MOSAIC_HIP(hipMalloc((void**)&g->ring_start, n1 * sizeof(uint32_t)));
    MOSAIC_HIP(hipMalloc((void**)&g->ring_bbox, n1 * sizeof(pip::Box)));
    MOSAIC_HIP(hipMalloc((void**)&g->part_ring, n1 * sizeof(uint32_t)));
    MOSAIC_HIP(hipMalloc((void**)&g->part_kind, n1));
    MOSAIC_HIP(hipMalloc((void**)&g->geom_part, n1 * sizeof(uint32_t)));
    MOSAIC_HIP(hipMalloc((void**)&g->geom_bbox, n1 * sizeof(pip::Box)));
    MOSAIC_HIP(hipMalloc((void**)&g->geom_facets, n1 * sizeof(uint32_t)));
    MOSAIC_HIP(hipMalloc((void**)&g->row_status, n1 * sizeof(int32_t)));
    Buf sx, sy, cnt;
    const double *dx = nullptr, *dy = nullptr;
    if (n > 0) {
        MOSAIC_RC(dev::on_device(x, n, sx, stream, &dx));
        MOSAIC_RC(dev::on_device(y, n, sy, stream, &dy));
    }
    MOSAIC_RC(cnt.reserve(sizeof(unsigned long long)));
    MOSAIC_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_points_col, dim3((unsigned)blocks_for(n + 1, kBlock, (int64_t)ex.n_cu * 16)), dim3(kBlock), 0, stream, dx, dy, n,
                       g->verts, g->ring_start, g->ring_bbox, g->part_ring, g->part_kind, g->geom_part, g->geom_bbox,
                       g->geom_facets, g->row_status, (unsigned long long*)cnt.p);
    MOSAIC_HIP(hipGetLastError());
    unsigned long long n_path = 0;
    MOSAIC_HIP(hipMemcpyAsync(&n_path, cnt.p, sizeof(n_path), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    g->n_row_path = (int64_t)n_path;
    *out = g.release();
    return MOSAIC_OK;
}

int mosaic_geoms_info(const mosaic_geoms* g, int64_t* n_geoms, int64_t* n_vertices, int64_t* n_row_path) {
    if (!g) return mosaic_tess_fail(MOSAIC_E_ARG, "null geometry column");
    if (n_geoms) *n_geoms = g->n_geoms;
    if (n_vertices) *n_vertices = g->n_vertices;
    if (n_row_path) *n_row_path = g->n_row_path;
    return MOSAIC_OK;
}

int mosaic_geoms_destroy(mosaic_geoms* g) {
    if (!g) return MOSAIC_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return MOSAIC_OK;
}

int mosaic_st_distance(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                       const int64_t* right_row, int64_t n_pairs, double* out, int32_t* status) {
    pairs::Call<double> c;
    MOSAIC_RC(c.open("st_distance", ctx, left, right, left_row, right_row, n_pairs, out));
    if (n_pairs == 0) return MOSAIC_OK;
    MOSAIC_RC(c.stage(4));
    hipLaunchKernelGGL(k_dist_plan, c.lanes(c.n), dim3(kBlock), 0, c.stream, c.pa);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_RC(c.planned());
    MOSAIC_RC(c.bind(out, status));
    hipLaunchKernelGGL(k_dist_fill, c.lanes(c.n), dim3(kBlock), 0, c.stream, c.pa.plan, c.n, c.out.dev, c.status.dev);
    MOSAIC_HIP(hipGetLastError());
    if (c.n_small()) {
        hipLaunchKernelGGL(k_dist_small, c.lanes(c.n_small()), dim3(kBlock), 0, c.stream, DistArgs{c.small_list(), c.out.dev, c.tile, c.prune});
        MOSAIC_HIP(hipGetLastError());
    }
    if (c.n_block()) {
        hipLaunchKernelGGL(k_dist_block, c.groups(c.n_block()), dim3(kBlock), 0, c.stream, DistArgs{c.block_list(), c.out.dev, c.tile, c.prune});
        MOSAIC_HIP(hipGetLastError());
    }
    return c.finish(false);
}

}  // extern "C"
