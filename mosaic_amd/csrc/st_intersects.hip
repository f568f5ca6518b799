// st_intersects over device-resident geometry columns (mosaic_st_intersects): JTS Geometry.intersects
// for Point / MultiPoint / LineString / MultiLineString / Polygon / MultiPolygon rows on (left row,
// right row) pairs -- the public ST_Intersects (expressions/geometry/ST_Intersects.scala ->
// MosaicGeometryJTS.intersects) and the flat side of the reference's check of st_intersects_aggregate
// (ST_IntersectsBehaviors.scala:45-68).  st_intersects.h holds the semantics and the sequential driver
// whose value these kernels return; the columns are those of st_distance.hip.
//
// Per call:
//   k_isect_plan   one lane per pair: row range check and row status as in k_dist_plan, then steps 1
//                  and 2 of the definition (a side without facets, geometry boxes that do not meet):
//                  such a pair is false and ends here.  The others go by facets(left) x facets(right)
//                  to the front (<= dist_small_work) or the back of one list.
//   k_isect_fill   status[] of every pair and out = 0 (only after the host has seen that no row index
//                  was out of range: such a call writes nothing)
//   k_isect_small  one lane per pair: the sequential driver isect::intersects
//   k_isect_block  one workgroup per pair.  The side with fewer facets is staged in LDS, a tile of
//                  dist_tile segments at a time; the other side's segments are streamed across the
//                  lanes.  A staged ring, a tile, a (tile, streamed ring) or a (tile, streamed segment)
//                  block whose boxes do not meet is skipped: segments inside disjoint boxes share no
//                  point, so nothing is bounded or snapshotted.  A hit sets an LDS flag that every lane
//                  reads before each streamed segment and the workgroup reads at every tile; it ends
//                  the pair.  Only if no facets met does containment run: one wave per (polygon part,
//                  component, direction) task, the component's first vertex located by the
//                  wave-cooperative locate of pip_coop.h (its flags per segment are those of
//                  pip::locate_in_ring, see that header), until a task hits.
#include "dev_rt.h"
#include "geoms_device.h"
#include "pair_lists.h"
#include "pip_coop.h"
#include "st_intersects.h"

using namespace mosaic;

namespace {

using dev::blocks_for;
using dev::Buf;
using dev::is_device_ptr;
using pairs::Col;
using pairs::kBlock;
using pairs::view;
using pairs::wave_append;
constexpr int kMaxTile = 1024;
constexpr int kWaves = kBlock / 64;

// the last call of this thread: pairs ended in the plan kernel, on the one-lane list, on the workgroup list
thread_local int64_t t_last[3] = {0, 0, 0};

struct PlanArgs {
    Col L, R;
    const int64_t *lrow, *rrow;  // both null: pair i is (row i, row i)
    int64_t n;
    unsigned long long small_work;
    int32_t* plan;               // the pair's status
    int64_t* list;               // small pairs from the front, block pairs from the back
    unsigned long long* counts;  // [0] small, [1] block, [2] row indices out of range
};

__global__ void __launch_bounds__(kBlock) k_isect_plan(PlanArgs a) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool small = false, block = false;
        if (i < a.n) {
            const int64_t g = a.lrow ? a.lrow[i] : i, h = a.rrow ? a.rrow[i] : i;
            if (g < 0 || g >= a.L.n || h < 0 || h >= a.R.n) {
                atomicAdd(&a.counts[2], 1ull);
                a.plan[i] = -1;
            } else {
                const int32_t sl = a.L.status[g], sr = a.R.status[h];
                int32_t st = MOSAIC_ROW_OK;
                if (sl == MOSAIC_ROW_NULL || sr == MOSAIC_ROW_NULL)
                    st = MOSAIC_ROW_NULL;
                else if (sl != MOSAIC_ROW_OK || sr != MOSAIC_ROW_OK)
                    st = MOSAIC_ROW_PATH;
                a.plan[i] = st;
                if (st == MOSAIC_ROW_OK) {
                    const unsigned long long work = (unsigned long long)a.L.facets[g] * a.R.facets[h];
                    // steps 1 and 2 of the definition: false, and the pair reaches no other kernel
                    if (work != 0 && pip::boxes_meet(a.L.s.geom_bbox[g], a.R.s.geom_bbox[h])) {
                        small = work <= a.small_work;
                        block = !small;
                    }
                }
            }
        }
        const unsigned long long ps = wave_append(&a.counts[0], small);
        const unsigned long long pb = wave_append(&a.counts[1], block);
        if (small) a.list[ps] = i;
        if (block) a.list[a.n - 1 - (int64_t)pb] = i;
    }
}

__global__ void __launch_bounds__(kBlock) k_isect_fill(const int32_t* plan, int64_t n, uint8_t* out, int32_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (status) status[i] = plan[i];
        out[i] = 0;
    }
}

struct IsectArgs {
    Col L, R;
    const int64_t *lrow, *rrow;
    const int64_t* list;
    int64_t n_list;
    uint8_t* out;
    int tile;
};

__global__ void __launch_bounds__(kBlock) k_isect_small(IsectArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n_list; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = a.list[k];
        const uint32_t g = (uint32_t)(a.lrow ? a.lrow[i] : i), h = (uint32_t)(a.rrow ? a.rrow[i] : i);
        a.out[i] = isect::intersects(a.L.s, a.L.part_kind, g, a.R.s, a.R.part_kind, h) ? 1 : 0;
    }
}

// dist::component_in_part with the locate spread over the calling wave (p, q wave-uniform): the
// first coordinate of part q's shell lies in or on polygon part p
__device__ inline bool coop_component_in_part(const pip::GeomStore& sp, uint32_t p, const pip::GeomStore& sq, uint32_t q) {
    const uint32_t r = sq.part_ring[q];
    if (sq.part_ring[q + 1] <= r || sq.ring_start[r + 1] <= sq.ring_start[r]) return false;
    const pip::Vec2 pt = sq.verts[sq.ring_start[r]];
    return pip::coop_locate_in_polygon(sp, p, pt.x, pt.y) != pip::LOC_EXTERIOR;
}

__global__ void __launch_bounds__(kBlock) k_isect_block(IsectArgs a) {
    __shared__ pip::Vec2 s_v[kMaxTile + 1];
    __shared__ pip::Box s_box;
    __shared__ int s_hit, s_snap;
    const uint32_t tid = threadIdx.x;
    const uint32_t T = (uint32_t)a.tile;
    for (int64_t k = blockIdx.x; k < a.n_list; k += gridDim.x) {
        const int64_t i = a.list[k];
        const uint32_t g = (uint32_t)(a.lrow ? a.lrow[i] : i), h = (uint32_t)(a.rrow ? a.rrow[i] : i);
        // S: the staged side (fewer facets), W: the streamed side; flip: S is the right geometry
        const bool flip = a.L.facets[g] > a.R.facets[h];
        const Col& CS = flip ? a.R : a.L;
        const Col& CW = flip ? a.L : a.R;
        const pip::GeomStore& S = CS.s;
        const pip::GeomStore& W = CW.s;
        const uint32_t gs = flip ? h : g, gw = flip ? g : h;
        __syncthreads();  // the previous pair's readers of s_hit are done
        if (tid == 0) s_hit = 0;
        // ---- facets ----
        uint32_t rs0, rs1, rw0, rw1;
        dist::geom_rings(S, gs, rs0, rs1);
        dist::geom_rings(W, gw, rw0, rw1);
        const pip::Box wbox = W.geom_bbox[gw];
        bool done = false;
        for (uint32_t rs = rs0; rs < rs1 && !done; rs++) {
            const uint32_t v0 = S.ring_start[rs], n = S.ring_start[rs + 1] - v0;
            const uint32_t nf = dist::ring_facets(n);
            if (nf == 0 || !pip::boxes_meet(S.ring_bbox[rs], wbox)) continue;  // uniform
            for (uint32_t f0 = 0; f0 < nf; f0 += T) {
                const uint32_t cnt = nf - f0 < T ? nf - f0 : T;
                __syncthreads();  // the previous tile's readers of s_v / s_box / s_snap are done; s_hit = 0 is visible
                for (uint32_t t = tid; t <= cnt; t += kBlock) {
                    const uint32_t vi = f0 + t < n ? f0 + t : n - 1;
                    s_v[t] = S.verts[v0 + vi];
                }
                if (tid == 0) s_snap = *(volatile int*)&s_hit;
                __syncthreads();
                if (s_snap) {  // uniform: a hit ends the pair
                    done = true;
                    break;
                }
                if (tid < 64) {
                    pip::Box b = {INFINITY, INFINITY, -INFINITY, -INFINITY};
                    for (uint32_t t = tid; t <= cnt; t += 64) {
                        const pip::Vec2 v = s_v[t];
                        b.minx = fmin(b.minx, v.x);
                        b.miny = fmin(b.miny, v.y);
                        b.maxx = fmax(b.maxx, v.x);
                        b.maxy = fmax(b.maxy, v.y);
                    }
                    for (int off = 32; off; off >>= 1) {
                        b.minx = fmin(b.minx, __shfl_xor(b.minx, off, 64));
                        b.miny = fmin(b.miny, __shfl_xor(b.miny, off, 64));
                        b.maxx = fmax(b.maxx, __shfl_xor(b.maxx, off, 64));
                        b.maxy = fmax(b.maxy, __shfl_xor(b.maxy, off, 64));
                    }
                    if (tid == 0) s_box = b;
                }
                __syncthreads();
                const pip::Box tb = s_box;
                if (!pip::boxes_meet(tb, wbox)) continue;  // uniform
                for (uint32_t rw = rw0; rw < rw1; rw++) {
                    const uint32_t w0 = W.ring_start[rw], nw = W.ring_start[rw + 1] - w0;
                    const uint32_t nfw = dist::ring_facets(nw);
                    if (nfw == 0 || !pip::boxes_meet(tb, W.ring_bbox[rw])) continue;
                    for (uint32_t j = tid; j < nfw; j += kBlock) {
                        if (*(volatile int*)&s_hit) break;
                        pip::Vec2 C, D;
                        dist::ring_facet(W.verts + w0, nw, j, C, D);
                        if (!pip::boxes_meet(tb, isect::facet_box(C, D))) continue;
                        bool hit = false;
                        if (flip) {
                            for (uint32_t t = 0; t < cnt && !hit; t++) hit = pip::segments_intersect(C, D, s_v[t], s_v[t + 1]);
                        } else {
                            for (uint32_t t = 0; t < cnt && !hit; t++) hit = pip::segments_intersect(s_v[t], s_v[t + 1], C, D);
                        }
                        if (hit) {
                            s_hit = 1;
                            break;
                        }
                    }
                }
            }
        }
        __syncthreads();
        const bool facets_met = s_hit != 0;  // uniform: every write of the facet phase is behind the barrier,
        __syncthreads();                     // and no containment task writes before every thread has read
        // ---- containment, only if no facets met: (polygon part p of one side, component q of the other), both directions ----
        if (!facets_met) {
            const uint32_t ps0 = S.geom_part[gs], nps = S.geom_part[gs + 1] - ps0;
            const uint32_t pw0 = W.geom_part[gw], npw = W.geom_part[gw + 1] - pw0;
            const uint64_t tasks = 2ull * nps * npw;
            for (uint64_t t = tid >> 6; t < tasks; t += kWaves) {
                if (__any(*(volatile int*)&s_hit)) break;
                const uint64_t u = t >> 1;
                const uint32_t p = ps0 + (uint32_t)(u / npw), q = pw0 + (uint32_t)(u % npw);
                bool hit;
                if (t & 1)
                    hit = CW.part_kind[q] == kPartPolygon && coop_component_in_part(W, q, S, p);
                else
                    hit = CS.part_kind[p] == kPartPolygon && coop_component_in_part(S, p, W, q);
                if (hit && (tid & 63) == 0) s_hit = 1;
            }
            __syncthreads();
        }
        if (tid == 0) a.out[i] = s_hit ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int mosaic_st_intersects(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                         const int64_t* right_row, int64_t n_pairs, uint8_t* out, int32_t* status) {
    if (!ctx || !left || !right || n_pairs < 0 || (n_pairs > 0 && !out))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    if ((left_row == nullptr) != (right_row == nullptr))
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_intersects: left_row and right_row are both given or both null");
    if (!left_row && (n_pairs > left->n_geoms || n_pairs > right->n_geoms))
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_intersects: row-wise form with more pairs than rows");
    int tile = 16, prune = 1;
    int64_t small_work = 512;
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    MOSAIC_RC(mosaic_ctx_dist_options(ctx, &tile, &small_work, &prune));
    if (left->device != ex.device || right->device != ex.device)
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_intersects: a geometry column of another device");
    t_last[0] = t_last[1] = t_last[2] = 0;
    if (n_pairs == 0) return MOSAIC_OK;
    tile = std::max(1, std::min(tile, kMaxTile));
    hipStream_t stream = ex.stream;
    const int64_t n = n_pairs;

    Buf s_lrow, s_rrow, s_plan, s_list, s_counts, s_out, s_status;
    PlanArgs pa{view(left), view(right), nullptr, nullptr, n, (unsigned long long)std::max<int64_t>(small_work, 0), nullptr, nullptr, nullptr};
    if (left_row) {
        MOSAIC_RC(dev::on_device(left_row, n, s_lrow, stream, &pa.lrow));
        MOSAIC_RC(dev::on_device(right_row, n, s_rrow, stream, &pa.rrow));
    }
    MOSAIC_RC(s_plan.reserve((size_t)n * sizeof(int32_t)));
    MOSAIC_RC(s_list.reserve((size_t)n * sizeof(int64_t)));
    MOSAIC_RC(s_counts.reserve(4 * sizeof(unsigned long long)));
    MOSAIC_HIP(hipMemsetAsync(s_counts.p, 0, 4 * sizeof(unsigned long long), stream));
    pa.plan = (int32_t*)s_plan.p;
    pa.list = (int64_t*)s_list.p;
    pa.counts = (unsigned long long*)s_counts.p;
    const int64_t wide = (int64_t)ex.n_cu * 16;
    hipLaunchKernelGGL(k_isect_plan, dim3((unsigned)blocks_for(n, kBlock, wide)), dim3(kBlock), 0, stream, pa);
    MOSAIC_HIP(hipGetLastError());
    unsigned long long counts[4] = {0, 0, 0, 0};
    MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, sizeof(counts), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    if (counts[2])
        return mosaic_tess_fail(MOSAIC_E_ARG, ("st_intersects: " + std::to_string(counts[2]) + " pair(s) name a row outside their column").c_str());

    const bool dev_out = is_device_ptr(out), dev_status = !status || is_device_ptr(status);
    uint8_t* d_out = out;
    int32_t* d_status = status;
    if (!dev_out) {
        MOSAIC_RC(s_out.reserve((size_t)n));
        d_out = (uint8_t*)s_out.p;
    }
    if (!dev_status) {
        MOSAIC_RC(s_status.reserve((size_t)n * sizeof(int32_t)));
        d_status = (int32_t*)s_status.p;
    }
    hipLaunchKernelGGL(k_isect_fill, dim3((unsigned)blocks_for(n, kBlock, wide)), dim3(kBlock), 0, stream, pa.plan, n, d_out, d_status);
    MOSAIC_HIP(hipGetLastError());
    IsectArgs ia{pa.L, pa.R, pa.lrow, pa.rrow, pa.list, (int64_t)counts[0], d_out, tile};
    if (counts[0]) {
        hipLaunchKernelGGL(k_isect_small, dim3((unsigned)blocks_for((int64_t)counts[0], kBlock, wide)), dim3(kBlock), 0, stream, ia);
        MOSAIC_HIP(hipGetLastError());
    }
    if (counts[1]) {
        ia.list = pa.list + (n - (int64_t)counts[1]);
        ia.n_list = (int64_t)counts[1];
        hipLaunchKernelGGL(k_isect_block, dim3((unsigned)std::min<int64_t>(ia.n_list, (int64_t)1 << 20)), dim3(kBlock), 0, stream, ia);
        MOSAIC_HIP(hipGetLastError());
    }
    if (!dev_out) MOSAIC_HIP(hipMemcpyAsync(out, d_out, (size_t)n, hipMemcpyDeviceToHost, stream));
    if (!dev_status) MOSAIC_HIP(hipMemcpyAsync(status, d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    t_last[0] = n - (int64_t)counts[0] - (int64_t)counts[1];
    t_last[1] = (int64_t)counts[0];
    t_last[2] = (int64_t)counts[1];
    return MOSAIC_OK;
}

int mosaic_st_intersects_last_split(int64_t* ended_in_plan, int64_t* one_lane, int64_t* workgroup) {
    if (ended_in_plan) *ended_in_plan = t_last[0];
    if (one_lane) *one_lane = t_last[1];
    if (workgroup) *workgroup = t_last[2];
    return MOSAIC_OK;
}

}  // extern "C"
