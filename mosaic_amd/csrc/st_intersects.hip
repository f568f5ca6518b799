// st_intersects over device-resident geometry columns (mosaic_st_intersects): JTS Geometry.intersects
// for Point / MultiPoint / LineString / MultiLineString / Polygon / MultiPolygon rows on (left row,
// right row) pairs -- the public ST_Intersects (expressions/geometry/ST_Intersects.scala ->
// MosaicGeometryJTS.intersects) and the flat side of the reference's check of st_intersects_aggregate
// (ST_IntersectsBehaviors.scala:45-68).  st_intersects.h holds the semantics and the sequential driver
// whose value these kernels return; the columns are those of st_distance.hip.
//
// Per call:
//   k_isect_plan   one lane per pair: row range check and row status (pairs::plan_status), then steps 1
//                  and 2 of the definition (a side without facets, geometry boxes that do not meet):
//                  such a pair is false and ends here.  The others go by facets(left) x facets(right)
//                  to the front (<= dist_small_work) or the back of one list.
//   k_isect_fill   status[] of every pair and out = 0 (only after the host has seen that no row index
//                  was out of range: such a call writes nothing)
//   k_isect_small  one lane per pair: the sequential driver isect::intersects
//   k_isect_block  one workgroup per pair.  pairs::sweep_tiles stages the side with fewer facets in LDS, a
//                  tile of dist_tile segments at a time, streams the other side's segments across the
//                  lanes and skips the blocks whose boxes do not meet; the body given to it here is
//                  the hit test of one streamed segment against the tile.  A hit sets the sweep's stop
//                  flag, which every lane reads before each streamed segment and the workgroup reads
//                  at every tile; it ends the pair.  Only if no facets met does containment run: one wave per (polygon part,
//                  component, direction) task, the component's first vertex located by the
//                  wave-cooperative locate of pip_coop.h (its flags per segment are those of
//                  pip::locate_in_ring, see that header), until a task hits.
#include "geoms_device.h"
#include "pair_call.h"
#include "pip_coop.h"
#include "st_intersects.h"

using namespace mosaic;

namespace {

using pairs::kBlock;
using pairs::kMaxTile;
constexpr int kWaves = kBlock / 64;

// the last call of this thread: pairs ended in the plan kernel, on the one-lane list, on the workgroup list
thread_local int64_t t_last[3] = {0, 0, 0};

__global__ void __launch_bounds__(kBlock) k_isect_plan(pairs::PlanArgs a) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool small = false, block = false;
        if (i < a.n) {
            int64_t g, h;
            const int32_t st = pairs::plan_status(a, i, g, h);
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
        pairs::plan_append(a, i, small, block);
    }
}

__global__ void __launch_bounds__(kBlock) k_isect_fill(const int32_t* plan, int64_t n, uint8_t* out, int32_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (status) status[i] = plan[i];
        out[i] = 0;
    }
}

struct IsectArgs : pairs::ListArgs {
    uint8_t* out;
    int tile;
};

__global__ void __launch_bounds__(kBlock) k_isect_small(IsectArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n_list; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = a.list[k];
        uint32_t g, h;
        pairs::pair_rows(a, i, g, h);
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
        __syncthreads();  // the previous pair's readers of s_hit are done
        if (tid == 0) s_hit = 0;
        // ---- facets ----
        uint32_t rs0, rs1, rw0, rw1;
        dist::geom_rings(S, gs, rs0, rs1);
        dist::geom_rings(W, gw, rw0, rw1);
        // flip by reference: a bool captured by value stays a byte per lane, which the compiler moves into LDS
        pairs::sweep_tiles(S, rs0, rs1, W, rw0, rw1, W.geom_bbox[gw], (uint32_t)a.tile, s_v, &s_box, &s_hit, &s_snap,
                           [&flip](const pip::Vec2* v, uint32_t cnt, pip::Vec2 C, pip::Vec2 D) {
                               bool hit = false;
                               if (flip) {
                                   for (uint32_t t = 0; t < cnt && !hit; t++) hit = pip::segments_intersect(C, D, v[t], v[t + 1]);
                               } else {
                                   for (uint32_t t = 0; t < cnt && !hit; t++) hit = pip::segments_intersect(v[t], v[t + 1], C, D);
                               }
                               return hit;
                           });
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
    pairs::Call<uint8_t> c;
    MOSAIC_RC(c.open("st_intersects", ctx, left, right, left_row, right_row, n_pairs, out));
    t_last[0] = t_last[1] = t_last[2] = 0;
    if (n_pairs == 0) return MOSAIC_OK;
    MOSAIC_RC(c.stage(4));
    hipLaunchKernelGGL(k_isect_plan, c.lanes(c.n), dim3(kBlock), 0, c.stream, c.pa);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_RC(c.planned());
    MOSAIC_RC(c.bind(out, status));
    hipLaunchKernelGGL(k_isect_fill, c.lanes(c.n), dim3(kBlock), 0, c.stream, c.pa.plan, c.n, c.out.dev, c.status.dev);
    MOSAIC_HIP(hipGetLastError());
    if (c.n_small()) {
        hipLaunchKernelGGL(k_isect_small, c.lanes(c.n_small()), dim3(kBlock), 0, c.stream, IsectArgs{c.small_list(), c.out.dev, c.tile});
        MOSAIC_HIP(hipGetLastError());
    }
    if (c.n_block()) {
        hipLaunchKernelGGL(k_isect_block, c.groups(c.n_block()), dim3(kBlock), 0, c.stream, IsectArgs{c.block_list(), c.out.dev, c.tile});
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_RC(c.finish(false));
    t_last[0] = c.n - c.n_small() - c.n_block();
    t_last[1] = c.n_small();
    t_last[2] = c.n_block();
    return MOSAIC_OK;
}

int mosaic_st_intersects_last_split(int64_t* ended_in_plan, int64_t* one_lane, int64_t* workgroup) {
    if (ended_in_plan) *ended_in_plan = t_last[0];
    if (one_lane) *one_lane = t_last[1];
    if (workgroup) *workgroup = t_last[2];
    return MOSAIC_OK;
}

}  // extern "C"
