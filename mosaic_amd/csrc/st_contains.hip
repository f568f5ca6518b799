// st_contains over device-resident geometry columns (mosaic_st_contains_geoms): JTS Geometry.contains
// for Point / MultiPoint / LineString / MultiLineString / Polygon / MultiPolygon rows on (left row,
// right row) pairs -- the public ST_Contains (expressions/geometry/ST_Contains.scala ->
// MosaicGeometryJTS.contains) beyond "polygon contains point".  st_contains.h holds the semantics and
// the sequential driver whose value and status these kernels return; the columns are those of
// st_distance.hip.
//
// Per call:
//   k_cont_plan    one lane per pair: row range check and row status (pairs::plan_status), then steps 1, 2
//                  and 6 of the definition (a side without facets, B's box not inside A's, a left side
//                  that is not polygonal): such a pair ends here.  So does a points-only B (steps 3 and
//                  4) of at most dist_small_work facet pairs, decided by this lane.  The others go by
//                  facets(left) x facets(right) to the front (<= dist_small_work) or the back of one list.
//                  A pair's status and value travel in plan[] (status | out << 8), since nothing may be
//                  written before the host has seen that no row index was out of range.
//   k_cont_fill    status[] and out[] of every pair from plan[]
//   k_cont_small   one lane per pair: the sequential driver contains::contains_how
//   k_cont_block   one workgroup per pair.
//                  Step 5: pairs::sweep_tiles stages A's segments in LDS, a tile of dist_tile segments at
//                  a time, streams B's across the lanes and skips the blocks whose boxes do not meet.
//                  Unlike k_isect_block's, the body given to it here does not stop at the first contact:
//                  it sets `contact` and goes on, and stops at the first proper crossing (the sweep's
//                  stop flag: every lane reads it before each streamed segment, the workgroup at every
//                  tile).  Then the location phase, for the pairs without a crossing: with contact every vertex of B is
//                  located in A, one wave per vertex, until one is EXTERIOR; without contact the first
//                  vertices of 5(c), one wave per (part of B) and per (ring of A, polygon part of B).
//                  The locate is the wave-cooperative one of pip_coop.h: lanes over the ring's segments,
//                  boundary hits as pip::locate_in_ring, the crossing parity summed over the wave.
//                  Steps 3 and 4 beyond dist_small_work: one wave per point of B against A's parts, or
//                  one lane per point of B against A's points.
// All results are written with ordinary vector stores; the split counts are atomic adds.
#include "geoms_device.h"
#include "pair_call.h"
#include "pip_coop.h"
#include "st_contains.h"

using namespace mosaic;

namespace {

using pairs::kBlock;
using pairs::kMaxTile;
constexpr int kWaves = kBlock / 64;

// counters of a call, above pairs::kCntSmall / kCntBlock / kCntBadRow
enum { kCntKinds = 3, kCntOut = 4, kCntClear = 5, kCntTouch = 6, kCounters = 8 };

// the last call of this thread: ended in plan, decided by a crossing or an exterior vertex, decided
// without contact, undecided, served by a workgroup
thread_local int64_t t_last[5] = {0, 0, 0, 0, 0};

// plan[i] here: the pair's status | out << 8
__global__ void __launch_bounds__(kBlock) k_cont_plan(pairs::PlanArgs a) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool small = false, block = false;
        if (i < a.n) {
            int64_t g, h;
            int32_t st = pairs::plan_status(a, i, g, h);
            int32_t out = 0;
            if (st == MOSAIC_ROW_OK) {
                const unsigned long long work = (unsigned long long)a.L.facets[g] * a.R.facets[h];
                // steps 1 and 2 of the definition: 0, and the pair reaches no other kernel
                if (work != 0 && contains::box_covers(a.L.s.geom_bbox[g], a.R.s.geom_bbox[h])) {
                    const uint32_t A = contains::geom_kinds(a.L.s, a.L.part_kind, (uint32_t)g);
                    const uint32_t B = contains::geom_kinds(a.R.s, a.R.part_kind, (uint32_t)h);
                    const bool points = B == contains::kHasPoint && (A == contains::kHasPolygon || A == contains::kHasPoint);
                    if (!points && A != contains::kHasPolygon) {  // step 6
                        st = MOSAIC_PAIR_UNDECIDED;
                        atomicAdd(&a.counts[kCntKinds], 1ull);
                    } else if (points && work <= a.small_work) {  // steps 3 and 4
                        int how;
                        out = (A == contains::kHasPolygon ? contains::points_in_polygonal(a.L.s, (uint32_t)g, a.R.s, (uint32_t)h, &how)
                                                          : contains::points_in_points(a.L.s, (uint32_t)g, a.R.s, (uint32_t)h, &how))
                                  ? 1 : 0;
                    } else {
                        small = work <= a.small_work;
                        block = !small;
                    }
                }
            }
            a.plan[i] = st | (out << 8);  // -1 stays -1
        }
        pairs::plan_append(a, i, small, block);
    }
}

__global__ void __launch_bounds__(kBlock) k_cont_fill(const int32_t* plan, int64_t n, uint8_t* out, int32_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = plan[i];
        if (status) status[i] = p & 0xff;
        out[i] = (uint8_t)(p >> 8);
    }
}

struct ContArgs : pairs::ListArgs {
    uint8_t* out;
    int32_t* status;  // nullable
    unsigned long long* counts;
    int tile;
};

// the counter of a decided pair
__device__ inline int how_counter(int how) {
    return how == contains::kHowTouch ? kCntTouch : (how == contains::kHowClear || how == contains::kHowPointsIn) ? kCntClear : kCntOut;
}

__global__ void __launch_bounds__(kBlock) k_cont_small(ContArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n_list; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = a.list[k];
        uint32_t g, h;
        pairs::pair_rows(a, i, g, h);
        int32_t st;
        int how;
        a.out[i] = contains::contains_how(a.L.s, a.L.part_kind, g, a.R.s, a.R.part_kind, h, &st, &how);
        if (a.status && st != MOSAIC_ROW_OK) a.status[i] = st;
        atomicAdd(&a.counts[how_counter(how)], 1ull);
    }
}

// contains::locate_union with every locate spread over the calling wave (g, px, py wave-uniform):
// whether (px, py) is EXTERIOR to the polygonal geometry g, *interior: whether some part says INTERIOR
__device__ inline bool coop_exterior(const pip::GeomStore& s, uint32_t g, double px, double py, bool* interior) {
    *interior = false;
    if (pip::box_excludes(s.geom_bbox[g], px, py)) return true;
    bool boundary = false;
    for (uint32_t p = s.geom_part[g]; p < s.geom_part[g + 1]; p++) {
        const int loc = pip::coop_locate_in_polygon(s, p, px, py);
        if (loc == pip::LOC_INTERIOR) {
            *interior = true;
            return false;
        }
        if (loc == pip::LOC_BOUNDARY) boundary = true;
    }
    return !boundary;
}

__global__ void __launch_bounds__(kBlock) k_cont_block(ContArgs a) {
    __shared__ pip::Vec2 s_v[kMaxTile + 1];
    __shared__ pip::Box s_box;
    // s_contact, s_crossed: the sweep (s_crossed is its stop flag); s_out: an exterior vertex or point;
    // s_in: an interior point (step 3); s_fail: a first-vertex test of 5(c) failed
    // As in pairs::sweep_tiles, the flags are set with plain stores and polled through volatile reads without
    // a fence: a poll only ends a loop early, and every read that decides the result sits behind a __syncthreads.
    __shared__ int s_contact, s_crossed, s_snap, s_out, s_in, s_fail;
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = tid >> 6;
    const pip::GeomStore& SA = a.L.s;
    const pip::GeomStore& SB = a.R.s;
    for (int64_t k = blockIdx.x; k < a.n_list; k += gridDim.x) {
        const int64_t i = a.list[k];
        uint32_t g, h;
        pairs::pair_rows(a, i, g, h);
        __syncthreads();  // the previous pair's readers of the flags are done
        if (tid == 0) s_contact = s_crossed = s_out = s_in = s_fail = 0;
        uint32_t ra0, ra1, rb0, rb1;
        dist::geom_rings(SA, g, ra0, ra1);
        dist::geom_rings(SB, h, rb0, rb1);
        const uint32_t vb0 = SB.ring_start[rb0], vb1 = SB.ring_start[rb1];  // B's vertices
        const uint32_t kinds_a = contains::geom_kinds(SA, a.L.part_kind, g);  // uniform
        const uint32_t kinds_b = contains::geom_kinds(SB, a.R.part_kind, h);
        int how;
        uint8_t out = 0;
        if (kinds_b == contains::kHasPoint) {
            // ---- steps 3 and 4: B points only (A is polygonal or points only: the plan kernel ended the others) ----
            __syncthreads();  // the flags are zero
            if (kinds_a == contains::kHasPolygon) {
                for (uint32_t v = vb0 + wave; v < vb1; v += kWaves) {
                    if (__any(*(volatile int*)&s_out)) break;
                    const pip::Vec2 pt = SB.verts[v];
                    bool interior;
                    const bool ext = coop_exterior(SA, g, pt.x, pt.y, &interior);
                    if ((tid & 63) == 0) {
                        if (ext) s_out = 1;
                        if (interior) s_in = 1;
                    }
                }
            } else {
                const uint32_t va0 = SA.ring_start[ra0], va1 = SA.ring_start[ra1];
                for (uint32_t v = vb0 + tid; v < vb1; v += kBlock) {
                    if (*(volatile int*)&s_out) break;
                    const pip::Vec2 pt = SB.verts[v];
                    bool found = false;
                    for (uint32_t u = va0; u < va1 && !found; u++) found = contains::same_point(SA.verts[u], pt);
                    if (!found) s_out = 1;
                }
                if (tid == 0) s_in = 1;  // a matched point is an interior point of both
            }
            __syncthreads();
            how = s_out ? contains::kHowPointsOut : contains::kHowPointsIn;
            out = !s_out && s_in ? 1 : 0;
        } else {
            // ---- step 5(a) and the contact of 5(c): the sweep ----
            pairs::sweep_tiles(SA, ra0, ra1, SB, rb0, rb1, SB.geom_bbox[h], (uint32_t)a.tile, s_v, &s_box, &s_crossed, &s_snap,
                               [](const pip::Vec2* v, uint32_t cnt, pip::Vec2 C, pip::Vec2 D) {
                                   int worst = 0;
                                   for (uint32_t t = 0; t < cnt && worst < 2; t++) {
                                       const int c = contains::facet_contact(v[t], v[t + 1], C, D);
                                       worst = c > worst ? c : worst;
                                   }
                                   if (worst) s_contact = 1;
                                   return worst == 2;
                               });
            __syncthreads();
            const bool crossed = s_crossed != 0, contact = s_contact != 0;  // uniform: every write of the sweep is behind the barrier
            // ---- the location phase ----
            if (crossed) {
                how = contains::kHowOut;
            } else if (contact) {
                // 5(b): every vertex of B, one wave each, until one is EXTERIOR
                for (uint32_t v = vb0 + wave; v < vb1; v += kWaves) {
                    if (__any(*(volatile int*)&s_out)) break;
                    const pip::Vec2 pt = SB.verts[v];
                    bool interior;
                    if (coop_exterior(SA, g, pt.x, pt.y, &interior) && (tid & 63) == 0) s_out = 1;
                }
                __syncthreads();
                how = s_out ? contains::kHowOut : contains::kHowTouch;
            } else {
                // 5(c): (i) the first vertex of every part of B is INTERIOR to a part of A;
                // (ii) no ring of A starts INTERIOR to a polygon part of B
                const uint32_t pa0 = SA.geom_part[g], npa = SA.geom_part[g + 1] - pa0;
                const uint32_t pb0 = SB.geom_part[h], npb = SB.geom_part[h + 1] - pb0;
                const uint64_t nra = ra1 - ra0;
                const uint64_t tasks = npb + ((kinds_b & contains::kHasPolygon) ? nra * npb : 0);
                for (uint64_t t = wave; t < tasks; t += kWaves) {
                    if (__any(*(volatile int*)&s_fail)) break;
                    bool fail = false;
                    if (t < npb) {
                        pip::Vec2 v;
                        if (contains::part_first_vertex(SB, pb0 + (uint32_t)t, &v)) {
                            bool inside = false;
                            for (uint32_t p = pa0; p < pa0 + npa && !inside; p++)
                                inside = pip::coop_locate_in_polygon(SA, p, v.x, v.y) == pip::LOC_INTERIOR;
                            fail = !inside;
                        }
                    } else {
                        const uint64_t u = t - npb;
                        const uint32_t ra = ra0 + (uint32_t)(u / npb), q = pb0 + (uint32_t)(u % npb);
                        if (a.R.part_kind[q] == kPartPolygon && SA.ring_start[ra + 1] > SA.ring_start[ra]) {
                            const pip::Vec2 w = SA.verts[SA.ring_start[ra]];
                            fail = pip::coop_locate_in_polygon(SB, q, w.x, w.y) == pip::LOC_INTERIOR;
                        }
                    }
                    if (fail && (tid & 63) == 0) s_fail = 1;
                }
                __syncthreads();
                how = contains::kHowClear;
                out = s_fail ? 0 : 1;
            }
        }
        if (tid == 0) {
            a.out[i] = out;
            if (a.status && how == contains::kHowTouch) a.status[i] = MOSAIC_PAIR_UNDECIDED;
            atomicAdd(&a.counts[how_counter(how)], 1ull);
        }
    }
}

}  // namespace

extern "C" {

int mosaic_st_contains_geoms(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                             const int64_t* right_row, int64_t n_pairs, uint8_t* out, int32_t* status) {
    pairs::Call<uint8_t> c;
    MOSAIC_RC(c.open("st_contains", ctx, left, right, left_row, right_row, n_pairs, out));
    for (int64_t& v : t_last) v = 0;
    if (n_pairs == 0) return MOSAIC_OK;
    MOSAIC_RC(c.stage(kCounters));
    hipLaunchKernelGGL(k_cont_plan, c.lanes(c.n), dim3(kBlock), 0, c.stream, c.pa);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_RC(c.planned());
    MOSAIC_RC(c.bind(out, status));
    hipLaunchKernelGGL(k_cont_fill, c.lanes(c.n), dim3(kBlock), 0, c.stream, c.pa.plan, c.n, c.out.dev, c.status.dev);
    MOSAIC_HIP(hipGetLastError());
    if (c.n_small()) {
        hipLaunchKernelGGL(k_cont_small, c.lanes(c.n_small()), dim3(kBlock), 0, c.stream,
                           ContArgs{c.small_list(), c.out.dev, c.status.dev, c.pa.counts, c.tile});
        MOSAIC_HIP(hipGetLastError());
    }
    if (c.n_block()) {
        hipLaunchKernelGGL(k_cont_block, c.groups(c.n_block()), dim3(kBlock), 0, c.stream,
                           ContArgs{c.block_list(), c.out.dev, c.status.dev, c.pa.counts, c.tile});
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_RC(c.finish(c.n_small() || c.n_block()));  // the small and block kernels count how each pair was decided
    t_last[0] = c.n - c.n_small() - c.n_block() - (int64_t)c.counts[kCntKinds];
    t_last[1] = (int64_t)c.counts[kCntOut];
    t_last[2] = (int64_t)c.counts[kCntClear];
    t_last[3] = (int64_t)c.counts[kCntKinds] + (int64_t)c.counts[kCntTouch];
    t_last[4] = c.n_block();
    return MOSAIC_OK;
}

int mosaic_st_contains_last_split(int64_t out5[5]) {
    if (!out5) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    for (int k = 0; k < 5; k++) out5[k] = t_last[k];
    return MOSAIC_OK;
}

}  // extern "C"
