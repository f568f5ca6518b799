// What the kernels over geometry columns share on the device.  All of them (st_distance.hip,
// st_intersects.hip, st_contains.hip, st_measures.hip): the view of a column, the per-wave append to a
// work list and the block size.  The three pair predicates also: the plan kernel's prologue and
// epilogue, the (left row, right row) of a pair, the tile stage of the block kernels, and the
// boxes-meet sweep of k_isect_block / k_cont_block.  pair_call.h is the host side of a pair call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geoms_device.h"
#include "pip_device.h"
#include "st_distance.h"

namespace mosaic {
namespace pairs {

constexpr int kBlock = 256;
constexpr int kMaxTile = 1024;  // segments of a block kernel's tile: s_v holds kMaxTile + 1 vertices

struct Col {
    pip::GeomStore s;
    const uint8_t* part_kind;
    const uint32_t* facets;
    const int32_t* status;
    int64_t n;
};

inline Col view(const mosaic_geoms* g) {
    return Col{pip::GeomStore{g->verts, g->ring_start, g->ring_bbox, g->part_ring, g->geom_part, g->geom_bbox},
               g->part_kind, g->geom_facets, g->row_status, g->n_geoms};
}

// the calling lane's slot in a list that grows by one atomicAdd per wave; every lane of the wave calls it
__device__ inline unsigned long long wave_append(unsigned long long* counter, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m == 0) return 0;
    const int leader = __ffsll((long long)m) - 1;
    const int lane = (int)__lane_id();
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = (unsigned long long)__shfl((long long)base, leader, 64);
    return base + (unsigned long long)__popcll(m & (((unsigned long long)1 << lane) - 1));
}

// The counters of a pair call.  These three are the contract between the plan kernels and pair_call.h;
// a predicate's own counters sit above them.
enum { kCntSmall = 0, kCntBlock = 1, kCntBadRow = 2 };

// the pairs of a call: pair i is (lrow[i], rrow[i]) or, with both null, (row i, row i)
struct Pairs {
    Col L, R;
    const int64_t *lrow, *rrow;
};

struct PlanArgs : Pairs {
    int64_t n;
    unsigned long long small_work;
    int32_t* plan;               // per pair: its status (a predicate may pack more above it); -1: a row index out of range
    int64_t* list;               // small pairs from the front, block pairs from the back
    unsigned long long* counts;  // kCnt*
};

// what a small or a block kernel works through: n_list pair ids
struct ListArgs : Pairs {
    const int64_t* list;
    int64_t n_list;
};

template <class I>
__device__ inline void pair_rows(const Pairs& a, int64_t i, I& g, I& h) {
    g = (I)(a.lrow ? a.lrow[i] : i);
    h = (I)(a.rrow ? a.rrow[i] : i);
}

// The prologue of a plan kernel: the rows of pair i and its status, null over row-path over ok.  A row
// index outside its column counts in counts[kCntBadRow] and gives -1.
__device__ inline int32_t plan_status(const PlanArgs& a, int64_t i, int64_t& g, int64_t& h) {
    pair_rows(a, i, g, h);
    if (g < 0 || g >= a.L.n || h < 0 || h >= a.R.n) {
        atomicAdd(&a.counts[kCntBadRow], 1ull);
        return -1;
    }
    const int32_t sl = a.L.status[g], sr = a.R.status[h];
    if (sl == MOSAIC_ROW_NULL || sr == MOSAIC_ROW_NULL) return MOSAIC_ROW_NULL;
    return sl != MOSAIC_ROW_OK || sr != MOSAIC_ROW_OK ? MOSAIC_ROW_PATH : MOSAIC_ROW_OK;
}

// The epilogue of a plan kernel, called by every lane of the wave: pair i to the front of the list
// (small), to its back (block), or to neither.
__device__ inline void plan_append(const PlanArgs& a, int64_t i, bool small, bool block) {
    const unsigned long long ps = wave_append(&a.counts[kCntSmall], small);
    const unsigned long long pb = wave_append(&a.counts[kCntBlock], block);
    if (small) a.list[ps] = i;
    if (block) a.list[a.n - 1 - (int64_t)pb] = i;
}

// ---- the tile stage of a block kernel (kBlock lanes) ----
// The cnt + 1 vertices of the segments [f0, f0 + cnt) of a ring (v, n vertices) into s_v.  The index is
// clamped to the ring's last vertex: a point's facet is (v, v), and nothing closes an open line.
__device__ inline void stage_tile(pip::Vec2* s_v, const pip::Vec2* v, uint32_t n, uint32_t f0, uint32_t cnt) {
    for (uint32_t t = threadIdx.x; t <= cnt; t += kBlock) s_v[t] = v[f0 + t < n ? f0 + t : n - 1];
}

// wave 0: the box of s_v[0 .. cnt] into *s_box; a barrier lies between stage_tile and this, and another
// between this and the readers of *s_box
__device__ inline void tile_box(const pip::Vec2* s_v, uint32_t cnt, pip::Box* s_box) {
    if (threadIdx.x >= 64) return;
    pip::Box b = {INFINITY, INFINITY, -INFINITY, -INFINITY};
    for (uint32_t t = threadIdx.x; t <= cnt; t += 64) {
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
    if (threadIdx.x == 0) *s_box = b;
}

// The boxes-meet sweep of one pair by a workgroup of kBlock lanes: the rings [rs0, rs1) of S are staged
// in LDS (s_v, s_box), a tile of T segments at a time, and the segments of the rings [rw0, rw1) of W
// (wbox: their geometry's box) are streamed across the lanes.  A staged ring, a tile, a (tile, streamed
// ring) or a (tile, streamed segment) block whose boxes do not meet is skipped: segments inside disjoint
// boxes share no point.  For every other (tile, streamed segment C D) one lane calls
// body(s_v, cnt, C, D) -> bool; true sets *s_stop, which ends the sweep.
//
// *s_stop is zeroed by the caller (thread 0, after a barrier that ends the previous pair's reads); the
// first barrier here makes that visible.  It is set with a plain store and polled through volatile
// reads without a fence: a poll only ends a loop early.  What must be uniform is: thread 0 snapshots
// the flag into *s_snap between the two barriers of a tile, so every thread leaves the tile loop
// together; and the caller reads the flag, and whatever else body wrote, behind a __syncthreads of its
// own after the sweep.
template <class Body>
__device__ __forceinline__ void sweep_tiles(const pip::GeomStore& S, uint32_t rs0, uint32_t rs1, const pip::GeomStore& W,
                                            uint32_t rw0, uint32_t rw1, const pip::Box& wbox, uint32_t T, pip::Vec2* s_v,
                                            pip::Box* s_box, int* s_stop, int* s_snap, Body body) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t rs = rs0; rs < rs1; rs++) {
        const uint32_t v0 = S.ring_start[rs], n = S.ring_start[rs + 1] - v0;
        const uint32_t nf = dist::ring_facets(n);
        if (nf == 0 || !pip::boxes_meet(S.ring_bbox[rs], wbox)) continue;  // uniform
        for (uint32_t f0 = 0; f0 < nf; f0 += T) {
            const uint32_t cnt = nf - f0 < T ? nf - f0 : T;
            __syncthreads();  // the previous tile's readers of s_v / s_box / s_snap are done; the zeroed flag is visible
            stage_tile(s_v, S.verts + v0, n, f0, cnt);
            if (tid == 0) *s_snap = *(volatile int*)s_stop;
            __syncthreads();
            if (*s_snap) return;  // uniform
            tile_box(s_v, cnt, s_box);
            __syncthreads();
            const pip::Box tb = *s_box;
            if (!pip::boxes_meet(tb, wbox)) continue;  // uniform
            for (uint32_t rw = rw0; rw < rw1; rw++) {
                const uint32_t w0 = W.ring_start[rw], nw = W.ring_start[rw + 1] - w0;
                const uint32_t nfw = dist::ring_facets(nw);
                if (nfw == 0 || !pip::boxes_meet(tb, W.ring_bbox[rw])) continue;
                for (uint32_t j = tid; j < nfw; j += kBlock) {
                    if (*(volatile int*)s_stop) break;
                    pip::Vec2 C, D;
                    dist::ring_facet(W.verts + w0, nw, j, C, D);
                    if (!pip::boxes_meet(tb, dist::facet_box(C, D))) continue;
                    if (body(s_v, cnt, C, D)) {
                        *s_stop = 1;
                        break;
                    }
                }
            }
        }
    }
}

}  // namespace pairs
}  // namespace mosaic
