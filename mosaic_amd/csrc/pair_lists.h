// What the pair kernels over geometry columns share (st_distance.hip, st_intersects.hip): the device
// view of a column, the per-wave append to a work list, and the block size of their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geoms_device.h"
#include "pip_device.h"

namespace mosaic {
namespace pairs {

constexpr int kBlock = 256;

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

}  // namespace pairs
}  // namespace mosaic
