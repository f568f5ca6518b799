// The device-resident geometry column behind the C ABI's mosaic_geoms handle, shared by the translation
// units that read one (st_distance.hip, st_intersects.hip, ring_neighbours.hip): the GeomStore layout of pip_device.h in
// HBM plus a kind per part (point / polygon), a facet count per geometry and a status per row.
// Immutable after creation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pip_device.h"

struct mosaic_geoms {
    int device = 0;
    int64_t n_geoms = 0, n_vertices = 0, n_row_path = 0;
    mosaic::pip::Vec2* verts = nullptr;
    uint32_t* ring_start = nullptr;
    mosaic::pip::Box* ring_bbox = nullptr;
    uint32_t* part_ring = nullptr;
    uint8_t* part_kind = nullptr;
    uint32_t* geom_part = nullptr;
    mosaic::pip::Box* geom_bbox = nullptr;
    uint32_t* geom_facets = nullptr;
    int32_t* row_status = nullptr;
    ~mosaic_geoms() {
        for (void* p : {(void*)verts, (void*)ring_start, (void*)ring_bbox, (void*)part_ring, (void*)part_kind,
                        (void*)geom_part, (void*)geom_bbox, (void*)geom_facets, (void*)row_status})
            if (p) (void)hipFree(p);
    }
};
