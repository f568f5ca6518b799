// The device-resident geometry column behind the C ABI's mosaic_geoms handle, shared by the translation
// units that read one (st_distance.hip, st_intersects.hip, ring_neighbours.hip): the GeomStore layout of pip_device.h in
// HBM plus a kind per part (point / polygon), a facet count per geometry and a status per row.
// Immutable after creation.  Also the small device-memory helpers those translation units share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

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

namespace mosaic {
namespace dev {

struct DevMem {
    void* p = nullptr;
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 16)); }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};

inline bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// src (n elements, host or device) as a device pointer; a host array is copied into `stage`
template <class T>
hipError_t on_device(const T* src, int64_t n, DevMem& stage, hipStream_t stream, const T** out) {
    if (is_device_ptr(src)) {
        *out = src;
        return hipSuccess;
    }
    hipError_t e = stage.alloc((size_t)n * sizeof(T));
    if (e == hipSuccess) e = hipMemcpyAsync(stage.p, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, stream);
    *out = (const T*)stage.p;
    return e;
}

}  // namespace dev
}  // namespace mosaic
