// CPU build of the geometry k-ring code (mosaic_amd/csrc/geom_kring.h: the key / value packing, the
// order key and the sequential driver of the rounds the device kernels run, compiled by g++) as a
// small shared library, so tests/test_geometry_kring.py can compare it with a brute force over the
// oracle's k-rings without a GPU.
#include <stdint.h>

#include <algorithm>

#include "geom_kring.h"

// grid 0 = H3, 1 = BNG.  offsets[n_geoms + 1], status[n_geoms]; cells / dist hold cap entries.
// Returns the cell count, or -1 if it exceeds cap.
extern "C" int64_t geom_kring_host(int grid, int res, int64_t n_chips, const uint8_t* is_core, const int64_t* index_id,
                                   const int32_t* key, int64_t n_geoms, int k, int loop, int64_t* offsets,
                                   int64_t* cells, int32_t* dist, int32_t* status, int64_t cap) {
    mosaic::gk::HostLists l;
    mosaic::gk::host_run(grid == 1, res, n_chips, is_core, index_id, key, n_geoms, k, loop, &l);
    if ((int64_t)l.cells.size() > cap) return -1;
    std::copy(l.offsets.begin(), l.offsets.end(), offsets);
    std::copy(l.cells.begin(), l.cells.end(), cells);
    std::copy(l.dist.begin(), l.dist.end(), dist);
    std::copy(l.status.begin(), l.status.end(), status);
    return (int64_t)l.cells.size();
}
