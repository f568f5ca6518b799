// mosaic_cell_lists (include/mosaic_hip.h): per-row cell lists, the result of mosaic_polyfill and of
// mosaic_chips_kring / mosaic_geometry_kring.  Row g holds cells[offsets[g] .. offsets[g + 1]).
#pragma once
#include <stdint.h>

#include <vector>

struct mosaic_cell_lists {
    std::vector<int64_t> offsets{0};
    std::vector<int64_t> cells;
    std::vector<int32_t> status;
    std::vector<int32_t> dist;  // per cell, the geometry k-ring entries only (else empty)
};
