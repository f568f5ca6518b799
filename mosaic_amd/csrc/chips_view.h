// What a chip join reads from a polygon chip table (struct mosaic_chips of mosaic_hip.hip), for the
// translation units that join against one (line_join.hip): the cell hash (linear probing from
// mix64(cell) & (capacity - 1); an entry names chips [first, first + count) in table order), the
// chips' (key << 1) | is_core words and their geometry, all in table order and in HBM.
#pragma once
#include <stdint.h>

#include "../../include/mosaic_hip.h"
#include "join_common.h"
#include "pip_device.h"

namespace mosaic {

struct ChipsJoinView {
    const HashEntry* table;
    uint64_t capacity;  // a power of two
    const uint32_t* meta;
    pip::GeomStore store;
    int grid, res, device;
    int64_t n_chips;
};

}  // namespace mosaic

extern "C" int mosaic_chips_join_view(const mosaic_chips* chips, mosaic::ChipsJoinView* out);
