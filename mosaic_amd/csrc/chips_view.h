// What a chip join reads from a polygon chip table (struct mosaic_chips of mosaic_hip.hip), for the
// translation units that join against one (line_join.hip): the cell hash (linear probing from
// mix64(cell) & (capacity - 1); an entry names chips [first, first + count) in table order), the
// chips' (key << 1) | is_core words and their geometry, all in table order and in HBM.  Table order
// is the stable order by cell: within a cell the chips keep the order of their rows.
#pragma once
#include <stdint.h>

#include "../../include/mosaic_hip.h"
#include "join_common.h"
#include "line_clip_host.h"
#include "line_isect.h"
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

// What the line-polygon st_intersection_aggregate (line_clip.hip) reads from a line chip table (struct
// mosaic_line_chips of line_join.hip): the flat layout of line_isect.h, a cell id and a
// (key << 1) | is_core word per chip, all in HBM.
struct LineChipsView {
    lineisect::LineStore store;
    const int64_t* cell;
    const uint32_t* meta;
    int grid, res, device;
    int64_t n_chips, n_pieces, n_vertices;
};

namespace lineisect {
// layout fingerprint of what line_clip.hip shares with the other translation units (join_binned.h's rationale)
static constexpr uint64_t clip_layout_fingerprint() {
    return (uint64_t)sizeof(PairRec) * 1000003ull + (uint64_t)sizeof(Run) * 10007ull + (uint64_t)sizeof(LineChipsView) * 101ull +
           (uint64_t)sizeof(ChipsJoinView) * 7ull + (uint64_t)sizeof(mosaic_isect_geoms) + (uint64_t)kCutCap * 1000000007ull;
}
}  // namespace lineisect

}  // namespace mosaic

extern "C" int mosaic_line_chips_view(const mosaic_line_chips* lines, mosaic::LineChipsView* out);
extern "C" int mosaic_chips_join_view(const mosaic_chips* chips, mosaic::ChipsJoinView* out);
