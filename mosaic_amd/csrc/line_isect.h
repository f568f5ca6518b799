// JTS 1.19 `Geometry.intersects` of a line chip and a polygon chip -- the geometry test of
// st_intersects_aggregate over the join of line chips (Mosaic.lineFill) with polygon chips
// (expressions/geometry/ST_IntersectsAggregate.scala:28-39, whose update decodes whatever WKB a
// chip holds; core/Mosaic.scala:21-35 sends LINESTRING / MULTILINESTRING to lineFill).
//
// A line chip is LINESTRING / MULTILINESTRING pieces, or POINT / MULTIPOINT items where the line
// only touches its cell.  Flat layout (line_chips_build.h builds it, line_join.hip keeps it in HBM):
//   verts       Vec2[V]      all vertices, piece after piece
//   piece_start uint32[M+1]  piece m = verts[piece_start[m] .. piece_start[m+1]); one vertex: a point
//   piece_bbox  Box[M]
//   chip_piece  uint32[N+1]  chip c = pieces [chip_piece[c] .. chip_piece[c+1]); none: an empty chip
//   chip_bbox   Box[N]
//
// intersects(line chip, polygon chip): the closed point sets share a point.
//   1. either side without a coordinate: false
//   2. the chips' boxes do not meet: false
//   3. a segment of a piece meets a ring segment of the polygon chip (holes included): true
//   4. otherwise the first vertex of every piece (every point item is one) is located in every
//      polygon part; not exterior (boundary included) in one of them: true
//   5. otherwise false
// Step 4 decides the rest: once no segments meet, a piece lies wholly inside or wholly outside each
// polygon part, and a line has no area for the polygon to lie inside of.  Every decision is an
// exact predicate of pip_device.h (double-double orientation signs, envelope comparisons), so every
// evaluation order gives the same answer; `intersects` below is the sequential driver the wave
// kernels of line_join.hip and the host join of line_join_host.cpp are defined by.
#pragma once
#include <stdint.h>

#include "pip_device.h"

namespace mosaic {
namespace lineisect {

struct LineStore {
    const pip::Vec2* verts;
    const uint32_t* piece_start;
    const pip::Box* piece_bbox;
    const uint32_t* chip_piece;
    const pip::Box* chip_bbox;
};

// steps 1 and 2: false when the answer is false without looking at a segment
MOSAIC_HD bool may_meet(const LineStore& L, uint32_t c, const pip::GeomStore& P, uint32_t g) {
    if (L.chip_piece[c + 1] <= L.chip_piece[c] || P.geom_part[g + 1] <= P.geom_part[g]) return false;
    return pip::boxes_meet(L.chip_bbox[c], P.geom_bbox[g]);
}

// step 4 for one (piece, polygon part)
MOSAIC_HD bool piece_start_in_part(const LineStore& L, uint32_t piece, const pip::GeomStore& P, uint32_t part) {
    const pip::Vec2 v = L.verts[L.piece_start[piece]];
    const uint32_t r0 = P.part_ring[part];
    if (P.part_ring[part + 1] <= r0 || pip::box_excludes(P.ring_bbox[r0], v.x, v.y)) return false;
    return pip::locate_in_polygon(P, part, v.x, v.y) != pip::LOC_EXTERIOR;
}

MOSAIC_HD bool intersects(const LineStore& L, uint32_t c, const pip::GeomStore& P, uint32_t g) {
    if (!may_meet(L, c, P, g)) return false;
    const uint32_t m0 = L.chip_piece[c], m1 = L.chip_piece[c + 1];
    const uint32_t q0 = P.geom_part[g], q1 = P.geom_part[g + 1];
    const uint32_t r0 = P.part_ring[q0], r1 = P.part_ring[q1];
    const pip::Box gb = P.geom_bbox[g];
    for (uint32_t m = m0; m < m1; m++) {
        const uint32_t i0 = L.piece_start[m], i1 = L.piece_start[m + 1];
        if (i1 - i0 < 2 || !pip::boxes_meet(L.piece_bbox[m], gb)) continue;
        for (uint32_t r = r0; r < r1; r++) {
            if (!pip::boxes_meet(L.piece_bbox[m], P.ring_bbox[r])) continue;
            for (uint32_t i = i0; i + 1 < i1; i++)
                for (uint32_t j = P.ring_start[r]; j + 1 < P.ring_start[r + 1]; j++)
                    if (pip::segments_intersect(L.verts[i], L.verts[i + 1], P.verts[j], P.verts[j + 1])) return true;
        }
    }
    for (uint32_t m = m0; m < m1; m++)
        for (uint32_t q = q0; q < q1; q++)
            if (piece_start_in_part(L, m, P, q)) return true;
    return false;
}

}  // namespace lineisect
}  // namespace mosaic
