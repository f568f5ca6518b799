// Host stitching of st_intersection_aggregate's geometry (isect_geom.cpp): the directed boundary
// edges of a group's per-cell overlays (overlay.h, k_isect_overlay) -> the group's polygons as the
// WKB JTS writes (big-endian 2D Polygon / MultiPolygon; POLYGON EMPTY for an empty result).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// The result of an st_intersection_aggregate geometry call behind the C ABI's mosaic_isect_geoms handle
// (mosaic_hip.hip fills it for two polygon tables, line_clip.hip / line_clip_host.cpp for a line table
// against a polygon table, where `area` holds the length): groups sorted by key pair, group k's WKB at
// wkb[off[k] .. off[k + 1]).
struct mosaic_isect_geoms {
    std::vector<int32_t> lk, rk;
    std::vector<double> area;
    std::vector<uint8_t> status;
    std::vector<int64_t> off;
    std::vector<uint8_t> wkb;
};

namespace mosaic {
namespace isect_geom {

// edges: n x (x0, y0, x1, y1), interior on the left, in any order; the union of the cells' pieces is
// dissolved (shared cell sides cancel), rings are traced as minimal rings, holes assigned to the
// smallest shell holding them.  Shells are written clockwise, holes counter-clockwise, each ring
// starting at its smallest vertex, polygons ordered by that vertex (deterministic output).
// Returns false (out cleared) when the edges do not close into rings (a noding failure).
// snap: the node tolerance (coordinate units); pieces of adjacent cells computed from different
// cells' arithmetic meet within it (see isect_geom.cpp).
bool stitch_wkb(const double* edges, size_t n, double snap, std::vector<uint8_t>& out, double* area);

}  // namespace isect_geom
}  // namespace mosaic
