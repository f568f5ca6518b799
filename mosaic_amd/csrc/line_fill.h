// Host side of the line chip producers (mosaic_tessellate_lines[_gpu]): the records lines_host.cpp and
// line_fill.hip share, and the host routines (compiled by g++ in lines_host.cpp, where the H3 tables are
// host constants) that the device producer's orchestration calls for what its lanes hand off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "lineclip.h"

struct mosaic_chip_set;

namespace mosaic {
namespace linefill {

// The batch with consecutive repeated vertices removed (JTS GeometryGraph.addLineString): what both
// producers walk.  Vertex v of line l = xy[2 (line_off[l] + v)]; a segment is named by its first vertex.
struct Clean {
    std::vector<double> xy;
    std::vector<int64_t> line_off;   // n_lines + 1
    std::vector<int32_t> line_geom;  // per line
    std::vector<int32_t> vert_line;  // per vertex
    int64_t n_lines = 0, n_verts = 0;
};

// One (line, cell) group: the lane's (or the host's) verdict and where its items are.
struct GroupRec {
    int64_t cell;
    int64_t s0;     // lineclip::Work::s0 / t0
    double t0;
    int64_t item0;  // first item (device items array); unused for host-built groups
    int32_t n_items;
    int32_t has_piece;
    int32_t status;  // lineclip::Status: kNeedsMore = build on the host
    uint32_t seg_first;
};

// The host's cell polygons, remembered per thread (consecutive segments come to the same cells).
struct CachedPoly {
    lineclip::Grid g;
    bool operator()(int64_t id, lineclip::Cell& C) const;
};

// Validates and cleans the input; a mosaic status (the message set).
int prepare(int64_t n_geoms, const int64_t* geom_lines, const int64_t* line_offsets, const double* xy, Clean& out);
// The cells of span j of K of segment s with host scratch that grows: lineclip::kOk or kBadCell.
int walk_span_host(lineclip::Grid g, const Clean& c, int64_t s, int32_t j, int32_t K, std::vector<int64_t>& cells);
// Builds the groups whose status is kNeedsMore on host threads, orders the chips (line, position along
// the line, cell) and writes the chip set.  seg_start[n_groups + 1] indexes segs.  *bad_seg >= 0 on
// return: a segment whose group met a cell that is no planar polygon.
int finish(lineclip::Grid g, const Clean& c, int64_t n_groups, GroupRec* recs, const int64_t* seg_start, const uint32_t* segs,
           const lineclip::Item* items, int cells_only, mosaic_chip_set* cs, int64_t* bad_seg);
// MOSAIC_E_ARG naming the geometry of segment s
int fail_bad_cell(const Clean& c, int64_t s);

static constexpr uint64_t layout_fingerprint() {
    uint64_t h = 0xcbf29ce484222325ULL;
    for (uint64_t v : {(uint64_t)sizeof(GroupRec), (uint64_t)sizeof(lineclip::Item), (uint64_t)offsetof(GroupRec, status),
                       (uint64_t)lineclip::kWalkCap, (uint64_t)lineclip::kItems})
        h = h * 0x100000001b3ULL ^ v;
    return h;
}

}  // namespace linefill
}  // namespace mosaic
