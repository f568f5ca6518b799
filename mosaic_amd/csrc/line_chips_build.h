// Host-side decoding of line chip columns (the rows Mosaic.lineFill produces: is_core, index_id, key,
// wkb) into the flat layout of line_isect.h.  Accepts what JTS WKBReader gives ST_IntersectsAggregate
// for such a chip: Point (1), MultiPoint (4), LineString (2), MultiLineString (5), either byte order,
// the ISO Z/M and EWKB flag variants (GeomBuilder::header); Z and M ordinates are skipped.
//   POINT            one 1-vertex piece; NaN ordinates (POINT EMPTY): an empty chip
//   MULTIPOINT       one 1-vertex piece per non-empty member
//   LINESTRING       one piece; no points: an empty chip; exactly one: malformed (JTS refuses it)
//   MULTILINESTRING  one piece per non-empty member, in order
// A zero-length row is an empty chip.  Anything else (polygonal types, collections, unknown types, a
// truncated buffer, a member of another type) is malformed; a NaN inside a line is its own error.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mosaic_hip.h"
#include "geom_build.h"
#include "line_isect.h"

namespace mosaic {

struct LineChipBuilder {
    std::vector<pip::Vec2> verts;
    std::vector<uint32_t> piece_start{0};
    std::vector<pip::Box> piece_bbox;
    std::vector<uint32_t> chip_piece{0};
    std::vector<pip::Box> chip_bbox;
    std::vector<int64_t> cell;
    std::vector<int32_t> key;
    std::vector<uint8_t> is_core;
    std::string error;

    using Reader = GeomBuilder::Reader;

    lineisect::LineStore view() const {
        return lineisect::LineStore{verts.data(), piece_start.data(), piece_bbox.data(), chip_piece.data(), chip_bbox.data()};
    }
    size_t size() const { return chip_bbox.size(); }

    void end_piece(size_t v0) {
        pip::Box b = {INFINITY, INFINITY, -INFINITY, -INFINITY};
        for (size_t i = v0; i < verts.size(); i++) {
            b.minx = std::min(b.minx, verts[i].x);
            b.maxx = std::max(b.maxx, verts[i].x);
            b.miny = std::min(b.miny, verts[i].y);
            b.maxy = std::max(b.maxy, verts[i].y);
        }
        piece_bbox.push_back(b);
        piece_start.push_back((uint32_t)verts.size());
    }

    // MOSAIC_OK, MOSAIC_E_WKB or MOSAIC_E_NAN
    int point(Reader& r, bool le, int dims) {
        const double x = r.f64(le), y = r.f64(le);
        for (int d = 2; d < dims; d++) r.f64(le);
        if (r.fail) return MOSAIC_E_WKB;
        if (x != x || y != y) return MOSAIC_OK;  // POINT EMPTY
        const size_t v0 = verts.size();
        verts.push_back({x, y});
        end_piece(v0);
        return MOSAIC_OK;
    }

    int line(Reader& r, bool le, int dims) {
        const uint32_t npts = r.u32(le);
        if (r.fail || (uint64_t)npts * 8 * (uint64_t)dims > r.len - r.pos) return MOSAIC_E_WKB;
        if (npts == 0) return MOSAIC_OK;
        if (npts == 1) {
            error = "a LineString of one point";
            return MOSAIC_E_WKB;
        }
        const size_t v0 = verts.size();
        for (uint32_t i = 0; i < npts; i++) {
            const double x = r.f64(le), y = r.f64(le);
            for (int d = 2; d < dims; d++) r.f64(le);
            if (x != x || y != y) {
                error = "NaN coordinate in a line";
                return MOSAIC_E_NAN;
            }
            verts.push_back({x, y});
        }
        end_piece(v0);
        return MOSAIC_OK;
    }

    int geometry(const uint8_t* wkb, size_t len) {
        if (len == 0) return MOSAIC_OK;
        Reader r{wkb, len, 0};
        bool le;
        uint32_t type;
        int dims;
        if (!GeomBuilder::header(r, le, type, dims)) return MOSAIC_E_WKB;
        if (type == 1) return point(r, le, dims);
        if (type == 2) return line(r, le, dims);
        if (type == 4 || type == 5) {
            const uint32_t n = r.u32(le);
            if (r.fail) return MOSAIC_E_WKB;
            for (uint32_t k = 0; k < n; k++) {
                bool le2;
                uint32_t t2;
                int d2;
                if (!GeomBuilder::header(r, le2, t2, d2)) return MOSAIC_E_WKB;
                if (t2 != (type == 4 ? 1u : 2u)) {
                    error = "a member of type " + std::to_string(t2) + " in a multi-geometry of type " + std::to_string(type);
                    return MOSAIC_E_WKB;
                }
                if (int rc = type == 4 ? point(r, le2, d2) : line(r, le2, d2)) return rc;
            }
            return MOSAIC_OK;
        }
        error = "unsupported WKB geometry type " + std::to_string(type) +
                " (Point/MultiPoint/LineString/MultiLineString expected)";
        return MOSAIC_E_WKB;
    }

    // Appends one chip; a non-zero status leaves `error` set and the builder unusable.
    int add(const uint8_t* wkb, size_t len) {
        error.clear();
        const size_t m0 = piece_bbox.size();
        const int rc = geometry(wkb, len);
        if (rc) {
            if (error.empty()) error = "malformed WKB";
            return rc;
        }
        pip::Box b = {INFINITY, INFINITY, -INFINITY, -INFINITY};
        for (size_t m = m0; m < piece_bbox.size(); m++) {
            b.minx = std::min(b.minx, piece_bbox[m].minx);
            b.maxx = std::max(b.maxx, piece_bbox[m].maxx);
            b.miny = std::min(b.miny, piece_bbox[m].miny);
            b.maxy = std::max(b.maxy, piece_bbox[m].maxy);
        }
        chip_bbox.push_back(b);
        chip_piece.push_back((uint32_t)piece_bbox.size());
        return MOSAIC_OK;
    }
};

// The chip columns into `b`.  Returns a status and leaves the message in `err`.
inline int build_line_chips(int64_t n, const uint8_t* is_core, const int64_t* index_id, const int32_t* key,
                            const void* wkb_offsets, int offsets32, const uint8_t* wkb, LineChipBuilder& b, std::string& err) {
    if (n < 0 || (n > 0 && (!is_core || !index_id || !key || !wkb_offsets))) {
        err = "invalid argument";
        return MOSAIC_E_ARG;
    }
    if (n >= ((int64_t)1 << 31)) {
        err = "line chips: fewer than 2^31 chips at the most";
        return MOSAIC_E_CAPACITY;
    }
    const int32_t* o32 = (const int32_t*)wkb_offsets;
    const int64_t* o64 = (const int64_t*)wkb_offsets;
    b.cell.assign(index_id, index_id + n);
    b.key.assign(key, key + n);
    b.is_core.resize((size_t)n);
    b.chip_bbox.reserve((size_t)n);
    b.chip_piece.reserve((size_t)n + 1);
    for (int64_t i = 0; i < n; i++) {
        b.is_core[(size_t)i] = is_core[i] ? 1 : 0;
        if (key[i] < 0) {
            err = "line chip " + std::to_string(i) + ": negative key";
            return MOSAIC_E_ARG;
        }
        const int64_t lo = offsets32 ? (int64_t)o32[i] : o64[i], hi = offsets32 ? (int64_t)o32[i + 1] : o64[i + 1];
        if (lo < 0 || hi < lo || (hi > lo && !wkb)) {
            err = "line chip " + std::to_string(i) + ": bad wkb offsets";
            return MOSAIC_E_ARG;
        }
        if (int rc = b.add(hi > lo ? wkb + lo : nullptr, (size_t)(hi - lo))) {
            err = "line chip " + std::to_string(i) + ": " + b.error;
            return rc;
        }
        if (b.verts.size() >= 0xffffffffULL) {
            err = "line chips: fewer than 2^32 - 1 vertices at the most";
            return MOSAIC_E_CAPACITY;
        }
    }
    return MOSAIC_OK;
}

}  // namespace mosaic
