// Host-side builder of a geometry column (mosaic_geoms, st_distance.hip) in the flat ring layout of
// pip_device.h, for the geometry types st_distance serves: Point, MultiPoint, LineString,
// MultiLineString, Polygon, MultiPolygon.  A point is a part of kind kPartPoint with one ring of one
// vertex; a component line is a part of kind kPartLine with one open ring of two or more vertices
// (st_distance.h).  WKB rows are decoded with GeomBuilder's reader (either byte order, ISO Z/M and
// EWKB flag variants); what the chip tables and mosaic_st_contains accept is untouched.  Row status
// follows mosaic_point_geom_to_cell: null rows MOSAIC_ROW_NULL; GeometryCollection, POINT EMPTY and
// undecodable rows MOSAIC_ROW_PATH; both hold an empty geometry.
//
// Lines are opt-in per column (`lines`, MOSAIC_GEOMS_LINES).  Without it a LineString /
// MultiLineString WKB row is MOSAIC_ROW_PATH, as it was before the engine served lines: callers
// that route such rows to the reference's row path keep doing so.  With it LINESTRING EMPTY and
// MULTILINESTRING EMPTY are MOSAIC_ROW_OK rows without a facet (distance 0.0, like POLYGON EMPTY),
// an empty member of a MultiLineString adds no part, and a component of exactly one vertex makes
// the row MOSAIC_ROW_PATH (JTS cannot construct that LineString).
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "geom_build.h"
#include "st_distance.h"

namespace mosaic {

enum { kRowNull = 0, kRowOk = 1, kRowPath = 2 };  // MOSAIC_ROW_*

struct GeomColumn {
    GeomBuilder b;
    bool lines = false;  // decode WKB types 2 and 5 into line parts
    std::vector<uint8_t> part_kind;
    std::vector<int32_t> row_status;
    std::vector<uint32_t> geom_facets;
    int64_t n_row_path = 0;

    int64_t size() const { return (int64_t)row_status.size(); }
    pip::GeomStore store() const {
        return pip::GeomStore{b.verts.data(), b.ring_start.data(), b.ring_bbox.data(), b.part_ring.data(),
                              b.geom_part.data(), b.geom_bbox.data()};
    }

    struct Mark {
        size_t verts, rings, parts;
    };
    Mark mark() const { return Mark{b.verts.size(), b.ring_bbox.size(), b.part_ring.size()}; }
    void rollback(const Mark& m) {
        b.verts.resize(m.verts);
        b.ring_bbox.resize(m.rings);
        b.ring_start.resize(m.rings + 1);
        b.part_ring.resize(m.parts);
        part_kind.resize(m.parts - 1);
    }

    void point_part(double x, double y) {
        b.verts.push_back({x, y});
        b.ring_bbox.push_back({x, y, x, y});
        b.ring_start.push_back((uint32_t)b.verts.size());
        b.part_ring.push_back((uint32_t)b.ring_bbox.size());
        part_kind.push_back(kPartPoint);
    }
    bool polygon_part(GeomBuilder::Reader& r, bool le, int dims) {
        if (!b.polygon(r, le, dims)) return false;
        part_kind.push_back(kPartPolygon);
        return true;
    }
    // the part of the vertices pushed since v0: one open ring.  No vertex: no part.  false: one vertex
    bool close_line_part(size_t v0) {
        const size_t n = b.verts.size() - v0;
        if (n == 0) return true;
        if (n == 1) return false;
        pip::Box box = {INFINITY, INFINITY, -INFINITY, -INFINITY};
        for (size_t i = v0; i < b.verts.size(); i++) {
            box.minx = std::min(box.minx, b.verts[i].x);
            box.maxx = std::max(box.maxx, b.verts[i].x);
            box.miny = std::min(box.miny, b.verts[i].y);
            box.maxy = std::max(box.maxy, b.verts[i].y);
        }
        b.ring_bbox.push_back(box);
        b.ring_start.push_back((uint32_t)b.verts.size());
        b.part_ring.push_back((uint32_t)b.ring_bbox.size());
        part_kind.push_back(kPartLine);
        return true;
    }
    bool line_part(GeomBuilder::Reader& r, bool le, int dims) {
        const uint32_t npts = r.u32(le);
        if (r.fail || (uint64_t)npts * 8 * dims > r.len - r.pos) return false;
        const size_t v0 = b.verts.size();
        for (uint32_t i = 0; i < npts; i++) {
            const double x = r.f64(le), y = r.f64(le);
            for (int d = 2; d < dims; d++) r.f64(le);
            b.verts.push_back({x, y});
        }
        return !r.fail && close_line_part(v0);
    }
    // closes the row that began at mark m
    void end_row(const Mark& m, int32_t status) {
        b.geom_part.push_back((uint32_t)(b.part_ring.size() - 1));
        pip::Box box = {INFINITY, INFINITY, -INFINITY, -INFINITY};
        for (size_t i = m.verts; i < b.verts.size(); i++) {
            box.minx = std::min(box.minx, b.verts[i].x);
            box.maxx = std::max(box.maxx, b.verts[i].x);
            box.miny = std::min(box.miny, b.verts[i].y);
            box.maxy = std::max(box.maxy, b.verts[i].y);
        }
        b.geom_bbox.push_back(box);
        uint64_t f = 0;
        for (size_t r = m.rings; r < b.ring_bbox.size(); r++) f += dist::ring_facets(b.ring_start[r + 1] - b.ring_start[r]);
        geom_facets.push_back((uint32_t)f);
        row_status.push_back(status);
        if (status == kRowPath) n_row_path++;
    }
    void add_empty(int32_t status) { end_row(mark(), status); }

    // 1 decoded, 0 a row for the row path
    static bool read_point(GeomBuilder::Reader& r, bool le, int dims, double& x, double& y) {
        x = r.f64(le);
        y = r.f64(le);
        for (int d = 2; d < dims; d++) r.f64(le);
        return !r.fail;
    }
    bool decode(const uint8_t* wkb, size_t len) {
        GeomBuilder::Reader r{wkb, len, 0};
        bool le;
        uint32_t type;
        int dims;
        if (len == 0 || !GeomBuilder::header(r, le, type, dims)) return false;
        double x, y;
        if (type == 1) {
            if (!read_point(r, le, dims, x, y) || std::isnan(x) || std::isnan(y)) return false;  // POINT EMPTY: row path
            point_part(x, y);
            return true;
        }
        if (type == 3) return polygon_part(r, le, dims);
        if (type == 2 && lines) return line_part(r, le, dims);
        if (type != 4 && type != 6 && !(type == 5 && lines)) return false;
        const uint32_t n = r.u32(le);
        if (r.fail) return false;
        for (uint32_t k = 0; k < n; k++) {
            bool le2;
            uint32_t t2;
            int d2;
            if (!GeomBuilder::header(r, le2, t2, d2) || t2 != (type == 4 ? 1u : type == 5 ? 2u : 3u)) return false;
            if (type == 6) {
                if (!polygon_part(r, le2, d2)) return false;
            } else if (type == 5) {
                if (!line_part(r, le2, d2)) return false;
            } else {
                if (!read_point(r, le2, d2, x, y)) return false;
                if (!std::isnan(x) && !std::isnan(y)) point_part(x, y);  // an empty member adds no coordinate
            }
        }
        return true;
    }
    void add_wkb(const uint8_t* wkb, size_t len) {
        const Mark m = mark();
        if (decode(wkb, len)) {
            end_row(m, kRowOk);
        } else {
            rollback(m);
            end_row(m, kRowPath);
        }
    }
    void add_point(double x, double y) {
        const Mark m = mark();
        const bool ok = !std::isnan(x) && !std::isnan(y);
        if (ok) point_part(x, y);
        end_row(m, ok ? kRowOk : kRowPath);
    }
    // a PolygonSet: geom_parts[n + 1], part_rings, ring_offsets, xy interleaved; false on inconsistent offsets
    bool add_arrays(int64_t n, const int64_t* geom_parts, const int64_t* part_rings, const int64_t* ring_offsets,
                    const double* xy) {
        for (int64_t g = 0; g < n; g++) {
            const Mark m = mark();
            if (geom_parts[g + 1] < geom_parts[g]) return false;
            for (int64_t p = geom_parts[g]; p < geom_parts[g + 1]; p++) {
                if (part_rings[p + 1] < part_rings[p]) return false;
                for (int64_t r = part_rings[p]; r < part_rings[p + 1]; r++) {
                    if (ring_offsets[r + 1] < ring_offsets[r]) return false;
                    pip::Box box = {INFINITY, INFINITY, -INFINITY, -INFINITY};
                    for (int64_t i = ring_offsets[r]; i < ring_offsets[r + 1]; i++) {
                        const double x = xy[2 * i], y = xy[2 * i + 1];
                        b.verts.push_back({x, y});
                        box.minx = std::min(box.minx, x);
                        box.maxx = std::max(box.maxx, x);
                        box.miny = std::min(box.miny, y);
                        box.maxy = std::max(box.maxy, y);
                    }
                    b.ring_bbox.push_back(box);
                    b.ring_start.push_back((uint32_t)b.verts.size());
                }
                b.part_ring.push_back((uint32_t)b.ring_bbox.size());
                part_kind.push_back(kPartPolygon);
            }
            end_row(m, kRowOk);
        }
        return true;
    }
    // a LineSet: geom_lines[n + 1], line_offsets, xy interleaved; false on inconsistent offsets.  A
    // component of one vertex makes its row a row for the row path.
    bool add_lines(int64_t n, const int64_t* geom_lines, const int64_t* line_offsets, const double* xy) {
        for (int64_t g = 0; g < n; g++) {
            const Mark m = mark();
            if (geom_lines[g] < 0 || geom_lines[g + 1] < geom_lines[g]) return false;
            bool ok = true;
            for (int64_t l = geom_lines[g]; l < geom_lines[g + 1]; l++) {
                if (line_offsets[l] < 0 || line_offsets[l + 1] < line_offsets[l]) return false;
                if (!ok) continue;
                const size_t v0 = b.verts.size();
                for (int64_t i = line_offsets[l]; i < line_offsets[l + 1]; i++) b.verts.push_back({xy[2 * i], xy[2 * i + 1]});
                ok = close_line_part(v0);
            }
            if (!ok) rollback(m);
            end_row(m, ok ? kRowOk : kRowPath);
        }
        return true;
    }
    bool too_large() const { return b.verts.size() >= 0xffffffffull || row_status.size() >= 0xffffffffull; }
};

}  // namespace mosaic
