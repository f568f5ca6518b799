// The measures of one stored geometry -- st_area, st_length / st_perimeter, st_centroid / st_centroid2D,
// st_numpoints, st_xmin / st_xmax / st_ymin / st_ymax -- on the host and on gfx950: the reference's
// functions/MosaicContext.scala ST_Area, ST_Length (ST_Perimeter is the same expression), ST_Centroid,
// ST_NumPoints, ST_XMin .. ST_YMax -> core/geometry/MosaicGeometryJTS.{getArea, getLength, getCentroid,
// numPoints, minMaxCoord} -> JTS 1.19 Geometry.getArea / getLength / getCentroid / getNumPoints.
// The columns are the GeomStore + part-kind layout that st_distance.h documents: a point is a part of
// one ring of one vertex, a component line a part of one open ring, polygon rings are stored closed.
//
// The arithmetic is restated from recall of JTS 1.19 (no JTS source or JVM was at hand), as llclip.h
// and st_distance.h were: Area.ofRingSigned, Polygon.getArea, GeometryCollection.getArea, Length.ofLine,
// Polygon.getLength, Centroid (addShell / addHole / addTriangle / addLineSegments / addPoint /
// getCentroid) and Orientation.isCCW.  Every operation is one IEEE double operation in the order
// written (-ffp-contract=off).
//
// Semantics of `measure`, the sequential definition:
//   area      per ring of n stored vertices: 0 if n < 3, else sum += (x[i] - x[0]) * (y[i-1] - y[i+1]) for
//             i = 1 .. n-2 in that order, halved.  A polygon part is ((0 + |shell|) - |hole 1|) - ...,
//             a geometry the in-order sum of its parts from 0.0; line and point parts add 0.0.
//   length    per ring or component line the in-order sum of sqrt(dx * dx + dy * dy); a part is the
//             in-order sum of its rings (shell plus holes: the perimeter), a geometry that of its parts;
//             point parts add 0.0.
//   centroid  one accumulation over the whole geometry, part after part and ring after ring:
//             area part (polygon rings): the base point is the first vertex of the part's shell, the sign
//               of a shell is +1 unless isCCW, of a hole +1 if isCCW; per segment (p1, p2):
//               area2 = (p1x - bx)(p2y - by) - (p2x - bx)(p1y - by), cg3 += sign * area2 * (b + p1 + p2),
//               areasum2 += sign * area2.  This is jts_centroid of polyfill.hip / oracle/polyfill.c.
//             line part (polygon rings too, and component lines): per segment d = its length; d == 0.0 is
//               skipped; run_len += d, line_sum += d * ((a + b) / 2); after the run total_len += run_len,
//               and a run of length 0.0 adds its first vertex as a point.
//             point part: pt_sum += v, pt_count += 1.
//             Result: |areasum2| > 0 -> cg3 / 3 / areasum2; else total_len > 0 -> line_sum / total_len;
//             else pt_count > 0 -> pt_sum / pt_count; else (NaN, NaN) (JTS: null).
//   numpoints the stored vertex count (a closed ring counts its closing vertex).
//   bounds    the stored geom_bbox; NaN on all four for a geometry without a vertex (the reference
//             throws there).
// An empty geometry: area 0.0, length 0.0, centroid (NaN, NaN), numpoints 0, bounds NaN.
//
// The kernels of st_measures.hip compute the per-segment terms (`area_term`, `tri_terms`,
// `line_terms`: products, differences and square roots that do not depend on any order) on many
// lanes and run the additions (`Acc::add_tri`, `Acc::add_seg`, ...) on one lane in the order of
// `measure`, so they return its bits.  isCCW's first loop is a search for the last rising vertex of
// the greatest y (`ccw_up_hi`), which a wave answers by a reduction; the rest (`ccw_from_up_hi`) is
// shared.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pip_device.h"
#include "st_distance.h"

namespace mosaic {
namespace meas {

using pip::Box;
using pip::GeomStore;
using pip::Vec2;

enum { kArea = 1, kLength = 2, kCentroid = 4 };  // what `measure` computes besides numpoints

// ---- terms: no addition into a running sum ----
// Area.ofRingSigned's term i, 1 <= i <= n - 2
MOSAIC_HD double area_term(const Vec2* v, uint32_t i) {
    const double x = v[i].x - v[0].x;
    return x * (v[i - 1].y - v[i + 1].y);
}

// Centroid.addTriangle(base, p1, p2, sign > 0): the three addends
MOSAIC_HD void tri_terms(Vec2 b, Vec2 p1, Vec2 p2, double sign, double& tx, double& ty, double& ta) {
    const double cx = b.x + p1.x + p2.x;
    const double cy = b.y + p1.y + p2.y;
    const double area2 = (p1.x - b.x) * (p2.y - b.y) - (p2.x - b.x) * (p1.y - b.y);
    tx = sign * area2 * cx;
    ty = sign * area2 * cy;
    ta = sign * area2;
}

// a segment's length (Length.ofLine, Coordinate.distance) and Centroid.addLineSegments's two addends
MOSAIC_HD void line_terms(Vec2 a, Vec2 b, double& d, double& mx, double& my) {
    const double dx = a.x - b.x;
    const double dy = a.y - b.y;
    d = sqrt(dx * dx + dy * dy);
    mx = d * ((a.x + b.x) / 2);
    my = d * ((a.y + b.y) / 2);
}

// ---- Orientation.isCCW of a closed ring of n stored vertices ----
// the first loop: the last i in [1, n - 1] with y[i] > y[i-1] and y[i] >= every such y before it and
// y[0]; 0 if there is none.  Equivalently: the greatest i among the rising vertices of the greatest y,
// if that y >= y[0] -- what the wave reduction of st_measures.hip computes.
MOSAIC_HD uint32_t ccw_up_hi(const Vec2* v, uint32_t n) {
    uint32_t up_hi = 0;
    double prev_y = v[0].y, hi_y = v[0].y;
    for (uint32_t i = 1; i < n; i++) {
        const double py = v[i].y;
        if (py > prev_y && py >= hi_y) {
            up_hi = i;
            hi_y = py;
        }
        prev_y = py;
    }
    return up_hi;
}

MOSAIC_HD bool eq2(Vec2 a, Vec2 b) { return a.x == b.x && a.y == b.y; }

MOSAIC_HD bool ccw_from_up_hi(const Vec2* v, uint32_t n, uint32_t up_hi) {
    const uint32_t npts = n - 1;
    if (up_hi == 0) return false;
    const uint32_t up_low = up_hi - 1;
    const double hi_y = v[up_hi].y;
    uint32_t down_low = up_hi;
    do {
        down_low = (down_low + 1) % npts;
    } while (down_low != up_hi && v[down_low].y == hi_y);
    const uint32_t down_hi = down_low > 0 ? down_low - 1 : npts - 1;
    if (eq2(v[up_hi], v[down_hi])) {
        if (eq2(v[up_low], v[up_hi]) || eq2(v[down_low], v[up_hi]) || eq2(v[up_low], v[down_low])) return false;
        return pip::orientation_index(v[up_low].x, v[up_low].y, v[up_hi].x, v[up_hi].y, v[down_low].x, v[down_low].y) == 1;
    }
    return v[down_hi].x - v[up_hi].x < 0;
}

MOSAIC_HD bool is_ccw(const Vec2* v, uint32_t n) {
    if (n < 4) return false;  // nPts = n - 1 < 3
    return ccw_from_up_hi(v, n, ccw_up_hi(v, n));
}

// the sign of a ring's triangles: a shell counts positive unless it is CCW, a hole if it is
MOSAIC_HD double ring_sign(bool shell, bool ccw) { return (shell ? !ccw : ccw) ? 1.0 : -1.0; }

// ---- the additions, in the order of `measure` ----
struct Acc {
    // area
    double ring_sum = 0, part_area = 0, area = 0;
    // length
    double ring_len = 0, part_len = 0, length = 0;
    // Centroid
    double cg3x = 0, cg3y = 0, a2 = 0, lsx = 0, lsy = 0, run_len = 0, total_len = 0, psx = 0, psy = 0;
    int64_t pts = 0;

    MOSAIC_HD void begin_ring() { ring_sum = ring_len = run_len = 0; }
    MOSAIC_HD void add_area_term(double t) { ring_sum += t; }
    MOSAIC_HD void add_len(double d) { ring_len += d; }
    MOSAIC_HD void add_tri(double tx, double ty, double ta) {
        cg3x += tx;
        cg3y += ty;
        a2 += ta;
    }
    MOSAIC_HD void add_seg(double d, double mx, double my) {
        if (d == 0.0) return;
        run_len += d;
        lsx += mx;
        lsy += my;
    }
    MOSAIC_HD void add_point(Vec2 p) {
        pts += 1;
        psx += p.x;
        psy += p.y;
    }
    // the end of a ring of a polygon part: Polygon.getArea / getLength's step, addLineSegments's tail
    MOSAIC_HD void end_polygon_ring(bool shell, uint32_t n, Vec2 first, int what) {
        if (what & kArea) {
            const double a = fabs(n < 3 ? 0.0 : ring_sum / 2.0);
            if (shell)
                part_area += a;
            else
                part_area -= a;
        }
        if (what & kLength) part_len += ring_len;
        if (what & kCentroid) end_run(first);
    }
    // the end of a component line
    MOSAIC_HD void end_line(Vec2 first, int what) {
        if (what & kLength) part_len += ring_len;
        if (what & kCentroid) end_run(first);
    }
    MOSAIC_HD void end_run(Vec2 first) {
        total_len += run_len;
        if (run_len == 0.0) add_point(first);
    }
    MOSAIC_HD void end_part() {
        area += part_area;
        length += part_len;
        part_area = part_len = 0;
    }
    MOSAIC_HD void centroid(double& cx, double& cy) const {
        if (fabs(a2) > 0.0) {
            cx = cg3x / 3 / a2;
            cy = cg3y / 3 / a2;
        } else if (total_len > 0.0) {
            cx = lsx / total_len;
            cy = lsy / total_len;
        } else if (pts > 0) {
            cx = psx / (double)pts;
            cy = psy / (double)pts;
        } else {
            cx = cy = NAN;
        }
    }
};

// the vertices of geometry g: [v0, v1) of the store (its rings are contiguous)
MOSAIC_HD void geom_span(const GeomStore& s, uint32_t g, uint32_t& v0, uint32_t& v1) {
    uint32_t r0, r1;
    dist::geom_rings(s, g, r0, r1);
    v0 = s.ring_start[r0];
    v1 = s.ring_start[r1];
}

struct Measures {
    double area, length, cx, cy;
    int64_t numpoints;
    Box box;
};

// numpoints and the bounds, which need no walk
MOSAIC_HD void stored(const GeomStore& s, uint32_t g, Measures& m) {
    uint32_t v0, v1;
    geom_span(s, g, v0, v1);
    m.numpoints = (int64_t)(v1 - v0);
    m.box = v1 > v0 ? s.geom_bbox[g] : Box{NAN, NAN, NAN, NAN};
}

// The definition.  kinds: the column's part kinds; what: kArea | kLength | kCentroid.
MOSAIC_HD Measures measure(const GeomStore& s, const uint8_t* kinds, uint32_t g, int what) {
    Measures m;
    stored(s, g, m);
    Acc acc;
    Vec2 base = {0, 0};
    for (uint32_t p = s.geom_part[g]; p < s.geom_part[g + 1]; p++) {
        const uint8_t kind = kinds[p];
        for (uint32_t r = s.part_ring[p]; r < s.part_ring[p + 1]; r++) {
            const Vec2* v = s.verts + s.ring_start[r];
            const uint32_t n = s.ring_start[r + 1] - s.ring_start[r];
            if (n == 0) continue;
            if (kind == kPartPoint) {
                if (what & kCentroid) acc.add_point(v[0]);
                continue;
            }
            acc.begin_ring();
            const bool polygon = kind == kPartPolygon, shell = r == s.part_ring[p];
            double sign = 1.0;
            if (polygon && (what & kCentroid)) {
                if (shell) base = v[0];
                sign = ring_sign(shell, is_ccw(v, n));
            }
            for (uint32_t k = 0; k + 1 < n; k++) {
                if (polygon && (what & kArea) && k >= 1) acc.add_area_term(area_term(v, k));
                if (polygon && (what & kCentroid)) {
                    double tx, ty, ta;
                    tri_terms(base, v[k], v[k + 1], sign, tx, ty, ta);
                    acc.add_tri(tx, ty, ta);
                }
                if (what & (kLength | kCentroid)) {
                    double d, mx, my;
                    line_terms(v[k], v[k + 1], d, mx, my);
                    if (what & kLength) acc.add_len(d);
                    if (what & kCentroid) acc.add_seg(d, mx, my);
                }
            }
            if (polygon)
                acc.end_polygon_ring(shell, n, v[0], what);
            else
                acc.end_line(v[0], what);
        }
        acc.end_part();
    }
    m.area = acc.area;
    m.length = acc.length;
    acc.centroid(m.cx, m.cy);
    return m;
}

}  // namespace meas
}  // namespace mosaic
