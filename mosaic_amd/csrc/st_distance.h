// JTS 1.19 `Geometry.distance` (DistanceOp.distance) for the geometry types this engine serves --
// Point, MultiPoint, LineString, MultiLineString, Polygon and MultiPolygon on either side -- on the
// host and on gfx950: the
// reference's st_distance (functions/MosaicContext.scala:146 ST_Distance ->
// expressions/geometry/ST_Distance.scala:34-36 -> core/geometry/MosaicGeometryJTS.distance -> JTS
// Geometry.distance; docs/source/api/spatial-functions.rst:416-471).
//
// Semantics (st_distance(g, h), g the left geometry):
//   * either geometry empty (no coordinate)                                   -> 0.0
//   * containment (computeContainmentDistance: PolygonExtracter x ConnectedElementLocationFilter),
//     in both directions: for each polygon part P of one side and each connected component of the
//     other side (a point, a component line, or a polygon's shell), the component's first
//     coordinate pt: locate_in_polygon(P, pt) != EXTERIOR -> 0.0.  Boundary counts; each polygon
//     part is located on its own (no MultiPolygon Mod-2 rule).  Only polygon parts can contain: a
//     line part is a component and never a container, whether its first vertex equals its last or
//     not (a point strictly inside a closed LineString is at a positive distance).
//   * otherwise the minimum over (facets of g) x (facets of h) of segment_segment / point_segment /
//     point_point below (Distance.segmentToSegment, Distance.pointToSegment, Coordinate.distance).
//     Facets are every ring's segments, holes included, every component line's segments
//     (LinearComponentExtracter yields lines and polygon rings alike) and every point
//     (PointExtracter).  A line of n >= 2 vertices has n - 1 segments: nothing closes it.
// Every operation is one IEEE double operation in the order written (-ffp-contract=off).  `min` is
// exact, so the result does not depend on the order the facet pairs are visited in: the kernels of
// st_distance.hip, which prune and reorder, return the bits of the sequential driver `distance`.
//
// Layout: a point is stored as a part with one ring of one vertex, and a ring of one vertex has the
// single facet (v, v).  segment_segment on such a facet takes its A == B / C == D branches and is
// then point_segment / point_point exactly, so the drivers treat every facet as a segment.  A
// one-vertex ring never contains anything (locate_in_ring sees no segment), so point parts need no
// special case in the containment step either.  A component line of a LineString /
// MultiLineString is a part of kind kPartLine with one open ring of n >= 2 vertices; polygon rings
// are stored closed (first == last), so "n - 1 segments per ring" serves both and no driver ever
// adds a closing segment.  An open ring of two or more vertices would be a container to a driver
// that does not know the part kinds, so the definition takes them: `distance` with the two
// part_kind arrays.  The form without them treats every part as a possible container; it is the
// same function on columns of points and polygons and is kept for those.
//
// Two caveats:
//   * The arithmetic is restated from recall of JTS 1.19 (no JTS source or JVM was at hand), as
//     llclip.h was.
//   * The reference's only committed number is one ulp from this arithmetic: the docs' example
//     st_distance('POLYGON ((30 10, 40 40, 20 40, 10 20, 30 10))', 'POINT (5 5)') prints
//     15.652475842498529; this arithmetic gives 15.652475842498527 (the exact value is 7 sqrt(5) =
//     15.6524758424985278...).  The documented digits equal sqrt(245), the distance to the projected
//     foot point (12, 19): that is how the ESRI API, the docs' default when they were written,
//     computes it.  The JTS form is kept.  Should the reference become runnable, first check whether
//     Coordinate.distance in 1.19 is Math.hypot rather than sqrt(dx * dx + dy * dy).
#pragma once
#include <math.h>
#include <stdint.h>

#include "pip_device.h"

namespace mosaic {

// kind of a part of a geometry column (geoms_build.h): a polygon with its rings, a point (one ring
// of one vertex), a component line (one open ring)
enum { kPartPolygon = 0, kPartPoint = 1, kPartLine = 2 };

namespace dist {

using pip::Box;
using pip::GeomStore;
using pip::Vec2;

// Coordinate.distance
MOSAIC_HD double point_point(Vec2 p, Vec2 q) {
    const double dx = p.x - q.x;
    const double dy = p.y - q.y;
    return sqrt(dx * dx + dy * dy);
}

// Distance.pointToSegment(p, A, B)
MOSAIC_HD double point_segment(Vec2 p, Vec2 A, Vec2 B) {
    if (A.x == B.x && A.y == B.y) return point_point(p, A);
    const double len2 = (B.x - A.x) * (B.x - A.x) + (B.y - A.y) * (B.y - A.y);
    const double r = ((p.x - A.x) * (B.x - A.x) + (p.y - A.y) * (B.y - A.y)) / len2;
    if (r <= 0.0) return point_point(p, A);
    if (r >= 1.0) return point_point(p, B);
    const double s = ((A.y - p.y) * (B.x - A.x) - (A.x - p.x) * (B.y - A.y)) / len2;
    return fabs(s) * sqrt(len2);
}

MOSAIC_HD double min2(double a, double b) { return b < a ? b : a; }

// Envelope.intersects(p1, p2, q1, q2)
MOSAIC_HD bool envelopes_intersect(Vec2 p1, Vec2 p2, Vec2 q1, Vec2 q2) {
    double minq = q1.x < q2.x ? q1.x : q2.x;
    double maxq = q1.x > q2.x ? q1.x : q2.x;
    double minp = p1.x < p2.x ? p1.x : p2.x;
    double maxp = p1.x > p2.x ? p1.x : p2.x;
    if (minp > maxq) return false;
    if (maxp < minq) return false;
    minq = q1.y < q2.y ? q1.y : q2.y;
    maxq = q1.y > q2.y ? q1.y : q2.y;
    minp = p1.y < p2.y ? p1.y : p2.y;
    maxp = p1.y > p2.y ? p1.y : p2.y;
    if (minp > maxq) return false;
    if (maxp < minq) return false;
    return true;
}

// Distance.segmentToSegment(A, B, C, D): AB from the left geometry, CD from the right
MOSAIC_HD double segment_segment(Vec2 A, Vec2 B, Vec2 C, Vec2 D) {
    if (A.x == B.x && A.y == B.y) return point_segment(A, C, D);
    if (C.x == D.x && C.y == D.y) return point_segment(D, A, B);
    bool no_intersection = false;
    if (!envelopes_intersect(A, B, C, D)) {
        no_intersection = true;
    } else {
        const double denom = (B.x - A.x) * (D.y - C.y) - (B.y - A.y) * (D.x - C.x);
        if (denom == 0) {
            no_intersection = true;
        } else {
            const double r_num = (A.y - C.y) * (D.x - C.x) - (A.x - C.x) * (D.y - C.y);
            const double s_num = (A.y - C.y) * (B.x - A.x) - (A.x - C.x) * (B.y - A.y);
            const double s = s_num / denom;
            const double r = r_num / denom;
            if ((r < 0) || (r > 1) || (s < 0) || (s > 1)) no_intersection = true;
        }
    }
    if (no_intersection)
        return min2(min2(point_segment(A, C, D), point_segment(B, C, D)),
                    min2(point_segment(C, A, B), point_segment(D, A, B)));
    return 0.0;
}

// ---- facets of the flat layout ----
// a ring of n vertices: n - 1 segments; a ring of one vertex (a point): the facet (v, v)
MOSAIC_HD uint32_t ring_facets(uint32_t n) { return n > 1 ? n - 1 : n; }
MOSAIC_HD void ring_facet(const Vec2* v, uint32_t n, uint32_t i, Vec2& A, Vec2& B) {
    A = v[i];
    B = v[i + 1 < n ? i + 1 : i];
}
MOSAIC_HD Box facet_box(Vec2 a, Vec2 b) {
    return Box{a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y};
}
MOSAIC_HD void geom_rings(const GeomStore& s, uint32_t g, uint32_t& r0, uint32_t& r1) {
    r0 = s.part_ring[s.geom_part[g]];
    r1 = s.part_ring[s.geom_part[g + 1]];
}
MOSAIC_HD uint64_t geom_facets(const GeomStore& s, uint32_t g) {
    uint32_t r0, r1;
    geom_rings(s, g, r0, r1);
    uint64_t f = 0;
    for (uint32_t r = r0; r < r1; r++) f += ring_facets(s.ring_start[r + 1] - s.ring_start[r]);
    return f;
}

// the first coordinate of part q's shell lies in or on polygon part p: one task of the containment step
MOSAIC_HD bool component_in_part(const GeomStore& sp, uint32_t p, const GeomStore& sq, uint32_t q) {
    const uint32_t r = sq.part_ring[q];
    if (sq.part_ring[q + 1] <= r || sq.ring_start[r + 1] <= sq.ring_start[r]) return false;
    const Vec2 pt = sq.verts[sq.ring_start[r]];
    return pip::locate_in_polygon(sp, p, pt.x, pt.y) != pip::LOC_EXTERIOR;
}
// ka: the part kinds of sa, or null for "every part may contain" (columns without line parts)
MOSAIC_HD bool contained(const GeomStore& sa, const uint8_t* ka, uint32_t a, const GeomStore& sb, uint32_t b) {
    for (uint32_t p = sa.geom_part[a]; p < sa.geom_part[a + 1]; p++) {
        if (ka && ka[p] != kPartPolygon) continue;
        for (uint32_t q = sb.geom_part[b]; q < sb.geom_part[b + 1]; q++)
            if (component_in_part(sa, p, sb, q)) return true;
    }
    return false;
}

// The definition of the result: sequential and unpruned.  ka / kb: the part kinds of the two columns.
MOSAIC_HD double distance(const GeomStore& sa, const uint8_t* ka, uint32_t g, const GeomStore& sb, const uint8_t* kb,
                          uint32_t h) {
    if (geom_facets(sa, g) == 0 || geom_facets(sb, h) == 0) return 0.0;
    if (contained(sa, ka, g, sb, h) || contained(sb, kb, h, sa, g)) return 0.0;
    uint32_t ra0, ra1, rb0, rb1;
    geom_rings(sa, g, ra0, ra1);
    geom_rings(sb, h, rb0, rb1);
    double m = INFINITY;
    for (uint32_t ra = ra0; ra < ra1; ra++) {
        const Vec2* va = sa.verts + sa.ring_start[ra];
        const uint32_t na = sa.ring_start[ra + 1] - sa.ring_start[ra];
        for (uint32_t i = 0; i < ring_facets(na); i++) {
            Vec2 A, B;
            ring_facet(va, na, i, A, B);
            for (uint32_t rb = rb0; rb < rb1; rb++) {
                const Vec2* vb = sb.verts + sb.ring_start[rb];
                const uint32_t nb = sb.ring_start[rb + 1] - sb.ring_start[rb];
                for (uint32_t j = 0; j < ring_facets(nb); j++) {
                    Vec2 C, D;
                    ring_facet(vb, nb, j, C, D);
                    m = min2(m, segment_segment(A, B, C, D));
                }
            }
        }
    }
    return m;
}

// The same for columns that hold points and polygons only: every part is taken as a possible
// container (a one-vertex ring contains nothing).  Not for columns with line parts.
MOSAIC_HD double distance(const GeomStore& sa, uint32_t g, const GeomStore& sb, uint32_t h) {
    return distance(sa, nullptr, g, sb, nullptr, h);
}

// ---- pruning (st_distance.hip) ----
// A value that no segment_segment of a facet inside box a with a facet inside box b can fall below.
// The exact distance of two such facets is at least the exact box gap; the computed gap is within a
// few ulps of that, and the pair arithmetic's absolute error is bounded by a small multiple of
// 2^-53 times the largest coordinate difference it forms (the cancellation in point_segment's cross
// product), which is at most the extent of the two boxes' union.  So the gap is scaled down by
// 2^-50 and lowered by 2^-47 times that extent.  A pair that takes segment_segment's intersection
// branch has meeting envelopes, hence a zero gap and a negative bound.
MOSAIC_HD double box_lower_bound(const Box& a, const Box& b) {
    double dx = 0, dy = 0;
    if (b.minx > a.maxx) dx = b.minx - a.maxx;
    if (a.minx > b.maxx) dx = a.minx - b.maxx;
    if (b.miny > a.maxy) dy = b.miny - a.maxy;
    if (a.miny > b.maxy) dy = a.miny - b.maxy;
    const double ex = (a.maxx > b.maxx ? a.maxx : b.maxx) - (a.minx < b.minx ? a.minx : b.minx);
    const double ey = (a.maxy > b.maxy ? a.maxy : b.maxy) - (a.miny < b.miny ? a.miny : b.miny);
    const double gap = sqrt(dx * dx + dy * dy);
    return gap * (1.0 - 0x1p-50) - (ex + ey) * 0x1p-47;
}

// layout fingerprint of what st_distance.hip shares with the other translation units (join_binned.h's rationale)
static constexpr uint64_t layout_fingerprint() {
    uint64_t h = 0xcbf29ce484222325ULL;
    for (uint64_t v : {(uint64_t)sizeof(GeomStore), (uint64_t)sizeof(Vec2), (uint64_t)sizeof(Box)})
        h = h * 0x100000001b3ULL ^ v;
    return h;
}

}  // namespace dist
}  // namespace mosaic
