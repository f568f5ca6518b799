// JTS 1.19 `Geometry.contains` (DE-9IM T*****FF*: no point of B lies in the exterior of A, and the two
// interiors share a point) for the geometry types this engine serves, on the host and on gfx950: the
// reference's st_contains over any two geometries (expressions/geometry/ST_Contains.scala ->
// core/geometry/MosaicGeometryJTS.contains -> JTS Geometry.contains).  st_within(b, a) is st_contains(a, b).
// The columns are the GeomStore + part-kind layout that st_distance.h documents; a row is of one kind
// (Point / MultiPoint: point parts, LineString / MultiLineString: line parts, Polygon / MultiPolygon:
// polygon parts), so "points only", "polygonal" and "has a line part" below sort every row.
//
// The engine decides every pair it can decide on exact predicates (orientation signs from
// CGAlgorithmsDD, comparisons) without constructing a point that is not an input vertex, and hands the
// rest to the caller's row path with a status of their own, MOSAIC_PAIR_UNDECIDED.  It never guesses.
//
// Semantics (st_contains(A = left row g, B = right row h)), the sequential driver `contains` below.
// It returns out (1 or 0) and sets *status (MOSAIC_ROW_OK or MOSAIC_PAIR_UNDECIDED; then out is 0):
//   1. either geometry has no facet                                             -> 0, OK
//   2. B's box is not covered by A's box (box_covers: four comparisons)         -> 0, OK
//      (a point of B outside A's box is in A's exterior)
//   3. B points only, A polygonal: every point of B is located in A (locate_union below).
//      1 iff no point is EXTERIOR and at least one is INTERIOR; OK.
//   4. A and B points only: 1 iff every point of B equals some point of A; OK.
//      (a point set has no boundary; its interior is the set.  Equal as Coordinate.equals2D has it,
//      x == x' and y == y': the same bits, except that -0.0 equals 0.0; no NaN is stored.)
//   5. A polygonal, B with line or polygon parts:
//      (a) some facet of B properly crosses a facet of a ring of A (proper_crossing: the four orientation
//          signs are non-zero and the two of each pair opposite)                -> 0, OK
//          The facets cross at one point interior to both and B's facet passes from one side of the
//          ring edge to the other.  One side of a ring edge of a valid polygon is A's exterior, near
//          every point of the edge that is on no other ring; the crossing point has such points of B's
//          facet arbitrarily close on either side.  So B has a point in A's exterior.
//      (b) some vertex of B is EXTERIOR to A (locate_union)                      -> 0, OK
//      (c) no facet of B meets a facet of A (pip::segments_intersect false on every pair):
//          1 iff (i) the first vertex of every part of B (a component line, a polygon part's shell) is
//          INTERIOR to a part of A, and (ii) if B has polygon parts, no ring of A (holes included) has
//          its first vertex INTERIOR to a polygon part of B (pip::locate_in_polygon, which respects
//          B's holes); otherwise 0.  OK either way.
//      (d) otherwise (the boundaries touch, nothing crosses, no vertex is outside)
//                                                                                -> 0, MOSAIC_PAIR_UNDECIDED
//          Deciding these pairs needs the midpoints of noded sub-segments: the next step.
//   6. any other left side (A with a line part, or A points only against a B that is not)
//                                                                                -> 0, MOSAIC_PAIR_UNDECIDED
//
// Proof of 5(c).  Let no facet of B meet a facet of A; A is a valid polygonal geometry, so the plane
// without A's rings is the disjoint union of the open sets int(A) and ext(A), int(A) is the disjoint
// union of the parts' interiors, and every neighbourhood of a point of a ring of A holds points of
// ext(A).  A connected set that meets no ring of A lies wholly in int(A) or wholly in ext(A); the same
// holds for a ring of A against the rings of a polygon part Q of B and int(Q), ext(Q).
//   * (i) and (ii) hold => 1.  A component line of B is connected, meets no ring of A and starts in
//     int(A): it lies in int(A).  For a polygon part Q of B the shell S lies in int(A) likewise.
//     Suppose a point x of Q is not in int(A).  If x is on a ring R of A, x is not on a ring of Q (no
//     contact), so x is in int(Q), hence all of R is, and R's first vertex is INTERIOR to Q: (ii) fails.
//     If x is in ext(A), x is in int(Q) again (Q's rings lie in int(A)); int(Q) is connected and holds
//     points of int(A) next to S, so a path inside int(Q) from there to x passes a ring of A at a
//     point of int(Q), and (ii) fails as before.  So B lies in int(A): nothing of B is in ext(A), and
//     int(B), which is not empty, lies in int(A).
//   * (i) fails => 0.  The first vertex v of a part is an end of a facet of B, so it is on no ring of
//     A; not INTERIOR, it is in ext(A).
//   * (ii) fails => 0.  The first vertex w of a ring of A lies in int(Q): a neighbourhood of w inside
//     int(Q) holds points of ext(A).
// With no contact every ring and component line of B lies wholly inside or outside A; a hole of A
// inside a polygon part of B is the only remaining way out.  Given no contact, (b) fires iff (c) would
// answer 0 through a vertex: both answer 0 then, so a kernel that locates only the first vertices of
// (c) when there was no contact returns the driver's value.
//
// locate_union: the location of a point in a polygonal geometry, from pip::locate_in_polygon of every
// part: INTERIOR if some part says INTERIOR, otherwise BOUNDARY if some part says BOUNDARY, otherwise
// EXTERIOR.  EXTERIOR is exactly pip::contains' "no part says INTERIOR or BOUNDARY".  Where
// pip::contains (PointLocator with the Mod-2 rule) calls a point on the rings of an even number of
// parts INTERIOR, this one says BOUNDARY: two parts of a valid MultiPolygon touch at single points
// only, such a point has A's exterior in every neighbourhood, and JTS' Geometry.contains (RelateOp
// nodes the rings of a MultiPolygon against each other and labels that node BOUNDARY) says false.  On
// every other point the two agree, so a POINT row gives what mosaic_st_contains gives, except for a
// point on a vertex shared by two parts.
//
// Degenerate facets (a point as the facet (v, v), a zero-length segment) go through
// pip::segments_intersect as st_intersects.h derives: a point on a vertex or on a segment's interior is
// contact, never a proper crossing (orientation_index(P, P, q) is 0 for every q).
//
// "Some facet pair crosses properly", "some vertex of B is EXTERIOR", "no facet pair meets" and the
// first-vertex tests of (c) are properties of the pair, not of a visiting order, and (a) and (b) both
// end in (0, OK).  So out and status do not depend on the order in which facet pairs and vertices are
// visited: the kernels of st_contains.hip, which skip disjoint blocks, reorder and stop at the first
// proper crossing or exterior vertex, return the value and the status of the sequential driver.
#pragma once
#include <stdint.h>

#include "st_intersects.h"

namespace mosaic {
namespace contains {

using pip::Box;
using pip::GeomStore;
using pip::Vec2;

enum { kPairOk = 1, kPairUndecided = 3 };  // MOSAIC_ROW_OK, MOSAIC_PAIR_UNDECIDED
enum { kHasPolygon = 1u << kPartPolygon, kHasPoint = 1u << kPartPoint, kHasLine = 1u << kPartLine };

// how a pair was decided (mosaic_st_contains_last_split counts these)
enum {
    kHowEmpty = 0,      // step 1
    kHowBox = 1,        // step 2
    kHowKinds = 2,      // step 6: undecided without looking at a vertex
    kHowPointsOut = 3,  // steps 3, 4: a point of B is EXTERIOR / matches no point of A
    kHowPointsIn = 4,   // steps 3, 4: every point located, none outside
    kHowOut = 5,        // 5(a), 5(b): a proper crossing or an exterior vertex
    kHowClear = 6,      // 5(c): no contact
    kHowTouch = 7       // 5(d): undecided
};

// the kinds of the parts of geometry g, as a mask of kHas*
MOSAIC_HD uint32_t geom_kinds(const GeomStore& s, const uint8_t* kind, uint32_t g) {
    uint32_t m = 0;
    for (uint32_t p = s.geom_part[g]; p < s.geom_part[g + 1]; p++) m |= 1u << kind[p];
    return m;
}

// box b lies in box a
MOSAIC_HD bool box_covers(const Box& a, const Box& b) {
    return b.minx >= a.minx && b.miny >= a.miny && b.maxx <= a.maxx && b.maxy <= a.maxy;
}

MOSAIC_HD bool same_point(Vec2 a, Vec2 b) { return a.x == b.x && a.y == b.y; }

// closed segments p1p2 and q1q2 cross at one point interior to both
MOSAIC_HD bool proper_crossing(Vec2 p1, Vec2 p2, Vec2 q1, Vec2 q2) {
    const int pq1 = pip::orientation_index(p1.x, p1.y, p2.x, p2.y, q1.x, q1.y);
    if (pq1 == 0) return false;
    const int pq2 = pip::orientation_index(p1.x, p1.y, p2.x, p2.y, q2.x, q2.y);
    if (pq2 == 0 || pq2 == pq1) return false;
    const int qp1 = pip::orientation_index(q1.x, q1.y, q2.x, q2.y, p1.x, p1.y);
    if (qp1 == 0) return false;
    const int qp2 = pip::orientation_index(q1.x, q1.y, q2.x, q2.y, p2.x, p2.y);
    return qp2 != 0 && qp2 != qp1;
}

// 0: the facets do not meet, 1: they meet, 2: they cross properly
MOSAIC_HD int facet_contact(Vec2 p1, Vec2 p2, Vec2 q1, Vec2 q2) {
    if (!pip::segments_intersect(p1, p2, q1, q2)) return 0;
    return proper_crossing(p1, p2, q1, q2) ? 2 : 1;
}

// the location of (px, py) in the polygonal geometry g (see the header comment)
MOSAIC_HD int locate_union(const GeomStore& s, uint32_t g, double px, double py) {
    if (pip::box_excludes(s.geom_bbox[g], px, py)) return pip::LOC_EXTERIOR;
    bool boundary = false;
    for (uint32_t p = s.geom_part[g]; p < s.geom_part[g + 1]; p++) {
        const int loc = pip::locate_in_polygon(s, p, px, py);
        if (loc == pip::LOC_INTERIOR) return pip::LOC_INTERIOR;
        if (loc == pip::LOC_BOUNDARY) boundary = true;
    }
    return boundary ? pip::LOC_BOUNDARY : pip::LOC_EXTERIOR;
}

// step 3: B (geometry h of sb) points only, A polygonal
MOSAIC_HD bool points_in_polygonal(const GeomStore& sa, uint32_t g, const GeomStore& sb, uint32_t h, int* how) {
    uint32_t r0, r1;
    dist::geom_rings(sb, h, r0, r1);
    bool inside = false;
    for (uint32_t i = sb.ring_start[r0]; i < sb.ring_start[r1]; i++) {
        const int loc = locate_union(sa, g, sb.verts[i].x, sb.verts[i].y);
        if (loc == pip::LOC_EXTERIOR) {
            *how = kHowPointsOut;
            return false;
        }
        if (loc == pip::LOC_INTERIOR) inside = true;
    }
    *how = kHowPointsIn;
    return inside;
}

// step 4: both points only
MOSAIC_HD bool points_in_points(const GeomStore& sa, uint32_t g, const GeomStore& sb, uint32_t h, int* how) {
    uint32_t ra0, ra1, rb0, rb1;
    dist::geom_rings(sa, g, ra0, ra1);
    dist::geom_rings(sb, h, rb0, rb1);
    for (uint32_t j = sb.ring_start[rb0]; j < sb.ring_start[rb1]; j++) {
        bool found = false;
        for (uint32_t i = sa.ring_start[ra0]; i < sa.ring_start[ra1] && !found; i++) found = same_point(sa.verts[i], sb.verts[j]);
        if (!found) {
            *how = kHowPointsOut;
            return false;
        }
    }
    *how = kHowPointsIn;
    return true;
}

// 5(a) and the contact of 5(c): 2 a facet of B crosses a facet of A properly, else 1 some facets meet, else 0
MOSAIC_HD int facets_contact(const GeomStore& sa, uint32_t g, const GeomStore& sb, uint32_t h) {
    uint32_t ra0, ra1, rb0, rb1;
    dist::geom_rings(sa, g, ra0, ra1);
    dist::geom_rings(sb, h, rb0, rb1);
    const Box hbox = sb.geom_bbox[h];
    int contact = 0;
    for (uint32_t ra = ra0; ra < ra1; ra++) {
        const Vec2* va = sa.verts + sa.ring_start[ra];
        const uint32_t na = sa.ring_start[ra + 1] - sa.ring_start[ra];
        if (na == 0 || !pip::boxes_meet(sa.ring_bbox[ra], hbox)) continue;
        for (uint32_t rb = rb0; rb < rb1; rb++) {
            const Vec2* vb = sb.verts + sb.ring_start[rb];
            const uint32_t nb = sb.ring_start[rb + 1] - sb.ring_start[rb];
            if (nb == 0 || !pip::boxes_meet(sa.ring_bbox[ra], sb.ring_bbox[rb])) continue;
            for (uint32_t i = 0; i < dist::ring_facets(na); i++) {
                Vec2 A, B;
                dist::ring_facet(va, na, i, A, B);
                for (uint32_t j = 0; j < dist::ring_facets(nb); j++) {
                    Vec2 C, D;
                    dist::ring_facet(vb, nb, j, C, D);
                    const int c = facet_contact(A, B, C, D);
                    if (c == 2) return 2;
                    if (c) contact = 1;
                }
            }
        }
    }
    return contact;
}

// the first vertex of part q of sb, if it has one
MOSAIC_HD bool part_first_vertex(const GeomStore& sb, uint32_t q, Vec2* v) {
    const uint32_t r = sb.part_ring[q];
    if (sb.part_ring[q + 1] <= r || sb.ring_start[r + 1] <= sb.ring_start[r]) return false;
    *v = sb.verts[sb.ring_start[r]];
    return true;
}

// 5(c), given that no facets meet
MOSAIC_HD bool clear_contains(const GeomStore& sa, uint32_t g, const GeomStore& sb, const uint8_t* kb, uint32_t h) {
    for (uint32_t q = sb.geom_part[h]; q < sb.geom_part[h + 1]; q++) {
        Vec2 v;
        if (!part_first_vertex(sb, q, &v)) continue;
        bool inside = false;
        for (uint32_t p = sa.geom_part[g]; p < sa.geom_part[g + 1] && !inside; p++)
            inside = pip::locate_in_polygon(sa, p, v.x, v.y) == pip::LOC_INTERIOR;
        if (!inside) return false;
    }
    uint32_t ra0, ra1;
    dist::geom_rings(sa, g, ra0, ra1);
    for (uint32_t q = sb.geom_part[h]; q < sb.geom_part[h + 1]; q++) {
        if (kb[q] != kPartPolygon) continue;
        for (uint32_t ra = ra0; ra < ra1; ra++) {
            if (sa.ring_start[ra + 1] <= sa.ring_start[ra]) continue;
            const Vec2 w = sa.verts[sa.ring_start[ra]];
            if (pip::locate_in_polygon(sb, q, w.x, w.y) == pip::LOC_INTERIOR) return false;
        }
    }
    return true;
}

// The definition of the result, with how it was reached.  ka / kb: the part kinds of the two columns.
MOSAIC_HD uint8_t contains_how(const GeomStore& sa, const uint8_t* ka, uint32_t g, const GeomStore& sb, const uint8_t* kb,
                               uint32_t h, int32_t* status, int* how) {
    *status = kPairOk;
    *how = kHowEmpty;
    if (dist::geom_facets(sa, g) == 0 || dist::geom_facets(sb, h) == 0) return 0;
    *how = kHowBox;
    if (!box_covers(sa.geom_bbox[g], sb.geom_bbox[h])) return 0;
    const uint32_t A = geom_kinds(sa, ka, g), B = geom_kinds(sb, kb, h);
    if (B == kHasPoint && A == kHasPolygon) return points_in_polygonal(sa, g, sb, h, how) ? 1 : 0;
    if (B == kHasPoint && A == kHasPoint) return points_in_points(sa, g, sb, h, how) ? 1 : 0;
    if (A != kHasPolygon) {
        *how = kHowKinds;
        *status = kPairUndecided;
        return 0;
    }
    const int contact = facets_contact(sa, g, sb, h);
    // without contact the pair counts as decided by (c) even where (b) sees it first: the value is the same
    *how = contact ? kHowOut : kHowClear;
    if (contact == 2) return 0;
    uint32_t rb0, rb1;
    dist::geom_rings(sb, h, rb0, rb1);
    for (uint32_t i = sb.ring_start[rb0]; i < sb.ring_start[rb1]; i++)
        if (locate_union(sa, g, sb.verts[i].x, sb.verts[i].y) == pip::LOC_EXTERIOR) return 0;
    if (contact == 0) return clear_contains(sa, g, sb, kb, h) ? 1 : 0;
    *how = kHowTouch;
    *status = kPairUndecided;
    return 0;
}

// The definition of the result: out, and *status MOSAIC_ROW_OK or MOSAIC_PAIR_UNDECIDED (out 0).
MOSAIC_HD uint8_t contains(const GeomStore& sa, const uint8_t* ka, uint32_t g, const GeomStore& sb, const uint8_t* kb,
                           uint32_t h, int32_t* status) {
    int how;
    return contains_how(sa, ka, g, sb, kb, h, status, &how);
}

}  // namespace contains
}  // namespace mosaic
