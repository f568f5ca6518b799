// JTS 1.19 `Geometry.intersects` (RelateOp: the two closed point sets share a point) for the geometry
// types this engine serves -- Point, MultiPoint, LineString, MultiLineString, Polygon and MultiPolygon
// on either side -- on the host and on gfx950: the reference's st_intersects
// (functions/MosaicContext.scala ST_Intersects -> expressions/geometry/ST_Intersects.scala ->
// core/geometry/MosaicGeometryJTS.intersects -> JTS Geometry.intersects; python/mosaic/api/predicates.py).
// The columns are the GeomStore + part-kind layout that st_distance.h documents: a point is a part of
// one ring of one vertex, a component line a part of one open ring, polygon rings are stored closed.
//
// Semantics (st_intersects(g, h)), the sequential driver `intersects` below:
//   1. either geometry has no facet                                            -> false
//      (the opposite of st_distance's 0.0: LINESTRING EMPTY is a served row that intersects nothing)
//   2. the geometry boxes do not meet (pip::boxes_meet)                        -> false
//   3. some facet of g meets some facet of h (pip::segments_intersect)         -> true
//      Facets are those of dist::ring_facets / dist::ring_facet: every ring's segments, holes
//      included, every component line's segments (nothing closes an open line) and every point as
//      the facet (v, v).  Ring pairs whose boxes do not meet are skipped: segments inside disjoint
//      boxes share no point.
//   4. containment, both directions: for every polygon part P of one side and every component of
//      the other (a point, a component line, a polygon's shell), the component's first vertex v:
//      locate_in_polygon(P, v) != EXTERIOR -> true (dist::component_in_part).  Only polygon parts
//      contain; a line never does, closed or not.  Each part is located on its own: the union of the
//      parts holds v iff some part does, so no Mod-2 rule is involved.
//   5. otherwise false.
//
// Step 4 decides the rest.  Suppose no facet of g meets a facet of h and the sets still share a point
// x.  The boundaries of polygon parts and all of every line and point are facets, so x is no point of
// a facet of both; hence x is interior to a polygon part P of (say) h, or of g with the roles swapped.
// Let C be the connected component of g that holds x: a point, a component line, or a polygon part.
//   * C a point or a line: C is connected, meets no ring of P (they are facets), and has a point in
//     P's open interior, so all of C lies there -- in particular its first vertex.
//   * C a polygon part: every ring of C is connected and meets no ring of P, so it lies wholly in
//     P's interior or wholly in P's exterior (the complement of the closed part, holes' insides
//     included), and the same holds for P's rings against C.  If C's shell lies in P's interior, or
//     P's shell in C's, its first vertex is located there and step 4 says true.  Otherwise each
//     shell lies in the other part's exterior: outside the other shell, or inside one of its holes.
//     A shell inside a hole of the other part puts its whole part inside that hole, away from the
//     other part; two shells outside each other that do not cross bound disjoint regions.  Neither
//     leaves a shared point x, so this case does not arise.
// This is the argument of pip_device.h (shell_vertex_in) and line_isect.h, extended to points: a
// point is a connected component with one vertex.  Conversely a first vertex located in or on P is a
// shared point, so step 4 never says true wrongly.
//
// Degenerate facets.  pip::segments_intersect(p1, p2, q1, q2) with P = p1 = p2 (the same holds with the
// roles swapped; the function is symmetric in its steps):
//   * orientation_index(P, P, q) is 0 for every q: detleft = (Px - qx)(Py - qy) and detright =
//     (Py - qy)(Px - qx) are the same product, so det = 0; the filter then either returns signum(0) or
//     falls to the double-double path, where dx1 = dy1 = 0 make both products and their difference 0.
//     So pq1 = pq2 = 0 and the first sign test never rejects.
//   * P on a segment's interior: the envelope test passes; qp1 = qp2 = orientation(q1, q2, P) = 0
//     (exact sign), so all four are 0 and the collinear branch returns in_seg_env(q1, q2, P), which
//     the envelope test has just established: true.
//   * P on a vertex (P == q1 or q2): orientation(q1, q2, q1) has detleft = 0 and det = 0: as above, true.
//   * P collinear with q1q2 but beyond it: a point's envelope is the point, and it is outside the
//     segment's envelope in x or in y (collinear and inside the envelope means on the segment), so
//     the envelope test returns false.
//   * P off the line: qp1 = qp2 != 0, same sign: false.
//   * two equal points: the envelopes meet, all four orientations are 0, in_seg_env(P, P, Q): true.
//   * two unequal points: the envelopes (two distinct points) do not meet: false.
// So every facet is treated as a segment and no case is handled here; tests/test_st_intersects.py
// runs each of these.
//
// Every decision is an exact predicate (orientation signs from CGAlgorithmsDD, comparisons), so the
// answer does not depend on the order in which facet pairs and containment tasks are visited: the
// kernels of st_intersects.hip, which skip disjoint blocks, reorder and stop at the first hit, return
// the value of the sequential driver.
#pragma once
#include <stdint.h>

#include "st_distance.h"

namespace mosaic {
namespace isect {

using pip::Box;
using pip::GeomStore;
using pip::Vec2;

// step 3: some facet of g meets some facet of h
MOSAIC_HD bool facets_meet(const GeomStore& sa, uint32_t g, const GeomStore& sb, uint32_t h) {
    uint32_t ra0, ra1, rb0, rb1;
    dist::geom_rings(sa, g, ra0, ra1);
    dist::geom_rings(sb, h, rb0, rb1);
    const Box hbox = sb.geom_bbox[h];
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
                    if (pip::segments_intersect(A, B, C, D)) return true;
                }
            }
        }
    }
    return false;
}

// The definition of the result.  ka / kb: the part kinds of the two columns.
MOSAIC_HD bool intersects(const GeomStore& sa, const uint8_t* ka, uint32_t g, const GeomStore& sb, const uint8_t* kb,
                          uint32_t h) {
    if (dist::geom_facets(sa, g) == 0 || dist::geom_facets(sb, h) == 0) return false;
    if (!pip::boxes_meet(sa.geom_bbox[g], sb.geom_bbox[h])) return false;
    if (facets_meet(sa, g, sb, h)) return true;
    return dist::contained(sa, ka, g, sb, h) || dist::contained(sb, kb, h, sa, g);
}

}  // namespace isect
}  // namespace mosaic
