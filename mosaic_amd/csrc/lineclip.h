// Mosaic.lineFill (core/Mosaic.scala:89-97, 146-194): grid_tessellateexplode for LineString and
// MultiLineString, one chip per (component line, cell the line meets).  Shared by the host producer
// (lines_host.cpp, g++) and the device producer (line_fill.hip, hipcc): both run exactly this code with
// the same IEEE operations (-ffp-contract=off), so they write the same bytes.
//
// Cells.  The reference's lineDecompose walks breadth-first from pointToIndex(first vertex) through the
// cells whose indexToGeometry meets the line, trying the kRing(1) of every such cell (and of the start
// cell once when its own intersection is empty).  Here the walk runs per span of a segment (span_count,
// walk_span): seeded with kRing(cell(span start), 1), expanded through the cells the *segment* meets
// whose envelope meets the span's (widened) box; the union over spans and segments is the set of cells
// the line meets, which is what the reference's traversal reaches ("lineFill").  "Meets" is
// segment against the closed cell polygon: llclip::locate_cell(start) != 0 or llclip::meet against a
// side, JTS's DD orientation signs.
//
// Chip geometry (build).  JTS's old overlay of a line against an area, restated from its algorithm (no
// JTS output was available to check piece order or direction: they are derived, not pinned).  The line
// is cut where it meets the cell's boundary (llclip::meet with the line's segment as a-b; crossing
// points by llclip::intersection; endpoint and collinear hits copy the original vertex); a piece
// between two cuts is kept when its midpoint is inside or on the cell (pieces bounded by a vertex
// strictly inside / outside take that vertex's location); every kept piece, from one boundary contact
// (or line end) to the next, is one LineString in the line's direction, original vertices copied -- a
// vertex on a side splits the piece there; a contact that ends no kept piece is an isolated point.  A chip is its pieces (LINESTRING / MULTILINESTRING) or, without any, its distinct
// isolated points (POINT / MULTIPOINT), both in line order.
// Divergences from the reference: (a) a cell with pieces and isolated points gives its pieces (JTS
// returns a GeometryCollection, which MosaicGeometryJTS.apply collapses to POLYGON EMPTY: the reference
// drops the chip and stops expanding there); (b) the line is not noded at its own crossings (same point
// set, fewer and longer pieces); (c) a cell the walk has to try that is no planar lon / lat polygon
// (llclip::cell_ok false: over the antimeridian or a pole) is an error (MOSAIC_E_ARG).
#pragma once
#include <math.h>
#include <stdint.h>

#include "bng_device.h"
#include "h3_device.h"
#include "h3_geom.h"
#include "h3_neighbors.h"
#include "llclip.h"

namespace mosaic {
namespace lineclip {

using llclip::Cell;
using llclip::Pt;

enum Status : int { kOk = 0, kNeedsMore = 1, kBadCell = 2 };

static constexpr int kWalkCap = 64;  // device lane: cells one span's walk may try
static constexpr int kSlot = 8;      // device lane: cells of one span the counting walk keeps for the writing pass
static constexpr int kItems = 8;     // device lane: pieces (or isolated points) of one chip
static constexpr int kMaxEvents = 34;  // boundary contacts of one segment: two per side at the most

struct Grid {
    int grid;  // 0 H3, 1 BNG
    int res;
};

MOSAIC_HD Pt vtx(const double* xy, int64_t v) { return Pt{xy[2 * v], xy[2 * v + 1]}; }

// pointToIndex; false where the grid has no cell for the point
MOSAIC_HD bool point_cell(Grid g, Pt p, int64_t* id) {
    if (g.grid == 0) {
        const uint64_t h = h3::h3_exact(h3::to_radians(p.y, 8), h3::to_radians(p.x, 8), g.res);
        *id = (int64_t)h;
        return h != 0;
    }
    return bng::point_to_index(p.x, p.y, g.res, id) && bng::is_valid(*id);
}

// indexToGeometry as the polygon producer clips against it; false: no planar polygon (cell_ok)
MOSAIC_HD bool cell_poly(Grid g, int64_t id, Cell& C) {
    if (g.grid == 0) {
        double b[20];
        const int nb = h3geom::h3_to_geo_boundary((uint64_t)id, b);
        if (nb < 3 || nb > 16) return false;
        C.nc = nb;
        for (int v = 0; v < nb; v++) C.v[v] = Pt{h3geom::to_degrees(b[2 * v + 1], 8), h3geom::to_degrees(b[2 * v], 8)};
        llclip::cell_init(C);
        return llclip::cell_ok(C, true);
    }
    int res;
    int32_t e, x, y;
    if (!bng::cell_origin(id, &res, &e, &x, &y)) return false;
    const double x0 = (double)x, y0 = (double)y, ed = (double)e;
    C.nc = 4;
    C.v[0] = Pt{x0, y0};
    C.v[1] = Pt{x0 + ed, y0};
    C.v[2] = Pt{x0 + ed, y0 + ed};
    C.v[3] = Pt{x0, y0 + ed};
    llclip::cell_init(C);
    return llclip::cell_ok(C, false);
}

// cell_poly as the walks take it: a functor, so that the host can remember the polygons it has built
struct DirectPoly {
    Grid g;
    MOSAIC_HD bool operator()(int64_t id, Cell& C) const { return cell_poly(g, id, C); }
};

// kRing(id, 1), the cell itself included: at most 9 cells
MOSAIC_HD int ring1(Grid g, int64_t id, int64_t out[9]) {
    if (g.grid == 0) {
        int n = h3nb::kring_fast((uint64_t)id, 1, 0, out);
        if (n == -3) {
            int64_t tab[8];
            int32_t dist[7];
            n = h3nb::kring_slow((uint64_t)id, 1, 0, out, tab, dist);
        }
        return n < 0 ? 0 : n;
    }
    const int n = bng::kring(id, 1, out);
    return n < 0 ? 0 : n;
}

// segment a-b against the closed cell
MOSAIC_HD bool segment_meets(Pt a, Pt b, const Cell& C) {
    if (llclip::mx(a.x, b.x) < C.x0 || llclip::mn(a.x, b.x) > C.x1 || llclip::mx(a.y, b.y) < C.y0 || llclip::mn(a.y, b.y) > C.y1)
        return false;
    if (llclip::locate_cell(a, C) != 0) return true;
    for (int j = 0; j < C.nc; j++) {
        Pt q[2];
        if (llclip::meet(a, b, C.v[j], llclip::cv(C, j + 1), q)) return true;
    }
    return false;
}

// The spans a segment is walked in: about two cells (of the size of the start vertex's) each, so that
// no lane walks a long segment alone.
template <class P>
MOSAIC_HD int span_count(Grid g, P poly, Pt a, Pt b, int32_t* spans) {
    int64_t id;
    Cell C;
    *spans = 0;
    if (!point_cell(g, a, &id) || !poly(id, C)) return kBadCell;
    const double w = C.x1 - C.x0, h = C.y1 - C.y0;
    const double r = llclip::mx(fabs(b.x - a.x) / w, fabs(b.y - a.y) / h) / 2.0;
    if (!(r < 1e9)) return kBadCell;
    const int32_t k = (int32_t)ceil(r);
    *spans = k < 1 ? 1 : k;
    return kOk;
}

MOSAIC_HD Pt along(Pt a, Pt b, double t) {
    if (t <= 0.0) return a;
    if (t >= 1.0) return b;
    return Pt{a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t};
}

// The cells segment a-b meets around its span j of K: emit(cell) once per cell found here (another span
// may find it too).  seen: scratch of cap >= 9 cells.
template <class P, class F>
MOSAIC_HD int walk_span(Grid g, P poly, Pt a, Pt b, int32_t j, int32_t K, int64_t* seen, int32_t cap, F emit) {
    const Pt p = along(a, b, (double)j / (double)K);
    // the span's box, widened by half a span on either side (neighbouring spans overlap)
    const Pt lo = along(a, b, ((double)j - 0.5) / (double)K), hi = along(a, b, ((double)j + 1.5) / (double)K);
    const double bx0 = llclip::mn(lo.x, hi.x), bx1 = llclip::mx(lo.x, hi.x), by0 = llclip::mn(lo.y, hi.y), by1 = llclip::mx(lo.y, hi.y);
    int64_t id;
    if (!point_cell(g, p, &id)) return kBadCell;
    int32_t n = ring1(g, id, seen);
    if (n == 0) return kBadCell;
    for (int32_t i = 0; i < n; i++) {
        Cell C;
        if (!poly(seen[i], C)) return kBadCell;
        if (C.x1 < bx0 || C.x0 > bx1 || C.y1 < by0 || C.y0 > by1) continue;
        if (!segment_meets(a, b, C)) continue;
        emit(seen[i]);
        int64_t nb[9];
        const int m = ring1(g, seen[i], nb);
        for (int u = 0; u < m; u++) {
            bool have = false;
            for (int32_t q = 0; q < n && !have; q++) have = seen[q] == nb[u];
            if (have) continue;
            if (n == cap) return kNeedsMore;
            seen[n++] = nb[u];
        }
    }
    return kOk;
}

// One piece or isolated point of a chip: in, the original vertices [v0, v0 + nv), out.
struct Item {
    Pt in, out;
    int64_t v0;
    int32_t nv;
    int32_t kind;  // 0 piece, 1 isolated point (in == out, nv == 0)
};

// Caller-owned workspace and the chip's summary.
struct Work {
    Item* it;
    int32_t cap;
    int32_t n;          // items: pieces when has_piece, else distinct isolated points
    int32_t has_piece;
    int32_t lost;       // an isolated point did not fit (matters only when no piece follows)
    int64_t s0;         // where the chip begins along the line: segment (or last vertex) and parameter
    double t0;
};

// The chip of one line against C.  segs: the line's segments (index of their first vertex) that meet C,
// ascending.  kNeedsMore: the chip has more items than w.cap.
MOSAIC_HD int build(const double* xy, const Cell& C, const uint32_t* segs, int64_t n_segs, Work& w) {
    w.n = 0;
    w.has_piece = 0;
    w.lost = 0;
    w.s0 = -1;
    w.t0 = 0.0;
    bool open = false;
    Item cur = Item{Pt{0, 0}, Pt{0, 0}, 0, 0, 0};
    auto add_point = [&](Pt p, int64_t s, double t) {
        if (w.has_piece) return;
        for (int32_t i = 0; i < w.n; i++)
            if (llclip::same(w.it[i].in, p)) return;
        if (w.s0 < 0 && !w.lost) w.s0 = s, w.t0 = t;
        if (w.n == w.cap) {
            w.lost = 1;
            return;
        }
        w.it[w.n++] = Item{p, p, 0, 0, 1};
    };
    int64_t prev = -2;
    for (int64_t k = 0; k < n_segs; k++) {
        const int64_t s = (int64_t)segs[k];
        const Pt a = vtx(xy, s), b = vtx(xy, s + 1);
        if (s != prev + 1 && open) {  // (not reachable: a kept piece ends inside or on C, so s - 1 is listed)
            cur.out = vtx(xy, prev + 1);
            cur.nv = (int32_t)(prev - cur.v0 + 1);
            if (w.n == w.cap) return kNeedsMore;
            w.it[w.n++] = cur;
            open = false;
        }
        prev = s;
        Pt ev[kMaxEvents];
        double evt[kMaxEvents];
        int ne = 0;
        const double dx = b.x - a.x, dy = b.y - a.y;
        for (int j = 0; j < C.nc; j++) {
            Pt q[2];
            const int m = llclip::meet(a, b, C.v[j], llclip::cv(C, j + 1), q);
            for (int t = 0; t < m; t++) {
                if (llclip::same(q[t], a) || llclip::same(q[t], b)) continue;
                bool dup = false;
                for (int u = 0; u < ne; u++) dup = dup || llclip::same(ev[u], q[t]);
                if (dup || ne == kMaxEvents) continue;
                const double tt = fabs(dx) >= fabs(dy) ? (q[t].x - a.x) / dx : (q[t].y - a.y) / dy;
                int u = ne++;
                while (u > 0 && evt[u - 1] > tt) {
                    ev[u] = ev[u - 1];
                    evt[u] = evt[u - 1];
                    u--;
                }
                ev[u] = q[t];
                evt[u] = tt;
            }
        }
        const int la = llclip::locate_cell(a, C), lb = llclip::locate_cell(b, C);
        for (int i = 0; i <= ne; i++) {
            const Pt p0 = i == 0 ? a : ev[i - 1], p1 = i == ne ? b : ev[i];
            bool kept;
            if (i == 0 && la != 1) kept = la == 2;
            else if (i == ne && lb != 1) kept = lb == 2;
            else kept = llclip::locate_cell(Pt{(p0.x + p1.x) / 2, (p0.y + p1.y) / 2}, C) != 0;
            const double t = i == 0 ? 0.0 : evt[i - 1];
            const bool cut = i > 0 || la == 1;  // p0 is on C's boundary: pieces end and begin there
            const bool was_open = open;
            if (open && (cut || !kept)) {
                cur.out = p0;
                cur.nv = (int32_t)((i == 0 ? s - 1 : s) - cur.v0 + 1);
                if (w.n == w.cap) return kNeedsMore;
                w.it[w.n++] = cur;
                open = false;
            }
            if (kept && !open) {
                cur = Item{p0, p0, s + 1, 0, 0};
                open = true;
                if (!w.has_piece) {
                    w.has_piece = 1;
                    w.n = 0;
                    w.lost = 0;
                    w.s0 = s;
                    w.t0 = t;
                }
            } else if (!kept && !was_open && cut) {
                add_point(p0, s, t);
            }
        }
        // the segment's end vertex is the next listed segment's start unless the line (or the run) ends
        if (!(k + 1 < n_segs && (int64_t)segs[k + 1] == s + 1)) {
            if (open) {
                cur.out = b;
                cur.nv = (int32_t)(s - cur.v0 + 1);
                if (w.n == w.cap) return kNeedsMore;
                w.it[w.n++] = cur;
                open = false;
            } else if (lb == 1) {
                add_point(b, s + 1, 0.0);
            }
        }
    }
    if (!w.has_piece && w.lost) return kNeedsMore;
    return kOk;
}

}  // namespace lineclip
}  // namespace mosaic
