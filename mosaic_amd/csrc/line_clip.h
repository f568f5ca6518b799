// The clip of a line chip against a polygon chip -- the geometry step of st_intersection_aggregate over
// the join of line chips (Mosaic.lineFill) with polygon chips: "how much of each trip lies in each
// zone" (expressions/geometry/ST_IntersectionAggregate.scala:40-72: the equi-join on index_id folded
// per (line key, polygon key); its `update` takes the left chip whole when the right chip is core and
// `left.intersection(right)` when neither is).  The layouts are those of line_isect.h and
// pip_device.h; crossing points are JTS's (llclip::meet), every decision an exact predicate.
//
// Increment of one joined chip pair (line chip c, polygon chip g):
//   polygon chip core   the whole line chip: every piece of at least 2 vertices (POINT / MULTIPOINT
//                       items contribute nothing); the polygon chip's geometry is not read
//   neither side core   clip(c, g), below
//   line chip core      refused (MOSAIC_E_ARG naming the chip): lineFill never makes one, and the
//                       reference would union the polygon chip in, which is not a line result
//
// clip(c, g) -- `clip_pair` below is the sequential driver the wave kernel of line_clip.hip and the
// host join of line_clip_host.cpp are defined by:
//   1. may_meet(c, g) false: empty.
//   2. Every piece of at least 2 vertices, in order; every segment a -> b with a != b, in order (a
//      segment with a == b is skipped and does not end a run):
//        the segment's box misses geom_bbox[g]: wholly outside (a run ends here);
//        otherwise the cut list is {a, b} plus every point llclip::meet(a, b, c, d) returns for the
//        ring segments c -> d of every ring of every part of g (holes included) whose box meets the
//        segment's; sorted by (p - a).(b - a), then x, then y (then the ordinates' bit patterns, which
//        orders -0.0 and 0.0: a total order, so every evaluation order gives one list); bit-equal
//        neighbours dropped.
//   3. The interval between consecutive cuts p, q is kept iff its midpoint ((p.x + q.x) / 2,
//      (p.y + q.y) / 2) is not LOC_EXTERIOR in some part of g.  The boundary counts: a stretch along
//      a polygon edge is in the closed intersection, as in JTS.  A kept interval contributes
//      sqrt(dx * dx + dy * dy) (JTS Length.ofLine; llclip::pt_dist).
//   4. A run is a maximal chain of kept intervals within a piece; it continues over a vertex when
//      the last interval of one segment and the first of the next are both kept.  Its LineString is
//      its first cut point, the original vertices in between (copied), its last cut point, with
//      bit-equal consecutive points dropped (a run left with one point is dropped).
//   5. The pair's length is the sum of interval lengths in (piece, segment, interval) order.
//
// Divergences from the reference (JTS intersection, then union over the group):
//   * isolated touch points are not emitted (the reference's union would carry a POINT);
//   * runs are not noded at ring vertices they pass, nor merged across cells (JTS's union does not
//     line-merge either; no JTS output pins piece order or direction here);
//   * a segment lying exactly along a side shared by two cells is in both cells' chips and is counted
//     twice.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "line_isect.h"
#include "llclip.h"

namespace mosaic {
namespace lineisect {

using llclip::Pt;

// meet points per segment the wave kernel holds (with a and b: 256 LDS slots of 16 bytes per wave);
// a pair with a segment over it is finished by the host driver (the same code, the same bits)
constexpr int kCutCap = 254;

MOSAIC_HD uint64_t f64_bits(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return u;
}
MOSAIC_HD bool bit_equal(Pt p, Pt q) { return f64_bits(p.x) == f64_bits(q.x) && f64_bits(p.y) == f64_bits(q.y); }
MOSAIC_HD double cut_key(Pt p, Pt a, Pt b) { return (p.x - a.x) * (b.x - a.x) + (p.y - a.y) * (b.y - a.y); }
// the total order of a segment's cut list
MOSAIC_HD bool cut_less(Pt p, Pt q, Pt a, Pt b) {
    const double kp = cut_key(p, a, b), kq = cut_key(q, a, b);
    if (kp != kq) return kp < kq;
    if (p.x != q.x) return p.x < q.x;
    if (p.y != q.y) return p.y < q.y;
    if (f64_bits(p.x) != f64_bits(q.x)) return f64_bits(p.x) < f64_bits(q.x);
    return f64_bits(p.y) < f64_bits(q.y);
}
MOSAIC_HD pip::Box seg_box(Pt a, Pt b) { return pip::Box{llclip::mn(a.x, b.x), llclip::mn(a.y, b.y), llclip::mx(a.x, b.x), llclip::mx(a.y, b.y)}; }
MOSAIC_HD Pt vert(const pip::Vec2* v, uint32_t i) { return Pt{v[i].x, v[i].y}; }

// step 3
MOSAIC_HD bool interval_kept(const pip::GeomStore& P, uint32_t g, Pt p, Pt q) {
    const double mx = (p.x + q.x) / 2.0, my = (p.y + q.y) / 2.0;
    for (uint32_t part = P.geom_part[g]; part < P.geom_part[g + 1]; part++)
        if (pip::locate_in_polygon(P, part, mx, my) != pip::LOC_EXTERIOR) return true;
    return false;
}

// a run: piece, the vertex indices (into LineStore::verts) that start its first and its last segment,
// its first and last cut point; the original vertices in between are seg0 + 1 .. seg1
struct Run {
    uint32_t pair, piece, seg0, seg1;
    Pt p0, p1;
};

// steps 4 and 5 as a state machine over the intervals in order
struct RunState {
    double sum;
    uint32_t n_runs;
    bool open;
    Run run;
};
MOSAIC_HD void run_init(RunState& s, uint32_t pair) {
    s.sum = 0.0;
    s.n_runs = 0;
    s.open = false;
    s.run = Run{pair, 0, 0, 0, Pt{0, 0}, Pt{0, 0}};
}
template <class Emit>
MOSAIC_HD void run_close(RunState& s, Emit&& emit) {
    if (!s.open) return;
    emit(s.run, s.n_runs);
    s.n_runs++;
    s.open = false;
}
template <class Emit>
MOSAIC_HD void run_interval(RunState& s, bool kept, Pt p, Pt q, uint32_t piece, uint32_t seg, Emit&& emit) {
    if (!kept) {
        run_close(s, emit);
        return;
    }
    s.sum += llclip::pt_dist(q, p);
    if (!s.open) {
        s.open = true;
        s.run.piece = piece;
        s.run.seg0 = seg;
        s.run.p0 = p;
    }
    s.run.seg1 = seg;
    s.run.p1 = q;
}

// The sequential driver.  cuts: room for cap + 2 points.  emit(run, index in the pair) per run, in
// order; s.sum the pair's length.  Returns false when a segment has more than `cap` meet points (s
// and what was emitted are then void; the caller repeats with more room).
template <class Emit>
MOSAIC_HD bool clip_pair(const LineStore& L, uint32_t c, const pip::GeomStore& P, uint32_t g, uint32_t pair, Pt* cuts, int64_t cap,
                         RunState& s, Emit&& emit) {
    run_init(s, pair);
    if (!may_meet(L, c, P, g)) return true;
    const uint32_t r0 = P.part_ring[P.geom_part[g]], r1 = P.part_ring[P.geom_part[g + 1]];
    const pip::Box gb = P.geom_bbox[g];
    for (uint32_t m = L.chip_piece[c]; m < L.chip_piece[c + 1]; m++) {
        const uint32_t i0 = L.piece_start[m], i1 = L.piece_start[m + 1];
        if (i1 - i0 < 2) continue;
        for (uint32_t i = i0; i + 1 < i1; i++) {
            const Pt a = vert(L.verts, i), b = vert(L.verts, i + 1);
            if (llclip::same(a, b)) continue;
            const pip::Box sb = seg_box(a, b);
            if (!pip::boxes_meet(sb, gb)) {
                run_close(s, emit);
                continue;
            }
            int64_t n = 0;
            cuts[n++] = a;
            cuts[n++] = b;
            for (uint32_t r = r0; r < r1; r++) {
                if (!pip::boxes_meet(sb, P.ring_bbox[r])) continue;
                for (uint32_t j = P.ring_start[r]; j + 1 < P.ring_start[r + 1]; j++) {
                    Pt o[2];
                    const int k = llclip::meet(a, b, vert(P.verts, j), vert(P.verts, j + 1), o);
                    if (n + k > cap + 2) return false;
                    for (int t = 0; t < k; t++) cuts[n++] = o[t];
                }
            }
            for (int64_t u = 1; u < n; u++) {  // insertion sort: a handful of cuts as a rule
                const Pt p = cuts[u];
                int64_t w = u;
                for (; w > 0 && cut_less(p, cuts[w - 1], a, b); w--) cuts[w] = cuts[w - 1];
                cuts[w] = p;
            }
            int64_t k = 1;
            for (int64_t u = 1; u < n; u++)
                if (!bit_equal(cuts[u], cuts[k - 1])) cuts[k++] = cuts[u];
            for (int64_t u = 0; u + 1 < k; u++) run_interval(s, interval_kept(P, g, cuts[u], cuts[u + 1]), cuts[u], cuts[u + 1], m, i, emit);
        }
        run_close(s, emit);
    }
    return true;
}

// the whole line chip's length: every piece of at least 2 vertices, segments in order
MOSAIC_HD double chip_length(const LineStore& L, uint32_t c) {
    double sum = 0.0;
    for (uint32_t m = L.chip_piece[c]; m < L.chip_piece[c + 1]; m++) {
        const uint32_t i0 = L.piece_start[m], i1 = L.piece_start[m + 1];
        if (i1 - i0 < 2) continue;
        for (uint32_t i = i0; i + 1 < i1; i++) sum += llclip::pt_dist(vert(L.verts, i + 1), vert(L.verts, i));
    }
    return sum;
}

// clip(c, g) on the host, the cut list growing as needed (no cap): the pair's length; its runs appended
// to `runs` when given
inline double clip_pair_host(const LineStore& L, uint32_t c, const pip::GeomStore& P, uint32_t g, uint32_t pair, std::vector<Pt>& cuts,
                             std::vector<Run>* runs, uint32_t* n_runs) {
    if (cuts.size() < 66) cuts.resize(66);
    const size_t r0 = runs ? runs->size() : 0;
    RunState s;
    for (;;) {
        auto emit = [&](const Run& r, uint32_t) {
            if (runs) runs->push_back(r);
        };
        if (clip_pair(L, c, P, g, pair, cuts.data(), (int64_t)cuts.size() - 2, s, emit)) break;
        if (runs) runs->resize(r0);
        cuts.resize(cuts.size() * 2);
    }
    if (n_runs) *n_runs = s.n_runs;
    return s.sum;
}

// length of clip(line chip c, polygon chip g)
inline double clip_length(const LineStore& L, uint32_t c, const pip::GeomStore& P, uint32_t g) {
    std::vector<Pt> cuts;
    return clip_pair_host(L, c, P, g, 0, cuts, nullptr, nullptr);
}

}  // namespace lineisect
}  // namespace mosaic
