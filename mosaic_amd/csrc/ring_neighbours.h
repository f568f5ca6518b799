// One iteration of the reference's KNN model (models/knn/GridRingNeighbours.scala:121-160) on the
// host and on gfx950: the join of a landmark column's ring cells with the candidates' chip cells,
// reduced to one row per (landmark, candidate), without self matches, with st_distance, ordered.
//
// Inputs: a landmark column L and a candidate column C (geometry columns, geoms_build.h); the
// candidates' chips as (cell, candidate row) -- grid_tessellateexplode(keepCoreGeometries = false) or
// one chip per point (Mosaic.pointChip) -- held as a cell index; and (landmark row, cell) rows, which
// the caller fills with grid_geometrykringexplode(l, res, 1) in iteration 1 and with
// grid_geometrykloopexplode(l, res, i) in iteration i > 1.  Whatever cells are given are joined;
// duplicate rows are allowed.
//
// Semantics:
//   * pairs: the set of (l, c) such that some given cell of l is the cell of a chip of c (the
//     reference's groupBy(leftRowID, rightRowID) of the left-outer join on index_id).
//   * unmatched[l] = 1 iff some given cell of l is the cell of no chip: the join's null row, which
//     SpatialKNN's bookkeeping counts.
//   * The reference then filters on st_intersects_aggregate(leftKringCol, rightGridCol).  That filter
//     is a no-op here and is not built: the left chips are wrapped with isCore = true
//     (GridRingNeighbours.scala:98) and ST_IntersectsAggregate.scala:32 returns true for a core chip
//     without looking at a geometry.
//   * Self matches are dropped unless keep_self.  The reference compares Spark's hash of the two
//     serialized geometries; here (l, c) is a self match iff both rows are MOSAIC_ROW_OK and have
//     identical flat content: the same parts, part kinds and rings, and bitwise-equal vertices
//     (self_match, same_geometry).  The comparison is exact, not a hash.  A WKB row in the other byte order decodes to the same flat
//     content and is a self match; a ring rotated to another start vertex is not.  A null or
//     row-path row (stored as an empty geometry) is never part of a self match: its pairs stay.
//   * distance: the bits of dist::distance with the part kinds (st_distance.h); NaN when either row's status is not
//     MOSAIC_ROW_OK (mosaic_st_distance's convention).
//   * Order: (landmark row, distance bits, candidate row).  The bits of a non-negative double order
//     like a uint64, and a NaN's bits come after every number's.  Spark's row_number leaves ties
//     undefined; the candidate row breaking them is this engine's own rule.
//
// `neighbours` below, sequential and built on std::sort / std::unique, is the definition of the
// result; ring_neighbours.hip returns the same rows.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "st_distance.h"

namespace mosaic {
namespace rn {

using pip::GeomStore;

// a geometry column as st_distance.hip and geoms_build.h hold it
struct Col {
    GeomStore s;
    const uint8_t* part_kind;
    const uint32_t* facets;  // per geometry
    const int32_t* status;   // per geometry, MOSAIC_ROW_*
    int64_t n;
};

// The candidates' chips as a map: cells[] sorted and distinct; the candidate rows of cells[j] are
// rows[start[j] .. start[j + 1]), sorted and distinct.
struct CellIndexView {
    const int64_t* cells;
    const int64_t* start;
    const int32_t* rows;
    int64_t n_cells;
};

constexpr int64_t kMaxRows = (int64_t)1 << 31;  // row counts and row indices stay below this

MOSAIC_HD uint64_t bits_of(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}

// the slot of `cell` in the index, or -1
MOSAIC_HD int64_t find_cell(const CellIndexView& ix, int64_t cell) {
    int64_t lo = 0, hi = ix.n_cells;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ix.cells[mid] < cell)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < ix.n_cells && ix.cells[lo] == cell ? lo : -1;
}

MOSAIC_HD bool same_box(const pip::Box& a, const pip::Box& b) {
    return bits_of(a.minx) == bits_of(b.minx) && bits_of(a.miny) == bits_of(b.miny) && bits_of(a.maxx) == bits_of(b.maxx) &&
           bits_of(a.maxy) == bits_of(b.maxy);
}

// rows g of a and h of b have identical flat content; the facet counts and the boxes decide most pairs
MOSAIC_HD bool same_geometry(const Col& a, uint32_t g, const Col& b, uint32_t h) {
    if (a.facets[g] != b.facets[h]) return false;
    const uint32_t pa = a.s.geom_part[g], pb = b.s.geom_part[h];
    const uint32_t np = a.s.geom_part[g + 1] - pa;
    if (np != b.s.geom_part[h + 1] - pb) return false;
    if (np == 0) return true;
    if (!same_box(a.s.geom_bbox[g], b.s.geom_bbox[h])) return false;
    for (uint32_t p = 0; p < np; p++) {
        if (a.part_kind[pa + p] != b.part_kind[pb + p]) return false;
        const uint32_t ra = a.s.part_ring[pa + p], rb = b.s.part_ring[pb + p];
        const uint32_t nr = a.s.part_ring[pa + p + 1] - ra;
        if (nr != b.s.part_ring[pb + p + 1] - rb) return false;
        for (uint32_t r = 0; r < nr; r++) {
            const uint32_t va = a.s.ring_start[ra + r], vb = b.s.ring_start[rb + r];
            const uint32_t nv = a.s.ring_start[ra + r + 1] - va;
            if (nv != b.s.ring_start[rb + r + 1] - vb) return false;
            for (uint32_t i = 0; i < nv; i++) {
                const pip::Vec2 x = a.s.verts[va + i], y = b.s.verts[vb + i];
                if (bits_of(x.x) != bits_of(y.x) || bits_of(x.y) != bits_of(y.y)) return false;
            }
        }
    }
    return true;
}

// (l, c) is a self match: both rows are MOSAIC_ROW_OK and hold the same geometry.  Null rows and
// row-path rows are all stored as empty geometries, whatever they held (geoms_build.h), so their
// content says nothing about them: a pair with such a side is never a self match and is kept, with
// distance NaN.
MOSAIC_HD bool self_match(const Col& L, uint32_t l, const Col& C, uint32_t c) {
    return L.status[l] == 1 && C.status[c] == 1 && same_geometry(L, l, C, c);  // 1: MOSAIC_ROW_OK
}

MOSAIC_HD uint64_t pack_pair(int64_t l, int64_t c) { return (uint64_t)l << 32 | (uint64_t)(uint32_t)c; }

// ---- the host definition ----
struct CellIndex {
    std::vector<int64_t> cells, start;
    std::vector<int32_t> rows;
    int64_t max_per_cell = 0;
    CellIndexView view() const { return CellIndexView{cells.data(), start.data(), rows.data(), (int64_t)cells.size()}; }
};

// false: a negative key
inline bool build_index(const int64_t* index_id, const int32_t* key, int64_t n, CellIndex* out) {
    std::vector<std::pair<int64_t, int32_t>> e((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (key[i] < 0) return false;
        e[(size_t)i] = {index_id[i], key[i]};
    }
    std::sort(e.begin(), e.end());
    e.erase(std::unique(e.begin(), e.end()), e.end());
    *out = CellIndex();
    for (size_t i = 0; i < e.size(); i++) {
        if (i == 0 || e[i].first != e[i - 1].first) {
            out->cells.push_back(e[i].first);
            out->start.push_back((int64_t)i);
        }
        out->rows.push_back(e[i].second);
    }
    out->start.push_back((int64_t)e.size());
    for (size_t j = 0; j + 1 < out->start.size(); j++) out->max_per_cell = std::max(out->max_per_cell, out->start[j + 1] - out->start[j]);
    return true;
}

struct Neighbours {
    std::vector<int64_t> left_row, right_row;
    std::vector<double> distance;
    std::vector<uint8_t> unmatched;  // per landmark row
};

// 0, or 1 (nothing written) when a landmark row is outside L or the index names a row outside C
inline int neighbours(const CellIndexView& ix, const Col& L, const Col& C, const int64_t* left_row, const int64_t* cell,
                      int64_t n, bool keep_self, Neighbours* out) {
    for (int64_t i = 0; i < n; i++)
        if (left_row[i] < 0 || left_row[i] >= L.n) return 1;
    const int64_t n_entries = ix.n_cells ? ix.start[ix.n_cells] : 0;
    for (int64_t e = 0; e < n_entries; e++)
        if (ix.rows[e] >= C.n) return 1;
    *out = Neighbours();
    out->unmatched.assign((size_t)L.n, 0);
    std::vector<uint64_t> keys;
    for (int64_t i = 0; i < n; i++) {
        const int64_t j = find_cell(ix, cell[i]);
        if (j < 0) {
            out->unmatched[(size_t)left_row[i]] = 1;
            continue;
        }
        for (int64_t e = ix.start[j]; e < ix.start[j + 1]; e++) keys.push_back(pack_pair(left_row[i], ix.rows[e]));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    struct Row {
        uint64_t l, d, c;
    };
    std::vector<Row> rows;
    for (uint64_t k : keys) {
        const uint32_t l = (uint32_t)(k >> 32), c = (uint32_t)k;
        if (!keep_self && self_match(L, l, C, c)) continue;
        const bool ok = L.status[l] == 1 && C.status[c] == 1;  // MOSAIC_ROW_OK
        const double d = ok ? dist::distance(L.s, L.part_kind, l, C.s, C.part_kind, c) : std::numeric_limits<double>::quiet_NaN();
        rows.push_back(Row{l, bits_of(d), c});
    }
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) {
        if (a.l != b.l) return a.l < b.l;
        if (a.d != b.d) return a.d < b.d;
        return a.c < b.c;
    });
    for (const Row& r : rows) {
        out->left_row.push_back((int64_t)r.l);
        out->right_row.push_back((int64_t)r.c);
        double d;
        __builtin_memcpy(&d, &r.d, sizeof d);
        out->distance.push_back(d);
    }
    return 0;
}

// ---- the distance-within join ----
// All (landmark, candidate) pairs with st_distance <= radius[landmark]: the candidates come from the
// geometries themselves, not from a cell index.  Row i asks for landmark left_row[i] (null: row i)
// with radius[i]; left_row is strictly ascending, so a landmark is asked for once.
//   * (l, c) is a pair iff both rows are eligible -- MOSAIC_ROW_OK with at least one facet -- and
//     within_radius(dist::distance(l, c), radius).  An empty geometry is within distance of nothing
//     (dist::distance's 0.0 for it does not leak, st_intersects' stance); null and row-path rows
//     never pair, so no distance here is NaN.
//   * A NaN or negative radius gives its row no pairs; +inf and DBL_MAX accept every eligible
//     candidate; -0.0 is the radius 0.
//   * Self matches are dropped unless keep_self (self_match, as above).
//   * Order: (landmark row, distance bits, candidate row); unmatched[] is all zero.
// `within` below is the definition of the result: plain loops over all pairs, no filter of any kind.
//
// The kernels find their candidates with an envelope filter, and within_candidates is that filter's
// own count: the eligible candidates c with dist::box_lower_bound(bbox(l), bbox(c)) <= radius[i].
// The filter drops no pair: for eligible rows with finite coordinates box_lower_bound is at most
// the bits dist::distance computes (st_distance.h; both geometries have a facet, every facet lies
// in its geometry's box, and a contained component gives 0.0 over meeting boxes, whose bound is
// <= 0), so distance <= radius implies bound <= radius, also for radius = +inf.  Eligibility is
// decided from the status and the facet count, never from the box: the empty box
// {inf, inf, -inf, -inf} has the bound +inf against a finite box, which the radius +inf accepts.
MOSAIC_HD bool eligible(const Col& c, int64_t g) { return c.status[g] == 1 && c.facets[g] > 0; }  // 1: MOSAIC_ROW_OK

MOSAIC_HD bool radius_ok(double r) { return r >= 0; }  // false for NaN

// d is a number >= 0 here, so the order of the bits is the order of the values
MOSAIC_HD bool within_radius(double d, double r) { return radius_ok(r) && bits_of(d) <= bits_of(r + 0.0); }

MOSAIC_HD bool box_within(const pip::Box& a, const pip::Box& b, double r) { return dist::box_lower_bound(a, b) <= r; }

// 0, or 1 when the rows are not strictly ascending rows of L (left_row null: n > L.n)
inline int within_rows_check(const Col& L, const int64_t* left_row, int64_t n) {
    if (n < 0 || (!left_row && n > L.n)) return 1;
    if (left_row)
        for (int64_t i = 0; i < n; i++)
            if (left_row[i] < 0 || left_row[i] >= L.n || (i > 0 && left_row[i - 1] >= left_row[i])) return 1;
    return 0;
}

// counts[i]: the filter's candidates of row i.  1 with nothing written on a row error.
inline int within_candidates(const Col& L, const Col& C, const int64_t* left_row, const double* radius, int64_t n, int64_t* counts) {
    if (within_rows_check(L, left_row, n)) return 1;
    for (int64_t i = 0; i < n; i++) {
        const int64_t l = left_row ? left_row[i] : i;
        int64_t k = 0;
        if (eligible(L, l) && radius_ok(radius[i]))
            for (int64_t c = 0; c < C.n; c++)
                if (eligible(C, c) && box_within(L.s.geom_bbox[l], C.s.geom_bbox[c], radius[i])) k++;
        counts[i] = k;
    }
    return 0;
}

// 1 with nothing written on a row error
inline int within(const Col& L, const Col& C, const int64_t* left_row, const double* radius, int64_t n, bool keep_self,
                  Neighbours* out) {
    if (within_rows_check(L, left_row, n)) return 1;
    *out = Neighbours();
    out->unmatched.assign((size_t)L.n, 0);
    struct Row {
        uint64_t l, d, c;
    };
    std::vector<Row> rows;
    for (int64_t i = 0; i < n; i++) {
        const int64_t l = left_row ? left_row[i] : i;
        if (!eligible(L, l) || !radius_ok(radius[i])) continue;
        for (int64_t c = 0; c < C.n; c++) {
            if (!eligible(C, c)) continue;
            if (!keep_self && self_match(L, (uint32_t)l, C, (uint32_t)c)) continue;
            const double d = dist::distance(L.s, L.part_kind, (uint32_t)l, C.s, C.part_kind, (uint32_t)c);
            if (within_radius(d, radius[i])) rows.push_back(Row{(uint64_t)l, bits_of(d), (uint64_t)c});
        }
    }
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) {
        if (a.l != b.l) return a.l < b.l;
        if (a.d != b.d) return a.d < b.d;
        return a.c < b.c;
    });
    for (const Row& r : rows) {
        out->left_row.push_back((int64_t)r.l);
        out->right_row.push_back((int64_t)r.c);
        double d;
        __builtin_memcpy(&d, &r.d, sizeof d);
        out->distance.push_back(d);
    }
    return 0;
}

// layout fingerprint of what ring_neighbours.hip shares with the other translation units (join_binned.h's rationale)
static constexpr uint64_t layout_fingerprint() {
    uint64_t h = 0xcbf29ce484222325ULL;
    for (uint64_t v : {(uint64_t)sizeof(Col), (uint64_t)sizeof(CellIndexView), (uint64_t)sizeof(GeomStore), (uint64_t)sizeof(pip::Vec2),
                       (uint64_t)sizeof(pip::Box)})
        h = h * 0x100000001b3ULL ^ v;
    return h;
}

}  // namespace rn
}  // namespace mosaic
