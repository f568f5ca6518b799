// Host side of the line-polygon st_intersection_aggregate, shared by the GPU entry points
// (line_clip.hip) and the host restatement (line_clip_host.cpp): the joined chip pair record and the
// fold of per-pair lengths and runs into groups -- one code path for both, so they agree bit for bit.
//
// Group = (line key, polygon key).  Its length is the sum of its pairs' lengths in the order (cell id,
// line chip row, polygon chip row); its geometry the pairs' runs in that order, then in run order, in
// JTS's big-endian 2D layout: LINESTRING for one run, MULTILINESTRING for several, LINESTRING EMPTY
// (type 2, zero points) for none.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "isect_geom.h"
#include "line_clip.h"

namespace mosaic {
namespace lineisect {

// one joined chip pair; pmeta = (polygon key << 1) | polygon chip is core
struct PairRec {
    int64_t cell;
    uint32_t line, poly, lkey, pmeta;
};

namespace detail {
inline void put_u32(std::vector<uint8_t>& o, uint32_t v) {
    for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s));
}
inline void put_line(std::vector<uint8_t>& o, const Pt* p, size_t n) {
    o.push_back(0);
    put_u32(o, 2);
    put_u32(o, (uint32_t)n);
    const size_t at = o.size();
    o.resize(at + 16 * n);
    uint8_t* w = o.data() + at;
    for (size_t i = 0; i < n; i++)
        for (double d : {p[i].x, p[i].y}) {
            uint64_t v;
            memcpy(&v, &d, 8);
            v = __builtin_bswap64(v);  // (little-endian hosts: the build's only targets)
            memcpy(w, &v, 8);
            w += 8;
        }
}
}  // namespace detail

// Folds the pairs into groups.  len[i]: pair i's length (a core-polygon pair: the line chip's whole
// length).  With geometry: run_off[i] .. run_off[i + 1] are pair i's records in `runs` (none for a
// core-polygon pair: its runs are the chip's pieces, read from L), and L holds the line chips' verts,
// piece_start and chip_piece on the host.  Without: L is not read and every WKB is left empty.
inline void fold_groups(const PairRec* pairs, size_t n, const double* len, bool geometry, const LineStore& L, const uint64_t* run_off,
                        const Run* runs, mosaic_isect_geoms& out) {
    std::vector<uint32_t> ord(n);
    for (size_t i = 0; i < n; i++) ord[i] = (uint32_t)i;
    auto gkey = [&](uint32_t i) { return ((uint64_t)pairs[i].lkey << 32) | (uint64_t)(pairs[i].pmeta >> 1); };
    std::sort(ord.begin(), ord.end(), [&](uint32_t p, uint32_t q) {
        const PairRec &a = pairs[p], &b = pairs[q];
        const uint64_t ka = gkey(p), kb = gkey(q);
        if (ka != kb) return ka < kb;
        if (a.cell != b.cell) return a.cell < b.cell;
        if (a.line != b.line) return a.line < b.line;
        return a.poly < b.poly;
    });
    out.off.assign(1, 0);
    std::vector<Pt> pts;
    std::vector<uint32_t> starts;  // run r of the group = pts[starts[r] .. starts[r + 1])
    auto end_run = [&]() {
        if (pts.size() - starts.back() < 2)
            pts.resize(starts.back());
        else
            starts.push_back((uint32_t)pts.size());
    };
    auto push = [&](Pt p) {
        if (pts.size() > starts.back() && bit_equal(pts.back(), p)) return;
        pts.push_back(p);
    };
    for (size_t s = 0; s < n;) {
        size_t e = s;
        double sum = 0.0;
        pts.clear();
        starts.assign(1, 0);
        for (; e < n && gkey(ord[e]) == gkey(ord[s]); e++) {
            const uint32_t i = ord[e];
            sum += len[i];
            if (!geometry) continue;
            if (pairs[i].pmeta & 1u) {
                for (uint32_t m = L.chip_piece[pairs[i].line]; m < L.chip_piece[pairs[i].line + 1]; m++) {
                    if (L.piece_start[m + 1] - L.piece_start[m] < 2) continue;
                    for (uint32_t v = L.piece_start[m]; v < L.piece_start[m + 1]; v++) push(vert(L.verts, v));
                    end_run();
                }
            } else {
                for (uint64_t r = run_off[i]; r < run_off[i + 1]; r++) {
                    push(runs[r].p0);
                    for (uint32_t v = runs[r].seg0 + 1; v <= runs[r].seg1; v++) push(vert(L.verts, v));
                    push(runs[r].p1);
                    end_run();
                }
            }
        }
        out.lk.push_back((int32_t)pairs[ord[s]].lkey);
        out.rk.push_back((int32_t)(pairs[ord[s]].pmeta >> 1));
        out.area.push_back(sum);
        out.status.push_back(0);
        if (geometry) {
            const size_t nr = starts.size() - 1;
            if (nr == 0) {
                detail::put_line(out.wkb, nullptr, 0);
            } else if (nr == 1) {
                detail::put_line(out.wkb, pts.data(), pts.size());
            } else {
                out.wkb.push_back(0);
                detail::put_u32(out.wkb, 5);
                detail::put_u32(out.wkb, (uint32_t)nr);
                for (size_t r = 0; r < nr; r++) detail::put_line(out.wkb, pts.data() + starts[r], starts[r + 1] - starts[r]);
            }
        }
        out.off.push_back((int64_t)out.wkb.size());
        s = e;
    }
}

}  // namespace lineisect
}  // namespace mosaic
