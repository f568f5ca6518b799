// mosaic_tessellate_lines: Mosaic.lineFill on the host (lineclip.h), and the host routines of the device
// producer (line_fill.h).  g++: the H3 tables are host constants here.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mosaic_hip.h"
#include "chip_set.h"
#include "fail.h"
#include "line_fill.h"

namespace mosaic {
namespace linefill {

namespace {

int n_threads(int64_t work, int64_t per_thread) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<unsigned>(16u, hw), work / per_thread));
}

template <class F>
void parallel_chunks(int64_t n, int64_t per_thread, F f) {  // f(thread, begin, end)
    const int nt = n_threads(n, per_thread);
    if (nt == 1) {
        f(0, (int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([=] { f(t, n * t / nt, n * (t + 1) / nt); });
    for (auto& t : th) t.join();
}

struct Wkb {  // JTS WKBWriter: big-endian, 2D
    uint8_t* b;
    void u8(uint8_t v) { *b++ = v; }
    void u32(uint32_t v) {
        v = __builtin_bswap32(v);
        memcpy(b, &v, 4);
        b += 4;
    }
    void f64(double d) {
        uint64_t u;
        memcpy(&u, &d, 8);
        u = __builtin_bswap64(u);
        memcpy(b, &u, 8);
        b += 8;
    }
    void pt(lineclip::Pt p) {
        f64(p.x);
        f64(p.y);
    }
};

int64_t chip_bytes(const lineclip::Item* it, int32_t n, bool pieces) {
    if (!pieces) return n == 1 ? 21 : 9 + 21 * (int64_t)n;
    int64_t b = n == 1 ? 0 : 9;
    for (int32_t i = 0; i < n; i++) b += 9 + 16 * ((int64_t)it[i].nv + 2);
    return b;
}

void chip_write(const double* xy, const lineclip::Item* it, int32_t n, bool pieces, uint8_t* dst) {
    Wkb w{dst};
    if (n != 1) {
        w.u8(0);
        w.u32(pieces ? 5 : 4);
        w.u32((uint32_t)n);
    }
    for (int32_t i = 0; i < n; i++) {
        w.u8(0);
        if (!pieces) {
            w.u32(1);
            w.pt(it[i].in);
            continue;
        }
        w.u32(2);
        w.u32((uint32_t)it[i].nv + 2);
        w.pt(it[i].in);
        for (int64_t v = it[i].v0; v < it[i].v0 + it[i].nv; v++) w.pt(lineclip::vtx(xy, v));
        w.pt(it[i].out);
    }
}

}  // namespace

bool CachedPoly::operator()(int64_t id, lineclip::Cell& C) const {
    struct Slot {
        int64_t id = 0;
        int32_t grid = -1, res = 0;
        bool ok = false;
        lineclip::Cell C;
    };
    thread_local std::vector<Slot> slots(4096);
    Slot& s = slots[(size_t)(((uint64_t)id * 0x9e3779b97f4a7c15ULL) >> 52)];
    if (s.id != id || s.grid != g.grid || s.res != g.res) {
        s.id = id;
        s.grid = g.grid;
        s.res = g.res;
        s.ok = lineclip::cell_poly(g, id, s.C);
    }
    C = s.C;
    return s.ok;
}

int prepare(int64_t n_geoms, const int64_t* geom_lines, const int64_t* line_offsets, const double* xy, Clean& out) {
    if (n_geoms < 0 || n_geoms > 0x7fffffff || (n_geoms > 0 && (!geom_lines || !line_offsets)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    out = Clean();
    out.line_off.push_back(0);
    if (n_geoms == 0) return MOSAIC_OK;
    const int64_t n_lines = geom_lines[n_geoms];
    if (geom_lines[0] != 0 || n_lines < 0 || n_lines > 0x7fffffff) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid line offsets");
    if (n_lines > 0 && (line_offsets[0] != 0 || line_offsets[n_lines] >= 0x7fffffff || (line_offsets[n_lines] > 0 && !xy)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid vertex offsets (at most 2^31 - 2 vertices)");
    out.xy.reserve((size_t)(n_lines ? line_offsets[n_lines] : 0) * 2);
    for (int64_t g = 0; g < n_geoms; g++) {
        if (geom_lines[g + 1] < geom_lines[g] || geom_lines[g + 1] > n_lines) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid line offsets");
        for (int64_t l = geom_lines[g]; l < geom_lines[g + 1]; l++) {
            const int64_t v0 = line_offsets[l], v1 = line_offsets[l + 1];
            if (v1 < v0 || v1 > line_offsets[n_lines]) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid vertex offsets");
            const size_t first = out.xy.size() / 2;
            for (int64_t v = v0; v < v1; v++) {
                const double x = xy[2 * v], y = xy[2 * v + 1];
                if (x != x || y != y)
                    return mosaic_tess_fail(MOSAIC_E_NAN, ("geometry " + std::to_string(g) + ": NaN coordinate").c_str());
                const size_t n = out.xy.size() / 2;
                if (n > first && out.xy[2 * n - 2] == x && out.xy[2 * n - 1] == y) continue;
                out.xy.push_back(x);
                out.xy.push_back(y);
                out.vert_line.push_back((int32_t)out.n_lines);
            }
            if (v1 > v0 && out.xy.size() / 2 - first < 2)
                return mosaic_tess_fail(MOSAIC_E_ARG, ("geometry " + std::to_string(g) + ": a line of one distinct vertex").c_str());
            out.line_off.push_back((int64_t)(out.xy.size() / 2));
            out.line_geom.push_back((int32_t)g);
            out.n_lines++;
        }
    }
    out.n_verts = (int64_t)(out.xy.size() / 2);
    return MOSAIC_OK;
}

int fail_bad_cell(const Clean& c, int64_t s) {
    const int32_t g = c.line_geom[(size_t)c.vert_line[(size_t)s]];
    return mosaic_tess_fail(MOSAIC_E_ARG, ("geometry " + std::to_string(g) +
                                           ": the line comes to a cell that is no planar polygon of the grid's coordinates "
                                           "(over the antimeridian or a pole) or leaves the grid")
                                              .c_str());
}

int walk_span_host(lineclip::Grid g, const Clean& c, int64_t s, int32_t j, int32_t K, std::vector<int64_t>& cells) {
    thread_local std::vector<int64_t> seen;
    const lineclip::Pt a = lineclip::vtx(c.xy.data(), s), b = lineclip::vtx(c.xy.data(), s + 1);
    for (size_t cap = lineclip::kWalkCap;; cap *= 4) {
        if (seen.size() < cap) seen.resize(cap);
        const size_t n0 = cells.size();
        const int st = lineclip::walk_span(g, CachedPoly{g}, a, b, j, K, seen.data(), (int32_t)cap, [&](int64_t cell) { cells.push_back(cell); });
        if (st != lineclip::kNeedsMore) return st;
        cells.resize(n0);
    }
}

int finish(lineclip::Grid g, const Clean& c, int64_t n_groups, GroupRec* recs, const int64_t* seg_start, const uint32_t* segs,
           const lineclip::Item* items, int cells_only, mosaic_chip_set* cs, int64_t* bad_seg) {
    *bad_seg = -1;
    // the groups left to the host
    std::vector<int64_t> todo;
    for (int64_t i = 0; i < n_groups; i++)
        if (recs[i].status == lineclip::kNeedsMore) todo.push_back(i);
    std::vector<std::vector<lineclip::Item>> built(todo.size());
    std::vector<int64_t> bad(16, -1);
    parallel_chunks((int64_t)todo.size(), 64, [&](int t, int64_t b0, int64_t b1) {
        std::vector<lineclip::Item> ws(64);
        for (int64_t q = b0; q < b1; q++) {
            GroupRec& r = recs[todo[(size_t)q]];
            const int64_t i = todo[(size_t)q];
            lineclip::Cell C;
            if (!CachedPoly{g}(r.cell, C)) {
                if (bad[(size_t)t] < 0) bad[(size_t)t] = (int64_t)r.seg_first;
                r.status = lineclip::kBadCell;
                continue;
            }
            for (;;) {
                lineclip::Work w{ws.data(), (int32_t)ws.size(), 0, 0, 0, -1, 0.0};
                const int st = lineclip::build(c.xy.data(), C, segs + seg_start[i], seg_start[i + 1] - seg_start[i], w);
                if (st == lineclip::kNeedsMore) {
                    ws.resize(ws.size() * 4);
                    continue;
                }
                r.status = lineclip::kOk;
                r.n_items = w.n;
                r.has_piece = w.has_piece;
                r.s0 = w.s0;
                r.t0 = w.t0;
                built[(size_t)q].assign(ws.begin(), ws.begin() + w.n);
                break;
            }
        }
    });
    for (int64_t b : bad)
        if (b >= 0 && (*bad_seg < 0 || b < *bad_seg)) *bad_seg = b;
    if (*bad_seg >= 0) return MOSAIC_OK;
    std::vector<const lineclip::Item*> where((size_t)n_groups, nullptr);
    for (int64_t i = 0; i < n_groups; i++) where[(size_t)i] = items ? items + recs[i].item0 : nullptr;
    for (size_t q = 0; q < todo.size(); q++) where[(size_t)todo[q]] = built[q].data();
    // row order: line (component order within the geometry), position along the line, cell
    std::vector<int64_t> order;
    order.reserve((size_t)n_groups);
    for (int64_t i = 0; i < n_groups; i++)
        if (recs[i].n_items > 0) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const GroupRec &a = recs[x], &b = recs[y];
        const int32_t la = c.vert_line[a.seg_first], lb = c.vert_line[b.seg_first];
        if (la != lb) return la < lb;
        if (a.s0 != b.s0) return a.s0 < b.s0;
        if (a.t0 != b.t0) return a.t0 < b.t0;
        return (uint64_t)a.cell < (uint64_t)b.cell;
    });
    const size_t n = order.size();
    cs->is_core.assign(n, 0);
    cs->index_id.resize(n);
    cs->key.resize(n);
    cs->wkb_offsets.assign(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        const GroupRec& r = recs[order[k]];
        cs->index_id[k] = r.cell;
        cs->key[k] = c.line_geom[(size_t)c.vert_line[r.seg_first]];
        cs->wkb_offsets[k + 1] = cs->wkb_offsets[k] + (cells_only ? 0 : chip_bytes(where[(size_t)order[k]], r.n_items, r.has_piece != 0));
    }
    if (cells_only) return MOSAIC_OK;
    cs->wkb.resize((size_t)cs->wkb_offsets[n]);
    parallel_chunks((int64_t)n, 4096, [&](int, int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; k++) {
            const GroupRec& r = recs[order[(size_t)k]];
            chip_write(c.xy.data(), where[(size_t)order[(size_t)k]], r.n_items, r.has_piece != 0, cs->wkb.data() + cs->wkb_offsets[(size_t)k]);
        }
    });
    return MOSAIC_OK;
}

}  // namespace linefill
}  // namespace mosaic

using namespace mosaic;

extern "C" {

uint64_t mosaic_layout_lines_host(void) { return linefill::layout_fingerprint(); }

int mosaic_tessellate_lines(int grid, int res, int64_t n_geoms, const int64_t* geom_lines, const int64_t* line_offsets,
                            const double* xy, int cells_only, mosaic_chip_set** out) {
    if (!out) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (grid == MOSAIC_GRID_H3 && (res < 0 || res > 15))
        return mosaic_tess_fail(MOSAIC_E_RES, ("H3 resolution has to be between 0 and 15; found " + std::to_string(res)).c_str());
    if (grid == MOSAIC_GRID_BNG && !(res != 0 && res >= -6 && res <= 6))
        return mosaic_tess_fail(MOSAIC_E_RES, ("BNG resolution not supported; found " + std::to_string(res)).c_str());
    if (grid != MOSAIC_GRID_H3 && grid != MOSAIC_GRID_BNG) return mosaic_tess_fail(MOSAIC_E_ARG, "unknown grid");
    linefill::Clean c;
    if (int rc = linefill::prepare(n_geoms, geom_lines, line_offsets, xy, c)) return rc;
    const lineclip::Grid G{grid == MOSAIC_GRID_H3 ? 0 : 1, res};
    // per thread: the (cell, segment) pairs of a run of lines, sorted into groups line by line
    struct Part {
        std::vector<linefill::GroupRec> recs;
        std::vector<int64_t> counts;
        std::vector<uint32_t> segs;
        int64_t bad = -1;
    };
    std::vector<Part> parts(16);
    linefill::parallel_chunks(c.n_lines, 8, [&](int t, int64_t l0, int64_t l1) {
        Part& P = parts[(size_t)t];
        std::vector<int64_t> cells;
        std::vector<std::pair<uint64_t, uint32_t>> pairs;
        for (int64_t l = l0; l < l1 && P.bad < 0; l++) {
            pairs.clear();
            for (int64_t s = c.line_off[(size_t)l]; s + 1 < c.line_off[(size_t)l + 1] && P.bad < 0; s++) {
                const lineclip::Pt a = lineclip::vtx(c.xy.data(), s), b = lineclip::vtx(c.xy.data(), s + 1);
                int32_t K = 0;
                if (lineclip::span_count(G, linefill::CachedPoly{G}, a, b, &K) != lineclip::kOk) {
                    P.bad = s;
                    break;
                }
                cells.clear();
                for (int32_t j = 0; j < K; j++)
                    if (linefill::walk_span_host(G, c, s, j, K, cells) != lineclip::kOk) {
                        P.bad = s;
                        break;
                    }
                for (int64_t cell : cells) pairs.emplace_back((uint64_t)cell, (uint32_t)s);
            }
            std::sort(pairs.begin(), pairs.end());
            pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
            for (size_t i = 0; i < pairs.size(); i++) {
                if (i == 0 || pairs[i].first != pairs[i - 1].first) {
                    P.recs.push_back(linefill::GroupRec{(int64_t)pairs[i].first, -1, 0.0, 0, 0, 0, lineclip::kNeedsMore, pairs[i].second});
                    P.counts.push_back(0);
                }
                P.counts.back()++;
                P.segs.push_back(pairs[i].second);
            }
        }
    });
    int64_t bad = -1;
    for (auto& P : parts)
        if (P.bad >= 0 && (bad < 0 || P.bad < bad)) bad = P.bad;
    if (bad >= 0) return linefill::fail_bad_cell(c, bad);
    std::vector<linefill::GroupRec> recs;
    std::vector<int64_t> seg_start{0};
    std::vector<uint32_t> segs;
    for (auto& P : parts) {
        recs.insert(recs.end(), P.recs.begin(), P.recs.end());
        for (int64_t n : P.counts) seg_start.push_back(seg_start.back() + n);
        segs.insert(segs.end(), P.segs.begin(), P.segs.end());
    }
    mosaic_chip_set* cs = new mosaic_chip_set();
    const int rc = linefill::finish(G, c, (int64_t)recs.size(), recs.data(), seg_start.data(), segs.data(), nullptr, cells_only, cs, &bad);
    if (rc || bad >= 0) {
        delete cs;
        return rc ? rc : linefill::fail_bad_cell(c, bad);
    }
    *out = cs;
    return MOSAIC_OK;
}

}  // extern "C"
