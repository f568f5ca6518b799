// st_intersection_aggregate over the join of line chips with polygon chips, on the host: the
// restatement mosaic_line_intersection_aggregate(_geometry) (line_clip.hip) is tested against, bit for
// bit.  Needs no context and no GPU.  Rows are the equi-join of the two chip sets on index_id; one
// group per (line key, polygon key) that shares a cell, present even when its length is 0; per pair the
// increment of line_clip.h, by its sequential driver; the fold of line_clip_host.h.
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mosaic_hip.h"
#include "fail.h"
#include "geom_build.h"
#include "line_chips_build.h"
#include "line_clip_host.h"

using namespace mosaic;

extern "C" int mosaic_line_intersection_aggregate_host(int grid, int res, int64_t n_l, const uint8_t* l_core, const int64_t* l_cell,
                                                       const int32_t* l_key, const int64_t* l_off, const uint8_t* l_wkb, int64_t n_p,
                                                       const uint8_t* p_core, const int64_t* p_cell, const int32_t* p_key,
                                                       const int64_t* p_off, const uint8_t* p_wkb, mosaic_isect_geoms** out) {
    (void)res;
    if (grid != MOSAIC_GRID_H3 && grid != MOSAIC_GRID_BNG) return mosaic_tess_fail(MOSAIC_E_ARG, "unknown grid");
    if (!out || n_p < 0 || (n_p > 0 && (!p_core || !p_cell || !p_key || !p_off))) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    LineChipBuilder lb;
    std::string err;
    if (int rc = build_line_chips(n_l, l_core, l_cell, l_key, l_off, 0, l_wkb, lb, err)) return mosaic_tess_fail(rc, err.c_str());
    GeomBuilder gb;
    for (int64_t i = 0; i < n_p; i++) {
        const int64_t a = p_off[i], b = p_off[i + 1];
        if (a < 0 || b < a || (b > a && !p_wkb))
            return mosaic_tess_fail(MOSAIC_E_ARG, ("polygon chip " + std::to_string(i) + ": bad wkb offsets").c_str());
        if (p_key[i] < 0) return mosaic_tess_fail(MOSAIC_E_ARG, ("polygon chip " + std::to_string(i) + ": negative key").c_str());
        if (!gb.add(b > a ? p_wkb + a : nullptr, (size_t)(b - a)))
            return mosaic_tess_fail(MOSAIC_E_WKB, ("polygon chip " + std::to_string(i) + ": " + gb.error).c_str());
    }
    // the polygon chips by cell, rows in order within a cell; then every joined pair
    std::vector<std::pair<int64_t, uint32_t>> by_cell((size_t)n_p);
    for (int64_t i = 0; i < n_p; i++) by_cell[(size_t)i] = {p_cell[i], (uint32_t)i};
    std::sort(by_cell.begin(), by_cell.end());
    std::vector<lineisect::PairRec> pairs;
    for (int64_t i = 0; i < n_l; i++) {
        auto it = std::lower_bound(by_cell.begin(), by_cell.end(), std::make_pair(lb.cell[(size_t)i], (uint32_t)0));
        for (; it != by_cell.end() && it->first == lb.cell[(size_t)i]; ++it) {
            if (lb.is_core[(size_t)i])
                return mosaic_tess_fail(MOSAIC_E_ARG, ("st_intersection_aggregate (lines): line chip " + std::to_string(i) +
                                                       " is a core chip; lineFill makes none and a line result cannot hold a cell")
                                                          .c_str());
            const uint32_t j = it->second;
            pairs.push_back(lineisect::PairRec{lb.cell[(size_t)i], (uint32_t)i, j, (uint32_t)lb.key[(size_t)i],
                                               ((uint32_t)p_key[j] << 1) | (p_core[j] ? 1u : 0u)});
        }
    }
    if (pairs.size() >= ((size_t)1 << 31)) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "st_intersection_aggregate (lines): 2^31 chip pairs or more");
    const lineisect::LineStore L = lb.view();
    const pip::GeomStore P{gb.verts.data(), gb.ring_start.data(), gb.ring_bbox.data(),
                           gb.part_ring.data(), gb.geom_part.data(), gb.geom_bbox.data()};
    const size_t n = pairs.size();
    std::vector<double> len(n, 0.0);
    std::vector<uint64_t> run_off(n + 1, 0);
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int nt = (int)std::max<size_t>(1, std::min<size_t>(std::min<unsigned>(16u, hw), n / 64));
    std::vector<std::vector<lineisect::Run>> part_runs((size_t)nt);
    auto work = [&](int t) {
        std::vector<lineisect::Pt> cuts;
        for (size_t i = n * (size_t)t / (size_t)nt; i < n * ((size_t)t + 1) / (size_t)nt; i++) {
            uint32_t nr = 0;
            if (pairs[i].pmeta & 1u)
                len[i] = lineisect::chip_length(L, pairs[i].line);
            else
                len[i] = lineisect::clip_pair_host(L, pairs[i].line, P, pairs[i].poly, (uint32_t)i, cuts, &part_runs[(size_t)t], &nr);
            run_off[i + 1] = nr;
        }
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++) th.emplace_back(work, t);
        for (auto& t : th) t.join();
    }
    std::vector<lineisect::Run> runs;
    for (auto& p : part_runs) runs.insert(runs.end(), p.begin(), p.end());  // threads took the pairs in order
    for (size_t i = 0; i < n; i++) run_off[i + 1] += run_off[i];
    std::unique_ptr<mosaic_isect_geoms> g(new mosaic_isect_geoms());
    lineisect::fold_groups(pairs.data(), n, len.data(), true, L, run_off.data(), runs.data(), *g);
    *out = g.release();
    return MOSAIC_OK;
}
