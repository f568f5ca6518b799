// st_intersects_aggregate over the join of line chips with polygon chips, on the host: the
// restatement mosaic_line_intersects_aggregate (line_join.hip) is tested against.  Needs no context
// and no GPU.  Rows are the equi-join of the two chip sets on index_id; one group per (line key,
// polygon key) that shares a cell; flag = OR over the group's chip pairs of line.is_core ||
// polygon.is_core || intersects(line.wkb, polygon.wkb), the last by the sequential driver of
// line_isect.h (ST_IntersectsAggregate.scala:28-39).
#include <stdint.h>

#include <algorithm>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/mosaic_hip.h"
#include "fail.h"
#include "geom_build.h"
#include "line_chips_build.h"
#include "line_isect.h"

using namespace mosaic;

namespace {

int n_threads(int64_t work, int64_t per_thread) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<unsigned>(16u, hw), work / per_thread));
}

}  // namespace

extern "C" int mosaic_line_intersects_aggregate_host(int grid, int res, int64_t n_l, const uint8_t* l_core, const int64_t* l_cell,
                                                     const int32_t* l_key, const int64_t* l_off, const uint8_t* l_wkb, int64_t n_p,
                                                     const uint8_t* p_core, const int64_t* p_cell, const int32_t* p_key,
                                                     const int64_t* p_off, const uint8_t* p_wkb, int32_t* out_line_key,
                                                     int32_t* out_polygon_key, uint8_t* out_flag, int64_t cap, int64_t* n_out) {
    (void)res;
    if (grid != MOSAIC_GRID_H3 && grid != MOSAIC_GRID_BNG) return mosaic_tess_fail(MOSAIC_E_ARG, "unknown grid");
    if (!n_out || cap < 0 || n_p < 0 || (cap > 0 && (!out_line_key || !out_polygon_key || !out_flag)) ||
        (n_p > 0 && (!p_core || !p_cell || !p_key || !p_off)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *n_out = 0;
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
    // the polygon chips by cell
    std::vector<std::pair<int64_t, uint32_t>> by_cell((size_t)n_p);
    for (int64_t i = 0; i < n_p; i++) by_cell[(size_t)i] = {p_cell[i], (uint32_t)i};
    std::sort(by_cell.begin(), by_cell.end());
    const lineisect::LineStore L = lb.view();
    const pip::GeomStore P{gb.verts.data(), gb.ring_start.data(), gb.ring_bbox.data(),
                           gb.part_ring.data(), gb.geom_part.data(), gb.geom_bbox.data()};
    // per thread: the groups of a run of line chips; a group already true skips the geometry test
    const int nt = n_threads(n_l, 256);
    std::vector<std::unordered_map<uint64_t, uint8_t>> parts((size_t)nt);
    auto run = [&](int t) {
        std::unordered_map<uint64_t, uint8_t>& groups = parts[(size_t)t];
        for (int64_t i = n_l * t / nt; i < n_l * (t + 1) / nt; i++) {
            auto it = std::lower_bound(by_cell.begin(), by_cell.end(), std::make_pair(lb.cell[(size_t)i], (uint32_t)0));
            for (; it != by_cell.end() && it->first == lb.cell[(size_t)i]; ++it) {
                const uint32_t j = it->second;
                uint8_t& flag = groups.emplace(((uint64_t)(uint32_t)lb.key[(size_t)i] << 32) | (uint32_t)p_key[j], 0).first->second;
                if (flag) continue;
                flag = lb.is_core[(size_t)i] || p_core[j] || lineisect::intersects(L, (uint32_t)i, P, j);
            }
        }
    };
    if (nt == 1) {
        run(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++) th.emplace_back(run, t);
        for (auto& t : th) t.join();
    }
    for (int t = 1; t < nt; t++)
        for (const auto& g : parts[(size_t)t]) parts[0][g.first] |= g.second;
    std::vector<std::pair<uint64_t, uint8_t>> groups(parts[0].begin(), parts[0].end());
    std::sort(groups.begin(), groups.end());
    *n_out = (int64_t)groups.size();
    if ((int64_t)groups.size() > cap)
        return mosaic_tess_fail(MOSAIC_E_CAPACITY, ("st_intersects_aggregate (lines): " + std::to_string(groups.size()) + " groups").c_str());
    for (size_t i = 0; i < groups.size(); i++) {
        out_line_key[i] = (int32_t)(groups[i].first >> 32);
        out_polygon_key[i] = (int32_t)(groups[i].first & 0xffffffffULL);
        out_flag[i] = groups[i].second;
    }
    return MOSAIC_OK;
}
