// Host side of the records k_tess_clip_ll returns (tess_gpu.h): the check every copied-back record
// passes before anything reads the vertices it points at (filter_records), and the records indexed by
// candidate and turned into WKB (ClippedChips).  Plain C++ (g++ and hipcc): mosaic_hip.hip filters,
// tessellate.cpp indexes and writes, tests/native/clip_records_host.cpp runs both on hand-made records.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "tess_gpu.h"

namespace mosaic {
namespace tessclip {

// Keeps exactly the records of tasks the device finished (status 0 or 2) and makes them safe to read.
// A record is dropped when its `cand` names no task or a task that went to the host (status 1; any
// status byte other than 0 / 2 counts as 1).  A record naming a finished task must have part, ring,
// off >= 0, n >= 1 and off + n within verts; one that does not demotes its task to status 1 -- the host
// clips it -- and all of the task's records go.  Returns the number of tasks demoted.
inline int64_t filter_records(const std::vector<int64_t>& tasks, ClipResult* out) {
    const int64_t n_tasks = (int64_t)tasks.size(), n_verts = (int64_t)(out->verts.size() / 2);
    out->status.resize((size_t)n_tasks, 1);
    for (uint8_t& s : out->status)
        if (s != 0 && s != 2) s = 1;
    std::unordered_map<int64_t, int64_t> pos;
    pos.reserve((size_t)n_tasks);
    for (int64_t t = 0; t < n_tasks; t++) pos[tasks[(size_t)t]] = t;
    auto task_of = [&](int64_t cand) -> int64_t {
        auto it = pos.find(cand);
        return it == pos.end() ? -1 : it->second;
    };
    // the task of every record (-1: none), demoting the tasks of malformed ones
    std::vector<int64_t> rt(out->rings.size()), pt(out->parts.size());
    int64_t demoted = 0;
    auto demote = [&](int64_t t) {
        if (out->status[(size_t)t] != 1) out->status[(size_t)t] = 1, demoted++;
    };
    for (size_t i = 0; i < out->rings.size(); i++) {
        const ClipRing& r = out->rings[i];
        const int64_t t = rt[i] = task_of(r.cand);
        if (t < 0 || out->status[(size_t)t] == 1) continue;
        if (r.part < 0 || r.ring < 0 || r.off < 0 || r.n < 1 || r.off > n_verts - (int64_t)r.n) demote(t);
    }
    for (size_t i = 0; i < out->parts.size(); i++) {
        const ClipPart& p = out->parts[i];
        const int64_t t = pt[i] = task_of(p.cand);
        if (t < 0 || out->status[(size_t)t] == 1) continue;
        if (p.part < 0) demote(t);
    }
    auto compact = [&](auto& v, const std::vector<int64_t>& vt) {
        size_t n = 0;
        for (size_t i = 0; i < v.size(); i++)
            if (vt[i] >= 0 && out->status[(size_t)vt[i]] != 1) v[n++] = v[i];
        v.resize(n);
    };
    compact(out->rings, rt);
    compact(out->parts, pt);
    return demoted;
}

// The border chips the GPU clipped, indexed by candidate: rings sorted by (candidate, part, ring),
// parts by (candidate, part).  `r` has passed filter_records.
struct ClippedChips {
    ClipResult r;
    std::vector<int64_t> task_of;  // candidate -> task (-1: not a border task)
    std::vector<int64_t> ring_at, part_at;  // candidate c's rings / parts: [ring_at[c], ring_at[c + 1])
    void index(int64_t n_cand, const std::vector<int64_t>& tasks) {
        // stable counting sort by candidate (the kernels append each candidate's rings / parts in
        // (part, ring) order from one wave or lane; a candidate whose entries are not is sorted on
        // its own), keeping each candidate's start
        auto by_cand = [&](auto& v, auto less, std::vector<int64_t>& start) {
            start.assign((size_t)n_cand + 1, 0);
            for (auto& e : v) start[(size_t)e.cand + 1]++;
            for (int64_t c = 0; c < n_cand; c++) start[(size_t)c + 1] += start[(size_t)c];
            std::remove_reference_t<decltype(v)> out(v.size());
            std::vector<int64_t> pos(start.begin(), start.end() - 1);
            for (auto& e : v) out[(size_t)pos[(size_t)e.cand]++] = e;
            for (int64_t c = 0; c < n_cand; c++) {
                auto b = out.begin() + start[(size_t)c], e = out.begin() + start[(size_t)c + 1];
                if (e - b > 1 && !std::is_sorted(b, e, less)) std::sort(b, e, less);
            }
            v.swap(out);
        };
        by_cand(r.rings, [](const ClipRing& a, const ClipRing& b) {
            return a.part != b.part ? a.part < b.part : a.ring < b.ring;
        }, ring_at);
        by_cand(r.parts, [](const ClipPart& a, const ClipPart& b) { return a.part < b.part; }, part_at);
        task_of.assign((size_t)n_cand, -1);
        for (size_t t = 0; t < tasks.size(); t++) task_of[(size_t)tasks[t]] = (int64_t)t;
    }
    bool redo(int64_t k) const { return task_of[(size_t)k] < 0 || r.status[(size_t)task_of[(size_t)k]] == 1; }
    bool is_cell(int64_t k) const { return task_of[(size_t)k] >= 0 && r.status[(size_t)task_of[(size_t)k]] == 2; }
    // candidate k's clipped geometry as clip_cell's out_parts (kept parts with rings, closed rings);
    // G3: parts -> rings -> points {x, y}
    template <class G3>
    void parts_of(int64_t k, G3& out) const {
        using Rings = typename G3::value_type;
        using Ring = typename Rings::value_type;
        out.clear();
        size_t jr = (size_t)ring_at[(size_t)k];
        for (size_t jp = (size_t)part_at[(size_t)k]; jp < r.parts.size() && r.parts[jp].cand == k; jp++) {
            const int32_t part = r.parts[jp].part;
            while (jr < r.rings.size() && r.rings[jr].cand == k && r.rings[jr].part < part) jr++;
            const size_t r0 = jr;
            while (jr < r.rings.size() && r.rings[jr].cand == k && r.rings[jr].part == part) jr++;
            if (!r.parts[jp].keep || jr == r0) continue;
            Rings rings;
            for (size_t q = r0; q < jr; q++) {
                const ClipRing& cr = r.rings[q];
                Ring ring((size_t)cr.n);
                for (int32_t v = 0; v < cr.n; v++) ring[(size_t)v] = {r.verts[2 * (cr.off + v)], r.verts[2 * (cr.off + v) + 1]};
                rings.push_back(std::move(ring));
            }
            out.push_back(std::move(rings));
        }
    }
    // candidate k's chip as WKB appended to w (to_wkb's bytes); false (nothing written): no chip
    template <class W>
    bool chip(int64_t k, W& w) const {
        const size_t ir = (size_t)ring_at[(size_t)k], ip = (size_t)part_at[(size_t)k];
        // the kept parts that have rings: (first ring, ring count)
        std::pair<size_t, size_t> kept[64];
        std::vector<std::pair<size_t, size_t>> more;
        size_t n_kept = 0, jr = ir;
        for (size_t jp = ip; jp < r.parts.size() && r.parts[jp].cand == k; jp++) {
            const int32_t part = r.parts[jp].part;
            while (jr < r.rings.size() && r.rings[jr].cand == k && r.rings[jr].part < part) jr++;
            const size_t r0 = jr;
            while (jr < r.rings.size() && r.rings[jr].cand == k && r.rings[jr].part == part) jr++;
            if (!r.parts[jp].keep || jr == r0) continue;
            if (n_kept < 64) kept[n_kept] = {r0, jr - r0};
            else more.push_back({r0, jr - r0});
            n_kept++;
        }
        if (n_kept == 0) return false;
        auto part_at = [&](size_t i) { return i < 64 ? kept[i] : more[i - 64]; };
        if (n_kept > 1) {
            w.u8(0);
            w.u32(6);
            w.u32((uint32_t)n_kept);
        }
        for (size_t i = 0; i < n_kept; i++) {
            const auto pr = part_at(i);
            w.u8(0);
            w.u32(3);
            w.u32((uint32_t)pr.second);
            for (size_t q = pr.first; q < pr.first + pr.second; q++) {
                const ClipRing& cr = r.rings[q];
                w.u32((uint32_t)cr.n);
                for (int32_t v = 0; v < cr.n; v++) {
                    w.f64(r.verts[2 * (cr.off + v)]);
                    w.f64(r.verts[2 * (cr.off + v) + 1]);
                }
            }
        }
        return true;
    }
};

}  // namespace tessclip
}  // namespace mosaic
