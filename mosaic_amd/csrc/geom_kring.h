// grid_geometrykring / grid_geometrykloop (core/Mosaic.scala:111-144, 211-223; expressions/index/
// GeometryKRing*.scala, GeometryKLoop*.scala), the pieces the device kernels (geom_kring.hip) and a
// sequential host driver share.
//
// Per geometry, from the chips of getChips(geometry, res, keepCoreGeom = false): core = the cells of
// the is_core chips, border = the cells of the others, and with dist(c) = the smallest j with
// c in kLoop(b, j) for a border cell b (0 for the border cells themselves)
//   geometryKRing(k) = core + {c : dist(c) <= k}        (k >= 0)
//   geometryKLoop(k) = {c : dist(c) == k} - core         (k >= 1)
// H3: dist is the breadth-first layer under kRing(., 1) (h3fill::kring1), so the search is k rounds
// over a frontier.  BNG: the reference's loop arithmetic on origins at the grid's edge keeps cells a
// neighbour walk never reaches, so every border cell's loops 1..k are inserted directly
// (bng::kloop_cell) with dist = the smallest j.
//
// One open-addressing table serves a batch of geometries: the key packs (geometry in batch, cell),
// the value word holds the layer, the core flag and the not-yet-reached state.  Rows are emitted
// in Scala 2.12 immutable HashSet iteration order (h3nb::scala_set_order_key ascending, equal
// hashes by ascending id); sets of <= 4 cells iterate in insertion order in Scala, which is not
// restated (as in grid_polyfill).  No reference fixture pins these orders ("order unpinned").
#pragma once
#include <stdint.h>

#include "bng_device.h"
#include "h3_neighbors.h"
#include "h3_polyfill.h"

#if !defined(__HIPCC__)
#include <algorithm>
#include <utility>
#include <vector>
#endif

namespace mosaic {
namespace gk {

static const uint64_t kEmpty = ~0ull;
static const int64_t kGeomBatch = 4094;  // geometries per table (12 key bits, all-ones kept free)
static const int kMaxK = 1000;

MOSAIC_HD uint64_t hmix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

// ---- key: (geometry in batch, cell).  H3: 12 + 52 bits (mode and resolution are restored from
// res); BNG: 13 + 51 bits (ids are decimal numbers of at most 16 digits with a leading 1).
MOSAIC_HD int key_shift(bool bng) { return bng ? 51 : 52; }
MOSAIC_HD uint64_t pack(bool bng, int g, int64_t cell) {
    const int s = key_shift(bng);
    return (uint64_t)g << s | ((uint64_t)cell & (((uint64_t)1 << s) - 1));
}
MOSAIC_HD int key_geom(bool bng, uint64_t key) { return (int)(key >> key_shift(bng)); }
MOSAIC_HD int64_t key_cell(bool bng, int res, uint64_t key) {
    const uint64_t low = key & (((uint64_t)1 << key_shift(bng)) - 1);
    return (int64_t)(bng ? low : ((uint64_t)1 << 59 | (uint64_t)res << 52 | low));
}

// a chip id the search can take: a valid cell of the call's resolution
MOSAIC_HD bool chip_valid(bool bng, int res, int64_t id) {
    if (bng) {
        int r;
        int32_t e, x, y;
        return id < ((int64_t)1 << 51) && bng::cell_origin(id, &r, &e, &x, &y) && r == res;
    }
    return h3nb::is_valid_cell((uint64_t)id) && h3nb::res_of((uint64_t)id) == res;
}

// ---- value word: bit 0 = "not core", bits 1..31 = layer (kUnreached until the search arrives).
// A fresh slot is all ones.  Seeding a core chip clears bit 0, seeding a border chip clears the
// layer: both are atomicAnd and commute.  Bit 0 is final once the seeds are in (cells found later
// are never core), so a lane that reaches a cell at layer j takes the bit from the word it read
// and an atomicMin of (j << 1 | bit) lowers the layer without touching the flag.
static const uint32_t kValFresh = 0xffffffffu;
static const uint32_t kSeedCore = ~1u;   // and-mask
static const uint32_t kSeedBorder = 1u;  // and-mask
static const uint32_t kUnreached = 0x7fffffffu;
MOSAIC_HD uint32_t val_layer(uint32_t v) { return v >> 1; }
MOSAIC_HD bool val_core(uint32_t v) { return (v & 1u) == 0; }
MOSAIC_HD uint32_t val_reach(uint32_t cur, int layer) { return (uint32_t)layer << 1 | (cur & 1u); }
MOSAIC_HD bool val_keep(uint32_t v, int k, int loop) {
    return loop ? (!val_core(v) && val_layer(v) == (uint32_t)k) : (val_core(v) || val_layer(v) <= (uint32_t)k);
}
// dist of a kept cell; -1: a core cell the search did not reach within k
MOSAIC_HD int32_t val_dist(uint32_t v, int k) { return val_layer(v) <= (uint32_t)k ? (int32_t)val_layer(v) : -1; }

// ---- emitted records: sort key (geometry, Scala set order key: 12 + 35 bits) and the cell with its
// dist + 1 above the cell bits
MOSAIC_HD uint64_t sort_key(int g, int64_t cell) { return (uint64_t)g << 35 | h3nb::scala_set_order_key(cell); }
MOSAIC_HD int sort_key_geom(uint64_t sk) { return (int)(sk >> 35); }
static const int kSortKeyBits = 47;
MOSAIC_HD uint64_t pack_record(bool bng, uint64_t key, int32_t dist) {
    return (uint64_t)(dist + 1) << 52 | (key & (((uint64_t)1 << key_shift(bng)) - 1));
}
MOSAIC_HD int32_t record_dist(uint64_t rec) { return (int32_t)(rec >> 52) - 1; }
MOSAIC_HD int64_t record_cell(bool bng, int res, uint64_t rec) {
    return key_cell(bng, res, rec & (((uint64_t)1 << key_shift(bng)) - 1));
}

// table slots for n entries: a power of two, at most half full
MOSAIC_HD uint64_t slots_for(uint64_t n, uint64_t at_least) {
    uint64_t c = at_least;
    while (c < 2 * n) c <<= 1;
    return c;
}

#if !defined(__HIPCC__)
// ---- sequential driver of the same rounds (host builds only: tests/native/geom_kring_host.cpp).
// key[i] in [0, n_geoms); rows with an invalid chip get status -2 (MOSAIC_POLYFILL_UNSUPPORTED) and
// no cells.
struct HostLists {
    std::vector<int64_t> offsets{0};
    std::vector<int64_t> cells;
    std::vector<int32_t> dist;
    std::vector<int32_t> status;
};

struct HostTable {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    uint64_t mask = 0, count = 0;
    explicit HostTable(uint64_t slots) : keys(slots, kEmpty), vals(slots, kValFresh), mask(slots - 1) {}
    uint64_t insert(uint64_t key) {
        uint64_t h = hmix(key) & mask;
        for (uint64_t n = 0; n <= mask; n++, h = (h + 1) & mask) {
            if (keys[h] == kEmpty) {
                keys[h] = key;
                count++;
                return h;
            }
            if (keys[h] == key) return h;
        }
        return kEmpty;
    }
    // room for `more` entries: grows by rehashing
    void reserve(uint64_t more) {
        const uint64_t need = slots_for(count + more, mask + 1);
        if (need == mask + 1) return;
        HostTable t(need);
        for (uint64_t s = 0; s <= mask; s++)
            if (keys[s] != kEmpty) t.vals[t.insert(keys[s])] = vals[s];
        *this = std::move(t);
    }
};

inline void host_batch(bool bng, int res, const std::vector<int64_t>& chips, const uint8_t* is_core,
                       const int64_t* id, const int32_t* key, int64_t g0, int64_t g1, int k, int loop,
                       HostLists* out) {
    const int64_t ng = g1 - g0;
    std::vector<char> bad((size_t)ng, 0);
    HostTable tab(16);
    tab.reserve(chips.size());
    std::vector<uint64_t> frontier;
    for (int64_t i : chips) {
        const int g = (int)(key[i] - g0);
        if (!chip_valid(bng, res, id[i])) {
            bad[g] = 1;
            continue;
        }
        const uint64_t pk = pack(bng, g, id[i]);
        const uint64_t s = tab.insert(pk);
        if (is_core[i]) {
            tab.vals[s] &= kSeedCore;
        } else {
            if (val_layer(tab.vals[s]) != 0) frontier.push_back(pk);
            tab.vals[s] &= kSeedBorder;
        }
    }
    auto reach = [&](uint64_t pk, int layer) {
        const uint64_t s = tab.insert(pk);
        const uint32_t cur = tab.vals[s], cand = val_reach(cur, layer);
        const bool first = val_layer(cur) == kUnreached;
        if (cand < cur) tab.vals[s] = cand;
        return first;
    };
    if (!bng) {
        for (int round = 1; round <= k && !frontier.empty(); round++) {
            tab.reserve(7 * frontier.size());
            std::vector<uint64_t> next;
            for (uint64_t pk : frontier) {
                int64_t ring[7];
                const int g = key_geom(bng, pk);
                const int n = h3fill::kring1((uint64_t)key_cell(bng, res, pk), res, ring);
                if (n < 0) bad[g] = 1;
                for (int j = 0; j < n; j++) {
                    const uint64_t k2 = pack(bng, g, ring[j]);
                    if (reach(k2, round)) next.push_back(k2);
                }
            }
            frontier.swap(next);
        }
    } else {
        for (int j = 1; j <= k && !frontier.empty(); j++) {
            tab.reserve(8 * (uint64_t)j * frontier.size());
            for (uint64_t pk : frontier) {
                const int g = key_geom(bng, pk);
                int r;
                int32_t e, x, y;
                if (!bng::cell_origin(key_cell(bng, res, pk), &r, &e, &x, &y)) continue;
                for (int side = 0; side < 4; side++)
                    for (int c = 0; c < 2 * j; c++) {
                        int64_t cell;
                        if (bng::kloop_cell(r, e, x, y, j, side, c, &cell)) reach(pack(bng, g, cell), j);
                    }
            }
        }
    }
    struct Rec {
        uint64_t sk;
        int64_t cell;
        int32_t dist;
    };
    std::vector<Rec> recs;
    for (uint64_t s = 0; s <= tab.mask; s++) {
        const uint64_t pk = tab.keys[s];
        if (pk == kEmpty || bad[key_geom(bng, pk)] || !val_keep(tab.vals[s], k, loop)) continue;
        const int64_t cell = key_cell(bng, res, pk);
        recs.push_back({sort_key(key_geom(bng, pk), cell), cell, val_dist(tab.vals[s], k)});
    }
    std::sort(recs.begin(), recs.end(),
              [](const Rec& a, const Rec& b) { return a.sk != b.sk ? a.sk < b.sk : a.cell < b.cell; });
    size_t at = 0;
    for (int64_t g = 0; g < ng; g++) {
        for (; at < recs.size() && sort_key_geom(recs[at].sk) == g; at++) {
            out->cells.push_back(recs[at].cell);
            out->dist.push_back(recs[at].dist);
        }
        out->offsets.push_back((int64_t)out->cells.size());
        out->status.push_back(bad[g] ? -2 : 0);
    }
}

inline void host_run(bool bng, int res, int64_t n_chips, const uint8_t* is_core, const int64_t* id,
                     const int32_t* key, int64_t n_geoms, int k, int loop, HostLists* out) {
    for (int64_t g0 = 0; g0 < n_geoms; g0 += kGeomBatch) {
        const int64_t g1 = std::min(n_geoms, g0 + kGeomBatch);
        std::vector<int64_t> chips;
        for (int64_t i = 0; i < n_chips; i++)
            if (key[i] >= g0 && key[i] < g1) chips.push_back(i);
        host_batch(bng, res, chips, is_core, id, key, g0, g1, k, loop, out);
    }
}
#endif

}  // namespace gk
}  // namespace mosaic
