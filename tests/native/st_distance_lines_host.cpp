// CPU build of st_distance with line geometries (mosaic_amd/csrc/st_distance.h: the kind-aware
// sequential driver dist::distance; mosaic_amd/csrc/geoms_build.h: the column builder with its
// opt-in LineString / MultiLineString decode and the LineSet form) and of GridRingNeighbours over
// such columns (mosaic_amd/csrc/ring_neighbours.h), compiled by g++ as a small shared library, so
// tests/test_st_distance_lines.py can check the definitions without a GPU and the GPU tests can
// compare the kernels with them bit for bit.
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <limits>
#include <thread>
#include <vector>

#include "geoms_build.h"
#include "ring_neighbours.h"
#include "st_distance.h"

using mosaic::GeomColumn;
namespace rn = mosaic::rn;

static rn::Col col_of(const void* handle) {
    const GeomColumn* c = (const GeomColumn*)handle;
    return rn::Col{c->store(), c->part_kind.data(), c->geom_facets.data(), c->row_status.data(), c->size()};
}

extern "C" {

// flags: 1 decodes line rows (MOSAIC_GEOMS_LINES)
void* sdl_col_wkb(int64_t n, const int64_t* offsets, const uint8_t* wkb, const uint8_t* valid, uint32_t flags) {
    GeomColumn* c = new GeomColumn();
    c->lines = (flags & 1u) != 0;
    for (int64_t i = 0; i < n; i++) {
        if (valid && !valid[i])
            c->add_empty(mosaic::kRowNull);
        else
            c->add_wkb(wkb + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    }
    return c;
}

// null: inconsistent offsets
void* sdl_col_lines(int64_t n, const int64_t* geom_lines, const int64_t* line_offsets, const double* xy) {
    GeomColumn* c = new GeomColumn();
    c->lines = true;
    if (!c->add_lines(n, geom_lines, line_offsets, xy)) {
        delete c;
        return nullptr;
    }
    return c;
}

void* sdl_col_arrays(int64_t n, const int64_t* geom_parts, const int64_t* part_rings, const int64_t* ring_offsets,
                     const double* xy) {
    GeomColumn* c = new GeomColumn();
    if (!c->add_arrays(n, geom_parts, part_rings, ring_offsets, xy)) {
        delete c;
        return nullptr;
    }
    return c;
}

void* sdl_col_points(const double* x, const double* y, int64_t n) {
    GeomColumn* c = new GeomColumn();
    for (int64_t i = 0; i < n; i++) c->add_point(x[i], y[i]);
    return c;
}

// out4: rows, vertices, row-path rows, parts
void sdl_col_info(const void* col, int64_t* out4) {
    const GeomColumn* c = (const GeomColumn*)col;
    out4[0] = c->size();
    out4[1] = (int64_t)c->b.verts.size();
    out4[2] = c->n_row_path;
    out4[3] = (int64_t)c->part_kind.size();
}

void sdl_col_status(const void* col, int32_t* status, uint32_t* facets) {
    const GeomColumn* c = (const GeomColumn*)col;
    std::copy(c->row_status.begin(), c->row_status.end(), status);
    std::copy(c->geom_facets.begin(), c->geom_facets.end(), facets);
}

void sdl_col_part_kinds(const void* col, uint8_t* kinds) {
    const GeomColumn* c = (const GeomColumn*)col;
    std::copy(c->part_kind.begin(), c->part_kind.end(), kinds);
}

void sdl_col_free(void* col) { delete (GeomColumn*)col; }

// mosaic_st_distance's contract on the host, with the kind-aware definition: 0, or 1 (nothing
// written) when a row index is out of range.  left_row == right_row == null: row i with row i.
int sdl_distance(const void* left, const void* right, const int64_t* left_row, const int64_t* right_row, int64_t n,
                 double* out, int32_t* status, int n_threads) {
    const GeomColumn* L = (const GeomColumn*)left;
    const GeomColumn* R = (const GeomColumn*)right;
    for (int64_t i = 0; i < n; i++) {
        const int64_t g = left_row ? left_row[i] : i, h = right_row ? right_row[i] : i;
        if (g < 0 || g >= L->size() || h < 0 || h >= R->size()) return 1;
    }
    const mosaic::pip::GeomStore sl = L->store(), sr = R->store();
    const uint8_t *kl = L->part_kind.data(), *kr = R->part_kind.data();
    std::atomic<int64_t> next{0};
    const int64_t chunk = n >= (1 << 18) ? 256 : 1;  // pairs taken at a time
    auto work = [&]() {
        for (;;) {
            const int64_t i0 = next.fetch_add(chunk);
            if (i0 >= n) return;
            for (int64_t i = i0; i < std::min(n, i0 + chunk); i++) {
                const int64_t g = left_row ? left_row[i] : i, h = right_row ? right_row[i] : i;
                const int32_t a = L->row_status[(size_t)g], b = R->row_status[(size_t)h];
                int32_t st = mosaic::kRowOk;
                if (a == mosaic::kRowNull || b == mosaic::kRowNull)
                    st = mosaic::kRowNull;
                else if (a != mosaic::kRowOk || b != mosaic::kRowOk)
                    st = mosaic::kRowPath;
                if (status) status[i] = st;
                out[i] = st == mosaic::kRowOk ? mosaic::dist::distance(sl, kl, (uint32_t)g, sr, kr, (uint32_t)h)
                                              : std::numeric_limits<double>::quiet_NaN();
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return 0;
}

// rn::neighbours over the chips (index_id, key) of the candidates; null: a negative key, a landmark
// row outside `left`, or a chip naming a row outside `right`
void* sdl_neighbours(const int64_t* index_id, const int32_t* key, int64_t n_chips, const void* left, const void* right,
                     const int64_t* left_row, const int64_t* cell, int64_t n, int keep_self) {
    rn::CellIndex ix;
    if (!rn::build_index(index_id, key, n_chips, &ix)) return nullptr;
    rn::Neighbours* out = new rn::Neighbours();
    if (rn::neighbours(ix.view(), col_of(left), col_of(right), left_row, cell, n, keep_self != 0, out)) {
        delete out;
        return nullptr;
    }
    return out;
}

// out2: pairs, landmark rows
void sdl_result_info(const void* result, int64_t* out2) {
    const rn::Neighbours* r = (const rn::Neighbours*)result;
    out2[0] = (int64_t)r->left_row.size();
    out2[1] = (int64_t)r->unmatched.size();
}

void sdl_result_export(const void* result, int64_t* left_row, int64_t* right_row, double* distance, uint8_t* unmatched) {
    const rn::Neighbours* r = (const rn::Neighbours*)result;
    std::copy(r->left_row.begin(), r->left_row.end(), left_row);
    std::copy(r->right_row.begin(), r->right_row.end(), right_row);
    std::copy(r->distance.begin(), r->distance.end(), distance);
    std::copy(r->unmatched.begin(), r->unmatched.end(), unmatched);
}

void sdl_result_free(void* result) { delete (rn::Neighbours*)result; }

int sdl_same_geometry(const void* a, int64_t g, const void* b, int64_t h) {
    return rn::same_geometry(col_of(a), (uint32_t)g, col_of(b), (uint32_t)h) ? 1 : 0;
}

}  // extern "C"
