// CPU build of st_distance (mosaic_amd/csrc/st_distance.h: the JTS distance arithmetic and the
// unpruned sequential driver; mosaic_amd/csrc/geoms_build.h: the column builder and its WKB decode,
// compiled by g++) as a small shared library, so tests/test_st_distance.py can check the definition
// without a GPU and tests/test_gpu_st_distance.py can compare the kernels with it bit for bit.
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <limits>
#include <thread>
#include <vector>

#include "geoms_build.h"
#include "st_distance.h"

using mosaic::GeomColumn;

extern "C" {

void* sd_col_wkb(int64_t n, const int64_t* offsets, const uint8_t* wkb, const uint8_t* valid) {
    GeomColumn* c = new GeomColumn();
    for (int64_t i = 0; i < n; i++) {
        if (valid && !valid[i])
            c->add_empty(mosaic::kRowNull);
        else
            c->add_wkb(wkb + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    }
    return c;
}

void* sd_col_arrays(int64_t n, const int64_t* geom_parts, const int64_t* part_rings, const int64_t* ring_offsets,
                    const double* xy) {
    GeomColumn* c = new GeomColumn();
    if (!c->add_arrays(n, geom_parts, part_rings, ring_offsets, xy)) {
        delete c;
        return nullptr;
    }
    return c;
}

void* sd_col_points(const double* x, const double* y, int64_t n) {
    GeomColumn* c = new GeomColumn();
    for (int64_t i = 0; i < n; i++) c->add_point(x[i], y[i]);
    return c;
}

// out4: rows, vertices, row-path rows, parts
void sd_col_info(const void* col, int64_t* out4) {
    const GeomColumn* c = (const GeomColumn*)col;
    out4[0] = c->size();
    out4[1] = (int64_t)c->b.verts.size();
    out4[2] = c->n_row_path;
    out4[3] = (int64_t)c->part_kind.size();
}

void sd_col_status(const void* col, int32_t* status, uint32_t* facets) {
    const GeomColumn* c = (const GeomColumn*)col;
    std::copy(c->row_status.begin(), c->row_status.end(), status);
    std::copy(c->geom_facets.begin(), c->geom_facets.end(), facets);
}

void sd_col_free(void* col) { delete (GeomColumn*)col; }

// The entry's contract on the host: 0, or 1 (nothing written) when a row index is out of range.
// left_row == right_row == null: row i with row i.
int sd_distance(const void* left, const void* right, const int64_t* left_row, const int64_t* right_row, int64_t n,
                double* out, int32_t* status, int n_threads) {
    const GeomColumn* L = (const GeomColumn*)left;
    const GeomColumn* R = (const GeomColumn*)right;
    for (int64_t i = 0; i < n; i++) {
        const int64_t g = left_row ? left_row[i] : i, h = right_row ? right_row[i] : i;
        if (g < 0 || g >= L->size() || h < 0 || h >= R->size()) return 1;
    }
    const mosaic::pip::GeomStore sl = L->store(), sr = R->store();
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
                out[i] = st == mosaic::kRowOk ? mosaic::dist::distance(sl, (uint32_t)g, sr, (uint32_t)h)
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

double sd_box_lower_bound(const double* a4, const double* b4) {
    return mosaic::dist::box_lower_bound(mosaic::pip::Box{a4[0], a4[1], a4[2], a4[3]},
                                         mosaic::pip::Box{b4[0], b4[1], b4[2], b4[3]});
}

}  // extern "C"
