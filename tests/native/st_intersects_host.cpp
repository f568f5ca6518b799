// CPU build of st_intersects (mosaic_amd/csrc/st_intersects.h: the sequential driver
// isect::intersects over pip::segments_intersect and dist::component_in_part) as a small shared
// library, so tests/test_st_intersects.py can check the definition without a GPU,
// tests/test_gpu_st_intersects.py can compare the kernels with it, and tools/kbench_st_intersects.py
// has its 16-thread baseline.  The column builders are those of st_distance_lines_host.cpp (sdl_col_*),
// included here, so one library serves both predicates over the same columns.
#include "st_distance_lines_host.cpp"
#include "st_intersects.h"

extern "C" {

// mosaic_st_intersects's contract on the host: 0, or 1 (nothing written) when a row index is out of
// range.  left_row == right_row == null: row i with row i.  out is 0 where the status is not OK.
int si_intersects(const void* left, const void* right, const int64_t* left_row, const int64_t* right_row, int64_t n,
                  uint8_t* out, int32_t* status, int n_threads) {
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
                out[i] = st == mosaic::kRowOk && mosaic::isect::intersects(sl, kl, (uint32_t)g, sr, kr, (uint32_t)h) ? 1 : 0;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < std::min(n_threads, 16); t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return 0;
}

// pip::segments_intersect on one pair of facets: (p1, p2) and (q1, q2) as 8 doubles
int si_segments_intersect(const double* c8) {
    using mosaic::pip::Vec2;
    return mosaic::pip::segments_intersect(Vec2{c8[0], c8[1]}, Vec2{c8[2], c8[3]}, Vec2{c8[4], c8[5]}, Vec2{c8[6], c8[7]}) ? 1 : 0;
}

}  // extern "C"
