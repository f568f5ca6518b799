// CPU build of st_contains over geometry columns (mosaic_amd/csrc/st_contains.h: the sequential driver
// contains::contains) as a small shared library, so tests/test_st_contains.py can check the definition
// without a GPU, tests/test_gpu_st_contains.py can compare the kernels with it, and
// profiles/st_contains.py has its 16-thread baseline.  The column builders are those of
// st_distance_lines_host.cpp (sdl_col_*), included here; si_intersects comes along for the profile.
#include "st_intersects_host.cpp"
#include "st_contains.h"

extern "C" {

// mosaic_st_contains_geoms's contract on the host: 0, or 1 (nothing written) when a row index is out of
// range.  left_row == right_row == null: row i with row i.  out is 0 where the status is not OK.
// how (nullable): contains::kHow* of the pair, -1 where a row is null or a row-path row.
int sc_contains(const void* left, const void* right, const int64_t* left_row, const int64_t* right_row, int64_t n,
                uint8_t* out, int32_t* status, int32_t* how, int n_threads) {
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
                int hw = -1;
                uint8_t o = 0;
                if (st == mosaic::kRowOk) o = mosaic::contains::contains_how(sl, kl, (uint32_t)g, sr, kr, (uint32_t)h, &st, &hw);
                out[i] = o;
                if (status) status[i] = st;
                if (how) how[i] = hw;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < std::min(n_threads, 16); t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return 0;
}

// contains::facet_contact on one pair of facets: (p1, p2) and (q1, q2) as 8 doubles
int sc_facet_contact(const double* c8) {
    using mosaic::pip::Vec2;
    return mosaic::contains::facet_contact(Vec2{c8[0], c8[1]}, Vec2{c8[2], c8[3]}, Vec2{c8[4], c8[5]}, Vec2{c8[6], c8[7]});
}

}  // extern "C"
