// CPU build of the measures of one geometry per row (mosaic_amd/csrc/st_measures.h: the sequential
// definition meas::measure) as a small shared library, so tests/test_st_measures.py can check the
// definition without a GPU, tests/test_gpu_st_measures.py can compare the kernels with it bit for bit,
// and tools/kbench_st_measures.py has its 16-thread baseline.  The column builders are those of
// st_distance_lines_host.cpp (sdl_col_*), included here.
#include "st_distance_lines_host.cpp"
#include "st_measures.h"

extern "C" {

// mosaic_st_measures's contract on the host: 0, or 1 (nothing written) when a row index is out of
// range.  rows == null: row i.  Every output is nullable; out9 order: area, length, cx, cy, xmin,
// ymin, xmax, ymax as doubles, numpoints as int64.
int sm_measures(const void* col, const int64_t* rows, int64_t n, double* area, double* length, double* cx, double* cy,
                int64_t* numpoints, double* xmin, double* ymin, double* xmax, double* ymax, int32_t* status, int n_threads) {
    namespace meas = mosaic::meas;
    const GeomColumn* C = (const GeomColumn*)col;
    for (int64_t i = 0; i < n; i++) {
        const int64_t g = rows ? rows[i] : i;
        if (g < 0 || g >= C->size()) return 1;
    }
    const mosaic::pip::GeomStore s = C->store();
    const uint8_t* kinds = C->part_kind.data();
    const int what = (area ? meas::kArea : 0) | (length ? meas::kLength : 0) | (cx || cy ? meas::kCentroid : 0);
    std::atomic<int64_t> next{0};
    const int64_t chunk = n >= (1 << 12) ? 256 : 1;  // rows taken at a time
    auto work = [&]() {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (;;) {
            const int64_t i0 = next.fetch_add(chunk);
            if (i0 >= n) return;
            for (int64_t i = i0; i < std::min(n, i0 + chunk); i++) {
                const int64_t g = rows ? rows[i] : i;
                const int32_t st = C->row_status[(size_t)g];
                meas::Measures m = {nan, nan, nan, nan, 0, {nan, nan, nan, nan}};
                if (st == mosaic::kRowOk) m = meas::measure(s, kinds, (uint32_t)g, what);
                if (area) area[i] = m.area;
                if (length) length[i] = m.length;
                if (cx) cx[i] = m.cx;
                if (cy) cy[i] = m.cy;
                if (numpoints) numpoints[i] = m.numpoints;
                if (xmin) xmin[i] = m.box.minx;
                if (ymin) ymin[i] = m.box.miny;
                if (xmax) xmax[i] = m.box.maxx;
                if (ymax) ymax[i] = m.box.maxy;
                if (status) status[i] = st;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < std::min(n_threads, 16); t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return 0;
}

// Orientation.isCCW of one closed ring of n vertices (xy interleaved)
int sm_is_ccw(const double* xy, int64_t n) { return mosaic::meas::is_ccw((const mosaic::pip::Vec2*)xy, (uint32_t)n) ? 1 : 0; }

}  // extern "C"
