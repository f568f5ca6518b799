// Stand-alone driver of the host line-polygon st_intersection_aggregate
// (mosaic_amd/csrc/line_clip_host.cpp, line_clip.h, line_clip_host.h) for the sanitizer run of
// tests/test_line_intersection.py.  Two joins, every column in a heap block of exactly its size:
//   comb     one segment crossing a comb polygon kCutCap + 6 times (the cut list outgrows its first
//            allocation twice; every tooth is a run of length 1)
//   members  a MULTILINESTRING with an empty member against a square: two runs
// Prints one line per join: "<name> <status> <groups> <length> <wkb type> <runs> <wkb bytes>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "line_clip_host.cpp"

extern "C" int mosaic_tess_fail(int code, const char* msg) {
    if (code) fprintf(stderr, "status %d: %s\n", code, msg);
    return code;
}

namespace {

struct Writer {
    std::vector<uint8_t> b;
    void u32(uint32_t v) {
        for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t)(v >> s));
    }
    void f64(double d) {
        uint64_t u;
        memcpy(&u, &d, 8);
        for (int s = 56; s >= 0; s -= 8) b.push_back((uint8_t)(u >> s));
    }
    void head(uint32_t type) {
        b.push_back(0);
        u32(type);
    }
    void line(const std::vector<double>& xy) {
        head(2);
        u32((uint32_t)(xy.size() / 2));
        for (double v : xy) f64(v);
    }
    void polygon(const std::vector<double>& xy) {
        head(3);
        u32(1);
        u32((uint32_t)(xy.size() / 2));
        for (double v : xy) f64(v);
    }
};

template <class T>
T* block(const std::vector<T>& v) {
    T* p = (T*)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

int run(const char* name, const std::vector<uint8_t>& line, const std::vector<uint8_t>& poly) {
    uint8_t* core = block(std::vector<uint8_t>{0});
    int64_t* cell = block(std::vector<int64_t>{77});
    int32_t* key = block(std::vector<int32_t>{3});
    int64_t* l_off = block(std::vector<int64_t>{0, (int64_t)line.size()});
    int64_t* p_off = block(std::vector<int64_t>{0, (int64_t)poly.size()});
    uint8_t* l_wkb = block(line);
    uint8_t* p_wkb = block(poly);
    mosaic_isect_geoms* g = nullptr;
    const int rc = mosaic_line_intersection_aggregate_host(MOSAIC_GRID_H3, 9, 1, core, cell, key, l_off, l_wkb, 1, core, cell, key, p_off,
                                                           p_wkb, &g);
    if (rc == MOSAIC_OK && g && g->lk.size() == 1) {
        uint32_t type = 0, n = 0;
        for (int i = 1; i < 5; i++) type = (type << 8) | g->wkb[(size_t)i];
        for (int i = 5; i < 9; i++) n = (n << 8) | g->wkb[(size_t)i];
        printf("%s %d %zu %.17g %u %u %zu\n", name, rc, g->lk.size(), g->area[0], type, type == 5 ? n : 1u, g->wkb.size());
    } else {
        printf("%s %d 0 0 0 0 0\n", name, rc);
    }
    delete g;
    for (void* p : {(void*)core, (void*)cell, (void*)key, (void*)l_off, (void*)p_off, (void*)l_wkb, (void*)p_wkb}) free(p);
    return rc;
}

}  // namespace

int main() {
    const int teeth = (mosaic::lineisect::kCutCap + 6) / 2;
    Writer comb, across, members, square;
    std::vector<double> ring = {0.0, -2.0, 2.0 * teeth, -2.0, 2.0 * teeth, 0.0};
    for (int k = teeth - 1; k >= 0; k--)
        for (double v : {2.0 * k + 1.5, 0.0, 2.0 * k + 1.5, 4.0, 2.0 * k + 0.5, 4.0, 2.0 * k + 0.5, 0.0}) ring.push_back(v);
    for (double v : {0.0, 0.0, 0.0, -2.0}) ring.push_back(v);
    comb.polygon(ring);
    across.line({-1.0, 1.0, 2.0 * teeth + 1.0, 1.0});
    members.head(5);
    members.u32(3);
    members.line({-2.0, 4.0, 10.0, 4.0});
    members.line({});
    members.line({1.0, 1.0, 4.0, 5.0});
    square.polygon({0.0, 0.0, 8.0, 0.0, 8.0, 8.0, 0.0, 8.0, 0.0, 0.0});
    int rc = run("comb", across.b, comb.b);
    rc |= run("members", members.b, square.b);
    return rc ? 1 : 0;
}
