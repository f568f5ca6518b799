// What k_line_spans and k_line_walk's lanes decide about a segment, computed on the host: lineclip::span_count
// and, per span, lineclip::walk_span (mosaic_amd/csrc/lineclip.h, the routines both producers compile) with
// the polygons of lineclip::cell_poly (as the lanes build them; remembered per cell here, neighbouring
// spans come to the same cells).  A span whose walk tries
// more than lineclip::kWalkCap cells (status 1, "needs more") is the host routine's to walk; a span that
// emits more than lineclip::kSlot cells walks twice on the device.  Tests count these to know that their
// inputs reach both paths, and to predict the host's share of a GPU line tessellation.
//
//   linewalk_caps <input file>  ->
//     caps <kWalkCap> <kSlot> <kItems>
//     per segment:  segment <index> <K>      K spans; -1: span_count failed (a bad cell), no span lines
//     per span:     <status> <cells> <bad>
//       status: lineclip::walk_span at cap kWalkCap: 0 ok, 1 needs more, 2 bad cell (lineclip::Status)
//       cells:  the cells the span emits when the cap is large enough for the walk to finish (0 when bad)
//       bad:    1 when that finished walk met a bad cell
//   input (native endian): int64 grid (0 H3, 1 BNG), res, n_segments; double ab[4 n_segments] (ax ay bx by)
//   g++ -O2 -std=c++17 -ffp-contract=off -I mosaic_amd/csrc -o linewalk_caps tests/native/linewalk_caps_host.cpp
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lineclip.h"

using namespace mosaic;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// lineclip::cell_poly, remembered: the polygon depends on the cell alone
struct MemoPoly {
    struct Slot {
        int64_t id = 0;
        bool full = false, ok = false;
        lineclip::Cell C;
    };
    lineclip::Grid g;
    std::vector<Slot>* slots;
    bool operator()(int64_t id, lineclip::Cell& C) const {
        Slot& s = (*slots)[(size_t)(((uint64_t)id * 0x9e3779b97f4a7c15ULL) >> 52)];
        if (!s.full || s.id != id) {
            s.id = id;
            s.full = true;
            s.ok = lineclip::cell_poly(g, id, s.C);
        }
        C = s.C;
        return s.ok;
    }
};

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> h;
    std::vector<double> ab;
    if (!rd(f, h, 3)) return 2;
    if ((h[0] != 0 && h[0] != 1) || h[1] < -6 || h[1] > 15 || h[2] < 0 || h[2] > (1 << 20)) return 2;
    if (!rd(f, ab, (size_t)h[2] * 4)) return 2;
    fclose(f);
    const lineclip::Grid G{(int)h[0], (int)h[1]};
    std::vector<MemoPoly::Slot> slots(4096);
    const MemoPoly poly{G, &slots};
    printf("caps %d %d %d\n", lineclip::kWalkCap, lineclip::kSlot, lineclip::kItems);
    std::vector<int64_t> seen((size_t)lineclip::kWalkCap);
    for (int64_t s = 0; s < h[2]; s++) {
        const lineclip::Pt a{ab[4 * (size_t)s], ab[4 * (size_t)s + 1]}, b{ab[4 * (size_t)s + 2], ab[4 * (size_t)s + 3]};
        int32_t K = 0;
        if (lineclip::span_count(G, poly, a, b, &K) != lineclip::kOk) {
            printf("segment %lld -1\n", (long long)s);
            continue;
        }
        printf("segment %lld %d\n", (long long)s, K);
        for (int32_t j = 0; j < K; j++) {
            int64_t n = 0;
            const int lane = lineclip::walk_span(G, poly, a, b, j, K, seen.data(), lineclip::kWalkCap, [&](int64_t) { n++; });
            int full = lane;
            for (size_t cap = (size_t)lineclip::kWalkCap * 4; full == lineclip::kNeedsMore; cap *= 4) {
                if (seen.size() < cap) seen.resize(cap);
                n = 0;
                full = lineclip::walk_span(G, poly, a, b, j, K, seen.data(), (int32_t)cap, [&](int64_t) { n++; });
            }
            printf("%d %lld %d\n", lane, (long long)(full == lineclip::kOk ? n : 0), full == lineclip::kBadCell ? 1 : 0);
        }
    }
    return 0;
}
