// What k_line_clip's lane decides about one (line, cell) group, computed on the host: lineclip::build
// (mosaic_amd/csrc/lineclip.h, the routine both producers compile) over a line and a cell polygon with a
// workspace of `cap` items (the device's is lineclip::kItems; cap 0 = that).  A group the lane cannot
// take (status 1, "needs more") is the host routine's to build; tests count these to predict the host's
// share of a GPU line tessellation.
//
//   lineclip_caps <input file>  ->  one line per cell: status n_items has_piece
//     status: 0 ok, 1 needs more than cap items, 2 bad cell (lineclip::Status)
//   input (native endian): int64 n_verts, n_cells, cap; double xy[2 n_verts] (one line, no repeated
//     vertices); int64 cell_nc[n_cells]; double cell_xy[32 n_cells] (16 vertices of room per cell,
//     counter-clockwise, open)
//   g++ -O2 -std=c++17 -ffp-contract=off -I mosaic_amd/csrc -o lineclip_caps tests/native/lineclip_caps_host.cpp
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

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> h, cnc;
    std::vector<double> xy, cxy;
    if (!rd(f, h, 3)) return 2;
    for (int64_t v : h)
        if (v < 0) return 2;
    const int64_t n_verts = h[0], n_cells = h[1];
    const int32_t cap = h[2] ? (int32_t)h[2] : lineclip::kItems;
    if (!rd(f, xy, (size_t)n_verts * 2) || !rd(f, cnc, (size_t)n_cells) || !rd(f, cxy, (size_t)n_cells * 32)) return 2;
    fclose(f);
    if (n_verts < 2) return 2;
    std::vector<lineclip::Item> items((size_t)cap);
    std::vector<uint32_t> segs;
    for (int64_t c = 0; c < n_cells; c++) {
        const int64_t nc = cnc[(size_t)c];
        llclip::Cell C;
        bool ok = nc >= 3 && nc <= 16;
        if (ok) {
            C.nc = (int)nc;
            for (int v = 0; v < nc; v++) C.v[v] = llclip::Pt{cxy[32 * (size_t)c + 2 * v], cxy[32 * (size_t)c + 2 * v + 1]};
            llclip::cell_init(C);
            ok = llclip::cell_ok(C, false);
        }
        if (!ok) {
            printf("%d 0 0\n", (int)lineclip::kBadCell);
            continue;
        }
        segs.clear();
        for (int64_t s = 0; s + 1 < n_verts; s++)
            if (lineclip::segment_meets(lineclip::vtx(xy.data(), s), lineclip::vtx(xy.data(), s + 1), C)) segs.push_back((uint32_t)s);
        lineclip::Work w{items.data(), cap, 0, 0, 0, -1, 0.0};
        const int st = lineclip::build(xy.data(), C, segs.data(), (int64_t)segs.size(), w);
        printf("%d %d %d\n", st, st ? 0 : w.n, st ? 0 : w.has_piece);
    }
    return 0;
}
