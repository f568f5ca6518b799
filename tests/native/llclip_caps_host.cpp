// What k_tess_clip_ll's lane decides about a border candidate, computed on the host: llclip::clip
// (mosaic_amd/csrc/llclip.h, the routine both sides compile) over a geometry and a cell polygon with
// the device's workspace (tess_gpu.h: kLLChains chains, kLLOut result rings).  A candidate the lane
// cannot take (status != 0 here) is the host producer's to clip; tests count these to predict the
// host's share of a GPU tessellation.
//
//   llclip_caps <input file>  ->  one line per cell: status n_ch n_out n_vertices polys is_cell
//     status: 0 ok, 1 workspace overflow, 2 inconsistent walk, 3 bad cell (llclip::Status); n_ch /
//     n_out: chains and result rings used (status 0); n_vertices: the vertices the lane would write
//     (closed rings); status 3 also when the cell is no planar polygon (cell_ok)
//   input (native endian): int64 n_geoms, n_parts, n_rings, n_verts, n_cells, lonlat; int64
//     geom_parts[n_geoms + 1], part_rings[n_parts + 1], ring_offsets[n_rings + 1]; double
//     xy[2 n_verts]; int64 cell_geom[n_cells], cell_nc[n_cells]; double cell_xy[32 n_cells] (16
//     vertices of room per cell, counter-clockwise, open)
//   g++ -O2 -std=c++17 -ffp-contract=off -I mosaic_amd/csrc -o llclip_caps tests/native/llclip_caps_host.cpp
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "llclip.h"
#include "tess_gpu.h"

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
    std::vector<int64_t> h, gp, pr, ro, cgeom, cnc;
    std::vector<double> xy, cxy;
    if (!rd(f, h, 6)) return 2;
    for (int64_t v : h)
        if (v < 0) return 2;
    const int64_t n_geoms = h[0], n_parts = h[1], n_rings = h[2], n_verts = h[3], n_cells = h[4];
    const bool lonlat = h[5] != 0;
    if (!rd(f, gp, (size_t)n_geoms + 1) || !rd(f, pr, (size_t)n_parts + 1) || !rd(f, ro, (size_t)n_rings + 1) ||
        !rd(f, xy, (size_t)n_verts * 2) || !rd(f, cgeom, (size_t)n_cells) || !rd(f, cnc, (size_t)n_cells) ||
        !rd(f, cxy, (size_t)n_cells * 32))
        return 2;
    fclose(f);
    if (gp[(size_t)n_geoms] != n_parts || pr[(size_t)n_parts] != n_rings || ro[(size_t)n_rings] != n_verts) return 2;
    // the ring indexes, as both producers build them
    std::vector<int64_t> ring_blk((size_t)n_rings + 1);
    std::vector<uint8_t> ccw((size_t)n_rings + 1);
    int64_t t = 0;
    for (int64_t r = 0; r < n_rings; r++) ring_blk[(size_t)r] = t, t += llclip::ring_block_count(ro.data(), r);
    std::vector<double> blk((size_t)(t + 1) * 4);
    for (int64_t r = 0; r < n_rings; r++)
        llclip::ring_blocks_one(ro.data(), xy.data(), r, blk.data() + 4 * ring_blk[(size_t)r], ccw.data() + r);
    std::vector<llclip::Chain> ch(tessll::kLLChains);
    std::vector<llclip::Out> out(tessll::kLLOut);
    for (int64_t c = 0; c < n_cells; c++) {
        const int64_t g = cgeom[(size_t)c], nc = cnc[(size_t)c];
        if (g < 0 || g >= n_geoms) return 2;
        llclip::Cell C;
        bool ok = nc >= 3 && nc <= 16;
        if (ok) {
            C.nc = (int)nc;
            for (int v = 0; v < nc; v++) C.v[v] = llclip::Pt{cxy[32 * (size_t)c + 2 * v], cxy[32 * (size_t)c + 2 * v + 1]};
            llclip::cell_init(C);
            ok = llclip::cell_ok(C, lonlat);
        }
        if (!ok) {
            printf("%d 0 0 0 0 0\n", (int)llclip::kBadCell);
            continue;
        }
        const llclip::Geom gg{xy.data(), ro.data(), pr.data(), gp[(size_t)g], gp[(size_t)g + 1], blk.data(), ring_blk.data(), ccw.data()};
        llclip::Work w{ch.data(), tessll::kLLChains, out.data(), tessll::kLLOut, 0, 0};
        int32_t polys = 0;
        bool is_cell = false;
        const int st = llclip::clip(gg, C, w, 1e-12 * llclip::cell_area2(C), &polys, &is_cell);
        int64_t tot = 0;
        if (st == llclip::kOk)
            for (int32_t o = 0; o < w.n_out; o++) tot += w.out[o].npts + 1;
        printf("%d %d %d %lld %d %d\n", st, st ? 0 : w.n_ch, st ? 0 : w.n_out, (long long)tot, st ? 0 : polys, (int)is_cell);
    }
    return 0;
}
