// CPU build of the distance-within join (mosaic_amd/csrc/ring_neighbours.h: the sequential driver
// rn::within over all pairs and the envelope filter's count rn::within_candidates) as a small shared
// library, so tests/test_within.py can check the definition without a GPU and
// tests/test_gpu_within.py can compare the kernels with it row for row.  The geometry columns are the
// GeomColumn handles of tests/native/st_distance_host.cpp and st_distance_lines_host.cpp (the same
// header, the same compiler).
#include <stdint.h>

#include <algorithm>

#include "geoms_build.h"
#include "ring_neighbours.h"

using mosaic::GeomColumn;
namespace rn = mosaic::rn;

static rn::Col col_of(const void* handle) {
    const GeomColumn* c = (const GeomColumn*)handle;
    return rn::Col{c->store(), c->part_kind.data(), c->geom_facets.data(), c->row_status.data(), c->size()};
}

extern "C" {

// null: the rows are not strictly ascending rows of `left` (left_row null: n rows of it)
void* wn_within(const void* left, const void* right, const int64_t* left_row, const double* radius, int64_t n, int keep_self) {
    rn::Neighbours* out = new rn::Neighbours();
    if (rn::within(col_of(left), col_of(right), left_row, radius, n, keep_self != 0, out)) {
        delete out;
        return nullptr;
    }
    return out;
}

// 1 with nothing written on a row error
int wn_candidates(const void* left, const void* right, const int64_t* left_row, const double* radius, int64_t n, int64_t* counts) {
    return rn::within_candidates(col_of(left), col_of(right), left_row, radius, n, counts);
}

// out2: pairs, landmark rows
void wn_result_info(const void* result, int64_t* out2) {
    const rn::Neighbours* r = (const rn::Neighbours*)result;
    out2[0] = (int64_t)r->left_row.size();
    out2[1] = (int64_t)r->unmatched.size();
}

void wn_result_export(const void* result, int64_t* left_row, int64_t* right_row, double* distance, uint8_t* unmatched) {
    const rn::Neighbours* r = (const rn::Neighbours*)result;
    std::copy(r->left_row.begin(), r->left_row.end(), left_row);
    std::copy(r->right_row.begin(), r->right_row.end(), right_row);
    std::copy(r->distance.begin(), r->distance.end(), distance);
    std::copy(r->unmatched.begin(), r->unmatched.end(), unmatched);
}

void wn_result_free(void* result) { delete (rn::Neighbours*)result; }

// the envelope of every row of a column: out[4 g .. 4 g + 3] = minx, miny, maxx, maxy
void wn_boxes(const void* col, double* out) {
    const rn::Col c = col_of(col);
    for (int64_t g = 0; g < c.n; g++) {
        const mosaic::pip::Box b = c.s.geom_bbox[g];
        out[4 * g] = b.minx;
        out[4 * g + 1] = b.miny;
        out[4 * g + 2] = b.maxx;
        out[4 * g + 3] = b.maxy;
    }
}

}  // extern "C"
