// GridRingNeighbours on the GPU (mosaic_cell_index_*, mosaic_ring_neighbours): one iteration of the
// reference's KNN model (models/knn/GridRingNeighbours.scala:121-160) over device-resident geometry
// columns.  ring_neighbours.h holds the semantics and the sequential driver whose rows this returns.
//
// The candidate cell index (built once per chip set, immutable afterwards):
//   two stable hipcub radix sorts order the chips by (cell, candidate row); k_ci_flags marks the first
//   chip of every distinct (cell, row) and of every cell, both counts packed into one uint64 so that
//   one device scan gives an entry's and a cell's position; k_ci_fill writes cells[], start[], rows[].
//
// Per call:
//   k_rn_count   one lane per (landmark, cell) row: range check, binary search of the cell in the
//                index, the number of candidates it holds; a miss sets unmatched[landmark]
//                (atomicOr, a vector atomic)
//   device scan  of the counts: every later size comes from it, nothing has a fixed capacity
//   k_rn_emit    one lane per hit (not per row: a cell may hold many candidates): the row is found by
//                binary search in the scanned offsets, the key landmark << 32 | candidate is written
//   radix sort + hipcub unique: one row per (landmark, candidate)
//   k_rn_self    one lane per surviving pair: rn::self_match (both rows MOSAIC_ROW_OK, then facet
//                counts and boxes, vertices only when they agree); hipcub flagged select keeps the
//                others in order
//   mosaic_st_distance on the device-resident pair list (the k_dist_* kernels of st_distance.hip)
//   order        a stable sort by the distance's bits, then a stable sort by the landmark, of pairs
//                that the unique step left ordered by (landmark, candidate):
//                (landmark, distance bits, candidate)
//
// The reference's st_intersects_aggregate filter is a no-op in this join (ring_neighbours.h) and is
// not built.
//
// The distance-within join (mosaic_within_candidates, mosaic_within_neighbours) finds its pairs without
// a cell index and then runs the same tail (finish_pairs):
//   k_wn_count   the envelope filter of every requested landmark against every candidate row, dense:
//                256 landmarks per workgroup in registers, the candidates' boxes through LDS, one
//                count per (row, candidate slice)
//   device scan  of the counts
//   k_wn_emit    the same walk again, writing the keys at the scanned places: distinct and ascending
//   k_rn_self, mosaic_st_distance as above, then k_wn_keep + two flagged selects keep the pairs whose
//   distance bits are within their row's radius, then the order as above
#include <memory>

#include "dev_rt.h"
#include "geoms_device.h"
#include "ring_neighbours.h"

using namespace mosaic;

struct mosaic_cell_index {
    int device = 0;
    int64_t n_cells = 0, n_entries = 0, max_per_cell = 0, max_row = -1;
    int64_t* cells = nullptr;
    int64_t* start = nullptr;
    int32_t* rows = nullptr;
    ~mosaic_cell_index() {
        for (void* p : {(void*)cells, (void*)start, (void*)rows})
            if (p) (void)hipFree(p);
    }
};

struct mosaic_neighbours {
    int device = 0;
    int64_t n_pairs = 0, n_left = 0;
    int64_t* left_row = nullptr;
    int64_t* right_row = nullptr;
    double* distance = nullptr;
    uint8_t* unmatched = nullptr;
    ~mosaic_neighbours() {
        for (void* p : {(void*)left_row, (void*)right_row, (void*)distance, (void*)unmatched})
            if (p) (void)hipFree(p);
    }
};

namespace {

constexpr int kBlock = 256;

using dev::blocks_for;
using dev::Buf;

int bits_for(int64_t n) {  // bits that hold every value below n
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < n) b++;
    return b;
}

rn::Col view(const mosaic_geoms* g) {
    return rn::Col{pip::GeomStore{g->verts, g->ring_start, g->ring_bbox, g->part_ring, g->geom_part, g->geom_bbox},
                   g->part_kind, g->geom_facets, g->row_status, g->n_geoms};
}

constexpr uint64_t kLow32 = 0xffffffffull;

// ---- the cell index ----
// counts[0]: negative keys; counts[1]: the largest key + 1
__global__ void __launch_bounds__(kBlock) k_ci_check(const int32_t* key, int64_t n, uint32_t* key_u, unsigned long long* counts) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        int64_t m = 0;
        bool bad = false;
        if (i < n) {
            const int32_t k = key[i];
            bad = k < 0;
            m = bad ? 0 : (int64_t)k + 1;
            key_u[i] = (uint32_t)k;
        }
        for (int off = 32; off; off >>= 1) {
            const int64_t o = __shfl_xor((long long)m, off, 64);
            m = o > m ? o : m;
        }
        const unsigned long long nb = __ballot(bad);
        if ((int)__lane_id() == 0) {
            if (nb) atomicAdd(&counts[0], (unsigned long long)__popcll(nb));
            atomicMax(&counts[1], (unsigned long long)m);
        }
    }
}

// chips sorted by (cell, row): low half 1 at the first chip of a distinct (cell, row), high half 1 at a cell's first
__global__ void __launch_bounds__(kBlock) k_ci_flags(const int64_t* cell, const uint32_t* row, int64_t n, uint64_t* flags) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool head = i == 0 || cell[i] != cell[i - 1];
        const bool distinct = head || row[i] != row[i - 1];
        flags[i] = (uint64_t)distinct | (uint64_t)head << 32;
    }
}

// scan: the inclusive sum of the flags.  cells / start hold n_cells slots, rows n_entries: the sums' last values.
__global__ void __launch_bounds__(kBlock) k_ci_fill(const int64_t* cell, const uint32_t* row, const uint64_t* scan, int64_t n,
                                                    int64_t* cells, int64_t* start, int32_t* rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t inc = scan[i], prev = i ? scan[i - 1] : 0;
        const int64_t entry = (int64_t)(inc & kLow32) - 1, slot = (int64_t)(inc >> 32) - 1;
        if ((inc & kLow32) != (prev & kLow32)) rows[entry] = (int32_t)row[i];
        if ((inc >> 32) != (prev >> 32)) {
            cells[slot] = cell[i];
            start[slot] = entry;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_ci_max(const int64_t* start, int64_t n_cells, unsigned long long* out) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n_cells; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        int64_t m = i < n_cells ? start[i + 1] - start[i] : 0;
        for (int off = 32; off; off >>= 1) {
            const int64_t o = __shfl_xor((long long)m, off, 64);
            m = o > m ? o : m;
        }
        if ((int)__lane_id() == 0) atomicMax(out, (unsigned long long)m);
    }
}

// ---- the probe ----
struct CountArgs {
    rn::CellIndexView ix;
    const int64_t *left_row, *cell;
    int64_t n, n_left;
    int32_t* slot;            // the cell's slot in the index, -1: a miss
    uint64_t* cnt;            // candidates of the row's cell
    uint32_t* unmatched;      // per landmark
    unsigned long long* bad;  // landmark rows out of range
};

__global__ void __launch_bounds__(kBlock) k_rn_count(CountArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = a.left_row[i];
        int64_t j = -1;
        uint64_t c = 0;
        if (l < 0 || l >= a.n_left) {
            atomicAdd(a.bad, 1ull);
        } else {
            j = rn::find_cell(a.ix, a.cell[i]);
            if (j < 0)
                atomicOr(&a.unmatched[l], 1u);
            else
                c = (uint64_t)(a.ix.start[j + 1] - a.ix.start[j]);
        }
        a.slot[i] = (int32_t)j;
        a.cnt[i] = c;
    }
}

// off[0 .. n]: the exclusive sum of cnt, off[n] = total
__global__ void __launch_bounds__(kBlock) k_rn_emit(rn::CellIndexView ix, const int64_t* left_row, const int32_t* slot,
                                                    const uint64_t* off, int64_t n, int64_t total, uint64_t* keys) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        // the last row i with off[i] <= t (rows without candidates share their successor's offset)
        int64_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= (uint64_t)t)
                lo = mid;
            else
                hi = mid;
        }
        const int64_t e = ix.start[slot[lo]] + (t - (int64_t)off[lo]);
        keys[t] = rn::pack_pair(left_row[lo], ix.rows[e]);
    }
}

__global__ void __launch_bounds__(kBlock) k_rn_self(rn::Col L, rn::Col C, const uint64_t* keys, int64_t n, uint8_t* keep) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        keep[i] = rn::self_match(L, (uint32_t)(k >> 32), C, (uint32_t)k) ? 0 : 1;
    }
}

__global__ void __launch_bounds__(kBlock) k_rn_unpack(const uint64_t* keys, int64_t n, int64_t* left_row, int64_t* right_row) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        left_row[i] = (int64_t)(k >> 32);
        right_row[i] = (int64_t)(k & kLow32);
    }
}

__global__ void __launch_bounds__(kBlock) k_rn_narrow(const uint32_t* in, int64_t n, uint8_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = in[i] ? 1 : 0;
}

// ---- the distance-within join: the envelope filter ----
// A workgroup takes kBlock requested rows, one per lane: the landmark's box and radius stay in
// registers.  blockIdx.y is a slice of the candidate rows, [y * slice_len, (y + 1) * slice_len): its
// boxes pass through LDS `tile` at a time, with the eligibility (status and facet count) decided as a
// box is staged, and every lane walks the tile at the same address (a broadcast read).  The decision
// is rn::box_within alone.  k_wn_count writes one count per (row, slice), row-major; their exclusive
// sum gives k_wn_emit, which repeats the walk, the place of every key: the keys come out distinct and
// ascending by (landmark, candidate) with no sort and no atomic.
struct WithinArgs {
    const pip::Box *lbox, *cbox;
    const int32_t *lstatus, *cstatus;
    const uint32_t *lfacets, *cfacets;
    const int64_t* left_row;  // null: row i asks for landmark i
    const double* radius;
    int64_t n, n_left, n_cand, slice_len;  // slice_len: a multiple of tile
    int tile, slices;
    uint64_t* cnt;            // [n * slices]
    const uint64_t* off;      // emit: [n * slices + 1], the exclusive sum of cnt and the total
    uint64_t* keys;           // emit
    unsigned long long* bad;  // count: rows outside the landmark column or not strictly ascending
};

template <bool kEmit>
__device__ __forceinline__ void wn_walk(const WithinArgs& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wn_lds[];
    pip::Box* s_box = (pip::Box*)wn_lds;
    uint8_t* s_ok = (uint8_t*)(s_box + a.tile);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t s = blockIdx.y;
    bool live = false;
    pip::Box lb{0, 0, 0, 0};
    double r = -1;
    int64_t l = -1;
    if (i < a.n) {
        l = a.left_row ? a.left_row[i] : i;
        const bool in = l >= 0 && l < a.n_left && (!a.left_row || i == 0 || a.left_row[i - 1] < l);
        if (!in) {
            if (!kEmit && s == 0) atomicAdd(a.bad, 1ull);
        } else {
            r = a.radius[i];
            live = a.lstatus[l] == 1 && a.lfacets[l] > 0 && rn::radius_ok(r);
            if (live) lb = a.lbox[l];
        }
    }
    const int64_t slot = i * a.slices + s;
    uint64_t pos = 0, end = 0;
    if (kEmit && i < a.n) {
        pos = a.off[slot];
        end = a.off[slot + 1];
    }
    const int64_t c0 = s * a.slice_len, c1 = c0 + a.slice_len < a.n_cand ? c0 + a.slice_len : a.n_cand;
    for (int64_t t0 = c0; t0 < c1; t0 += a.tile) {
        const int m = (int)(c1 - t0 < a.tile ? c1 - t0 : a.tile);
        __syncthreads();  // the last tile has been walked
        for (int j = threadIdx.x; j < m; j += kBlock) {
            const int64_t c = t0 + j;
            s_box[j] = a.cbox[c];
            s_ok[j] = a.cstatus[c] == 1 && a.cfacets[c] > 0;
        }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < m; j++) {
            if (!s_ok[j]) continue;  // uniform
            if (rn::box_within(lb, s_box[j], r)) {
                if (kEmit && pos < end) a.keys[pos] = rn::pack_pair(l, t0 + j);
                pos++;
            }
        }
    }
    if (!kEmit && i < a.n) a.cnt[slot] = pos;
}

__global__ void __launch_bounds__(kBlock) k_wn_count(WithinArgs a) { wn_walk<false>(a); }
__global__ void __launch_bounds__(kBlock) k_wn_emit(WithinArgs a) { wn_walk<true>(a); }

// the filter's count of a row: the sum over its slices
__global__ void __launch_bounds__(kBlock) k_wn_rowsum(const uint64_t* cnt, int64_t n, int slices, int64_t* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t t = 0;
        for (int s = 0; s < slices; s++) t += cnt[i * slices + s];
        out[i] = (int64_t)t;
    }
}

// keep[p] = the pair's distance is within the radius its landmark's row asked for (left_row ascending: a binary search)
__global__ void __launch_bounds__(kBlock) k_wn_keep(const uint64_t* keys, const double* distance, int64_t n_pairs, const int64_t* left_row,
                                                    const double* radius, int64_t n, uint8_t* keep) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = (int64_t)(keys[p] >> 32);
        int64_t i = l;
        if (left_row) {
            int64_t lo = 0, hi = n - 1;  // l is one of the rows
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (left_row[mid] < l)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            i = lo;
        }
        keep[p] = rn::within_radius(distance[p], radius[i]) ? 1 : 0;
    }
}

thread_local double g_last_ms[3] = {0, 0, 0};
thread_local double g_within_ms[3] = {0, 0, 0};

template <class T>
int select_flagged(Buf& tmp, const T* in, const uint8_t* flags, T* out, int64_t* d_num, int64_t n, hipStream_t st) {
    size_t bytes = 0;
    MOSAIC_HIP(hipcub::DeviceSelect::Flagged(nullptr, bytes, in, flags, out, d_num, (int)n, st));
    MOSAIC_RC(tmp.reserve(bytes));
    bytes = tmp.bytes;
    MOSAIC_HIP(hipcub::DeviceSelect::Flagged(tmp.p, bytes, in, flags, out, d_num, (int)n, st));
    return MOSAIC_OK;
}

// what the radius select of the distance-within join reads: the requested rows and their radii, on the device
struct RadiusSelect {
    const int64_t* left_row;  // nullable
    const double* radius;
    int64_t n;
};

// The tail both joins share.  k0 holds n_pairs distinct (landmark, candidate) keys, ascending; k1 has
// room for as many.  Self matches are dropped unless keep_self, mosaic_st_distance measures the pairs,
// `sel` (the distance-within join only) keeps the pairs within their row's radius, and two stable
// sorts order the rows by (landmark, distance bits, candidate) into nb's own arrays.  ev[1] .. ev[3]
// are recorded after the self filter, after the distances (and the select) and at the end.
int finish_pairs(mosaic_ctx* ctx, const dev::Exec& ex, const mosaic_geoms* left, const mosaic_geoms* right, Buf& k0, Buf& k1,
                 int64_t n_pairs, int keep_self, const RadiusSelect* sel, mosaic_neighbours* nb, dev::Events<4>& ev) {
    hipStream_t st = ex.stream;
    const int64_t wide = (int64_t)ex.n_cu * 16;
    const int64_t n_left = left->n_geoms;
    Buf d_num, d_keep, d_tmp, d_l, d_r, d_d0, d_d1, d_p1;
    MOSAIC_RC(d_num.reserve(8));
    uint64_t* pairs = k0.as<uint64_t>();
    uint64_t* other = k1.as<uint64_t>();
    if (!keep_self && n_pairs > 0) {
        MOSAIC_RC(d_keep.reserve((size_t)n_pairs));
        hipLaunchKernelGGL(k_rn_self, dim3(blocks_for(n_pairs, kBlock, wide)), dim3(kBlock), 0, st, view(left), view(right), pairs, n_pairs,
                           d_keep.as<uint8_t>());
        MOSAIC_HIP(hipGetLastError());
        MOSAIC_RC(select_flagged(d_tmp, pairs, d_keep.as<uint8_t>(), other, d_num.as<int64_t>(), n_pairs, st));
        MOSAIC_HIP(hipMemcpyAsync(&n_pairs, d_num.p, 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
        std::swap(pairs, other);
    }
    const uint64_t* dist_bits = nullptr;  // the kept pairs' distances
    if (!sel) {
        nb->n_pairs = n_pairs;
        const size_t pb = std::max<size_t>((size_t)n_pairs * 8, 16);
        MOSAIC_HIP(hipMalloc((void**)&nb->left_row, pb));
        MOSAIC_HIP(hipMalloc((void**)&nb->right_row, pb));
        MOSAIC_HIP(hipMalloc((void**)&nb->distance, pb));
        if (n_pairs > 0) {
            hipLaunchKernelGGL(k_rn_unpack, dim3(blocks_for(n_pairs, kBlock, wide)), dim3(kBlock), 0, st, pairs, n_pairs, nb->left_row,
                               nb->right_row);
            MOSAIC_HIP(hipGetLastError());
        }
        MOSAIC_HIP(hipEventRecord(ev.e[1], st));
        if (n_pairs > 0) MOSAIC_RC(mosaic_st_distance(ctx, left, right, nb->left_row, nb->right_row, n_pairs, nb->distance, nullptr));
        dist_bits = (const uint64_t*)nb->distance;
    } else {
        // the candidates may be many more than the pairs within: they are measured in scratch, and the
        // result's arrays get the size the select leaves
        if (n_pairs > 0) {
            MOSAIC_RC(d_l.reserve((size_t)n_pairs * 8));
            MOSAIC_RC(d_r.reserve((size_t)n_pairs * 8));
            MOSAIC_RC(d_d0.reserve((size_t)n_pairs * 8));
            hipLaunchKernelGGL(k_rn_unpack, dim3(blocks_for(n_pairs, kBlock, wide)), dim3(kBlock), 0, st, pairs, n_pairs, d_l.as<int64_t>(),
                               d_r.as<int64_t>());
            MOSAIC_HIP(hipGetLastError());
        }
        MOSAIC_HIP(hipEventRecord(ev.e[1], st));
        if (n_pairs > 0) {
            MOSAIC_RC(mosaic_st_distance(ctx, left, right, d_l.as<int64_t>(), d_r.as<int64_t>(), n_pairs, d_d0.as<double>(), nullptr));
            MOSAIC_RC(d_keep.reserve((size_t)n_pairs));
            hipLaunchKernelGGL(k_wn_keep, dim3(blocks_for(n_pairs, kBlock, wide)), dim3(kBlock), 0, st, pairs, d_d0.as<double>(), n_pairs,
                               sel->left_row, sel->radius, sel->n, d_keep.as<uint8_t>());
            MOSAIC_HIP(hipGetLastError());
            // d_l is free again: the kept distances go there
            MOSAIC_RC(select_flagged(d_tmp, pairs, d_keep.as<uint8_t>(), other, d_num.as<int64_t>(), n_pairs, st));
            MOSAIC_RC(select_flagged(d_tmp, d_d0.as<uint64_t>(), d_keep.as<uint8_t>(), d_l.as<uint64_t>(), d_num.as<int64_t>(), n_pairs, st));
            MOSAIC_HIP(hipMemcpyAsync(&n_pairs, d_num.p, 8, hipMemcpyDeviceToHost, st));
            MOSAIC_HIP(hipStreamSynchronize(st));
            std::swap(pairs, other);
            dist_bits = d_l.as<uint64_t>();
        }
        nb->n_pairs = n_pairs;
        const size_t pb = std::max<size_t>((size_t)n_pairs * 8, 16);
        MOSAIC_HIP(hipMalloc((void**)&nb->left_row, pb));
        MOSAIC_HIP(hipMalloc((void**)&nb->right_row, pb));
        MOSAIC_HIP(hipMalloc((void**)&nb->distance, pb));
    }
    MOSAIC_HIP(hipEventRecord(ev.e[2], st));
    if (n_pairs > 0) {
        // `pairs` is ordered by (landmark, candidate): stable by distance bits, then stable by landmark (the
        // second sort leaves the distances in the result's own array)
        MOSAIC_RC(d_d1.reserve((size_t)n_pairs * 8));
        MOSAIC_RC(d_p1.reserve((size_t)n_pairs * 8));
        MOSAIC_RC(dev::sort_pairs(d_tmp, dist_bits, d_d1.as<uint64_t>(), pairs, d_p1.as<uint64_t>(), (int)n_pairs, 0, 64, st));
        MOSAIC_RC(dev::sort_pairs(d_tmp, d_p1.as<uint64_t>(), other, d_d1.as<uint64_t>(), (uint64_t*)nb->distance, (int)n_pairs, 32, 32 + bits_for(n_left), st));
        hipLaunchKernelGGL(k_rn_unpack, dim3(blocks_for(n_pairs, kBlock, wide)), dim3(kBlock), 0, st, other, n_pairs, nb->left_row,
                           nb->right_row);
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_HIP(hipEventRecord(ev.e[3], st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    return MOSAIC_OK;
}

// The count pass of the distance-within join, shared by its two entries: the rows and radii on the
// device, the grid, and k_wn_count's counts in p.cnt.  MOSAIC_E_ARG when a row is outside the landmark
// column or the rows are not strictly ascending.
struct WithinPlan {
    Buf s_lrow, s_rad, cnt, bad;
    WithinArgs a;
    dim3 grid;
    size_t lds = 0;
};

int within_count(mosaic_ctx* ctx, const dev::Exec& ex, const char* who, const mosaic_geoms* left, const mosaic_geoms* right,
                 const int64_t* left_row, const double* radius, int64_t n, WithinPlan& p) {
    hipStream_t st = ex.stream;
    int tile = 256, slices_opt = 0;
    MOSAIC_RC(mosaic_ctx_within_options(ctx, &tile, &slices_opt));
    const int64_t n_cand = right->n_geoms;
    const int64_t blocks_x = (n + kBlock - 1) / kBlock;
    const int64_t n_tiles = std::max<int64_t>(1, (n_cand + tile - 1) / tile);
    // automatic: enough slices that four workgroups per CU have work, each at least one tile long
    int64_t slices = slices_opt > 0 ? slices_opt : ((int64_t)ex.n_cu * 4 + blocks_x - 1) / blocks_x;
    slices = std::max<int64_t>(1, std::min<int64_t>({slices, n_tiles, 65535, (rn::kMaxRows - 1) / std::max<int64_t>(n, 1)}));
    const int64_t slice_len = ((n_tiles + slices - 1) / slices) * tile;
    slices = std::max<int64_t>(1, (n_cand + slice_len - 1) / slice_len);
    p.a = WithinArgs{left->geom_bbox, right->geom_bbox, left->row_status, right->row_status, left->geom_facets, right->geom_facets,
                     nullptr, nullptr, n, left->n_geoms, n_cand, slice_len, tile, (int)slices, nullptr, nullptr, nullptr, nullptr};
    if (left_row) MOSAIC_RC(dev::on_device(left_row, n, p.s_lrow, st, &p.a.left_row));
    MOSAIC_RC(dev::on_device(radius, n, p.s_rad, st, &p.a.radius));
    MOSAIC_RC(p.cnt.reserve((size_t)(n * slices) * 8));
    MOSAIC_RC(p.bad.reserve(8));
    MOSAIC_HIP(hipMemsetAsync(p.bad.p, 0, 8, st));
    p.a.cnt = p.cnt.as<uint64_t>();
    p.a.bad = p.bad.as<unsigned long long>();
    p.grid = dim3((unsigned)blocks_x, (unsigned)slices);
    p.lds = ((size_t)tile * (sizeof(pip::Box) + 1) + 15) & ~(size_t)15;
    hipLaunchKernelGGL(k_wn_count, p.grid, dim3(kBlock), p.lds, st, p.a);
    MOSAIC_HIP(hipGetLastError());
    unsigned long long bad = 0;
    MOSAIC_HIP(hipMemcpyAsync(&bad, p.bad.p, 8, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    if (bad)
        return mosaic_tess_fail(MOSAIC_E_ARG, (std::string(who) + ": " + std::to_string(bad) +
                                               " row(s) outside the landmark column or not strictly ascending").c_str());
    return MOSAIC_OK;
}

// the checks both entries make before any device work
int within_args(const char* who, mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                const double* radius, int64_t n, bool has_out) {
    if (!ctx) return mosaic_tess_fail(MOSAIC_E_ARG, (std::string(who) + ": null context").c_str());
    if (!left || !right || !has_out || n < 0 || (n > 0 && !radius)) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    if (n >= rn::kMaxRows || left->n_geoms >= rn::kMaxRows || right->n_geoms >= rn::kMaxRows)
        return mosaic_tess_fail(MOSAIC_E_ARG, (std::string(who) + ": 2^31 - 1 rows at the most").c_str());
    if (!left_row && n > left->n_geoms)
        return mosaic_tess_fail(MOSAIC_E_ARG, (std::string(who) + ": more rows than the landmark column holds").c_str());
    return MOSAIC_OK;
}

}  // namespace

extern "C" {

uint64_t mosaic_layout_ring_neighbours(void) { return rn::layout_fingerprint(); }

int mosaic_cell_index_create(mosaic_ctx* ctx, int64_t n_chips, const int64_t* index_id, const int32_t* key,
                             mosaic_cell_index** out) {
    if (!ctx || !out || n_chips < 0 || (n_chips > 0 && (!index_id || !key))) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (n_chips >= rn::kMaxRows) return mosaic_tess_fail(MOSAIC_E_ARG, "cell index: 2^31 - 1 chips at the most");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    hipStream_t st = ex.stream;
    std::unique_ptr<mosaic_cell_index> ix(new mosaic_cell_index());
    ix->device = ex.device;
    const int64_t n = n_chips;
    if (n == 0) {
        MOSAIC_HIP(hipMalloc((void**)&ix->start, 16));
        MOSAIC_HIP(hipMemsetAsync(ix->start, 0, 16, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
        *out = ix.release();
        return MOSAIC_OK;
    }
    const int64_t wide = (int64_t)ex.n_cu * 16;
    Buf s_id, s_key, d_counts, d_row0, d_row1, d_cell0, d_cell1, d_flags, d_tmp;
    const int64_t* d_id = nullptr;
    const int32_t* d_key = nullptr;
    MOSAIC_RC(dev::on_device(index_id, n, s_id, st, &d_id));
    MOSAIC_RC(dev::on_device(key, n, s_key, st, &d_key));
    MOSAIC_RC(d_counts.reserve(2 * sizeof(unsigned long long)));
    MOSAIC_HIP(hipMemsetAsync(d_counts.p, 0, 2 * sizeof(unsigned long long), st));
    MOSAIC_RC(d_row0.reserve((size_t)n * 4));
    MOSAIC_RC(d_row1.reserve((size_t)n * 4));
    MOSAIC_RC(d_cell0.reserve((size_t)n * 8));
    MOSAIC_RC(d_cell1.reserve((size_t)n * 8));
    MOSAIC_RC(d_flags.reserve((size_t)n * 8));
    hipLaunchKernelGGL(k_ci_check, dim3(blocks_for(n, kBlock, wide)), dim3(kBlock), 0, st, d_key, n, d_row0.as<uint32_t>(),
                       d_counts.as<unsigned long long>());
    MOSAIC_HIP(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    MOSAIC_HIP(hipMemcpyAsync(counts, d_counts.p, sizeof(counts), hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    if (counts[0]) return mosaic_tess_fail(MOSAIC_E_ARG, ("cell index: " + std::to_string(counts[0]) + " chip(s) with a negative key").c_str());
    ix->max_row = (int64_t)counts[1] - 1;
    // by row, then (stable) by cell: (cell, row)
    MOSAIC_RC(dev::sort_pairs(d_tmp, d_row0.as<uint32_t>(), d_row1.as<uint32_t>(), d_id, d_cell0.as<int64_t>(), (int)n, 0, bits_for((int64_t)counts[1]), st));
    MOSAIC_RC(dev::sort_pairs(d_tmp, d_cell0.as<int64_t>(), d_cell1.as<int64_t>(), d_row1.as<uint32_t>(), d_row0.as<uint32_t>(), (int)n, 0, 64, st));
    const int64_t* cell = d_cell1.as<int64_t>();
    const uint32_t* row = d_row0.as<uint32_t>();
    hipLaunchKernelGGL(k_ci_flags, dim3(blocks_for(n, kBlock, wide)), dim3(kBlock), 0, st, cell, row, n, d_flags.as<uint64_t>());
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_RC(dev::inclusive_sum(d_tmp, d_flags.as<uint64_t>(), d_flags.as<uint64_t>(), (int)n, st));
    uint64_t last = 0;
    MOSAIC_HIP(hipMemcpyAsync(&last, d_flags.as<uint64_t>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    ix->n_entries = (int64_t)(last & kLow32);
    ix->n_cells = (int64_t)(last >> 32);
    MOSAIC_HIP(hipMalloc((void**)&ix->cells, (size_t)ix->n_cells * 8));
    MOSAIC_HIP(hipMalloc((void**)&ix->start, (size_t)(ix->n_cells + 1) * 8));
    MOSAIC_HIP(hipMalloc((void**)&ix->rows, (size_t)ix->n_entries * 4));
    hipLaunchKernelGGL(k_ci_fill, dim3(blocks_for(n, kBlock, wide)), dim3(kBlock), 0, st, cell, row, d_flags.as<uint64_t>(), n, ix->cells,
                       ix->start, ix->rows);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipMemcpyAsync(ix->start + ix->n_cells, &ix->n_entries, 8, hipMemcpyHostToDevice, st));
    MOSAIC_HIP(hipMemsetAsync(d_counts.p, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_ci_max, dim3(blocks_for(ix->n_cells, kBlock, wide)), dim3(kBlock), 0, st, ix->start, ix->n_cells,
                       d_counts.as<unsigned long long>());
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipMemcpyAsync(counts, d_counts.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    ix->max_per_cell = (int64_t)counts[0];
    *out = ix.release();
    return MOSAIC_OK;
}

int mosaic_cell_index_info(const mosaic_cell_index* index, int64_t* n_cells, int64_t* n_entries, int64_t* max_per_cell) {
    if (!index) return mosaic_tess_fail(MOSAIC_E_ARG, "null cell index");
    if (n_cells) *n_cells = index->n_cells;
    if (n_entries) *n_entries = index->n_entries;
    if (max_per_cell) *max_per_cell = index->max_per_cell;
    return MOSAIC_OK;
}

int mosaic_cell_index_destroy(mosaic_cell_index* index) {
    if (!index) return MOSAIC_OK;
    (void)hipSetDevice(index->device);
    delete index;
    return MOSAIC_OK;
}

int mosaic_ring_neighbours(mosaic_ctx* ctx, const mosaic_cell_index* index, const mosaic_geoms* left, const mosaic_geoms* right,
                           const int64_t* left_row, const int64_t* cell, int64_t n, int keep_self, mosaic_neighbours** out) {
    if (!ctx || !index || !left || !right || !out || n < 0 || (n > 0 && (!left_row || !cell)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (n >= rn::kMaxRows || left->n_geoms >= rn::kMaxRows || right->n_geoms >= rn::kMaxRows)
        return mosaic_tess_fail(MOSAIC_E_ARG, "ring_neighbours: 2^31 - 1 rows at the most");
    if (index->max_row >= right->n_geoms)
        return mosaic_tess_fail(MOSAIC_E_ARG, "ring_neighbours: the cell index names a row outside the candidate column");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    if (left->device != ex.device || right->device != ex.device || index->device != ex.device)
        return mosaic_tess_fail(MOSAIC_E_ARG, "ring_neighbours: a geometry column or cell index of another device");
    hipStream_t st = ex.stream;
    const int64_t wide = (int64_t)ex.n_cu * 16;
    const int64_t n_left = left->n_geoms;
    g_last_ms[0] = g_last_ms[1] = g_last_ms[2] = 0;

    std::unique_ptr<mosaic_neighbours> nb(new mosaic_neighbours());
    nb->device = ex.device;
    nb->n_left = n_left;
    dev::Events<4> ev;
    MOSAIC_RC(ev.create());
    MOSAIC_HIP(hipEventRecord(ev.e[0], st));

    Buf s_lrow, s_cell, d_un, d_slot, d_cnt, d_off, d_bad, d_tmp, d_k0, d_k1, d_num;
    MOSAIC_RC(d_un.reserve((size_t)n_left * 4));
    MOSAIC_HIP(hipMemsetAsync(d_un.p, 0, std::max<size_t>((size_t)n_left * 4, 16), st));
    MOSAIC_HIP(hipMalloc((void**)&nb->unmatched, std::max<size_t>((size_t)n_left, 16)));
    MOSAIC_RC(d_num.reserve(8));
    int64_t total = 0;
    const int64_t* d_lrow = nullptr;
    const int64_t* d_cell = nullptr;
    const rn::CellIndexView ix{index->cells, index->start, index->rows, index->n_cells};
    if (n > 0) {
        MOSAIC_RC(dev::on_device(left_row, n, s_lrow, st, &d_lrow));
        MOSAIC_RC(dev::on_device(cell, n, s_cell, st, &d_cell));
        MOSAIC_RC(d_slot.reserve((size_t)n * 4));
        MOSAIC_RC(d_cnt.reserve((size_t)n * 8));
        MOSAIC_RC(d_off.reserve((size_t)(n + 1) * 8));
        MOSAIC_RC(d_bad.reserve(8));
        MOSAIC_HIP(hipMemsetAsync(d_bad.p, 0, 8, st));
        MOSAIC_HIP(hipMemsetAsync(d_off.p, 0, 8, st));
        CountArgs ca{ix, d_lrow, d_cell, n, n_left, d_slot.as<int32_t>(), d_cnt.as<uint64_t>(), d_un.as<uint32_t>(),
                     d_bad.as<unsigned long long>()};
        hipLaunchKernelGGL(k_rn_count, dim3(blocks_for(n, kBlock, wide)), dim3(kBlock), 0, st, ca);
        MOSAIC_HIP(hipGetLastError());
        // off[0] = 0, off[i + 1] = cnt[0] + .. + cnt[i]: off[n] is the number of hits
        MOSAIC_RC(dev::inclusive_sum(d_tmp, d_cnt.as<uint64_t>(), d_off.as<uint64_t>() + 1, (int)n, st));
        unsigned long long bad = 0;
        uint64_t tot = 0;
        MOSAIC_HIP(hipMemcpyAsync(&bad, d_bad.p, 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipMemcpyAsync(&tot, d_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
        if (bad)
            return mosaic_tess_fail(MOSAIC_E_ARG, ("ring_neighbours: " + std::to_string(bad) + " row(s) name a landmark outside its column").c_str());
        if (tot >= (uint64_t)rn::kMaxRows)
            return mosaic_tess_fail(MOSAIC_E_CAPACITY, ("ring_neighbours: " + std::to_string(tot) +
                                                        " (landmark, candidate) hits in one call, 2^31 - 1 at the most: pass fewer rows").c_str());
        total = (int64_t)tot;
    }
    hipLaunchKernelGGL(k_rn_narrow, dim3(blocks_for(n_left, kBlock, wide)), dim3(kBlock), 0, st, d_un.as<uint32_t>(), n_left, nb->unmatched);
    MOSAIC_HIP(hipGetLastError());

    int64_t n_pairs = 0;  // (landmark, candidate) keys in d_k0, distinct and ascending
    if (total > 0) {
        MOSAIC_RC(d_k0.reserve((size_t)total * 8));
        MOSAIC_RC(d_k1.reserve((size_t)total * 8));
        hipLaunchKernelGGL(k_rn_emit, dim3(blocks_for(total, kBlock, wide)), dim3(kBlock), 0, st, ix, d_lrow, d_slot.as<int32_t>(),
                           d_off.as<uint64_t>(), n, total, d_k0.as<uint64_t>());
        MOSAIC_HIP(hipGetLastError());
        size_t bytes = 0;
        const int end_bit = 32 + bits_for(n_left);
        MOSAIC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, d_k0.as<uint64_t>(), d_k1.as<uint64_t>(), (int)total, 0, end_bit, st));
        Buf t1, t2;
        MOSAIC_RC(t1.reserve(bytes));
        MOSAIC_HIP(hipcub::DeviceRadixSort::SortKeys(t1.p, bytes, d_k0.as<uint64_t>(), d_k1.as<uint64_t>(), (int)total, 0, end_bit, st));
        bytes = 0;
        MOSAIC_HIP(hipcub::DeviceSelect::Unique(nullptr, bytes, d_k1.as<uint64_t>(), d_k0.as<uint64_t>(), d_num.as<int64_t>(), (int)total, st));
        MOSAIC_RC(t2.reserve(bytes));
        MOSAIC_HIP(hipcub::DeviceSelect::Unique(t2.p, bytes, d_k1.as<uint64_t>(), d_k0.as<uint64_t>(), d_num.as<int64_t>(), (int)total, st));
        MOSAIC_HIP(hipMemcpyAsync(&n_pairs, d_num.p, 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
    }
    MOSAIC_RC(finish_pairs(ctx, ex, left, right, d_k0, d_k1, n_pairs, keep_self, nullptr, nb.get(), ev));
    for (int i = 0; i < 3; i++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]);
        g_last_ms[i] = ms;
    }
    *out = nb.release();
    return MOSAIC_OK;
}

int mosaic_neighbours_info(const mosaic_neighbours* nb, int64_t* n_pairs, int64_t* n_left) {
    if (!nb) return mosaic_tess_fail(MOSAIC_E_ARG, "null neighbours");
    if (n_pairs) *n_pairs = nb->n_pairs;
    if (n_left) *n_left = nb->n_left;
    return MOSAIC_OK;
}

int mosaic_neighbours_export(const mosaic_neighbours* nb, int64_t* left_row, int64_t* right_row, double* distance, uint8_t* unmatched) {
    if (!nb) return mosaic_tess_fail(MOSAIC_E_ARG, "null neighbours");
    MOSAIC_HIP(hipSetDevice(nb->device));
    const size_t pb = (size_t)nb->n_pairs * 8;
    if (left_row && pb) MOSAIC_HIP(hipMemcpy(left_row, nb->left_row, pb, hipMemcpyDefault));
    if (right_row && pb) MOSAIC_HIP(hipMemcpy(right_row, nb->right_row, pb, hipMemcpyDefault));
    if (distance && pb) MOSAIC_HIP(hipMemcpy(distance, nb->distance, pb, hipMemcpyDefault));
    if (unmatched && nb->n_left) MOSAIC_HIP(hipMemcpy(unmatched, nb->unmatched, (size_t)nb->n_left, hipMemcpyDefault));
    return MOSAIC_OK;
}

int mosaic_neighbours_destroy(mosaic_neighbours* nb) {
    if (!nb) return MOSAIC_OK;
    (void)hipSetDevice(nb->device);
    delete nb;
    return MOSAIC_OK;
}

double mosaic_ring_neighbours_last_ms(double* split3) {
    if (split3)
        for (int i = 0; i < 3; i++) split3[i] = g_last_ms[i];
    return g_last_ms[0] + g_last_ms[1] + g_last_ms[2];
}

int mosaic_within_candidates(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                             const double* radius, int64_t n, int64_t* counts) {
    MOSAIC_RC(within_args("within_candidates", ctx, left, right, left_row, radius, n, counts || n == 0));
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    if (left->device != ex.device || right->device != ex.device)
        return mosaic_tess_fail(MOSAIC_E_ARG, "within_candidates: a geometry column of another device");
    if (n == 0) return MOSAIC_OK;
    hipStream_t st = ex.stream;
    WithinPlan p;
    MOSAIC_RC(within_count(ctx, ex, "within_candidates", left, right, left_row, radius, n, p));
    Buf d_out;
    MOSAIC_RC(d_out.reserve((size_t)n * 8));
    hipLaunchKernelGGL(k_wn_rowsum, dim3(blocks_for(n, kBlock, (int64_t)ex.n_cu * 16)), dim3(kBlock), 0, st, p.cnt.as<uint64_t>(), n,
                       p.a.slices, d_out.as<int64_t>());
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipMemcpyAsync(counts, d_out.p, (size_t)n * 8, hipMemcpyDefault, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    return MOSAIC_OK;
}

int mosaic_within_neighbours(mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
                             const double* radius, int64_t n, int keep_self, mosaic_neighbours** out) {
    MOSAIC_RC(within_args("within_neighbours", ctx, left, right, left_row, radius, n, out != nullptr));
    *out = nullptr;
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    if (left->device != ex.device || right->device != ex.device)
        return mosaic_tess_fail(MOSAIC_E_ARG, "within_neighbours: a geometry column of another device");
    hipStream_t st = ex.stream;
    const int64_t n_left = left->n_geoms;
    g_within_ms[0] = g_within_ms[1] = g_within_ms[2] = 0;

    std::unique_ptr<mosaic_neighbours> nb(new mosaic_neighbours());
    nb->device = ex.device;
    nb->n_left = n_left;
    dev::Events<4> ev;
    MOSAIC_RC(ev.create());
    MOSAIC_HIP(hipEventRecord(ev.e[0], st));
    MOSAIC_HIP(hipMalloc((void**)&nb->unmatched, std::max<size_t>((size_t)n_left, 16)));
    MOSAIC_HIP(hipMemsetAsync(nb->unmatched, 0, std::max<size_t>((size_t)n_left, 16), st));

    WithinPlan p;
    Buf d_off, d_tmp, d_k0, d_k1;
    int64_t total = 0;
    RadiusSelect sel{nullptr, nullptr, n};
    if (n > 0) {
        MOSAIC_RC(within_count(ctx, ex, "within_neighbours", left, right, left_row, radius, n, p));
        sel.left_row = p.a.left_row;
        sel.radius = p.a.radius;
        const int64_t slots = n * p.a.slices;
        // off[0] = 0, off[j + 1] = cnt[0] + .. + cnt[j]: off[slots] is the number of candidate pairs
        MOSAIC_RC(d_off.reserve((size_t)(slots + 1) * 8));
        MOSAIC_HIP(hipMemsetAsync(d_off.p, 0, 8, st));
        MOSAIC_RC(dev::inclusive_sum(d_tmp, p.cnt.as<uint64_t>(), d_off.as<uint64_t>() + 1, (int)slots, st));
        uint64_t tot = 0;
        MOSAIC_HIP(hipMemcpyAsync(&tot, d_off.as<uint64_t>() + slots, 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
        if (tot >= (uint64_t)rn::kMaxRows)
            return mosaic_tess_fail(MOSAIC_E_CAPACITY, ("within_neighbours: " + std::to_string(tot) +
                                                        " candidate pairs in one call, 2^31 - 1 at the most: pass fewer rows").c_str());
        total = (int64_t)tot;
    }
    if (total > 0) {
        MOSAIC_RC(d_k0.reserve((size_t)total * 8));
        MOSAIC_RC(d_k1.reserve((size_t)total * 8));
        p.a.off = d_off.as<uint64_t>();
        p.a.keys = d_k0.as<uint64_t>();
        hipLaunchKernelGGL(k_wn_emit, p.grid, dim3(kBlock), p.lds, st, p.a);
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_RC(finish_pairs(ctx, ex, left, right, d_k0, d_k1, total, keep_self, &sel, nb.get(), ev));
    for (int i = 0; i < 3; i++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]);
        g_within_ms[i] = ms;
    }
    *out = nb.release();
    return MOSAIC_OK;
}

double mosaic_within_neighbours_last_ms(double* split3) {
    if (split3)
        for (int i = 0; i < 3; i++) split3[i] = g_within_ms[i];
    return g_within_ms[0] + g_within_ms[1] + g_within_ms[2];
}

}  // extern "C"
