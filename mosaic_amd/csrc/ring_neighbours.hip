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

thread_local double g_last_ms[3] = {0, 0, 0};

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

    Buf s_lrow, s_cell, d_un, d_slot, d_cnt, d_off, d_bad, d_tmp, d_k0, d_k1, d_num, d_keep;
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

    int64_t n_pairs = 0;
    uint64_t* pairs = nullptr;  // (landmark, candidate) keys, distinct and ascending
    if (total > 0) {
        MOSAIC_RC(d_k0.reserve((size_t)total * 8));
        MOSAIC_RC(d_k1.reserve((size_t)total * 8));
        hipLaunchKernelGGL(k_rn_emit, dim3(blocks_for(total, kBlock, wide)), dim3(kBlock), 0, st, ix, d_lrow, d_slot.as<int32_t>(),
                           d_off.as<uint64_t>(), n, total, d_k0.as<uint64_t>());
        MOSAIC_HIP(hipGetLastError());
        size_t bytes = 0;
        const int end_bit = 32 + bits_for(n_left);
        MOSAIC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, d_k0.as<uint64_t>(), d_k1.as<uint64_t>(), (int)total, 0, end_bit, st));
        Buf t1, t2, t3;
        MOSAIC_RC(t1.reserve(bytes));
        MOSAIC_HIP(hipcub::DeviceRadixSort::SortKeys(t1.p, bytes, d_k0.as<uint64_t>(), d_k1.as<uint64_t>(), (int)total, 0, end_bit, st));
        bytes = 0;
        MOSAIC_HIP(hipcub::DeviceSelect::Unique(nullptr, bytes, d_k1.as<uint64_t>(), d_k0.as<uint64_t>(), d_num.as<int64_t>(), (int)total, st));
        MOSAIC_RC(t2.reserve(bytes));
        MOSAIC_HIP(hipcub::DeviceSelect::Unique(t2.p, bytes, d_k1.as<uint64_t>(), d_k0.as<uint64_t>(), d_num.as<int64_t>(), (int)total, st));
        MOSAIC_HIP(hipMemcpyAsync(&n_pairs, d_num.p, 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
        pairs = d_k0.as<uint64_t>();
        if (!keep_self && n_pairs > 0) {
            MOSAIC_RC(d_keep.reserve((size_t)n_pairs));
            hipLaunchKernelGGL(k_rn_self, dim3(blocks_for(n_pairs, kBlock, wide)), dim3(kBlock), 0, st, view(left), view(right), pairs, n_pairs,
                               d_keep.as<uint8_t>());
            MOSAIC_HIP(hipGetLastError());
            bytes = 0;
            MOSAIC_HIP(hipcub::DeviceSelect::Flagged(nullptr, bytes, pairs, d_keep.as<uint8_t>(), d_k1.as<uint64_t>(), d_num.as<int64_t>(),
                                                 (int)n_pairs, st));
            MOSAIC_RC(t3.reserve(bytes));
            MOSAIC_HIP(hipcub::DeviceSelect::Flagged(t3.p, bytes, pairs, d_keep.as<uint8_t>(), d_k1.as<uint64_t>(), d_num.as<int64_t>(),
                                                 (int)n_pairs, st));
            MOSAIC_HIP(hipMemcpyAsync(&n_pairs, d_num.p, 8, hipMemcpyDeviceToHost, st));
            MOSAIC_HIP(hipStreamSynchronize(st));
            pairs = d_k1.as<uint64_t>();
        }
    }
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
    MOSAIC_HIP(hipEventRecord(ev.e[2], st));
    if (n_pairs > 0) {
        // `pairs` is ordered by (landmark, candidate): stable by distance bits, then stable by landmark (the
        // second sort leaves the distances in the result's own array)
        Buf d_d1, d_p1;
        MOSAIC_RC(d_d1.reserve((size_t)n_pairs * 8));
        MOSAIC_RC(d_p1.reserve((size_t)n_pairs * 8));
        uint64_t* other = pairs == d_k0.as<uint64_t>() ? d_k1.as<uint64_t>() : d_k0.as<uint64_t>();
        MOSAIC_RC(dev::sort_pairs(d_tmp, (const uint64_t*)nb->distance, d_d1.as<uint64_t>(), pairs, d_p1.as<uint64_t>(), (int)n_pairs, 0, 64, st));
        MOSAIC_RC(dev::sort_pairs(d_tmp, d_p1.as<uint64_t>(), other, d_d1.as<uint64_t>(), (uint64_t*)nb->distance, (int)n_pairs, 32, 32 + bits_for(n_left), st));
        hipLaunchKernelGGL(k_rn_unpack, dim3(blocks_for(n_pairs, kBlock, wide)), dim3(kBlock), 0, st, other, n_pairs, nb->left_row,
                           nb->right_row);
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_HIP(hipEventRecord(ev.e[3], st));
    MOSAIC_HIP(hipStreamSynchronize(st));
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

}  // extern "C"
