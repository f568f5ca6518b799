// grid_geometrykring / grid_geometrykloop on the GPU (mosaic_chips_kring, mosaic_geometry_kring):
// the k-ring / k-loop of a geometry's chips (core/Mosaic.scala:111-144, 211-223) as one
// multi-source search from the border cells of a whole batch of geometries, work proportional to
// the output.  geom_kring.h holds the semantics, the key / value packing and a sequential driver.
//
// Per batch of <= 4094 geometries, one open-addressing table (uint64 keys claimed with a 64-bit
// atomicCAS, a parallel value word per slot):
//   k_gk_seed        chips -> table; border cells get layer 0 and form the first frontier, core cells
//                    the core flag only; a chip that is no valid cell of res marks its geometry
//   k_gk_expand_h3   one lane per frontier cell: kRing(1) (h3fill::kring1), each ring cell claimed or
//                    first-reached exactly once (atomicMin on the layer), appended to the next
//                    frontier with one atomicAdd per wave
//   k_gk_expand_bng  one lane per (border cell, side of loop j): the loop's cells by the reference's
//                    arithmetic (bng::kloop_cell), atomicMin on the layer
//   k_gk_rehash      the table into a larger one, between rounds
//   k_gk_emit        the kept cells as (geometry | Scala set order key, cell | dist) records, then a
//                    hipcub radix sort of the pairs and k_gk_offsets for the rows' bounds
// The host sizes the table before every round for the round's worst case (H3: 7 cells per frontier
// cell; BNG: 8 j cells per border cell), so no insert can find it full; probe loops are bounded by
// the capacity all the same.  One host sync per round reads the frontier and entry counts.
#include <memory>

#include "cell_lists.h"
#include "dev_rt.h"
#include "geom_kring.h"

using namespace mosaic;

namespace {

struct Table {
    uint64_t* keys;
    uint32_t* vals;
    uint64_t mask;
};

struct Args {
    Table t;
    int bng;
    int res;
    unsigned long long* counts;  // [0] cells appended to the next frontier, [1] table entries
    unsigned int* flags;         // bit 1: table full, bit 2: frontier / record overflow
    int32_t* bad;                // per geometry: holds an invalid chip
};

// Open-addressing insert; probes bounded by the capacity (flag bit 1 on overflow, never spins).
__device__ inline uint64_t tab_insert(const Table& t, uint64_t key, bool* inserted, unsigned int* flags) {
    uint64_t h = gk::hmix(key) & t.mask;
    for (uint64_t n = 0; n <= t.mask; n++, h = (h + 1) & t.mask) {
        const unsigned long long prev =
            atomicCAS((unsigned long long*)&t.keys[h], (unsigned long long)gk::kEmpty, (unsigned long long)key);
        if (prev == gk::kEmpty || prev == key) {
            *inserted = prev == gk::kEmpty;
            return h;
        }
    }
    atomicOr(flags, 2u);
    *inserted = false;
    return gk::kEmpty;
}

// Positions in a list for the lanes of a wave with pred set: one atomicAdd per wave.  Called by
// every lane of the wave together (the callers' loops have wave-uniform trip counts).
__device__ inline unsigned long long wave_append(unsigned long long* counter, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m == 0) return 0;
    const int leader = __ffsll((long long)m) - 1;
    const int lane = (int)__lane_id();
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = (unsigned long long)__shfl((long long)base, leader, 64);
    return base + (unsigned long long)__popcll(m & (((unsigned long long)1 << lane) - 1));
}

__global__ void __launch_bounds__(256) k_gk_seed(Args a, const uint8_t* is_core, const int64_t* id, const int32_t* geom,
                                                 int64_t n, uint64_t* frontier) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool push = false, ins = false;
        uint64_t pk = gk::kEmpty;
        if (i < n) {
            if (!gk::chip_valid(a.bng != 0, a.res, id[i])) {
                atomicExch(&a.bad[geom[i]], 1);
            } else {
                pk = gk::pack(a.bng != 0, geom[i], id[i]);
                const uint64_t slot = tab_insert(a.t, pk, &ins, a.flags);
                if (slot != gk::kEmpty) {
                    if (is_core[i]) {
                        atomicAnd(&a.t.vals[slot], gk::kSeedCore);
                    } else {
                        const uint32_t old = atomicAnd(&a.t.vals[slot], gk::kSeedBorder);
                        push = gk::val_layer(old) != 0;  // the first border chip of this cell
                    }
                }
            }
        }
        const unsigned long long at = wave_append(&a.counts[0], push);
        if (push) frontier[at] = pk;  // (at most one entry per chip: the list holds n)
        (void)wave_append(&a.counts[1], ins);
    }
}

__global__ void __launch_bounds__(256) k_gk_expand_h3(Args a, const uint64_t* frontier, int64_t f, int round,
                                                      uint64_t* next, int64_t next_cap) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < f; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        int64_t ring[7];
        int n = 0, g = 0;
        if (i < f) {
            const uint64_t pk = frontier[i];
            g = gk::key_geom(false, pk);
            n = h3fill::kring1((uint64_t)gk::key_cell(false, a.res, pk), a.res, ring);
            if (n < 0) {
                atomicExch(&a.bad[g], 1);
                n = 0;
            }
        }
        for (int j = 0; j < 7; j++) {
            bool first = false, ins = false;
            uint64_t k2 = gk::kEmpty;
            if (j < n) {
                k2 = gk::pack(false, g, ring[j]);
                const uint64_t slot = tab_insert(a.t, k2, &ins, a.flags);
                if (slot != gk::kEmpty) {
                    // bit 0 of the word is final since the seeds; a stale layer only costs an atomic
                    const uint32_t cur = a.t.vals[slot];
                    if (gk::val_layer(cur) == gk::kUnreached) {
                        const uint32_t old = atomicMin(&a.t.vals[slot], gk::val_reach(cur, round));
                        first = gk::val_layer(old) == gk::kUnreached;
                    }
                }
            }
            const unsigned long long at = wave_append(&a.counts[0], first);
            if (first) {
                if ((int64_t)at < next_cap) next[at] = k2;
                else atomicOr(a.flags, 4u);
            }
            (void)wave_append(&a.counts[1], ins);
        }
    }
}

__global__ void __launch_bounds__(256) k_gk_expand_bng(Args a, const uint64_t* border, int64_t nb, int j) {
    const int64_t items = nb * 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t pk = border[i >> 2];
        const int side = (int)(i & 3), g = gk::key_geom(true, pk);
        int r;
        int32_t e, x, y;
        if (!bng::cell_origin(gk::key_cell(true, a.res, pk), &r, &e, &x, &y)) continue;
        unsigned long long n_ins = 0;
        for (int c = 0; c < 2 * gk::kMaxK; c++) {
            if (c >= 2 * j) break;
            int64_t cell;
            if (!bng::kloop_cell(r, e, x, y, j, side, c, &cell)) continue;
            bool ins;
            const uint64_t slot = tab_insert(a.t, gk::pack(true, g, cell), &ins, a.flags);
            if (slot == gk::kEmpty) continue;
            n_ins += ins;
            const uint32_t cur = a.t.vals[slot], cand = gk::val_reach(cur, j);
            if (cand < cur) atomicMin(&a.t.vals[slot], cand);
        }
        if (n_ins) atomicAdd(&a.counts[1], n_ins);
    }
}

__global__ void __launch_bounds__(256) k_gk_rehash(Table from, Table to, unsigned int* flags) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= from.mask; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = from.keys[s];
        if (key == gk::kEmpty) continue;
        bool ins;
        const uint64_t slot = tab_insert(to, key, &ins, flags);
        if (slot != gk::kEmpty) to.vals[slot] = from.vals[s];
    }
}

__global__ void __launch_bounds__(256) k_gk_emit(Args a, int k, int loop, uint64_t* sk, uint64_t* rec, int64_t cap) {
    const uint64_t slots = a.t.mask + 1;
    for (uint64_t s0 = (uint64_t)blockIdx.x * blockDim.x; s0 < slots; s0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = s0 + threadIdx.x;
        bool keep = false;
        uint64_t key = gk::kEmpty;
        uint32_t v = 0;
        if (s < slots) {
            key = a.t.keys[s];
            if (key != gk::kEmpty) {
                v = a.t.vals[s];
                keep = gk::val_keep(v, k, loop) && !a.bad[gk::key_geom(a.bng != 0, key)];
            }
        }
        const unsigned long long at = wave_append(&a.counts[0], keep);
        if (keep) {
            if ((int64_t)at < cap) {
                const int g = gk::key_geom(a.bng != 0, key);
                sk[at] = gk::sort_key(g, gk::key_cell(a.bng != 0, a.res, key));
                rec[at] = gk::pack_record(a.bng != 0, key, gk::val_dist(v, k));
            } else {
                atomicOr(a.flags, 4u);
            }
        }
    }
}

// off[g] = the first sorted record of geometry g or a later one (off[ng] = n)
__global__ void __launch_bounds__(256) k_gk_offsets(const uint64_t* sk, int64_t n, int ng, int64_t* off) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int g = gk::sort_key_geom(sk[i]);
        const int gp = i ? gk::sort_key_geom(sk[i - 1]) : -1;
        for (int q = gp + 1; q <= g && q <= ng; q++) off[q] = i;
        if (i == n - 1)
            for (int q = g + 1; q <= ng; q++) off[q] = n;
    }
}

// ---- host ----
using dev::blocks_for;
using dev::Buf;
using dev::upload;

struct DevTable {
    Buf keys, vals;
    uint64_t slots = 0;
    int alloc(uint64_t n, hipStream_t st) {
        MOSAIC_RC(keys.reserve(n * 8));
        MOSAIC_RC(vals.reserve(n * 4));
        MOSAIC_HIP(hipMemsetAsync(keys.p, 0xff, n * 8, st));
        MOSAIC_HIP(hipMemsetAsync(vals.p, 0xff, n * 4, st));
        slots = n;
        return MOSAIC_OK;
    }
    Table view() const { return Table{keys.as<uint64_t>(), vals.as<uint32_t>(), slots - 1}; }
};

struct Chips {  // one batch, geometry indices batch-local
    std::vector<uint8_t> is_core;
    std::vector<int64_t> id;
    std::vector<int32_t> geom;
};

struct Limits {
    uint64_t first_slots, max_slots;
};

// Room for `more` entries beyond `entries`: grows the table by rehashing into `spare`.
int make_room(std::unique_ptr<DevTable>& tab, uint64_t entries, uint64_t more, const Limits& lim, unsigned int* flags,
              hipStream_t st, int n_cu) {
    if (entries + more > lim.max_slots) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry k-ring: more cells than option gk_max_cells allows");
    const uint64_t need = gk::slots_for(entries + more, tab->slots);
    if (need == tab->slots) return MOSAIC_OK;
    if (need > lim.max_slots) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry k-ring: more cells than option gk_max_cells allows");
    std::unique_ptr<DevTable> grown(new DevTable());
    MOSAIC_RC(grown->alloc(need, st));
    if (entries > 0) {
        hipLaunchKernelGGL(k_gk_rehash, dim3(blocks_for((int64_t)tab->slots, 256, n_cu * 16)), dim3(256), 0, st, tab->view(),
                           grown->view(), flags);
        MOSAIC_HIP(hipGetLastError());
        MOSAIC_HIP(hipStreamSynchronize(st));  // the old table is freed below
    }
    tab.swap(grown);
    return MOSAIC_OK;
}

// One batch of ng geometries: appends their rows to lists.
int run_batch(hipStream_t st, int n_cu, bool bng, int res, const Chips& ch, int64_t ng, int k, int loop,
              const Limits& lim, mosaic_cell_lists* lists, double* device_ms) {
    const int64_t n = (int64_t)ch.id.size();
    auto empty_rows = [&]() {
        for (int64_t g = 0; g < ng; g++) {
            lists->offsets.push_back((int64_t)lists->cells.size());
            lists->status.push_back(MOSAIC_POLYFILL_OK);
        }
    };
    if (n == 0) {
        empty_rows();
        return MOSAIC_OK;
    }
    Buf d_core, d_id, d_geom, d_counts, d_flags, d_bad, d_f0, d_f1;
    MOSAIC_RC(upload(d_core, ch.is_core, st));
    MOSAIC_RC(upload(d_id, ch.id, st));
    MOSAIC_RC(upload(d_geom, ch.geom, st));
    MOSAIC_RC(d_counts.reserve(16));
    MOSAIC_RC(d_flags.reserve(4));
    MOSAIC_RC(d_bad.reserve((size_t)ng * 4));
    MOSAIC_RC(d_f0.reserve((size_t)n * 8));
    MOSAIC_HIP(hipMemsetAsync(d_counts.p, 0, 16, st));
    MOSAIC_HIP(hipMemsetAsync(d_flags.p, 0, 4, st));
    MOSAIC_HIP(hipMemsetAsync(d_bad.p, 0, (size_t)ng * 4, st));
    if ((uint64_t)n > lim.max_slots) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry k-ring: more cells than option gk_max_cells allows");
    std::unique_ptr<DevTable> tab(new DevTable());
    {
        const uint64_t slots = gk::slots_for((uint64_t)n, lim.first_slots);
        if (slots > lim.max_slots) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry k-ring: more cells than option gk_max_cells allows");
        MOSAIC_RC(tab->alloc(slots, st));
    }
    dev::Events<2> ev;
    MOSAIC_RC(ev.create());
    const hipEvent_t e0 = ev.e[0], e1 = ev.e[1];
    MOSAIC_HIP(hipEventRecord(e0, st));
    Args a{};
    a.t = tab->view();
    a.bng = bng ? 1 : 0;
    a.res = res;
    a.counts = d_counts.as<unsigned long long>();
    a.flags = d_flags.as<unsigned int>();
    a.bad = d_bad.as<int32_t>();
    hipLaunchKernelGGL(k_gk_seed, dim3(blocks_for(n, 256, n_cu * 16)), dim3(256), 0, st, a, d_core.as<uint8_t>(), d_id.as<int64_t>(),
                       d_geom.as<int32_t>(), n, d_f0.as<uint64_t>());
    MOSAIC_HIP(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    MOSAIC_HIP(hipMemcpyAsync(counts, d_counts.p, 16, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    int64_t f = (int64_t)counts[0];
    if (!bng) {
        Buf* cur = &d_f0;
        Buf* nxt = &d_f1;
        for (int round = 1; round <= k && f > 0; round++) {
            const uint64_t worst = 7 * (uint64_t)f;
            MOSAIC_RC(make_room(tab, counts[1], worst, lim, a.flags, st, n_cu));
            a.t = tab->view();
            MOSAIC_RC(nxt->reserve((size_t)worst * 8));
            MOSAIC_HIP(hipMemsetAsync(d_counts.p, 0, 8, st));
            hipLaunchKernelGGL(k_gk_expand_h3, dim3(blocks_for(f, 256, n_cu * 16)), dim3(256), 0, st, a, cur->as<uint64_t>(), f, round,
                               nxt->as<uint64_t>(), (int64_t)worst);
            MOSAIC_HIP(hipGetLastError());
            MOSAIC_HIP(hipMemcpyAsync(counts, d_counts.p, 16, hipMemcpyDeviceToHost, st));
            MOSAIC_HIP(hipStreamSynchronize(st));
            f = (int64_t)counts[0];
            std::swap(cur, nxt);
        }
    } else {
        for (int j = 1; j <= k && f > 0; j++) {
            MOSAIC_RC(make_room(tab, counts[1], 8 * (uint64_t)j * (uint64_t)f, lim, a.flags, st, n_cu));
            a.t = tab->view();
            hipLaunchKernelGGL(k_gk_expand_bng, dim3(blocks_for(4 * f, 256, n_cu * 16)), dim3(256), 0, st, a, d_f0.as<uint64_t>(), f, j);
            MOSAIC_HIP(hipGetLastError());
            MOSAIC_HIP(hipMemcpyAsync(counts, d_counts.p, 16, hipMemcpyDeviceToHost, st));
            MOSAIC_HIP(hipStreamSynchronize(st));
        }
    }
    // the kept cells, sorted by (geometry, order key)
    const int64_t entries = (int64_t)counts[1];
    Buf d_sk0, d_sk1, d_rec0, d_rec1, d_off, d_tmp;
    MOSAIC_RC(d_sk0.reserve((size_t)entries * 8));
    MOSAIC_RC(d_sk1.reserve((size_t)entries * 8));
    MOSAIC_RC(d_rec0.reserve((size_t)entries * 8));
    MOSAIC_RC(d_rec1.reserve((size_t)entries * 8));
    MOSAIC_RC(d_off.reserve((size_t)(ng + 1) * 8));
    MOSAIC_HIP(hipMemsetAsync(d_counts.p, 0, 8, st));
    MOSAIC_HIP(hipMemsetAsync(d_off.p, 0, (size_t)(ng + 1) * 8, st));
    hipLaunchKernelGGL(k_gk_emit, dim3(blocks_for((int64_t)tab->slots, 256, n_cu * 16)), dim3(256), 0, st, a, k, loop,
                       d_sk0.as<uint64_t>(), d_rec0.as<uint64_t>(), entries);
    MOSAIC_HIP(hipGetLastError());
    unsigned int flags = 0;
    MOSAIC_HIP(hipMemcpyAsync(counts, d_counts.p, 8, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipMemcpyAsync(&flags, d_flags.p, 4, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    if (flags & 2u) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry k-ring: device hash table overflow");
    if (flags & 4u) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry k-ring: frontier overflow");
    const int64_t m = (int64_t)counts[0];
    std::vector<uint64_t> sk((size_t)m), rec((size_t)m);
    std::vector<int64_t> off((size_t)ng + 1, 0);
    std::vector<int32_t> bad((size_t)ng, 0);
    if (m > 0) {
        if (m >= ((int64_t)1 << 31)) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "geometry k-ring: result too large for one call");
        MOSAIC_RC(dev::sort_pairs(d_tmp, d_sk0.as<uint64_t>(), d_sk1.as<uint64_t>(), d_rec0.as<uint64_t>(), d_rec1.as<uint64_t>(),
                                  (int)m, 0, gk::kSortKeyBits, st));
        hipLaunchKernelGGL(k_gk_offsets, dim3(blocks_for(m, 256, n_cu * 16)), dim3(256), 0, st, d_sk1.as<uint64_t>(), m, (int)ng,
                           d_off.as<int64_t>());
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_HIP(hipEventRecord(e1, st));
    if (m > 0) {
        MOSAIC_HIP(hipMemcpyAsync(sk.data(), d_sk1.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipMemcpyAsync(rec.data(), d_rec1.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipMemcpyAsync(off.data(), d_off.p, (size_t)(ng + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    MOSAIC_HIP(hipMemcpyAsync(bad.data(), d_bad.p, (size_t)ng * 4, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *device_ms += ms;
    // equal 32-bit hashes (equal sort keys): by ascending id
    for (int64_t i = 0; i < m;) {
        int64_t e = i + 1;
        while (e < m && sk[e] == sk[i]) e++;
        if (e - i > 1)
            std::sort(rec.begin() + i, rec.begin() + e, [&](uint64_t x, uint64_t y) {
                return gk::record_cell(bng, res, x) < gk::record_cell(bng, res, y);
            });
        i = e;
    }
    for (int64_t g = 0; g < ng; g++) {
        if (bad[g]) {
            lists->status.push_back(MOSAIC_POLYFILL_UNSUPPORTED);
        } else {
            for (int64_t i = off[g]; i < off[g + 1]; i++) {
                lists->cells.push_back(gk::record_cell(bng, res, rec[i]));
                lists->dist.push_back(gk::record_dist(rec[i]));
            }
            lists->status.push_back(MOSAIC_POLYFILL_OK);
        }
        lists->offsets.push_back((int64_t)lists->cells.size());
    }
    return MOSAIC_OK;
}

thread_local double g_last_ms = 0;

}  // namespace

extern "C" {

int mosaic_chips_kring(mosaic_ctx* ctx, int grid, int res, int64_t n_chips, const uint8_t* is_core,
                       const int64_t* index_id, const int32_t* key, int64_t n_geoms, int k, int loop,
                       mosaic_cell_lists** out) {
    if (!ctx || !out || n_chips < 0 || n_geoms < 0 || (n_chips > 0 && (!is_core || !index_id || !key)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (grid == MOSAIC_GRID_H3 ? (res < 0 || res > 15) : (grid == MOSAIC_GRID_BNG ? !bng::valid_resolution(res) : true))
        return mosaic_tess_fail(grid == MOSAIC_GRID_H3 || grid == MOSAIC_GRID_BNG ? MOSAIC_E_RES : MOSAIC_E_ARG,
                                "invalid grid or resolution");
    if (k > gk::kMaxK || k < (loop ? 1 : 0))
        return mosaic_tess_fail(MOSAIC_E_ARG, loop ? "geometry k-loop: k must be in [1, 1000]"
                                                   : "geometry k-ring: k must be in [0, 1000]");
    for (int64_t i = 0; i < n_chips; i++)
        if (key[i] < 0 || key[i] >= n_geoms)
            return mosaic_tess_fail(MOSAIC_E_ARG, ("geometry k-ring: chip " + std::to_string(i) + " has a key outside [0, n_geoms)").c_str());
    int log2 = 16;
    int64_t max_cells = (int64_t)1 << 27;
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    MOSAIC_RC(mosaic_ctx_gk_options(ctx, &log2, &max_cells));
    const Limits lim{(uint64_t)1 << log2, (uint64_t)max_cells};
    const bool bng = grid == MOSAIC_GRID_BNG;
    const int64_t n_batches = (n_geoms + gk::kGeomBatch - 1) / gk::kGeomBatch;
    std::vector<Chips> batches((size_t)n_batches);
    for (int64_t i = 0; i < n_chips; i++) {
        Chips& b = batches[(size_t)(key[i] / gk::kGeomBatch)];
        b.is_core.push_back(is_core[i] ? 1 : 0);
        b.id.push_back(index_id[i]);
        b.geom.push_back((int32_t)(key[i] % gk::kGeomBatch));
    }
    std::unique_ptr<mosaic_cell_lists> lists(new mosaic_cell_lists());
    double ms = 0;
    for (int64_t b = 0; b < n_batches; b++) {
        const int64_t ng = std::min<int64_t>(gk::kGeomBatch, n_geoms - b * gk::kGeomBatch);
        MOSAIC_RC(run_batch(ex.stream, ex.n_cu, bng, res, batches[(size_t)b], ng, k, loop, lim, lists.get(), &ms));
    }
    g_last_ms = ms;
    *out = lists.release();
    return MOSAIC_OK;
}

int mosaic_geometry_kring(mosaic_ctx* ctx, int grid, int res, int64_t n_geoms, const int64_t* geom_parts,
                          const int64_t* part_rings, const int64_t* ring_offsets, const double* xy, int k, int loop,
                          mosaic_cell_lists** out) {
    if (!ctx || !out) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (k > gk::kMaxK || k < (loop ? 1 : 0))
        return mosaic_tess_fail(MOSAIC_E_ARG, loop ? "geometry k-loop: k must be in [1, 1000]"
                                                   : "geometry k-ring: k must be in [0, 1000]");
    mosaic_chip_set* cs = nullptr;
    MOSAIC_RC(mosaic_tessellate_gpu(ctx, grid, res, n_geoms, geom_parts, part_rings, ring_offsets, xy, 0, 1, &cs));
    struct SetGuard {
        mosaic_chip_set* s;
        ~SetGuard() { (void)mosaic_chip_set_destroy(s); }
    } guard{cs};
    int64_t n_chips = 0, wkb_bytes = 0;
    MOSAIC_RC(mosaic_chip_set_info(cs, &n_chips, &wkb_bytes));
    const uint8_t *is_core = nullptr, *wkb = nullptr;
    const int64_t *index_id = nullptr, *wkb_off = nullptr;
    const int32_t* key = nullptr;
    MOSAIC_RC(mosaic_chip_set_columns(cs, &is_core, &index_id, &key, &wkb_off, &wkb));
    return mosaic_chips_kring(ctx, grid, res, n_chips, is_core, index_id, key, n_geoms, k, loop, out);
}

int mosaic_cell_lists_export_dist(const mosaic_cell_lists* l, int32_t* dist) {
    if (!l || !dist) return mosaic_tess_fail(MOSAIC_E_ARG, "null argument");
    if (l->dist.size() != l->cells.size()) return mosaic_tess_fail(MOSAIC_E_ARG, "these cell lists carry no dist (not a geometry k-ring result)");
    std::copy(l->dist.begin(), l->dist.end(), dist);
    return MOSAIC_OK;
}

double mosaic_geometry_kring_last_ms(void) { return g_last_ms; }

}  // extern "C"
