// st_intersects_aggregate over the join of line chips (Mosaic.lineFill) with a polygon chip table
// (mosaic_line_chips_*, mosaic_line_intersects_aggregate): "which trips cross which zones", the
// equi-join of two grid_tessellateexplode outputs on index_id grouped by (line key, polygon key)
// (expressions/geometry/ST_IntersectsAggregate.scala:28-39, whose update decodes whatever WKB a chip
// holds; core/Mosaic.scala:21-35).  line_isect.h holds the semantics and the sequential driver whose
// answers these kernels return; line_chips_build.h the decoder.
//
// A line chip table is the flat layout of line_isect.h in HBM plus a cell id and a
// (key << 1) | is_core word per chip; it is immutable after creation.
//
// Per call:
//   k_lj_probe  one lane per line chip: linear probe of the polygon table's cell hash (as
//               k_isect_agg); run twice.  Pass 0 counts the chip pairs and those with no core side.
//               Pass 1 finds or inserts every pair's group in an atomicCAS hash of 2x the chip pairs
//               (a group exists even if it ends false), sets the flag of a pair with a core side, and
//               appends the others (line chip, polygon chip, group slot) to a list of exactly the
//               counted size, one atomicAdd per wave.  The lanes of a wave walk their cells' polygon
//               chips in step (the wave's longest list sets the trip count), so a cell holding
//               hundreds of polygon chips is a loop, not a capacity.
//   k_lj_test   one team of lanes per listed pair (the whole wave, or 16 lanes: mosaic_line_join_team).
//               A pair whose group is already true is skipped (the reference's `accumulator ||`).
//               Piece box against polygon box, then against ring box; the (line segment, ring
//               segment) pairs of a (piece, ring) go over the team's lanes with a team-uniform trip
//               count and a ballot ends the pair at the first hit; then the (piece, polygon part)
//               locations of step 4 go over the lanes the same way.
//   k_lj_groups packs the occupied slots of the group hash; the host copies them back and sorts them by
//               key pair.
#include <atomic>
#include <memory>
#include <utility>

#include "chips_view.h"
#include "dev_rt.h"
#include "line_chips_build.h"
#include "line_isect.h"

using namespace mosaic;

struct mosaic_line_chips {
    int grid = 0, res = 0, device = 0;
    int64_t n_chips = 0, n_pieces = 0, n_vertices = 0, device_bytes = 0;
    pip::Vec2* verts = nullptr;
    uint32_t* piece_start = nullptr;
    pip::Box* piece_bbox = nullptr;
    uint32_t* chip_piece = nullptr;
    pip::Box* chip_bbox = nullptr;
    int64_t* cell = nullptr;
    uint32_t* meta = nullptr;  // (key << 1) | is_core
    ~mosaic_line_chips() {
        for (void* p : {(void*)verts, (void*)piece_start, (void*)piece_bbox, (void*)chip_piece, (void*)chip_bbox,
                        (void*)cell, (void*)meta})
            if (p) (void)hipFree(p);
    }
};

namespace {

constexpr int kBlock = 256;
const unsigned long long kEmptyGroup = ~0ULL;

using dev::blocks_for;
using dev::Buf;

struct PairRec {
    uint32_t line, poly, group;
};

struct ProbeArgs {
    const int64_t* cell;  // the line chips
    const uint32_t* meta;
    int64_t n;
    const HashEntry* table;  // the polygon chips
    uint64_t mask;
    const uint32_t* pmeta;
    int pass;
    // [0] chip pairs, [1] pairs with no core side (pass 0); [2] list rows, [3] chips whose cell was found
    // (pass 1); [4] pairs tested (k_lj_test); [5] groups (k_lj_groups)
    unsigned long long* counts;
    unsigned long long* gkey;    // pass 1: group hash (kEmptyGroup = free)
    uint32_t* gflag;
    uint64_t gmask;
    PairRec* list;
    unsigned long long list_cap;
    int* overflow;
};

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
    return v;
}

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

__device__ inline uint64_t group_slot(const ProbeArgs& a, unsigned long long key) {
    uint64_t s = mix64(key) & a.gmask;
    for (uint64_t probes = 0; probes <= a.gmask; probes++) {
        const unsigned long long prev = atomicCAS(&a.gkey[s], kEmptyGroup, key);
        if (prev == kEmptyGroup || prev == key) return s;
        s = (s + 1) & a.gmask;
    }
    atomicExch(a.overflow, 1);
    return ~0ULL;
}

__global__ void __launch_bounds__(kBlock) k_lj_probe(ProbeArgs a) {
    // every lane of a wave stays in the loops below (an idle one has an empty range): the wave-wide
    // sums, the ballot of wave_append and the shared trip count need them all
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        uint32_t fb = 0, eb = 0, ml = 0;
        if (i < a.n) {
            const int64_t cell = a.cell[i];
            ml = a.meta[i];
            if (cell != kEmptyKey) {
                for (uint64_t s = mix64((uint64_t)cell) & a.mask, probes = 0; probes <= a.mask; s = (s + 1) & a.mask, probes++) {
                    const HashEntry f = a.table[s];
                    if (f.key == cell) {
                        fb = f.first;
                        eb = f.first + f.count;
                        break;
                    }
                    if (f.key == kEmptyKey) break;
                }
            }
        }
        if (a.pass == 0) {
            unsigned long long plain = 0;
            if (!(ml & 1u))
                for (uint32_t cb = fb; cb < eb; cb++) plain += (a.pmeta[cb] & 1u) ? 0 : 1;
            const unsigned long long all = wave_sum((unsigned long long)(eb - fb));
            plain = wave_sum(plain);
            if (__lane_id() == 0 && all) {
                atomicAdd(&a.counts[0], all);
                if (plain) atomicAdd(&a.counts[1], plain);
            }
            continue;
        }
        uint32_t trips = eb - fb;
        for (int off = 32; off; off >>= 1) trips = max(trips, (uint32_t)__shfl_xor((int)trips, off, 64));
        const unsigned long long probed = wave_sum(eb > fb ? 1ull : 0ull);
        if (__lane_id() == 0 && probed) atomicAdd(&a.counts[3], probed);
        for (uint32_t t = 0; t < trips; t++) {  // wave-uniform
            const uint32_t cb = fb + t;
            bool listed = false;
            uint64_t gs = 0;
            if (cb < eb) {
                const uint32_t mp = a.pmeta[cb];
                gs = group_slot(a, ((unsigned long long)(ml >> 1) << 32) | (unsigned long long)(mp >> 1));
                if (gs != ~0ULL) {
                    if ((ml | mp) & 1u)
                        atomicOr(&a.gflag[gs], 1u);
                    else
                        listed = true;
                }
            }
            const unsigned long long pos = wave_append(&a.counts[2], listed);
            if (listed) {
                if (pos < a.list_cap)
                    a.list[pos] = PairRec{(uint32_t)i, cb, (uint32_t)gs};
                else
                    atomicExch(a.overflow, 1);
            }
        }
    }
}

struct TestArgs {
    lineisect::LineStore L;
    pip::GeomStore P;
    const PairRec* list;
    unsigned long long n;
    uint32_t* gflag;
    unsigned long long* tested;
};

// the ballot of a team of T lanes (T = 64: the wave); every lane of the team is active at the call
template <int T>
__device__ inline unsigned long long team_ballot(bool pred, int lane) {
    const unsigned long long m = __ballot(pred);
    if (T == 64) return m;
    return (m >> (lane & ~(T - 1))) & ((1ull << (T & 63)) - 1);
}

// lineisect::intersects by the T lanes of a team (lane = lane in the wave)
template <int T>
__device__ bool team_intersects(const lineisect::LineStore& L, uint32_t c, const pip::GeomStore& P, uint32_t g, int lane) {
    if (!lineisect::may_meet(L, c, P, g)) return false;
    const uint32_t tl = (uint32_t)lane & (T - 1);
    const uint32_t m0 = L.chip_piece[c], m1 = L.chip_piece[c + 1];
    const uint32_t q0 = P.geom_part[g], q1 = P.geom_part[g + 1];
    const uint32_t r0 = P.part_ring[q0], r1 = P.part_ring[q1];
    const pip::Box gb = P.geom_bbox[g];
    for (uint32_t m = m0; m < m1; m++) {
        const uint32_t ia = L.piece_start[m], na = L.piece_start[m + 1] - ia;
        if (na < 2 || !pip::boxes_meet(L.piece_bbox[m], gb)) continue;
        const pip::Box mb = L.piece_bbox[m];
        for (uint32_t r = r0; r < r1; r++) {
            if (!pip::boxes_meet(mb, P.ring_bbox[r])) continue;
            const uint32_t ib = P.ring_start[r], nb = P.ring_start[r + 1] - ib;
            if (nb < 2) continue;
            const uint64_t total = (uint64_t)(na - 1) * (nb - 1);
            for (uint64_t base = 0; base < total; base += T) {  // team-uniform trip count
                const uint64_t k = base + tl;
                bool hit = false;
                if (k < total) {
                    const uint32_t i = (uint32_t)(k / (nb - 1)), j = (uint32_t)(k - (uint64_t)i * (nb - 1));
                    hit = pip::segments_intersect(L.verts[ia + i], L.verts[ia + i + 1], P.verts[ib + j], P.verts[ib + j + 1]);
                }
                if (team_ballot<T>(hit, lane)) return true;
            }
        }
    }
    const uint64_t tasks = (uint64_t)(m1 - m0) * (q1 - q0);
    for (uint64_t base = 0; base < tasks; base += T) {
        const uint64_t k = base + tl;
        bool hit = false;
        if (k < tasks) {
            const uint32_t m = m0 + (uint32_t)(k / (q1 - q0)), q = q0 + (uint32_t)(k % (q1 - q0));
            hit = lineisect::piece_start_in_part(L, m, P, q);
        }
        if (team_ballot<T>(hit, lane)) return true;
    }
    return false;
}

template <int T>
__global__ void __launch_bounds__(kBlock) k_lj_test(TestArgs a) {
    const int lane = (int)(threadIdx.x & 63);
    const bool lead = (lane & (T - 1)) == 0;
    const uint64_t n_teams = ((uint64_t)gridDim.x * blockDim.x) / T;
    unsigned long long tested = 0;
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / T; k < a.n; k += n_teams) {
        const PairRec p = a.list[k];
        // the team takes its leader's view of the flag: two lanes' own loads could differ and split it
        uint32_t done = lead ? __hip_atomic_load(&a.gflag[p.group], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        done = (uint32_t)__shfl((int)done, lane & ~(T - 1), 64);
        if (done) continue;
        if (lead) tested++;
        if (team_intersects<T>(a.L, p.line, a.P, p.poly, lane) && lead) atomicOr(&a.gflag[p.group], 1u);
    }
    tested = wave_sum(tested);
    if (lane == 0 && tested) atomicAdd(a.tested, tested);
}

// the occupied slots of the group hash, packed (any order: the host sorts them)
__global__ void __launch_bounds__(kBlock) k_lj_groups(const unsigned long long* gkey, const uint32_t* gflag, uint64_t gcap,
                                                      unsigned long long* out_key, uint8_t* out_flag, unsigned long long out_cap,
                                                      unsigned long long* count) {
    for (uint64_t s0 = (uint64_t)blockIdx.x * blockDim.x; s0 < gcap; s0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = s0 + threadIdx.x;
        const unsigned long long key = s < gcap ? gkey[s] : kEmptyGroup;
        const bool used = key != kEmptyGroup;
        const unsigned long long pos = wave_append(count, used);
        if (used && pos < out_cap) {
            out_key[pos] = key;
            out_flag[pos] = gflag[s] ? 1 : 0;
        }
    }
}

template <class T>
int upload(T** dst, const std::vector<T>& src, int64_t* bytes) {
    MOSAIC_HIP(hipMalloc((void**)dst, std::max<size_t>(src.size() * sizeof(T), 16)));
    if (!src.empty()) MOSAIC_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *bytes += (int64_t)(src.size() * sizeof(T));
    return MOSAIC_OK;
}

std::atomic<int> g_team{64};
thread_local int64_t t_last[4] = {0, 0, 0, 0};
thread_local double t_ms[2] = {0, 0};

}  // namespace

extern "C" {

int mosaic_line_chips_create(mosaic_ctx* ctx, int grid, int res, int64_t n_chips, const uint8_t* is_core, const int64_t* index_id,
                             const int32_t* key, const void* wkb_offsets, int offsets32, const uint8_t* wkb,
                             mosaic_line_chips** out) {
    if (!ctx || !out) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (grid != MOSAIC_GRID_H3 && grid != MOSAIC_GRID_BNG) return mosaic_tess_fail(MOSAIC_E_ARG, "unknown grid");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    LineChipBuilder b;
    std::string err;
    if (int rc = build_line_chips(n_chips, is_core, index_id, key, wkb_offsets, offsets32, wkb, b, err))
        return mosaic_tess_fail(rc, err.c_str());
    std::vector<uint32_t> meta((size_t)n_chips);
    for (int64_t i = 0; i < n_chips; i++) meta[(size_t)i] = ((uint32_t)b.key[(size_t)i] << 1) | b.is_core[(size_t)i];
    std::unique_ptr<mosaic_line_chips> t(new mosaic_line_chips());
    t->grid = grid;
    t->res = res;
    t->device = ex.device;
    t->n_chips = n_chips;
    t->n_pieces = (int64_t)b.piece_bbox.size();
    t->n_vertices = (int64_t)b.verts.size();
    MOSAIC_RC(upload(&t->verts, b.verts, &t->device_bytes));
    MOSAIC_RC(upload(&t->piece_start, b.piece_start, &t->device_bytes));
    MOSAIC_RC(upload(&t->piece_bbox, b.piece_bbox, &t->device_bytes));
    MOSAIC_RC(upload(&t->chip_piece, b.chip_piece, &t->device_bytes));
    MOSAIC_RC(upload(&t->chip_bbox, b.chip_bbox, &t->device_bytes));
    MOSAIC_RC(upload(&t->cell, b.cell, &t->device_bytes));
    MOSAIC_RC(upload(&t->meta, meta, &t->device_bytes));
    *out = t.release();
    return MOSAIC_OK;
}

int mosaic_line_chips_info(const mosaic_line_chips* t, int64_t* out4) {
    if (!t || !out4) return mosaic_tess_fail(MOSAIC_E_ARG, "null line chip table");
    out4[0] = t->n_chips;
    out4[1] = t->n_pieces;
    out4[2] = t->n_vertices;
    out4[3] = t->device_bytes;
    return MOSAIC_OK;
}

// what k_lx_probe / k_lx_clip read from a line chip table, for line_clip.hip
int mosaic_line_chips_view(const mosaic_line_chips* t, LineChipsView* out) {
    if (!t || !out) return mosaic_tess_fail(MOSAIC_E_ARG, "null line chip table");
    out->store = lineisect::LineStore{t->verts, t->piece_start, t->piece_bbox, t->chip_piece, t->chip_bbox};
    out->cell = t->cell;
    out->meta = t->meta;
    out->grid = t->grid;
    out->res = t->res;
    out->device = t->device;
    out->n_chips = t->n_chips;
    out->n_pieces = t->n_pieces;
    out->n_vertices = t->n_vertices;
    return MOSAIC_OK;
}

int mosaic_line_chips_destroy(mosaic_line_chips* t) {
    if (!t) return MOSAIC_OK;
    (void)hipSetDevice(t->device);
    delete t;
    return MOSAIC_OK;
}

int mosaic_line_join_team(int lanes) {
    const int prev = g_team.load();
    if (lanes == 16 || lanes == 64) g_team.store(lanes);
    return prev;
}

int mosaic_line_join_last(int64_t out[4], double ms[2]) {
    if (out) std::copy(t_last, t_last + 4, out);
    if (ms) std::copy(t_ms, t_ms + 2, ms);
    return MOSAIC_OK;
}

int mosaic_line_intersects_aggregate(mosaic_ctx* ctx, const mosaic_line_chips* lines, const mosaic_chips* polygons,
                                     int32_t* out_line_key, int32_t* out_polygon_key, uint8_t* out_flag, int64_t cap,
                                     int64_t* n_out) {
    if (!ctx || !lines || !polygons || !n_out || cap < 0 || (cap > 0 && (!out_line_key || !out_polygon_key || !out_flag)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *n_out = 0;
    ChipsJoinView pv;
    MOSAIC_RC(mosaic_chips_join_view(polygons, &pv));
    if (lines->grid != pv.grid || lines->res != pv.res)
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_intersects_aggregate: both chip tables must use the same grid and resolution");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    if (lines->device != ex.device || pv.device != ex.device)
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_intersects_aggregate: a chip table of another device");
    std::fill(t_last, t_last + 4, 0);
    t_ms[0] = t_ms[1] = 0;
    if (lines->n_chips == 0 || pv.n_chips == 0 || pv.capacity == 0) return MOSAIC_OK;
    hipStream_t stream = ex.stream;
    const int64_t n = lines->n_chips;
    const int64_t wide = (int64_t)ex.n_cu * 16;

    dev::Events<5> ev;
    MOSAIC_RC(ev.create());
    Buf s_counts, s_ovf, s_gkey, s_gflag, s_list, s_okey, s_oflag;
    MOSAIC_RC(s_counts.reserve(6 * sizeof(unsigned long long)));
    MOSAIC_RC(s_ovf.reserve(sizeof(int)));
    MOSAIC_HIP(hipMemsetAsync(s_counts.p, 0, 6 * sizeof(unsigned long long), stream));
    MOSAIC_HIP(hipMemsetAsync(s_ovf.p, 0, sizeof(int), stream));
    ProbeArgs pa{};
    pa.cell = lines->cell;
    pa.meta = lines->meta;
    pa.n = n;
    pa.table = pv.table;
    pa.mask = pv.capacity - 1;
    pa.pmeta = pv.meta;
    pa.pass = 0;
    pa.counts = s_counts.as<unsigned long long>();
    pa.overflow = s_ovf.as<int>();
    const dim3 pgrid((unsigned)blocks_for(n, kBlock, wide));
    MOSAIC_HIP(hipEventRecord(ev.e[0], stream));
    hipLaunchKernelGGL(k_lj_probe, pgrid, dim3(kBlock), 0, stream, pa);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipEventRecord(ev.e[1], stream));
    unsigned long long counts[6] = {0, 0, 0, 0, 0, 0};
    MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    const unsigned long long pairs = counts[0], plain = counts[1];
    if (pairs == 0) return MOSAIC_OK;
    if (pairs >= (1ull << 31)) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "st_intersects_aggregate (lines): 2^31 chip pairs or more");
    uint64_t gcap = 1024;
    while (gcap < 2 * pairs) gcap <<= 1;
    MOSAIC_RC(s_gkey.reserve(gcap * 8));
    MOSAIC_RC(s_gflag.reserve(gcap * 4));
    MOSAIC_RC(s_list.reserve((size_t)plain * sizeof(PairRec)));
    MOSAIC_HIP(hipMemsetAsync(s_gkey.p, 0xff, gcap * 8, stream));
    MOSAIC_HIP(hipMemsetAsync(s_gflag.p, 0, gcap * 4, stream));
    pa.pass = 1;
    pa.gkey = s_gkey.as<unsigned long long>();
    pa.gflag = s_gflag.as<uint32_t>();
    pa.gmask = gcap - 1;
    pa.list = s_list.as<PairRec>();
    pa.list_cap = plain;
    MOSAIC_HIP(hipEventRecord(ev.e[2], stream));
    hipLaunchKernelGGL(k_lj_probe, pgrid, dim3(kBlock), 0, stream, pa);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipEventRecord(ev.e[3], stream));
    if (plain) {
        // the list length is the count of pass 0 (the same enumeration), so it is known before pass 1 ends
        TestArgs ta{lineisect::LineStore{lines->verts, lines->piece_start, lines->piece_bbox, lines->chip_piece, lines->chip_bbox},
                    pv.store, pa.list, plain, pa.gflag, pa.counts + 4};
        const int team = g_team.load();
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((int64_t)plain * team + kBlock - 1) / kBlock, wide));
        if (team == 16)
            hipLaunchKernelGGL(k_lj_test<16>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, ta);
        else
            hipLaunchKernelGGL(k_lj_test<64>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, ta);
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_HIP(hipEventRecord(ev.e[4], stream));
    // the groups are at most the chip pairs: the occupied slots are packed on the device and only they come back
    MOSAIC_RC(s_okey.reserve((size_t)pairs * 8));
    MOSAIC_RC(s_oflag.reserve((size_t)pairs));
    hipLaunchKernelGGL(k_lj_groups, dim3((unsigned)blocks_for((int64_t)gcap, kBlock, wide)), dim3(kBlock), 0, stream, pa.gkey, pa.gflag, gcap,
                       s_okey.as<unsigned long long>(), s_oflag.as<uint8_t>(), pairs, pa.counts + 5);
    MOSAIC_HIP(hipGetLastError());
    int hov = 0;
    MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, sizeof(counts), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipMemcpyAsync(&hov, s_ovf.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    if (hov || counts[2] != plain || counts[5] > pairs)
        return mosaic_tess_fail(MOSAIC_E_CAPACITY, "st_intersects_aggregate (lines): group table overflow");
    const size_t n_groups = (size_t)counts[5];
    std::vector<unsigned long long> hk(n_groups);
    std::vector<uint8_t> hf(n_groups);
    if (n_groups) {
        MOSAIC_HIP(hipMemcpyAsync(hk.data(), s_okey.p, n_groups * 8, hipMemcpyDeviceToHost, stream));
        MOSAIC_HIP(hipMemcpyAsync(hf.data(), s_oflag.p, n_groups, hipMemcpyDeviceToHost, stream));
        MOSAIC_HIP(hipStreamSynchronize(stream));
    }
    float m01 = 0, m23 = 0, m34 = 0;
    MOSAIC_HIP(hipEventElapsedTime(&m01, ev.e[0], ev.e[1]));
    MOSAIC_HIP(hipEventElapsedTime(&m23, ev.e[2], ev.e[3]));
    MOSAIC_HIP(hipEventElapsedTime(&m34, ev.e[3], ev.e[4]));
    std::vector<std::pair<unsigned long long, uint8_t>> groups(n_groups);
    for (size_t s = 0; s < n_groups; s++) groups[s] = {hk[s], hf[s]};
    std::sort(groups.begin(), groups.end());
    t_last[0] = (int64_t)counts[3];
    t_last[1] = (int64_t)pairs;
    t_last[2] = (int64_t)counts[4];
    t_last[3] = (int64_t)groups.size();
    t_ms[0] = (double)m01 + (double)m23;
    t_ms[1] = (double)m34;
    *n_out = (int64_t)groups.size();
    if ((int64_t)groups.size() > cap)
        return mosaic_tess_fail(MOSAIC_E_CAPACITY, ("st_intersects_aggregate (lines): " + std::to_string(groups.size()) + " groups").c_str());
    for (size_t i = 0; i < groups.size(); i++) {
        out_line_key[i] = (int32_t)(groups[i].first >> 32);
        out_polygon_key[i] = (int32_t)(groups[i].first & 0xffffffffULL);
        out_flag[i] = groups[i].second;
    }
    return MOSAIC_OK;
}

}  // extern "C"
