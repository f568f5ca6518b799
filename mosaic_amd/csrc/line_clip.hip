// st_intersection_aggregate over the join of line chips (Mosaic.lineFill) with a polygon chip table
// (mosaic_line_intersection_aggregate, mosaic_line_intersection_aggregate_geometry): "how much of each
// trip lies in each zone", the equi-join of two grid_tessellateexplode outputs on index_id folded per
// (line key, polygon key) (expressions/geometry/ST_IntersectionAggregate.scala:40-72).  line_clip.h
// holds the semantics and the sequential driver whose answers these kernels return; line_clip_host.h
// the fold into groups, shared with the host restatement (line_clip_host.cpp).
//
// Per call:
//   k_lx_probe     one lane per line chip: linear probe of the polygon table's cell hash, as k_lj_probe
//                  (line_join.hip; that kernel and its counters are untouched), run twice.  Pass 0
//                  counts the chip pairs, those whose polygon chip is not core, and finds the first
//                  joined line chip with is_core set (refused).  Pass 1 writes every pair (cell, line
//                  chip, polygon chip, keys) into a list of exactly the counted size: the pairs to clip
//                  from the front, the core-polygon pairs from the back, one atomicAdd per wave each.
//   k_lx_chip_len  one lane per line chip: its whole length (the increment of a core-polygon pair).
//   k_lx_clip      one wave per pair to clip.  Pieces and segments are taken in order, so the run state
//                  (line_clip.h RunState) is wave-uniform.  Per segment the lanes stride over the ring
//                  segments with llclip::meet and append the cuts to the wave's LDS list by ballot and
//                  popcount; the list is rank-sorted by the total order of line_clip.h and bit-equal
//                  neighbours dropped; the intervals go over the lanes for the midpoint test
//                  (locate_in_polygon); then every lane walks the kept flags in interval order, so the
//                  length is folded in that order and not in lane-arrival order.  A segment with more
//                  than kCutCap meet points puts the pair on an overflow list, and the host driver
//                  finishes it (the same code: no group is ever refused).  The first pass returns each
//                  pair's length and run count; the geometry call adds a second pass that writes the
//                  run records at the offsets the counts give.
// The host copies pairs, lengths and runs back and folds them (line_clip_host.h fold_groups): groups
// sorted by key pair, each summed in (cell id, line chip row, polygon chip row) order.
#include <memory>

#include "chips_view.h"
#include "dev_rt.h"
#include "line_clip.h"
#include "line_clip_host.h"

using namespace mosaic;
using lineisect::PairRec;
using lineisect::Pt;
using lineisect::Run;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSlots = lineisect::kCutCap + 2;
constexpr uint32_t kOverflowed = 0xffffffffu;

using dev::blocks_for;
using dev::Buf;

struct ProbeArgs {
    const int64_t* cell;  // the line chips
    const uint32_t* meta;
    int64_t n;
    const HashEntry* table;  // the polygon chips
    uint64_t mask;
    const uint32_t* pmeta;
    int pass;
    // [0] chip pairs, [1] pairs to clip (pass 0); [2] pairs to clip written, [3] core-polygon pairs written
    // (pass 1); [4] the first joined line chip with is_core set (pass 0; ~0: none); [5] pairs over the cut cap,
    // [6] a run record out of its range (k_lx_clip)
    unsigned long long* counts;
    PairRec* list;
    unsigned long long n_pairs, n_clip;
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

__global__ void __launch_bounds__(kBlock) k_lx_probe(ProbeArgs a) {
    // every lane of a wave stays in the loops below (an idle one has an empty range): the wave-wide
    // sums, the ballots of wave_append and the shared trip count need them all
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        uint32_t fb = 0, eb = 0, ml = 0;
        int64_t cell = kEmptyKey;
        if (i < a.n) {
            cell = a.cell[i];
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
            for (uint32_t cb = fb; cb < eb; cb++) plain += (a.pmeta[cb] & 1u) ? 0 : 1;
            if ((ml & 1u) && eb > fb) atomicMin(&a.counts[4], (unsigned long long)i);
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
        for (uint32_t t = 0; t < trips; t++) {  // wave-uniform
            const uint32_t cb = fb + t;
            const bool have = cb < eb;
            const uint32_t mp = have ? a.pmeta[cb] : 0u;
            const bool core = have && (mp & 1u), plain = have && !(mp & 1u);
            const unsigned long long pp = wave_append(&a.counts[2], plain);
            const unsigned long long pc = wave_append(&a.counts[3], core);
            const PairRec rec{cell, (uint32_t)i, cb, ml >> 1, mp};
            // the counts of pass 0 bound both ranges; a table changed between the passes would miss them
            if (plain && pp < a.n_clip) a.list[pp] = rec;
            if (core && pc < a.n_pairs - a.n_clip) a.list[a.n_pairs - 1 - pc] = rec;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_lx_chip_len(lineisect::LineStore L, int64_t n, double* out) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x)
        out[c] = lineisect::chip_length(L, (uint32_t)c);
}

struct ClipArgs {
    lineisect::LineStore L;
    pip::GeomStore P;
    const PairRec* list;
    unsigned long long n;  // the pairs to clip: list[0 .. n)
    int fill;              // 0: lengths and run counts; 1: run records
    double* len;
    uint32_t* n_runs;  // kOverflowed: a pair over the cut cap (the host finishes it)
    const unsigned long long* run_off;  // fill: pair k's records are runs[run_off[k] .. run_off[k + 1])
    Run* runs;
    unsigned long long* counts;  // ProbeArgs::counts
    uint32_t* over;              // the pairs over the cut cap (n slots)
};

// the lanes of a wave exchange data through LDS without a workgroup barrier: order the accesses
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(kBlock) k_lx_clip(ClipArgs a) {
    __shared__ Pt s_a[kWaves][kSlots];
    __shared__ Pt s_b[kWaves][kSlots];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    Pt* const A = s_a[wv];
    Pt* const B = s_b[wv];
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const lineisect::LineStore& L = a.L;
    const pip::GeomStore& P = a.P;
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < a.n; k += n_waves) {  // wave-uniform
        if (a.fill && a.n_runs[k] == kOverflowed) continue;
        const uint32_t c = a.list[k].line, g = a.list[k].poly;
        const unsigned long long rbase = a.fill ? a.run_off[k] : 0, rend = a.fill ? a.run_off[k + 1] : 0;
        auto emit = [&](const Run& r, uint32_t idx) {
            if (!a.fill || lane != 0) return;
            if (rbase + idx < rend)
                a.runs[rbase + idx] = r;
            else
                atomicAdd(&a.counts[6], 1ull);
        };
        lineisect::RunState s;
        lineisect::run_init(s, (uint32_t)k);
        bool over = false;
        if (lineisect::may_meet(L, c, P, g)) {
            const uint32_t r0 = P.part_ring[P.geom_part[g]], r1 = P.part_ring[P.geom_part[g + 1]];
            const pip::Box gb = P.geom_bbox[g];
            for (uint32_t m = L.chip_piece[c]; m < L.chip_piece[c + 1] && !over; m++) {
                const uint32_t i0 = L.piece_start[m], i1 = L.piece_start[m + 1];
                if (i1 - i0 < 2) continue;
                for (uint32_t i = i0; i + 1 < i1 && !over; i++) {
                    const Pt pa = lineisect::vert(L.verts, i), pb = lineisect::vert(L.verts, i + 1);
                    if (llclip::same(pa, pb)) continue;
                    const pip::Box sb = lineisect::seg_box(pa, pb);
                    if (!pip::boxes_meet(sb, gb)) {
                        lineisect::run_close(s, emit);
                        continue;
                    }
                    // the cut list: a, b and the meet points, in arrival order
                    wave_lds_sync();  // (the previous segment's readers are done with A and B)
                    if (lane == 0) {
                        A[0] = pa;
                        A[1] = pb;
                    }
                    int n = 2;
                    for (uint32_t r = r0; r < r1 && !over; r++) {
                        if (!pip::boxes_meet(sb, P.ring_bbox[r])) continue;
                        const uint32_t jb = P.ring_start[r], je = P.ring_start[r + 1];
                        if (je - jb < 2) continue;
                        const uint32_t nseg = je - jb - 1;
                        for (uint32_t base = 0; base < nseg; base += 64) {
                            const uint32_t j = base + (uint32_t)lane;
                            Pt o[2];
                            int cnt = 0;
                            if (j < nseg) cnt = llclip::meet(pa, pb, lineisect::vert(P.verts, jb + j), lineisect::vert(P.verts, jb + j + 1), o);
                            const unsigned long long m1 = __ballot(cnt >= 1), m2 = __ballot(cnt == 2);
                            const int c1 = __popcll(m1), c2 = __popcll(m2);
                            if (n + c1 + c2 > kSlots) {
                                over = true;
                                break;
                            }
                            if (cnt >= 1) A[n + __popcll(m1 & below)] = o[0];
                            if (cnt == 2) A[n + c1 + __popcll(m2 & below)] = o[1];
                            n += c1 + c2;
                        }
                    }
                    if (over) break;
                    wave_lds_sync();
                    // rank sort into B by the total order; bit-equal points take their arrival order
                    for (int e = lane; e < n; e += 64) {
                        const Pt p = A[e];
                        int rank = 0;
                        for (int f = 0; f < n; f++) {
                            const Pt q = A[f];
                            if (lineisect::cut_less(q, p, pa, pb) || (f < e && !lineisect::cut_less(p, q, pa, pb))) rank++;
                        }
                        B[rank] = p;
                    }
                    wave_lds_sync();
                    // bit-equal neighbours dropped: back into A
                    int u = 0;
                    for (int base = 0; base < n; base += 64) {
                        const int e = base + lane;
                        const bool keep = e < n && (e == 0 || !lineisect::bit_equal(B[e], B[e - 1]));
                        const unsigned long long mk = __ballot(keep);
                        if (keep) A[u + __popcll(mk & below)] = B[e];
                        u += __popcll(mk);
                    }
                    wave_lds_sync();
                    // the intervals' midpoint tests over the lanes: B[e].x = kept
                    for (int e = lane; e + 1 < u; e += 64) B[e].x = lineisect::interval_kept(P, g, A[e], A[e + 1]) ? 1.0 : 0.0;
                    wave_lds_sync();
                    // every lane folds the intervals in order: the state stays wave-uniform
                    for (int e = 0; e + 1 < u; e++) lineisect::run_interval(s, B[e].x != 0.0, A[e], A[e + 1], m, i, emit);
                }
                if (!over) lineisect::run_close(s, emit);
            }
        }
        if (a.fill || lane != 0) continue;
        if (over) {
            a.n_runs[k] = kOverflowed;
            a.len[k] = 0.0;
            const unsigned long long pos = atomicAdd(&a.counts[5], 1ull);
            if (pos < a.n) a.over[pos] = (uint32_t)k;
        } else {
            a.n_runs[k] = s.n_runs;
            a.len[k] = s.sum;
        }
    }
}

thread_local int64_t t_last[6] = {0, 0, 0, 0, 0, lineisect::kCutCap};
thread_local double t_ms[3] = {0, 0, 0};

template <class T>
int download(std::vector<T>& dst, const T* src, size_t n, hipStream_t stream) {
    dst.resize(n);
    if (n) MOSAIC_HIP(hipMemcpyAsync(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    return MOSAIC_OK;
}

// a polygon chip store on the host, for the pairs the host finishes
struct HostGeoms {
    std::vector<pip::Vec2> verts;
    std::vector<uint32_t> ring_start, part_ring, geom_part;
    std::vector<pip::Box> ring_bbox, geom_bbox;
    pip::GeomStore view() const {
        return pip::GeomStore{verts.data(), ring_start.data(), ring_bbox.data(), part_ring.data(), geom_part.data(), geom_bbox.data()};
    }
};
int download_geoms(const ChipsJoinView& pv, HostGeoms& h, hipStream_t stream) {
    const size_t ng = (size_t)pv.n_chips;
    MOSAIC_RC(download(h.geom_part, pv.store.geom_part, ng + 1, stream));
    MOSAIC_RC(download(h.geom_bbox, pv.store.geom_bbox, ng, stream));
    const size_t np = h.geom_part[ng];
    MOSAIC_RC(download(h.part_ring, pv.store.part_ring, np + 1, stream));
    const size_t nr = h.part_ring[np];
    MOSAIC_RC(download(h.ring_start, pv.store.ring_start, nr + 1, stream));
    MOSAIC_RC(download(h.ring_bbox, pv.store.ring_bbox, nr, stream));
    MOSAIC_RC(download(h.verts, pv.store.verts, (size_t)h.ring_start[nr], stream));
    return MOSAIC_OK;
}

struct HostLines {
    std::vector<pip::Vec2> verts;
    std::vector<uint32_t> piece_start, chip_piece;
    std::vector<pip::Box> piece_bbox, chip_bbox;
    bool have = false, boxes = false;
    lineisect::LineStore view() const {
        return lineisect::LineStore{verts.data(), piece_start.data(), piece_bbox.data(), chip_piece.data(), chip_bbox.data()};
    }
};
int download_lines(const LineChipsView& lv, HostLines& h, bool boxes, hipStream_t stream) {
    if (!h.have) {
        MOSAIC_RC(download(h.verts, lv.store.verts, (size_t)lv.n_vertices, stream));
        MOSAIC_RC(download(h.piece_start, lv.store.piece_start, (size_t)lv.n_pieces + 1, stream));
        MOSAIC_RC(download(h.chip_piece, lv.store.chip_piece, (size_t)lv.n_chips + 1, stream));
        h.have = true;
    }
    if (boxes && !h.boxes) {
        MOSAIC_RC(download(h.piece_bbox, lv.store.piece_bbox, (size_t)lv.n_pieces, stream));
        MOSAIC_RC(download(h.chip_bbox, lv.store.chip_bbox, (size_t)lv.n_chips, stream));
        h.boxes = true;
    }
    return MOSAIC_OK;
}

int aggregate(mosaic_ctx* ctx, const mosaic_line_chips* lines, const mosaic_chips* polygons, bool geometry, mosaic_isect_geoms& out) {
    out.off.assign(1, 0);
    LineChipsView lv;
    ChipsJoinView pv;
    MOSAIC_RC(mosaic_line_chips_view(lines, &lv));
    MOSAIC_RC(mosaic_chips_join_view(polygons, &pv));
    if (lv.grid != pv.grid || lv.res != pv.res)
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_intersection_aggregate: both chip tables must use the same grid and resolution");
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    if (lv.device != ex.device || pv.device != ex.device)
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_intersection_aggregate: a chip table of another device");
    std::fill(t_last, t_last + 5, 0);
    t_last[5] = lineisect::kCutCap;
    t_ms[0] = t_ms[1] = t_ms[2] = 0;
    if (lv.n_chips == 0 || pv.n_chips == 0 || pv.capacity == 0) return MOSAIC_OK;
    hipStream_t stream = ex.stream;
    const int64_t n = lv.n_chips;
    const int64_t wide = (int64_t)ex.n_cu * 16;

    dev::Events<8> ev;
    MOSAIC_RC(ev.create());
    Buf s_counts, s_list, s_chiplen, s_len, s_nruns, s_over, s_runoff, s_runs;
    unsigned long long counts[7] = {0, 0, 0, 0, ~0ull, 0, 0};
    MOSAIC_RC(s_counts.reserve(sizeof(counts)));
    MOSAIC_HIP(hipMemcpyAsync(s_counts.p, counts, sizeof(counts), hipMemcpyHostToDevice, stream));
    ProbeArgs pa{};
    pa.cell = lv.cell;
    pa.meta = lv.meta;
    pa.n = n;
    pa.table = pv.table;
    pa.mask = pv.capacity - 1;
    pa.pmeta = pv.meta;
    pa.pass = 0;
    pa.counts = s_counts.as<unsigned long long>();
    const dim3 pgrid((unsigned)blocks_for(n, kBlock, wide));
    MOSAIC_HIP(hipEventRecord(ev.e[0], stream));
    hipLaunchKernelGGL(k_lx_probe, pgrid, dim3(kBlock), 0, stream, pa);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipEventRecord(ev.e[1], stream));
    MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, sizeof(counts), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    const unsigned long long pairs = counts[0], n_clip = counts[1], n_core = pairs - n_clip;
    if (counts[4] != ~0ull)
        return mosaic_tess_fail(MOSAIC_E_ARG, ("st_intersection_aggregate (lines): line chip " + std::to_string(counts[4]) +
                                               " is a core chip; lineFill makes none and a line result cannot hold a cell")
                                                  .c_str());
    if (pairs == 0) return MOSAIC_OK;
    if (pairs >= (1ull << 31)) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "st_intersection_aggregate (lines): 2^31 chip pairs or more");
    MOSAIC_RC(s_list.reserve((size_t)pairs * sizeof(PairRec)));
    pa.pass = 1;
    pa.list = s_list.as<PairRec>();
    pa.n_pairs = pairs;
    pa.n_clip = n_clip;
    MOSAIC_HIP(hipEventRecord(ev.e[2], stream));
    hipLaunchKernelGGL(k_lx_probe, pgrid, dim3(kBlock), 0, stream, pa);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipEventRecord(ev.e[3], stream));
    if (n_core) {
        MOSAIC_RC(s_chiplen.reserve((size_t)n * sizeof(double)));
        hipLaunchKernelGGL(k_lx_chip_len, dim3((unsigned)blocks_for(n, kBlock, wide)), dim3(kBlock), 0, stream, lv.store, n, s_chiplen.as<double>());
        MOSAIC_HIP(hipGetLastError());
    }
    ClipArgs ca{};
    const int64_t cblocks = std::max<int64_t>(1, std::min<int64_t>(((int64_t)n_clip + kWaves - 1) / kWaves, wide));
    if (n_clip) {
        MOSAIC_RC(s_len.reserve((size_t)n_clip * sizeof(double)));
        MOSAIC_RC(s_nruns.reserve((size_t)n_clip * sizeof(uint32_t)));
        MOSAIC_RC(s_over.reserve((size_t)n_clip * sizeof(uint32_t)));
        ca.L = lv.store;
        ca.P = pv.store;
        ca.list = pa.list;
        ca.n = n_clip;
        ca.fill = 0;
        ca.len = s_len.as<double>();
        ca.n_runs = s_nruns.as<uint32_t>();
        ca.counts = pa.counts;
        ca.over = s_over.as<uint32_t>();
        hipLaunchKernelGGL(k_lx_clip, dim3((unsigned)cblocks), dim3(kBlock), 0, stream, ca);
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_HIP(hipEventRecord(ev.e[4], stream));
    MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, sizeof(counts), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    if (counts[2] != n_clip || counts[3] != n_core || counts[5] > n_clip)
        return mosaic_tess_fail(MOSAIC_E_CAPACITY, "st_intersection_aggregate (lines): the pair list does not match its count");
    const size_t n_over = (size_t)counts[5];
    std::vector<PairRec> hp;
    std::vector<double> len, chip_len;
    std::vector<uint32_t> n_runs, over;
    MOSAIC_RC(download(hp, pa.list, (size_t)pairs, stream));
    MOSAIC_RC(download(len, s_len.as<double>(), (size_t)n_clip, stream));
    MOSAIC_RC(download(n_runs, s_nruns.as<uint32_t>(), (size_t)n_clip, stream));
    MOSAIC_RC(download(over, s_over.as<uint32_t>(), n_over, stream));
    if (n_core) MOSAIC_RC(download(chip_len, s_chiplen.as<double>(), (size_t)n, stream));
    len.resize((size_t)pairs);
    for (size_t i = (size_t)n_clip; i < (size_t)pairs; i++) len[i] = chip_len[hp[i].line];
    // the pairs over the cut cap: the host driver on the tables' arrays
    HostLines hl;
    std::vector<std::vector<Run>> over_runs(n_over);
    if (n_over) {
        HostGeoms hg;
        MOSAIC_RC(download_geoms(pv, hg, stream));
        MOSAIC_RC(download_lines(lv, hl, true, stream));
        const lineisect::LineStore L = hl.view();
        const pip::GeomStore P = hg.view();
        std::vector<Pt> cuts;
        for (size_t q = 0; q < n_over; q++) {
            const uint32_t k = over[q];
            uint32_t nr = 0;
            len[k] = lineisect::clip_pair_host(L, hp[k].line, P, hp[k].poly, k, cuts, &over_runs[q], &nr);
            n_runs[k] = nr;
        }
    }
    std::vector<uint64_t> run_off;
    std::vector<Run> runs;
    unsigned long long total_runs = 0;
    for (size_t k = 0; k < (size_t)n_clip; k++) total_runs += n_runs[k];
    if (geometry) {
        run_off.assign((size_t)pairs + 1, 0);
        for (size_t k = 0; k < (size_t)n_clip; k++) run_off[k + 1] = run_off[k] + n_runs[k];
        for (size_t k = (size_t)n_clip; k < (size_t)pairs; k++) run_off[k + 1] = run_off[k];
        MOSAIC_HIP(hipEventRecord(ev.e[5], stream));
        if (total_runs) {
            // the pairs the host finished keep the marker on the device: the fill pass skips them
            MOSAIC_RC(s_runoff.reserve(((size_t)n_clip + 1) * sizeof(unsigned long long)));
            MOSAIC_RC(s_runs.reserve((size_t)total_runs * sizeof(Run)));
            MOSAIC_HIP(hipMemcpyAsync(s_runoff.p, run_off.data(), ((size_t)n_clip + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
            ca.fill = 1;
            ca.run_off = s_runoff.as<unsigned long long>();
            ca.runs = s_runs.as<Run>();
            hipLaunchKernelGGL(k_lx_clip, dim3((unsigned)cblocks), dim3(kBlock), 0, stream, ca);
            MOSAIC_HIP(hipGetLastError());
        }
        MOSAIC_HIP(hipEventRecord(ev.e[6], stream));
        MOSAIC_RC(download(runs, s_runs.as<Run>(), (size_t)total_runs, stream));
        MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, sizeof(counts), hipMemcpyDeviceToHost, stream));
        MOSAIC_HIP(hipStreamSynchronize(stream));
        if (counts[6]) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "st_intersection_aggregate (lines): the run records do not match their count");
        for (size_t q = 0; q < n_over; q++) std::copy(over_runs[q].begin(), over_runs[q].end(), runs.begin() + (long)run_off[over[q]]);
        MOSAIC_RC(download_lines(lv, hl, false, stream));
    }
    float m01 = 0, m23 = 0, m34 = 0, m56 = 0;
    MOSAIC_HIP(hipEventElapsedTime(&m01, ev.e[0], ev.e[1]));
    MOSAIC_HIP(hipEventElapsedTime(&m23, ev.e[2], ev.e[3]));
    MOSAIC_HIP(hipEventElapsedTime(&m34, ev.e[3], ev.e[4]));
    if (geometry) MOSAIC_HIP(hipEventElapsedTime(&m56, ev.e[5], ev.e[6]));
    lineisect::fold_groups(hp.data(), hp.size(), len.data(), geometry, hl.view(), run_off.data(), runs.data(), out);
    t_last[0] = (int64_t)pairs;
    t_last[1] = (int64_t)n_clip;
    t_last[2] = (int64_t)n_over;
    t_last[3] = (int64_t)total_runs;
    t_last[4] = (int64_t)out.lk.size();
    t_ms[0] = (double)m01 + (double)m23;
    t_ms[1] = (double)m34;
    t_ms[2] = (double)m56;
    return MOSAIC_OK;
}

}  // namespace

extern "C" {

uint64_t mosaic_layout_line_clip(void) { return lineisect::clip_layout_fingerprint(); }

int mosaic_line_intersection_last(int64_t out[6], double ms[3]) {
    if (out) std::copy(t_last, t_last + 6, out);
    if (ms) std::copy(t_ms, t_ms + 3, ms);
    return MOSAIC_OK;
}

int mosaic_line_intersection_aggregate(mosaic_ctx* ctx, const mosaic_line_chips* lines, const mosaic_chips* polygons,
                                       int32_t* out_line_key, int32_t* out_polygon_key, double* out_length, int64_t cap,
                                       int64_t* n_out) {
    if (!ctx || !lines || !polygons || !n_out || cap < 0 || (cap > 0 && (!out_line_key || !out_polygon_key || !out_length)))
        return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *n_out = 0;
    mosaic_isect_geoms g;
    MOSAIC_RC(aggregate(ctx, lines, polygons, false, g));
    *n_out = (int64_t)g.lk.size();
    if ((int64_t)g.lk.size() > cap)
        return mosaic_tess_fail(MOSAIC_E_CAPACITY, ("st_intersection_aggregate (lines): " + std::to_string(g.lk.size()) + " groups").c_str());
    std::copy(g.lk.begin(), g.lk.end(), out_line_key);
    std::copy(g.rk.begin(), g.rk.end(), out_polygon_key);
    std::copy(g.area.begin(), g.area.end(), out_length);
    return MOSAIC_OK;
}

int mosaic_line_intersection_aggregate_geometry(mosaic_ctx* ctx, const mosaic_line_chips* lines, const mosaic_chips* polygons,
                                                mosaic_isect_geoms** out) {
    if (!ctx || !lines || !polygons || !out) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    std::unique_ptr<mosaic_isect_geoms> g(new mosaic_isect_geoms());
    MOSAIC_RC(aggregate(ctx, lines, polygons, true, *g));
    *out = g.release();
    return MOSAIC_OK;
}

}  // extern "C"
