// mosaic_tessellate_lines_gpu: Mosaic.lineFill (lineclip.h) on the GPU, the host producer's chip set row
// for row and byte for byte.
//
//   k_line_spans  one lane per segment: lineclip::span_count -- spans of about two cells, so a segment
//                 crossing hundreds of cells becomes hundreds of lanes' work, not one lane's
//   device scan   of the span counts
//   k_line_walk   one lane per span (grid-stride, the lane's list of tried cells in global memory):
//                 lineclip::walk_span, first counting the (cell, segment) pairs, then, after a scan,
//                 writing them -- nothing is appended through an atomic, nothing has a fixed capacity.
//                 The counting pass keeps a span's first eight cells, so only a span with more walks
//                 twice (a trip's segment meets 1.2 cells on average).
//                 A span that tries more than kWalkCap cells is walked by the host routine and its
//                 pairs are appended.
//   radix sort    by cell (stable; the pairs are written in segment order, so every (cell, line) group
//                 comes out contiguous with its segments ascending; pairs from the host are first
//                 sorted in by segment).  Overlapping spans find a cell twice: k_line_flags marks the
//                 first of equal pairs and the first of every group, one scan places both,
//                 k_line_fill writes the groups.
//   k_line_clip   one lane per group (grid-stride, the lane's kItems items in global memory):
//                 lineclip::build, first counting the chip's items, then, after a scan, writing them.
//                 A chip of more than kItems pieces is built by the host routine.
//   host          linefill::finish: the handed-off groups, the row order, the WKB.
#include <memory>

#include "chip_set.h"
#include "dev_rt.h"
#include "line_fill.h"

using namespace mosaic;

extern "C" uint64_t mosaic_layout_lines_host(void);

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kNone = ~0ull;

using dev::blocks_for;
using dev::Buf;

struct Last {
    int64_t n[4] = {0, 0, 0, 0};
    int64_t walk[3] = {0, 0, 0};  // spans walked, spans handed to the host routine, the pairs those added
    double ms[3] = {0, 0, 0};
};
thread_local Last g_last;

struct Batch {
    lineclip::Grid g;
    const double* xy;
    const int32_t* vert_line;
    const int64_t* line_off;
    int64_t n_verts;
};

// counters[0]: the first segment that came to a bad cell (atomicMin; the host reads it after the walk has
// added its own, so that a call names the first bad segment of the batch whichever stage finds it);
// [1]: spans / groups for the host
__global__ void __launch_bounds__(kBlock) k_line_spans(Batch b, int64_t* spans, unsigned long long* counters) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= b.n_verts; s += step) {
        int32_t k = 0;
        if (s + 1 < b.n_verts && s + 1 < b.line_off[b.vert_line[s] + 1]) {
            if (lineclip::span_count(b.g, lineclip::DirectPoly{b.g}, lineclip::vtx(b.xy, s), lineclip::vtx(b.xy, s + 1), &k) != lineclip::kOk) {
                atomicMin(&counters[0], (unsigned long long)s);
                k = 0;
            }
        }
        spans[s] = k;
    }
}

// the segment of span i: the last s with span_off[s] <= i
__device__ int64_t span_segment(const int64_t* span_off, int64_t n_verts, int64_t i) {
    int64_t lo = 0, hi = n_verts;  // span_off[lo] <= i < span_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (span_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// kWrite = false: counts span i's pairs and keeps the first kSlot of its cells in slot; kWrite = true (cnt
// scanned): writes the pairs, from the slot where it holds them all, else by walking again.
using lineclip::kSlot;
template <bool kWrite>
__global__ void __launch_bounds__(kBlock) k_line_walk(Batch b, const int64_t* span_off, int64_t n_spans, int64_t* seen_all,
                                                      int64_t* cnt, uint8_t* status, unsigned long long* counters, uint64_t* slot,
                                                      uint64_t* out_cell, uint32_t* out_seg) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    int64_t* seen = seen_all + lane * lineclip::kWalkCap;
    for (int64_t i = lane; i < n_spans; i += step) {
        if (kWrite && status[i] != lineclip::kOk) continue;
        const int64_t s = span_segment(span_off, b.n_verts, i);
        const int64_t at = kWrite ? cnt[i] : 0;  // (after the scan: the span's first pair)
        if (kWrite && cnt[i + 1] - at <= kSlot) {
            for (int64_t k = 0; k < cnt[i + 1] - at; k++) {
                out_cell[at + k] = slot[i * kSlot + k];
                out_seg[at + k] = (uint32_t)s;
            }
            continue;
        }
        const int32_t j = (int32_t)(i - span_off[s]), K = (int32_t)(span_off[s + 1] - span_off[s]);
        int64_t n = 0;
        const int st = lineclip::walk_span(b.g, lineclip::DirectPoly{b.g}, lineclip::vtx(b.xy, s), lineclip::vtx(b.xy, s + 1), j, K, seen,
                                           lineclip::kWalkCap, [&](int64_t cell) {
                                               if (kWrite) {
                                                   out_cell[at + n] = (uint64_t)cell;
                                                   out_seg[at + n] = (uint32_t)s;
                                               } else if (n < kSlot) {
                                                   slot[i * kSlot + n] = (uint64_t)cell;
                                               }
                                               n++;
                                           });
        if (!kWrite) {
            status[i] = (uint8_t)st;
            cnt[i] = st == lineclip::kOk ? n : 0;
            if (st == lineclip::kBadCell) atomicMin(&counters[0], (unsigned long long)s);
            if (st == lineclip::kNeedsMore) atomicAdd(&counters[1], 1ull);
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_line_flags(const uint64_t* cell, const uint32_t* seg, const int32_t* vert_line, int64_t n,
                                                       uint64_t* flags) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const bool cell_new = i == 0 || cell[i] != cell[i - 1];
        const bool uniq = cell_new || seg[i] != seg[i - 1];
        const bool head = cell_new || vert_line[seg[i]] != vert_line[seg[i - 1]];
        flags[i] = (uint64_t)head << 32 | (uint64_t)uniq;
    }
}

// scan: the inclusive sums of flags
__global__ void __launch_bounds__(kBlock) k_line_fill(const uint64_t* cell, const uint32_t* seg, const uint64_t* scan, int64_t n,
                                                      int64_t* g_cell, int64_t* seg_start, uint32_t* useg) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint64_t here = scan[i], before = i ? scan[i - 1] : 0;
        const uint32_t u = (uint32_t)here, u0 = (uint32_t)before;
        if (u == u0) continue;  // a pair found twice
        useg[u - 1] = seg[i];
        if ((here >> 32) != (before >> 32)) {
            g_cell[(here >> 32) - 1] = (int64_t)cell[i];
            seg_start[(here >> 32) - 1] = (int64_t)u - 1;
        }
    }
}

template <bool kWrite>
__global__ void __launch_bounds__(kBlock) k_line_clip(Batch b, const int64_t* g_cell, const int64_t* seg_start, const uint32_t* useg,
                                                      int64_t n_groups, lineclip::Item* work_all, linefill::GroupRec* recs,
                                                      int64_t* cnt, unsigned long long* counters, lineclip::Item* items) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = lane; i < n_groups; i += step) {
        if (kWrite && (recs[i].status != lineclip::kOk || recs[i].n_items == 0)) continue;
        const uint32_t* segs = useg + seg_start[i];
        lineclip::Work w{work_all + lane * lineclip::kItems, lineclip::kItems, 0, 0, 0, -1, 0.0};
        lineclip::Cell C;
        int st = lineclip::kBadCell;
        if (lineclip::cell_poly(b.g, g_cell[i], C)) st = lineclip::build(b.xy, C, segs, seg_start[i + 1] - seg_start[i], w);
        if (kWrite) {
            const int64_t at = cnt[i];
            recs[i].item0 = at;
            for (int32_t k = 0; k < w.n; k++) items[at + k] = w.it[k];
        } else {
            const int32_t n = st == lineclip::kOk ? w.n : 0;
            recs[i] = linefill::GroupRec{g_cell[i], w.s0, w.t0, 0, n, w.has_piece, st, segs[0]};
            cnt[i] = n;
            if (st == lineclip::kBadCell) atomicMin(&counters[0], (unsigned long long)segs[0]);
            if (st == lineclip::kNeedsMore) atomicAdd(&counters[1], 1ull);
        }
    }
}

constexpr int64_t kMaxRows = 0x7fffffff;

}  // namespace

extern "C" {

uint64_t mosaic_layout_line_fill(void) { return linefill::layout_fingerprint(); }

int mosaic_tess_lines_last(int64_t out[4], double ms[3]) {
    if (!out || !ms) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    for (int i = 0; i < 4; i++) out[i] = g_last.n[i];
    for (int i = 0; i < 3; i++) ms[i] = g_last.ms[i];
    return MOSAIC_OK;
}

int mosaic_tess_lines_last_walk(int64_t out[3]) {
    if (!out) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    for (int i = 0; i < 3; i++) out[i] = g_last.walk[i];
    return MOSAIC_OK;
}

int mosaic_tessellate_lines_gpu(mosaic_ctx* ctx, int grid, int res, int64_t n_geoms, const int64_t* geom_lines,
                                const int64_t* line_offsets, const double* xy, int cells_only, mosaic_chip_set** out) {
    if (!ctx || !out) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    *out = nullptr;
    if (mosaic_layout_line_fill() != mosaic_layout_lines_host())
        return mosaic_tess_fail(MOSAIC_E_ARG, "line_fill: the host and device objects disagree about the shared records");
    if (grid == MOSAIC_GRID_H3 && (res < 0 || res > 15))
        return mosaic_tess_fail(MOSAIC_E_RES, ("H3 resolution has to be between 0 and 15; found " + std::to_string(res)).c_str());
    if (grid == MOSAIC_GRID_BNG && !(res != 0 && res >= -6 && res <= 6))
        return mosaic_tess_fail(MOSAIC_E_RES, ("BNG resolution not supported; found " + std::to_string(res)).c_str());
    if (grid != MOSAIC_GRID_H3 && grid != MOSAIC_GRID_BNG) return mosaic_tess_fail(MOSAIC_E_ARG, "unknown grid");
    linefill::Clean c;
    MOSAIC_RC(linefill::prepare(n_geoms, geom_lines, line_offsets, xy, c));
    g_last = Last();
    std::unique_ptr<mosaic_chip_set> cs(new mosaic_chip_set());
    if (c.n_verts == 0) {
        *out = cs.release();
        return MOSAIC_OK;
    }
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    hipStream_t st = ex.stream;
    const lineclip::Grid G{grid == MOSAIC_GRID_H3 ? 0 : 1, res};
    const int64_t nv = c.n_verts;
    const int64_t light = (int64_t)ex.n_cu * 2048 / kBlock, heavy = (int64_t)ex.n_cu * 1024 / kBlock;  // blocks of the light / the walking kernels
    dev::Events<4> ev;
    MOSAIC_RC(ev.create());

    Buf d_xy, d_vl, d_lo, d_counters, d_spans, d_tmp;
    MOSAIC_RC(d_xy.reserve((size_t)nv * 16));
    MOSAIC_RC(d_vl.reserve((size_t)nv * 4));
    MOSAIC_RC(d_lo.reserve((size_t)(c.n_lines + 1) * 8));
    MOSAIC_RC(d_counters.reserve(16));
    MOSAIC_RC(d_spans.reserve((size_t)(nv + 1) * 8));
    MOSAIC_HIP(hipMemcpyAsync(d_xy.p, c.xy.data(), (size_t)nv * 16, hipMemcpyHostToDevice, st));
    MOSAIC_HIP(hipMemcpyAsync(d_vl.p, c.vert_line.data(), (size_t)nv * 4, hipMemcpyHostToDevice, st));
    MOSAIC_HIP(hipMemcpyAsync(d_lo.p, c.line_off.data(), (size_t)(c.n_lines + 1) * 8, hipMemcpyHostToDevice, st));
    unsigned long long counters[2] = {kNone, 0};
    MOSAIC_HIP(hipMemcpyAsync(d_counters.p, counters, 16, hipMemcpyHostToDevice, st));
    const Batch B{G, d_xy.as<double>(), d_vl.as<int32_t>(), d_lo.as<int64_t>(), nv};
    auto read_counters = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(counters, d_counters.p, 16, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    };

    // ---- spans
    MOSAIC_HIP(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(k_line_spans, dim3(blocks_for(nv + 1, kBlock, heavy)), dim3(kBlock), 0, st, B, d_spans.as<int64_t>(),
                       d_counters.as<unsigned long long>());
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_RC(dev::exclusive_sum(d_tmp, d_spans.as<int64_t>(), d_spans.as<int64_t>(), (int)(nv + 1), st));  // in place: the last input is 0, the last sum the total
    int64_t n_spans = 0;
    MOSAIC_HIP(hipMemcpyAsync(&n_spans, d_spans.as<int64_t>() + nv, 8, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    // (a segment whose span_count failed has no span and has put itself into counters[0], which is read
    // after the walk's counting pass: an earlier segment may be bad for the walk alone)
    if (n_spans >= kMaxRows) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "line_fill: 2^31 - 1 spans at the most");
    int64_t n_segments = 0;
    for (int64_t l = 0; l < c.n_lines; l++) n_segments += std::max<int64_t>(0, c.line_off[(size_t)l + 1] - c.line_off[(size_t)l] - 1);
    g_last.n[0] = n_segments;
    g_last.walk[0] = n_spans;

    // ---- walk: count, scan, write
    const unsigned walk_blocks = blocks_for(n_spans, kBlock, heavy);
    Buf d_seen, d_cnt, d_status, d_slot;
    MOSAIC_RC(d_slot.reserve((size_t)n_spans * kSlot * 8));
    MOSAIC_RC(d_seen.reserve((size_t)walk_blocks * kBlock * lineclip::kWalkCap * 8));
    MOSAIC_RC(d_cnt.reserve((size_t)(n_spans + 1) * 8));
    MOSAIC_RC(d_status.reserve((size_t)n_spans));
    MOSAIC_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)(n_spans + 1) * 8, st));
    hipLaunchKernelGGL((k_line_walk<false>), dim3(walk_blocks), dim3(kBlock), 0, st, B, d_spans.as<int64_t>(), n_spans,
                       d_seen.as<int64_t>(), d_cnt.as<int64_t>(), d_status.as<uint8_t>(), d_counters.as<unsigned long long>(),
                       d_slot.as<uint64_t>(), (uint64_t*)nullptr, (uint32_t*)nullptr);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_RC(dev::exclusive_sum(d_tmp, d_cnt.as<int64_t>(), d_cnt.as<int64_t>(), (int)(n_spans + 1), st));
    int64_t n_dev_pairs = 0;
    MOSAIC_HIP(hipMemcpyAsync(&n_dev_pairs, d_cnt.as<int64_t>() + n_spans, 8, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(read_counters());
    int64_t bad_seg = counters[0] == kNone ? -1 : (int64_t)counters[0];  // the first bad segment of both stages
    // spans for the host (ascending, so by segment: one of an earlier segment than bad_seg may be bad too)
    std::vector<uint64_t> extra_cell;
    std::vector<uint32_t> extra_seg;
    g_last.walk[1] = (int64_t)counters[1];
    if (counters[1]) {
        std::vector<uint8_t> status((size_t)n_spans);
        std::vector<int64_t> span_off((size_t)nv + 1);
        MOSAIC_HIP(hipMemcpyAsync(status.data(), d_status.p, (size_t)n_spans, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipMemcpyAsync(span_off.data(), d_spans.p, (size_t)(nv + 1) * 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
        std::vector<int64_t> cells;
        for (int64_t i = 0; i < n_spans; i++) {
            if (status[(size_t)i] != lineclip::kNeedsMore) continue;
            const int64_t s = std::upper_bound(span_off.begin(), span_off.end(), i) - span_off.begin() - 1;
            if (bad_seg >= 0 && s >= bad_seg) break;
            cells.clear();
            if (linefill::walk_span_host(G, c, s, (int32_t)(i - span_off[(size_t)s]), (int32_t)(span_off[(size_t)s + 1] - span_off[(size_t)s]),
                                         cells) != lineclip::kOk) {
                bad_seg = s;
                break;
            }
            for (int64_t cell : cells) extra_cell.push_back((uint64_t)cell), extra_seg.push_back((uint32_t)s);
        }
        counters[1] = 0;
        MOSAIC_HIP(hipMemcpyAsync(d_counters.as<unsigned long long>() + 1, &counters[1], 8, hipMemcpyHostToDevice, st));
    }
    if (bad_seg >= 0) return linefill::fail_bad_cell(c, bad_seg);
    g_last.walk[2] = (int64_t)extra_cell.size();
    const int64_t n_pairs = n_dev_pairs + (int64_t)extra_cell.size();
    g_last.n[3] = n_pairs;
    if (n_pairs >= kMaxRows) return mosaic_tess_fail(MOSAIC_E_CAPACITY, "line_fill: 2^31 - 1 (cell, segment) pairs at the most");
    if (n_pairs == 0) {
        *out = cs.release();
        return MOSAIC_OK;
    }
    Buf d_cell0, d_cell1, d_seg0, d_seg1;
    MOSAIC_RC(d_cell0.reserve((size_t)n_pairs * 8));
    MOSAIC_RC(d_cell1.reserve((size_t)n_pairs * 8));
    MOSAIC_RC(d_seg0.reserve((size_t)n_pairs * 4));
    MOSAIC_RC(d_seg1.reserve((size_t)n_pairs * 4));
    hipLaunchKernelGGL((k_line_walk<true>), dim3(walk_blocks), dim3(kBlock), 0, st, B, d_spans.as<int64_t>(), n_spans,
                       d_seen.as<int64_t>(), d_cnt.as<int64_t>(), d_status.as<uint8_t>(), d_counters.as<unsigned long long>(),
                       d_slot.as<uint64_t>(), d_cell0.as<uint64_t>(), d_seg0.as<uint32_t>());
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipEventRecord(ev.e[1], st));

    // ---- groups
    if (!extra_cell.empty()) {
        MOSAIC_HIP(hipMemcpyAsync(d_cell0.as<uint64_t>() + n_dev_pairs, extra_cell.data(), extra_cell.size() * 8, hipMemcpyHostToDevice, st));
        MOSAIC_HIP(hipMemcpyAsync(d_seg0.as<uint32_t>() + n_dev_pairs, extra_seg.data(), extra_seg.size() * 4, hipMemcpyHostToDevice, st));
        MOSAIC_RC(dev::sort_pairs(d_tmp, d_seg0.as<uint32_t>(), d_seg1.as<uint32_t>(), d_cell0.as<uint64_t>(), d_cell1.as<uint64_t>(), (int)n_pairs, 0, 32, st));
        std::swap(d_seg0.p, d_seg1.p);
        std::swap(d_cell0.p, d_cell1.p);
    }
    MOSAIC_RC(dev::sort_pairs(d_tmp, d_cell0.as<uint64_t>(), d_cell1.as<uint64_t>(), d_seg0.as<uint32_t>(), d_seg1.as<uint32_t>(), (int)n_pairs, 0, 64, st));
    const uint64_t* s_cell = d_cell1.as<uint64_t>();
    const uint32_t* s_seg = d_seg1.as<uint32_t>();
    uint64_t* flags = d_cell0.as<uint64_t>();  // (the unsorted keys are done with)
    hipLaunchKernelGGL(k_line_flags, dim3(blocks_for(n_pairs, kBlock, light)), dim3(kBlock), 0, st, s_cell, s_seg, B.vert_line, n_pairs, flags);
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_RC(dev::inclusive_sum(d_tmp, flags, flags, (int)n_pairs, st));
    uint64_t last = 0;
    MOSAIC_HIP(hipMemcpyAsync(&last, flags + (n_pairs - 1), 8, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipStreamSynchronize(st));
    const int64_t n_groups = (int64_t)(last >> 32), n_useg = (int64_t)(last & 0xffffffffull);
    g_last.n[1] = n_groups;
    Buf d_gcell, d_gstart, d_useg;
    MOSAIC_RC(d_gcell.reserve((size_t)n_groups * 8));
    MOSAIC_RC(d_gstart.reserve((size_t)(n_groups + 1) * 8));
    MOSAIC_RC(d_useg.reserve((size_t)n_useg * 4));
    hipLaunchKernelGGL(k_line_fill, dim3(blocks_for(n_pairs, kBlock, light)), dim3(kBlock), 0, st, s_cell, s_seg, flags, n_pairs,
                       d_gcell.as<int64_t>(), d_gstart.as<int64_t>(), d_useg.as<uint32_t>());
    MOSAIC_HIP(hipGetLastError());
    MOSAIC_HIP(hipMemcpyAsync(d_gstart.as<int64_t>() + n_groups, &n_useg, 8, hipMemcpyHostToDevice, st));
    MOSAIC_HIP(hipEventRecord(ev.e[2], st));

    // ---- clip: count, scan, write
    const unsigned clip_blocks = blocks_for(n_groups, kBlock, heavy);
    Buf d_work, d_recs, d_icnt, d_items;
    MOSAIC_RC(d_work.reserve((size_t)clip_blocks * kBlock * lineclip::kItems * sizeof(lineclip::Item)));
    MOSAIC_RC(d_recs.reserve((size_t)n_groups * sizeof(linefill::GroupRec)));
    MOSAIC_RC(d_icnt.reserve((size_t)(n_groups + 1) * 8));
    MOSAIC_HIP(hipMemsetAsync(d_icnt.p, 0, (size_t)(n_groups + 1) * 8, st));
    hipLaunchKernelGGL((k_line_clip<false>), dim3(clip_blocks), dim3(kBlock), 0, st, B, d_gcell.as<int64_t>(), d_gstart.as<int64_t>(),
                       d_useg.as<uint32_t>(), n_groups, d_work.as<lineclip::Item>(), d_recs.as<linefill::GroupRec>(),
                       d_icnt.as<int64_t>(), d_counters.as<unsigned long long>(), (lineclip::Item*)nullptr);
    MOSAIC_HIP(hipGetLastError());
    int64_t n_items = 0;
    if (!cells_only) {
        MOSAIC_RC(dev::exclusive_sum(d_tmp, d_icnt.as<int64_t>(), d_icnt.as<int64_t>(), (int)(n_groups + 1), st));
        MOSAIC_HIP(hipMemcpyAsync(&n_items, d_icnt.as<int64_t>() + n_groups, 8, hipMemcpyDeviceToHost, st));
        MOSAIC_HIP(hipStreamSynchronize(st));
        MOSAIC_RC(d_items.reserve((size_t)n_items * sizeof(lineclip::Item)));
        hipLaunchKernelGGL((k_line_clip<true>), dim3(clip_blocks), dim3(kBlock), 0, st, B, d_gcell.as<int64_t>(), d_gstart.as<int64_t>(),
                           d_useg.as<uint32_t>(), n_groups, d_work.as<lineclip::Item>(), d_recs.as<linefill::GroupRec>(),
                           d_icnt.as<int64_t>(), d_counters.as<unsigned long long>(), d_items.as<lineclip::Item>());
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_HIP(hipEventRecord(ev.e[3], st));
    std::vector<linefill::GroupRec> recs((size_t)n_groups);
    std::vector<int64_t> seg_start((size_t)n_groups + 1);
    std::vector<uint32_t> useg((size_t)n_useg);
    std::vector<lineclip::Item> items((size_t)std::max<int64_t>(1, n_items));
    MOSAIC_HIP(hipMemcpyAsync(recs.data(), d_recs.p, (size_t)n_groups * sizeof(linefill::GroupRec), hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipMemcpyAsync(seg_start.data(), d_gstart.p, (size_t)(n_groups + 1) * 8, hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(hipMemcpyAsync(useg.data(), d_useg.p, (size_t)n_useg * 4, hipMemcpyDeviceToHost, st));
    if (n_items) MOSAIC_HIP(hipMemcpyAsync(items.data(), d_items.p, (size_t)n_items * sizeof(lineclip::Item), hipMemcpyDeviceToHost, st));
    MOSAIC_HIP(read_counters());
    if (counters[0] != kNone) return linefill::fail_bad_cell(c, (int64_t)counters[0]);
    g_last.n[2] = (int64_t)counters[1];
    for (int i = 0; i < 3; i++) {
        float ms = 0;
        MOSAIC_HIP(hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
        g_last.ms[i] = ms;
    }
    int64_t bad = -1;
    MOSAIC_RC(linefill::finish(G, c, n_groups, recs.data(), seg_start.data(), useg.data(), items.data(), cells_only, cs.get(), &bad));
    if (bad >= 0) return linefill::fail_bad_cell(c, bad);
    *out = cs.release();
    return MOSAIC_OK;
}

}  // extern "C"
