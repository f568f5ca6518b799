// The measures of the rows of a device-resident geometry column (mosaic_st_measures): st_area,
// st_length / st_perimeter, st_centroid, st_numpoints and the four bounds.  st_measures.h holds the
// semantics and the sequential definition `meas::measure` whose bits these kernels return; the columns
// are those of st_distance.hip.
//
// The centroid is one running sum over all rings of a geometry, so the unit of work is the output
// row (one geometry), not the ring.  Per call:
//   k_meas_plan  one lane per row: row range check, then the row goes by its stored vertex count to
//                the front (< meas_wave_min, and every row that is not MOSAIC_ROW_OK) or the back of
//                one list.  Nothing is written to the outputs before the host has seen that no row
//                index was out of range.
//   k_meas_lane  one lane per row: the sequential definition.  Rows that are not MOSAIC_ROW_OK get
//                NaN (numpoints 0) here.
//   k_meas_wave  one wave per row.  Ring after ring, meas_tile segments at a time: all 64 lanes compute
//                the per-segment terms of the tile into LDS (products, differences, square roots: no
//                order), then lane 0 adds them in the definition's order into its accumulators, which
//                it carries across tiles, rings and parts.  Orientation.isCCW's search for the last
//                rising vertex of the greatest y is a wave reduction; its tail is the definition's.
#include "dev_rt.h"
#include "geoms_device.h"
#include "pair_lists.h"
#include "st_measures.h"

using namespace mosaic;

namespace {

using dev::blocks_for;
using dev::Buf;
using dev::OutSlot;
using pairs::Col;
using pairs::kBlock;
using pairs::view;
using pairs::wave_append;
constexpr int kMaxTile = 256;

// the last call of this thread: rows served by one lane, rows served by a wave
thread_local int64_t t_last[2] = {0, 0};

struct Outs {
    double *area, *length, *cx, *cy;
    int64_t* numpoints;
    double *xmin, *ymin, *xmax, *ymax;
    int32_t* status;
};

struct PlanArgs {
    Col C;
    const int64_t* rows;  // null: row i
    int64_t n;
    unsigned long long wave_min;
    int64_t* list;               // lane rows from the front, wave rows from the back
    unsigned long long* counts;  // [0] lane, [1] wave, [2] row indices out of range
};

__global__ void __launch_bounds__(kBlock) k_meas_plan(PlanArgs a) {
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        bool lane = false, wave = false;
        if (i < a.n) {
            const int64_t g = a.rows ? a.rows[i] : i;
            if (g < 0 || g >= a.C.n) {
                atomicAdd(&a.counts[2], 1ull);
            } else {
                uint32_t v0, v1;
                meas::geom_span(a.C.s, (uint32_t)g, v0, v1);
                wave = a.C.status[g] == MOSAIC_ROW_OK && v1 > v0 && (unsigned long long)(v1 - v0) >= a.wave_min;
                lane = !wave;
            }
        }
        const unsigned long long pl = wave_append(&a.counts[0], lane);
        const unsigned long long pw = wave_append(&a.counts[1], wave);
        if (lane) a.list[pl] = i;
        if (wave) a.list[a.n - 1 - (int64_t)pw] = i;
    }
}

struct MeasArgs {
    Col C;
    const int64_t* rows;
    const int64_t* list;
    int64_t n_list;
    Outs o;
    int what, tile;
};

__device__ inline void write_row(const Outs& o, int64_t i, const meas::Measures& m, int32_t st) {
    if (o.area) o.area[i] = m.area;
    if (o.length) o.length[i] = m.length;
    if (o.cx) o.cx[i] = m.cx;
    if (o.cy) o.cy[i] = m.cy;
    if (o.numpoints) o.numpoints[i] = m.numpoints;
    if (o.xmin) o.xmin[i] = m.box.minx;
    if (o.ymin) o.ymin[i] = m.box.miny;
    if (o.xmax) o.xmax[i] = m.box.maxx;
    if (o.ymax) o.ymax[i] = m.box.maxy;
    if (o.status) o.status[i] = st;
}

__global__ void __launch_bounds__(kBlock) k_meas_lane(MeasArgs a) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < a.n_list; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = a.list[k];
        const uint32_t g = (uint32_t)(a.rows ? a.rows[i] : i);
        const int32_t st = a.C.status[g];
        meas::Measures m = {NAN, NAN, NAN, NAN, 0, {NAN, NAN, NAN, NAN}};
        if (st == MOSAIC_ROW_OK) m = meas::measure(a.C.s, a.C.part_kind, g, a.what);
        write_row(a.o, i, m, st);
    }
}

// meas::ccw_up_hi over the calling wave: the greatest i among the rising vertices (y[i] > y[i-1]) of
// the greatest y, if that y >= y[0]; else 0
__device__ inline uint32_t wave_ccw_up_hi(const pip::Vec2* v, uint32_t n, uint32_t lane) {
    double best = -INFINITY;
    uint32_t at = 0;
    for (uint32_t i = 1 + lane; i < n; i += 64) {
        const double py = v[i].y;
        if (py > v[i - 1].y && py >= best) {  // i grows within a lane: >= keeps the last
            best = py;
            at = i;
        }
    }
    for (int off = 32; off; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const uint32_t oa = (uint32_t)__shfl_xor((int)at, off, 64);
        if (oa != 0 && (at == 0 || ob > best || (ob == best && oa > at))) {
            best = ob;
            at = oa;
        }
    }
    return at != 0 && best >= v[0].y ? at : 0;
}

__global__ void __launch_bounds__(64) k_meas_wave(MeasArgs a) {
    __shared__ double s_area[kMaxTile], s_d[kMaxTile], s_mx[kMaxTile], s_my[kMaxTile], s_tx[kMaxTile], s_ty[kMaxTile],
        s_ta[kMaxTile];
    const uint32_t lane = threadIdx.x;
    const uint32_t T = (uint32_t)a.tile;
    const int what = a.what;
    const pip::GeomStore& s = a.C.s;
    for (int64_t k = blockIdx.x; k < a.n_list; k += gridDim.x) {
        const int64_t i = a.list[k];
        const uint32_t g = (uint32_t)(a.rows ? a.rows[i] : i);
        meas::Acc acc;  // lane 0's is the one that counts
        pip::Vec2 base = {0, 0};
        for (uint32_t p = s.geom_part[g]; p < s.geom_part[g + 1]; p++) {
            const uint8_t kind = a.C.part_kind[p];
            for (uint32_t r = s.part_ring[p]; r < s.part_ring[p + 1]; r++) {
                const pip::Vec2* v = s.verts + s.ring_start[r];
                const uint32_t n = s.ring_start[r + 1] - s.ring_start[r];
                if (n == 0) continue;  // uniform
                if (kind == kPartPoint) {
                    if ((what & meas::kCentroid) && lane == 0) acc.add_point(v[0]);
                    continue;
                }
                acc.begin_ring();
                const bool polygon = kind == kPartPolygon, shell = r == s.part_ring[p];
                double sign = 1.0;
                if (polygon && (what & meas::kCentroid)) {
                    if (shell) base = v[0];
                    const bool ccw = n < 4 ? false : meas::ccw_from_up_hi(v, n, wave_ccw_up_hi(v, n, lane));
                    sign = meas::ring_sign(shell, ccw);
                }
                for (uint32_t f0 = 0; f0 + 1 < n; f0 += T) {
                    const uint32_t cnt = n - 1 - f0 < T ? n - 1 - f0 : T;
                    __syncthreads();  // lane 0 is done with the previous tile
                    for (uint32_t t = lane; t < cnt; t += 64) {
                        const uint32_t q = f0 + t;
                        const pip::Vec2 p1 = v[q], p2 = v[q + 1];
                        if (polygon && (what & meas::kArea) && q >= 1) s_area[t] = meas::area_term(v, q);
                        if (polygon && (what & meas::kCentroid)) meas::tri_terms(base, p1, p2, sign, s_tx[t], s_ty[t], s_ta[t]);
                        if (what & (meas::kLength | meas::kCentroid)) meas::line_terms(p1, p2, s_d[t], s_mx[t], s_my[t]);
                    }
                    __syncthreads();
                    if (lane == 0) {
                        for (uint32_t t = 0; t < cnt; t++) {
                            if (polygon && (what & meas::kArea) && f0 + t >= 1) acc.add_area_term(s_area[t]);
                            if (polygon && (what & meas::kCentroid)) acc.add_tri(s_tx[t], s_ty[t], s_ta[t]);
                            if (what & meas::kLength) acc.add_len(s_d[t]);
                            if (what & meas::kCentroid) acc.add_seg(s_d[t], s_mx[t], s_my[t]);
                        }
                    }
                }
                if (polygon)
                    acc.end_polygon_ring(shell, n, v[0], what);
                else
                    acc.end_line(v[0], what);
            }
            acc.end_part();
        }
        if (lane == 0) {
            meas::Measures m;
            meas::stored(s, g, m);
            m.area = acc.area;
            m.length = acc.length;
            acc.centroid(m.cx, m.cy);
            write_row(a.o, i, m, MOSAIC_ROW_OK);
        }
    }
}

}  // namespace

extern "C" {

int mosaic_st_measures(mosaic_ctx* ctx, const mosaic_geoms* geoms, const int64_t* rows, int64_t n, double* area,
                       double* length, double* centroid_x, double* centroid_y, int64_t* numpoints, double* xmin,
                       double* ymin, double* xmax, double* ymax, int32_t* status) {
    if (!ctx || !geoms || n < 0) return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
    if (!rows && n > geoms->n_geoms) return mosaic_tess_fail(MOSAIC_E_ARG, "st_measures: more rows than the column has");
    if (geoms->n_geoms >= 0xffffffffll || geoms->n_vertices >= 0xffffffffll)
        return mosaic_tess_fail(MOSAIC_E_ARG, "st_measures: a column beyond the store's 32-bit offsets");
    int tile = 256;
    int64_t wave_min = 128;
    dev::Exec ex;
    MOSAIC_RC(dev::enter(ctx, &ex));
    MOSAIC_RC(mosaic_ctx_meas_options(ctx, &tile, &wave_min));
    if (geoms->device != ex.device) return mosaic_tess_fail(MOSAIC_E_ARG, "st_measures: a geometry column of another device");
    t_last[0] = t_last[1] = 0;
    if (n == 0) return MOSAIC_OK;
    tile = std::max(1, std::min(tile, kMaxTile));
    hipStream_t stream = ex.stream;

    Buf s_rows, s_list, s_counts;
    PlanArgs pa{view(geoms), nullptr, n, (unsigned long long)std::max<int64_t>(wave_min, 0), nullptr, nullptr};
    if (rows) MOSAIC_RC(dev::on_device(rows, n, s_rows, stream, &pa.rows));
    MOSAIC_RC(s_list.reserve((size_t)n * sizeof(int64_t)));
    MOSAIC_RC(s_counts.reserve(4 * sizeof(unsigned long long)));
    MOSAIC_HIP(hipMemsetAsync(s_counts.p, 0, 4 * sizeof(unsigned long long), stream));
    pa.list = (int64_t*)s_list.p;
    pa.counts = (unsigned long long*)s_counts.p;
    const int64_t wide = (int64_t)ex.n_cu * 16;
    hipLaunchKernelGGL(k_meas_plan, dim3(blocks_for(n, kBlock, wide)), dim3(kBlock), 0, stream, pa);
    MOSAIC_HIP(hipGetLastError());
    unsigned long long counts[4] = {0, 0, 0, 0};
    MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, sizeof(counts), hipMemcpyDeviceToHost, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    if (counts[2])
        return mosaic_tess_fail(MOSAIC_E_ARG, ("st_measures: " + std::to_string(counts[2]) + " row(s) outside the column").c_str());

    OutSlot<double> o_area, o_len, o_cx, o_cy, o_x0, o_y0, o_x1, o_y1;
    OutSlot<int64_t> o_np;
    OutSlot<int32_t> o_st;
    MOSAIC_RC(o_area.bind(area, n));
    MOSAIC_RC(o_len.bind(length, n));
    MOSAIC_RC(o_cx.bind(centroid_x, n));
    MOSAIC_RC(o_cy.bind(centroid_y, n));
    MOSAIC_RC(o_np.bind(numpoints, n));
    MOSAIC_RC(o_x0.bind(xmin, n));
    MOSAIC_RC(o_y0.bind(ymin, n));
    MOSAIC_RC(o_x1.bind(xmax, n));
    MOSAIC_RC(o_y1.bind(ymax, n));
    MOSAIC_RC(o_st.bind(status, n));
    const int what = (area ? meas::kArea : 0) | (length ? meas::kLength : 0) | (centroid_x || centroid_y ? meas::kCentroid : 0);
    MeasArgs ma{pa.C, pa.rows, pa.list, (int64_t)counts[0],
                Outs{o_area.dev, o_len.dev, o_cx.dev, o_cy.dev, o_np.dev, o_x0.dev, o_y0.dev, o_x1.dev, o_y1.dev, o_st.dev},
                what, tile};
    if (counts[0]) {
        hipLaunchKernelGGL(k_meas_lane, dim3(blocks_for((int64_t)counts[0], kBlock, wide)), dim3(kBlock), 0, stream, ma);
        MOSAIC_HIP(hipGetLastError());
    }
    if (counts[1]) {
        ma.list = pa.list + (n - (int64_t)counts[1]);
        ma.n_list = (int64_t)counts[1];
        hipLaunchKernelGGL(k_meas_wave, dim3((unsigned)std::min<int64_t>(ma.n_list, (int64_t)1 << 20)), dim3(64), 0, stream, ma);
        MOSAIC_HIP(hipGetLastError());
    }
    MOSAIC_RC(o_area.back(n, stream));
    MOSAIC_RC(o_len.back(n, stream));
    MOSAIC_RC(o_cx.back(n, stream));
    MOSAIC_RC(o_cy.back(n, stream));
    MOSAIC_RC(o_np.back(n, stream));
    MOSAIC_RC(o_x0.back(n, stream));
    MOSAIC_RC(o_y0.back(n, stream));
    MOSAIC_RC(o_x1.back(n, stream));
    MOSAIC_RC(o_y1.back(n, stream));
    MOSAIC_RC(o_st.back(n, stream));
    MOSAIC_HIP(hipStreamSynchronize(stream));
    t_last[0] = (int64_t)counts[0];
    t_last[1] = (int64_t)counts[1];
    return MOSAIC_OK;
}

int mosaic_st_measures_last_split(int64_t* one_lane, int64_t* wave) {
    if (one_lane) *one_lane = t_last[0];
    if (wave) *wave = t_last[1];
    return MOSAIC_OK;
}

}  // extern "C"
