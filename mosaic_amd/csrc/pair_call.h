// The host side of a call of a pair predicate (mosaic_st_distance, mosaic_st_intersects,
// mosaic_st_contains_geoms): everything around the kernel launches, which each entry writes out itself.
//
//     pairs::Call<T> c;                          T: the element type of out[]
//     MOSAIC_RC(c.open("st_x", ...));            the checks, in the order every entry has had them
//     (reset the entry's last-call record)  if (n_pairs == 0) return MOSAIC_OK;
//     MOSAIC_RC(c.stage(n_counters));            then launch the plan kernel on c.pa
//     MOSAIC_RC(c.planned());                    counts[] on the host; nothing is written to out / status
//                                                before this has seen that no row index was out of range
//     MOSAIC_RC(c.bind(out, status));            then the fill, small and block kernels on c.out.dev / c.status.dev
//     MOSAIC_RC(c.finish(again));                the copies back; again: counts[] is read once more
#pragma once
#include "dev_rt.h"
#include "pair_lists.h"

namespace mosaic {
namespace pairs {

constexpr int kMaxCounters = 8;

template <class T>
struct Call {
    const char* name = "";
    dev::Exec ex;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    int tile = 16, prune = 1;
    int n_counters = 0;
    PlanArgs pa{};
    unsigned long long counts[kMaxCounters] = {};  // kCntSmall, kCntBlock, kCntBadRow, then the predicate's own
    dev::Buf s_lrow, s_rrow, s_plan, s_list, s_counts;
    dev::OutSlot<T> out;
    dev::OutSlot<int32_t> status;

    int fail(const std::string& what) const { return mosaic_tess_fail(MOSAIC_E_ARG, (std::string(name) + ": " + what).c_str()); }

    // null / shape checks, then dev::enter, then the options, then the device check
    int open(const char* entry, mosaic_ctx* ctx, const mosaic_geoms* left, const mosaic_geoms* right, const int64_t* left_row,
             const int64_t* right_row, int64_t n_pairs, const T* out_arg) {
        name = entry;
        if (!ctx || !left || !right || n_pairs < 0 || (n_pairs > 0 && !out_arg))
            return mosaic_tess_fail(MOSAIC_E_ARG, "invalid argument");
        if ((left_row == nullptr) != (right_row == nullptr)) return fail("left_row and right_row are both given or both null");
        if (!left_row && (n_pairs > left->n_geoms || n_pairs > right->n_geoms))
            return fail("row-wise form with more pairs than rows");
        int64_t small_work = 512;
        MOSAIC_RC(dev::enter(ctx, &ex));
        MOSAIC_RC(mosaic_ctx_dist_options(ctx, &tile, &small_work, &prune));
        if (left->device != ex.device || right->device != ex.device) return fail("a geometry column of another device");
        tile = std::max(1, std::min(tile, kMaxTile));
        stream = ex.stream;
        n = n_pairs;
        pa = PlanArgs{{view(left), view(right), left_row, right_row}, n, (unsigned long long)std::max<int64_t>(small_work, 0),
                      nullptr, nullptr, nullptr};
        return MOSAIC_OK;
    }

    // the row lists on the device, plan[] and list[] of n pairs, n_counters zeroed counters: pa is complete
    int stage(int counters) {
        n_counters = counters;
        if (pa.lrow) {
            MOSAIC_RC(dev::on_device(pa.lrow, n, s_lrow, stream, &pa.lrow));
            MOSAIC_RC(dev::on_device(pa.rrow, n, s_rrow, stream, &pa.rrow));
        }
        MOSAIC_RC(s_plan.reserve((size_t)n * sizeof(int32_t)));
        MOSAIC_RC(s_list.reserve((size_t)n * sizeof(int64_t)));
        MOSAIC_RC(s_counts.reserve(n_counters * sizeof(unsigned long long)));
        MOSAIC_HIP(hipMemsetAsync(s_counts.p, 0, n_counters * sizeof(unsigned long long), stream));
        pa.plan = s_plan.as<int32_t>();
        pa.list = s_list.as<int64_t>();
        pa.counts = s_counts.as<unsigned long long>();
        return MOSAIC_OK;
    }

    int read_counts() {
        MOSAIC_HIP(hipMemcpyAsync(counts, s_counts.p, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        return MOSAIC_OK;
    }

    // after the plan launch
    int planned() {
        MOSAIC_RC(read_counts());
        MOSAIC_HIP(hipStreamSynchronize(stream));
        if (counts[kCntBadRow]) return fail(std::to_string(counts[kCntBadRow]) + " pair(s) name a row outside their column");
        return MOSAIC_OK;
    }

    int bind(T* out_arg, int32_t* status_arg) {
        MOSAIC_RC(out.bind(out_arg, n));
        return status.bind(status_arg, n);
    }

    int finish(bool counts_again) {
        MOSAIC_RC(out.back(n, stream));
        MOSAIC_RC(status.back(n, stream));
        if (counts_again) MOSAIC_RC(read_counts());
        MOSAIC_HIP(hipStreamSynchronize(stream));
        return MOSAIC_OK;
    }

    int64_t n_small() const { return (int64_t)counts[kCntSmall]; }
    int64_t n_block() const { return (int64_t)counts[kCntBlock]; }
    ListArgs small_list() const { return ListArgs{pa, pa.list, n_small()}; }
    ListArgs block_list() const { return ListArgs{pa, pa.list + (n - n_block()), n_block()}; }
    // the grid of a one-lane-per-item kernel over m items, and of a one-workgroup-per-item kernel
    dim3 lanes(int64_t m) const { return dim3(dev::blocks_for(m, kBlock, (int64_t)ex.n_cu * 16)); }
    static dim3 groups(int64_t m) { return dim3((unsigned)std::min<int64_t>(m, (int64_t)1 << 20)); }
};

}  // namespace pairs
}  // namespace mosaic
