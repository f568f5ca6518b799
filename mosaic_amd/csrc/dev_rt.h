// The host scaffolding of a feature translation unit (.hip): the HIP error macro, the owning device
// buffer, the event guard, the grid size, the hipcub wrappers and the entry into a context.
// Host code only: nothing here adds to or changes a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mosaic_hip.h"
#include "fail.h"

// options of a context, read under its lock (defined in mosaic_hip.hip)
extern "C" int mosaic_ctx_gk_options(mosaic_ctx* ctx, int* table_log2, int64_t* max_cells);          // geom_kring.hip
extern "C" int mosaic_ctx_dist_options(mosaic_ctx* ctx, int* tile, int64_t* small_work, int* prune);  // the pair kernels
extern "C" int mosaic_ctx_meas_options(mosaic_ctx* ctx, int* tile, int64_t* wave_min);                // st_measures.hip
extern "C" int mosaic_ctx_within_options(mosaic_ctx* ctx, int* tile, int* slices);                    // the distance-within join

// the one HIP error macro: out of memory is MOSAIC_E_NOMEM, everything else MOSAIC_E_HIP
#define MOSAIC_HIP(expr)                                                         \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) return mosaic::dev::hip_fail(_e, __FILE__, #expr); \
    } while (0)

namespace mosaic {
namespace dev {

inline int hip_fail(hipError_t e, const char* file, const char* expr) {
    return mosaic_tess_fail(e == hipErrorOutOfMemory ? MOSAIC_E_NOMEM : MOSAIC_E_HIP,
                            (std::string(file) + ": " + hipGetErrorString(e) + " at " + expr).c_str());
}

// what a call runs with: mosaic_ctx_exec makes the context's device current and reports these
struct Exec {
    int device = 0;
    hipStream_t stream = nullptr;
    int jdk = 8;
    int n_cu = 256;
};

inline int enter(mosaic_ctx* ctx, Exec* x) {
    void* stream = nullptr;
    MOSAIC_RC(mosaic_ctx_exec(ctx, &x->device, &stream, &x->jdk, &x->n_cu));
    x->stream = (hipStream_t)stream;
    return MOSAIC_OK;
}

// An owning device buffer that only grows.  Growing frees the old block first (hipFree waits for the
// device), so the contents do not survive it; a new block is not initialised.
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() {
        if (p) (void)hipFree(p);
    }
    int reserve(size_t n) {
        n = std::max<size_t>(n, 16);
        if (n <= bytes) return MOSAIC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        if (hipMalloc(&p, n) != hipSuccess)
            return mosaic_tess_fail(MOSAIC_E_NOMEM, ("hipMalloc(" + std::to_string(n) + ") failed").c_str());
        bytes = n;
        return MOSAIC_OK;
    }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};

template <class T>
int upload(Buf& b, const std::vector<T>& v, hipStream_t s) {
    MOSAIC_RC(b.reserve(v.size() * sizeof(T)));
    if (!v.empty()) MOSAIC_HIP(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return MOSAIC_OK;
}

inline bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// src (n elements, host or device) as a device pointer; a host array is copied into `stage`
template <class T>
int on_device(const T* src, int64_t n, Buf& stage, hipStream_t stream, const T** out) {
    if (is_device_ptr(src)) {
        *out = src;
        return MOSAIC_OK;
    }
    MOSAIC_RC(stage.reserve((size_t)n * sizeof(T)));
    MOSAIC_HIP(hipMemcpyAsync(stage.p, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, stream));
    *out = (const T*)stage.p;
    return MOSAIC_OK;
}

// one output array of n elements: the caller's if it is on the device (or null), else a staging block
// that back() copies to the caller at the end
template <class T>
struct OutSlot {
    T* user = nullptr;
    T* dev = nullptr;
    Buf stage;
    int bind(T* p, int64_t n) {
        user = p;
        if (!p) return MOSAIC_OK;
        if (is_device_ptr(p)) {
            dev = p;
            return MOSAIC_OK;
        }
        MOSAIC_RC(stage.reserve((size_t)n * sizeof(T)));
        dev = (T*)stage.p;
        return MOSAIC_OK;
    }
    int back(int64_t n, hipStream_t stream) {
        if (user && user != dev) MOSAIC_HIP(hipMemcpyAsync(user, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, stream));
        return MOSAIC_OK;
    }
};

// N timing events, destroyed on every return path
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    ~Events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int create() {
        for (hipEvent_t& x : e) MOSAIC_HIP(hipEventCreate(&x));
        return MOSAIC_OK;
    }
};

// the grid of a one-lane-per-item kernel of `block` lanes: at least one block, cap_blocks at the most
inline unsigned blocks_for(int64_t n, int block, int64_t cap_blocks) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + block - 1) / block, cap_blocks));
}

// hipcub with its temporary storage in `tmp`, which has to outlive the work on the stream.  n keeps the
// caller's type: hipcub's entry points are templates over it.
template <class K, class V, class N>
int sort_pairs(Buf& tmp, const K* k_in, K* k_out, const V* v_in, V* v_out, N n, int begin_bit, int end_bit, hipStream_t st) {
    size_t bytes = 0;
    MOSAIC_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k_in, k_out, v_in, v_out, n, begin_bit, end_bit, st));
    MOSAIC_RC(tmp.reserve(bytes));
    bytes = tmp.bytes;
    MOSAIC_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, k_in, k_out, v_in, v_out, n, begin_bit, end_bit, st));
    return MOSAIC_OK;
}

template <class In, class Out, class N>
int inclusive_sum(Buf& tmp, In in, Out out, N n, hipStream_t st) {
    size_t bytes = 0;
    MOSAIC_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, bytes, in, out, n, st));
    MOSAIC_RC(tmp.reserve(bytes));
    bytes = tmp.bytes;
    MOSAIC_HIP(hipcub::DeviceScan::InclusiveSum(tmp.p, bytes, in, out, n, st));
    return MOSAIC_OK;
}

template <class In, class Out, class N>
int exclusive_sum(Buf& tmp, In in, Out out, N n, hipStream_t st) {
    size_t bytes = 0;
    MOSAIC_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n, st));
    MOSAIC_RC(tmp.reserve(bytes));
    bytes = tmp.bytes;
    MOSAIC_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, n, st));
    return MOSAIC_OK;
}

}  // namespace dev
}  // namespace mosaic
