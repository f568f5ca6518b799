// The chip-set container behind the C ABI's mosaic_chip_set handle, shared by the chip producers
// (tessellate.cpp, lines_host.cpp).
#pragma once
#include <stdint.h>

#include <memory>
#include <utility>
#include <vector>

// an allocator whose resize() leaves new bytes uninitialised (the writers fill them, in parallel)
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U>&) {}
    template <class U>
    void construct(U* p) noexcept {
        ::new ((void*)p) U;
    }
    template <class U, class... A>
    void construct(U* p, A&&... args) {
        ::new ((void*)p) U(std::forward<A>(args)...);
    }
};

struct mosaic_chip_set {
    std::vector<uint8_t> is_core;
    std::vector<int64_t> index_id;
    std::vector<int32_t> key;
    std::vector<int64_t> wkb_offsets{0};
    std::vector<uint8_t, NoInitAlloc<uint8_t>> wkb;
    void add(bool core, int64_t id, int32_t k, const std::vector<uint8_t>& blob) {
        is_core.push_back(core);
        index_id.push_back(id);
        key.push_back(k);
        wkb.insert(wkb.end(), blob.begin(), blob.end());
        wkb_offsets.push_back((int64_t)wkb.size());
    }
};

