// orb_layout.h -- how an ORBmatcher search (orb_matchers.cpp) carves a device buffer into regions.  A search
// names each region once, with its element type and count: `field = layout.add<T>(n)`.  Over an empty
// layout (base 0) that only sizes the buffer -- `bytes` is what it must hold -- and over the buffer itself
// it yields the region's address.  Size arithmetic only (no HIP), so the host harness checks it on the CPU
// (tests/test_host_harness.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace orbgpu {

constexpr size_t kSlotAlign = 256;  // every slot starts on it (the uint4 loads of f_desc / kf_desc rely on it)
constexpr size_t kSlotSlack = 256;  // bytes behind every slot that belong to no other slot

struct Layout {
    uintptr_t base = 0;  // the buffer (256-byte aligned, as hipMalloc returns it), or 0: sizing only
    size_t bytes = 0;    // the slots so far, the last one's slack included
    // n may be 0: the slot still gets an address of its own.  An optional input the caller did not pass
    // takes no slot: its field stays nullptr.
    template <class T>
    T* add(size_t n) {
        T* const slot = reinterpret_cast<T*>(base + bytes);
        bytes = (bytes + n * sizeof(T) + kSlotSlack + kSlotAlign - 1) & ~(kSlotAlign - 1);
        return slot;
    }
};

}  // namespace orbgpu
