// packet_common.hpp — what the packet-side kernel files (kernels_burst / bits / pdu / frame / tx .hip) share.
#pragma once
#include <algorithm>

#include "kernels.hpp"

namespace rr {

// the grid of a kernel whose workgroups stride over `ntiles` tiles: one per tile, at most eight per CU
static inline unsigned tiles_grid(long ntiles) {
    return (unsigned)std::max<long>(1, std::min(ntiles, (long)device_cu_count() * 8));
}

// every thread of the wave calls it: one atomic per wave that wants a slot at all; the list is unordered, and `count` goes on
// past `cap` (the host refuses such a count)
template <class T>
__device__ __forceinline__ void wave_append(bool want, const T& entry, unsigned long long* count, T* list, unsigned long long cap) {
    const unsigned long long m = __ballot(want);
    if (m == 0) return;
    const int lane = threadIdx.x & 63, leader = __ffsll(m) - 1;
    unsigned long long slot = 0;
    if (lane == leader) slot = atomicAdd(count, (unsigned long long)__popcll(m));
    slot = __shfl(slot, leader, 64);
    slot += __popcll(m & ((1ull << lane) - 1ull));
    if (want && slot < cap) list[slot] = entry;
}

}  // namespace rr
