// lcty_bitonic.hpp — the bitonic sorting network over P items in LDS, P a power of two: the vote keys of
// map_seed_kernel (lcty_map.hip), the minimizer lists of db_sort_kernel (lcty_db.hip), the (key, index) survivors of sel_sort_kernel
// (lcty_select.hip). The kernel loads its items, pads them to P with a value that sorts last and synchronises; all THREADS threads of
// the workgroup then call bitonic_sort_lds. It ends on a barrier: the items are in ascending order for every thread.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace lcty {

// cx(lo, hi, up): order the items at LDS positions lo < hi, the smaller first iff up
template <uint32_t THREADS, typename CompareExchange>
__device__ inline void bitonic_sort_lds(uint32_t P, CompareExchange cx) {
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < P / 2; t += THREADS) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                cx(lo, hi, (lo & size) == 0);
            }
            __syncthreads();
        }
}

// keys alone
struct BitonicKeys {
    uint64_t* key;
    __device__ void operator()(uint32_t lo, uint32_t hi, bool up) const {
        const uint64_t a = key[lo], b = key[hi];
        if ((a > b) == up) { key[lo] = b; key[hi] = a; }
    }
};
// keys with a 32-bit payload, ordered by (key, payload)
struct BitonicKeyIx {
    uint64_t* key; uint32_t* ix;
    __device__ void operator()(uint32_t lo, uint32_t hi, bool up) const {
        const uint64_t ka = key[lo], kb = key[hi];
        const uint32_t ia = ix[lo], ib = ix[hi];
        const bool a_after_b = ka > kb || (ka == kb && ia > ib);
        if (a_after_b == up) { key[lo] = kb; key[hi] = ka; ix[lo] = ib; ix[hi] = ia; }
    }
};

}  // namespace lcty
