// lcty_scan.hpp — in-order scans of one workgroup with any operation (sums, running maxima), used by lcty_panvcf.hip and lcty_pafvcf.hip.
#pragma once

#include "lcty_common.hpp"
#include "lcty_device.hpp"

namespace lcty {

constexpr int SCAN_THREADS = 1024;

template <typename T> __device__ inline T wave_scan_incl_add(T x) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    for (int off = 1; off < WAVE; off <<= 1) {
        const T y = __shfl_up(x, off);
        if (lane >= uint32_t(off)) x += y;
    }
    return x;
}

struct AddOp { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct MaxOp { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };

// One workgroup scans n values in order (launched with grid 1): exclusive writes out[0 .. n] (out[n] = the total), inclusive out[0 .. n - 1].
template <typename T, typename Load, typename Op>
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(uint64_t n, Load load, Op op, T identity, T* __restrict__ out, bool exclusive) {
    __shared__ T wsum[SCAN_THREADS / WAVE];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    T carry = identity;
    for (uint64_t base = 0; base < n; base += SCAN_THREADS) {
        const uint64_t i = base + tid;
        const T x = i < n ? load(i) : identity;
        T incl = x;
        for (int off = 1; off < WAVE; off <<= 1) {
            const T y = __shfl_up(incl, off);
            if (lane >= uint32_t(off)) incl = op(y, incl);
        }
        if (lane == WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        T before = carry;
        for (uint32_t w = 0; w < wave; w++) before = op(before, wsum[w]);
        T all = carry;
        for (uint32_t w = 0; w < SCAN_THREADS / WAVE; w++) all = op(all, wsum[w]);
        const T prev = __shfl_up(incl, 1);                              // every lane takes part
        if (i < n) out[i] = !exclusive ? op(before, incl) : lane ? op(before, prev) : before;
        carry = all;
        __syncthreads();
    }
    if (exclusive && tid == 0) out[n] = carry;
}

template <typename T, typename Load, typename Op>
void launch_scan(hipStream_t s, uint64_t n, Load load, Op op, T identity, T* out, bool exclusive) {
    hipLaunchKernelGGL((scan_kernel<T, Load, Op>), dim3(1), dim3(SCAN_THREADS), 0, s, n, load, op, identity, out, exclusive);
    LCTY_HIP(hipGetLastError());
}

}  // namespace lcty
