// lcty_scan.hpp — in-order scans and the wavefront's reduction, one definition each: of a wavefront (wave_scan_incl,
// every kernel that ranks or places the items of its lanes; wave_reduce, the minima, maxima and sums of lcty_score.hip, lcty_gram.hip
// and lcty_bg.hip: their kernels compile to the same registers, occupancy and scratch through it, so none of those loops stays written
// out), of one workgroup with any operation (launch_scan: sums and running maxima of lcty_panvcf.hip and
// lcty_pafvcf.hip) and of any number of workgroups over 32-bit counts (exclusive_scan, ScanTotal: the radix sort of lcty_sort.hpp, the
// run starts of lcty_map_index.hip, the offsets of lcty_pafvcf.hip; defined in lcty_sort.hip).
// Two loops scan two values per step with one shuffle pair each and stay as they are written: the anchor ranks of
// lcty_solve_kernels.hip and the (count, extent) pair of lcty_basis.hip. Four one-value loops of the measured path also stay written
// out (lcty_map.hip, lcty_map_internal.hpp, lcty_map_long.hip, lcty_transfer.hip): their kernels compile differently through a function.
#pragma once

#include "lcty_common.hpp"
#include "lcty_device.hpp"

namespace lcty {

constexpr int SCAN_THREADS = 1024;

struct AddOp { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
// doubles take fmax / fmin: a NaN loses to a number, as in the reference's f64::max / f64::min
struct MaxOp {
    template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
};
struct MinOp {
    template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; }
    __device__ double operator()(double a, double b) const { return fmin(a, b); }
};

// what a scan reads: element i of an array, widened where the sums need it
struct LoadU32 { const uint32_t* p; __device__ uint32_t operator()(uint64_t i) const { return p[i]; } };
struct LoadU64 { const uint64_t* p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };
struct LoadU32AsU64 { const uint32_t* p; __device__ uint64_t operator()(uint64_t i) const { return p[i]; } };

// Inclusive scan over the 64 lanes of the calling wavefront, lane order: lane l gets op(x of lane 0, .., x of lane l). Every lane of the
// wavefront calls it (the shuffles read inactive lanes otherwise); the wavefronts of a workgroup do not see each other.
template <typename T, typename Op> __device__ inline T wave_scan_incl(T x, Op op) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    for (int off = 1; off < WAVE; off <<= 1) {
        const T y = __shfl_up(x, off);
        if (lane >= uint32_t(off)) x = op(y, x);
    }
    return x;
}

// Reduction over the 64 lanes of the calling wavefront: EVERY lane gets op over all 64 values (a butterfly of xor shuffles; sums of
// doubles are added in that order, the same in every lane). Every lane of the wavefront calls it.
template <typename T, typename Op> __device__ inline T wave_reduce(T x, Op op) {
    for (int off = WAVE / 2; off > 0; off >>= 1) x = op(x, __shfl_xor(x, off));
    return x;
}

// One workgroup scans n values in order (launched with grid 1): exclusive writes out[0 .. n] (out[n] = the total), inclusive out[0 .. n - 1].
template <typename T, typename Load, typename Op>
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(uint64_t n, Load load, Op op, T identity, T* __restrict__ out, bool exclusive) {
    __shared__ T wsum[SCAN_THREADS / WAVE];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    T carry = identity;
    for (uint64_t base = 0; base < n; base += SCAN_THREADS) {
        const uint64_t i = base + tid;
        const T x = i < n ? load(i) : identity;
        const T incl = wave_scan_incl(x, op);
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

// ---- exclusive prefix sums of 32-bit counts over any number of workgroups: out[i] = in[0] + .. + in[i - 1], i < n (sums wrap at 2^32;
// in and out may not overlap). Chunks of 4 096, their sums scanned by the same code one level up and added back.
// scratch: at least scan_scratch_words(n) words. Asynchronous on s.
size_t scan_scratch_words(uint64_t n);
void exclusive_scan(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* scratch, hipStream_t s);

// exclusive_scan with its scratch, and the total: `out` is (re)allocated to n + 1 words and out[n] receives the total, which is also
// returned. Offsets stay below 2^31 - 16: LCTY_ERR_UNSUPPORTED for more items or a larger total. Synchronises the context's stream
// twice (the total comes to the host, and goes back from the stack).
struct ScanTotal {
    DevBuf<uint32_t> tmp;
    uint32_t run(const DevBuf<uint32_t>& in, DevBuf<uint32_t>& out, uint64_t n, lcty_ctx* ctx);
};

}  // namespace lcty
