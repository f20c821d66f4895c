// lcty_sort.hpp — exclusive prefix sums of 32-bit counts and the passes of a stable least-significant-digit radix sort of 64-bit keys
// (with or without a 64-bit value each), eight bits a pass: the k-mer index of the read mapper (lcty_map_index.hip) and the variant
// ranges of lcty_pafvcf.hip. A pass: sort_count_kernel over tiles of SORT_TILE pairs into counts[256][n_tiles], exclusive_scan of those
// cells, sort_scatter_kernel. At most 2^32 - 1 pairs (the offsets are 32-bit).
// One definition in source, a copy per includer: the kernels and host functions below sit in an anonymous namespace, so every translation
// unit that includes this header compiles its own code objects of them. Both users call all of them; an includer that uses only some gets
// unused-function warnings and dead copies — split the header then.
#pragma once

#include "lcty_common.hpp"
#include "lcty_device.hpp"

namespace lcty {
namespace {

// ---- exclusive prefix sums of 32-bit counts: out[i] = in[0] + .. + in[i - 1]
constexpr uint32_t SCAN_CHUNK = 4096;          // entries per workgroup: 256 threads x 16
__global__ __launch_bounds__(256) void scan_chunk_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * SCAN_CHUNK + threadIdx.x * 16ull;
    uint32_t v[16], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) { v[j] = first + j < n ? in[first + j] : 0u; mine += v[j]; }
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t up = __shfl_up(incl, o); if ((threadIdx.x & 63u) >= static_cast<uint32_t>(o)) incl += up; }
    if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wsum[w];
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) { if (first + j < n) out[first + j] = before; before += v[j]; }
    if (threadIdx.x == 255) sums[blockIdx.x] = before;
}
__global__ __launch_bounds__(256) void scan_add_kernel(uint32_t* __restrict__ out, uint64_t n, const uint32_t* __restrict__ chunk_before) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] += chunk_before[i / SCAN_CHUNK];
}
// scratch: at least scan_scratch_words(n) words
inline size_t scan_scratch_words(uint64_t n) {
    size_t words = 0;
    while (n > 1) { n = (n + SCAN_CHUNK - 1) / SCAN_CHUNK; words += 2 * n; if (n == 1) break; }
    return words + 2;
}
inline void exclusive_scan(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* scratch, hipStream_t s) {
    if (!n) return;
    const uint64_t chunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    uint32_t* sums = scratch, * before = scratch + chunks;
    hipLaunchKernelGGL(scan_chunk_kernel, dim3(static_cast<uint32_t>(chunks)), dim3(256), 0, s, in, out, n, sums);
    if (chunks > 1) {
        exclusive_scan(sums, before, chunks, scratch + 2 * chunks, s);
        hipLaunchKernelGGL(scan_add_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, out, n, before);
    }
    LCTY_HIP(hipGetLastError());
}

// ---- one pass of the stable radix sort of (key, value) pairs by the eight bits of the key from `shift` up (vals_in / vals_out null: keys alone)
constexpr uint32_t SORT_TILE = 4096;           // pairs per wavefront
__global__ __launch_bounds__(64) void sort_count_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint32_t shift, uint32_t* __restrict__ counts,
                                                        uint32_t n_tiles) {
    __shared__ uint32_t h[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t d = lane; d < 256; d += 64) h[d] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * SORT_TILE;
    for (uint32_t r = 0; r < SORT_TILE / 64; r++) {
        const uint64_t i = base + r * 64ull + lane;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 0xFFu], 1u);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t d = lane; d < 256; d += 64) counts[static_cast<size_t>(d) * n_tiles + blockIdx.x] = h[d];
}
__global__ __launch_bounds__(64) void sort_scatter_kernel(const uint64_t* __restrict__ keys_in, const uint64_t* __restrict__ vals_in,
                                                          uint64_t* __restrict__ keys_out, uint64_t* __restrict__ vals_out, uint64_t n, uint32_t shift,
                                                          const uint32_t* __restrict__ first, uint32_t n_tiles) {
    __shared__ uint32_t next[256];             // where the tile's next pair of every digit value goes
    const uint32_t lane = threadIdx.x;
    for (uint32_t d = lane; d < 256; d += 64) next[d] = first[static_cast<size_t>(d) * n_tiles + blockIdx.x];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * SORT_TILE;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < SORT_TILE / 64; r++) {
        const uint64_t i = base + r * 64ull + lane;
        const bool valid = i < n;
        const uint64_t k = valid ? keys_in[i] : 0ull, v = valid && vals_in ? vals_in[i] : 0ull;
        const uint32_t d = static_cast<uint32_t>(k >> shift) & 0xFFu;
        unsigned long long peers = __ballot(valid);                      // the lanes of this step with my digit value
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long vote = __ballot(valid && bit);
            peers &= bit ? vote : ~vote;
        }
        const uint32_t rank = static_cast<uint32_t>(__popcll(peers & below));
        const int leader = valid ? __ffsll(static_cast<long long>(peers)) - 1 : static_cast<int>(lane);
        uint32_t at = 0;
        if (valid && static_cast<int>(lane) == leader) { at = next[d]; next[d] = at + static_cast<uint32_t>(__popcll(peers)); }
        at = static_cast<uint32_t>(__shfl(static_cast<int>(at), leader));
        if (valid) { keys_out[at + rank] = k; if (vals_out) vals_out[at + rank] = v; }
    }
}

}  // namespace
}  // namespace lcty
