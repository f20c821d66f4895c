// lcty_sort.hip — the device primitives that span workgroups: exclusive prefix sums of 32-bit counts (lcty_scan.hpp:
// exclusive_scan, ScanTotal) and the stable radix sort of lcty_sort.hpp. A pass of the sort: sort_count_kernel over tiles of SORT_TILE
// pairs into counts[256][n_tiles], exclusive_scan of those cells in (digit, tile) order — the first place in the output of every (digit
// value, tile) —, sort_scatter_kernel.
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"

namespace lcty {

// ---- exclusive prefix sums of 32-bit counts: out[i] = in[0] + .. + in[i - 1]
constexpr uint32_t SCAN_CHUNK = 4096;          // entries per workgroup: 256 threads x 16
__global__ __launch_bounds__(256) void scan_chunk_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t wsum[4];
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * SCAN_CHUNK + threadIdx.x * 16ull;
    uint32_t v[16], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) { v[j] = first + j < n ? in[first + j] : 0u; mine += v[j]; }
    const uint32_t incl = wave_scan_incl(mine, AddOp{});
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
size_t scan_scratch_words(uint64_t n) {
    size_t words = 0;
    while (n > 1) { n = (n + SCAN_CHUNK - 1) / SCAN_CHUNK; words += 2 * n; if (n == 1) break; }
    return words + 2;
}
void exclusive_scan(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* scratch, hipStream_t s) {
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

uint32_t ScanTotal::run(const DevBuf<uint32_t>& in, DevBuf<uint32_t>& out, uint64_t n, lcty_ctx* ctx) {
    hipStream_t s = ctx->stream;
    if (n >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%llu items to scan (32-bit offsets)", static_cast<unsigned long long>(n));
    out.alloc(n + 1);
    uint32_t total = 0;
    if (n) {
        tmp.ensure(scan_scratch_words(n));
        exclusive_scan(in.p, out.p, n, tmp.p, s);
        uint32_t last_out = 0, last_in = 0;
        out.download(&last_out, 1, s, n - 1); in.download(&last_in, 1, s, n - 1);
        LCTY_HIP(hipStreamSynchronize(s));
        if (uint64_t(last_out) + last_in >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "more than 2^31 items (32-bit offsets)");
        total = last_out + last_in;
    }
    out.upload(&total, 1, s, n);
    LCTY_HIP(hipStreamSynchronize(s));                                  // `total` leaves the stack
    return total;
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

int RadixSort::run(uint64_t* keys_a, uint64_t* vals_a, uint64_t* keys_b, uint64_t* vals_b, uint64_t n, const std::vector<uint32_t>& shifts, hipStream_t s) {
    const int where = static_cast<int>(shifts.size() & 1);
    if (!n) return where;
    const uint32_t n_tiles = static_cast<uint32_t>((n + SORT_TILE - 1) / SORT_TILE);
    const uint64_t cells = 256ull * n_tiles;
    counts.ensure(cells); first.ensure(cells); tmp.ensure(scan_scratch_words(cells));
    for (uint32_t shift : shifts) {
        hipLaunchKernelGGL(sort_count_kernel, dim3(n_tiles), dim3(64), 0, s, keys_a, n, shift, counts.p, n_tiles);
        exclusive_scan(counts.p, first.p, cells, tmp.p, s);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3(n_tiles), dim3(64), 0, s, keys_a, vals_a, keys_b, vals_b, n, shift, first.p, n_tiles);
        LCTY_HIP(hipGetLastError());
        std::swap(keys_a, keys_b); std::swap(vals_a, vals_b);
    }
    return where;
}

}  // namespace lcty
