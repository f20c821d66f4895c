// lcty_text.hpp — what the kernels that write text lines share (lcty_pafvcf.hip: the records of paf-vcf; lcty_gtvcf.hip: the records of a
// cohort's genotypes): decimal digits, the sum of a workgroup and the place of every thread's bytes inside a chunk of its workgroup.
#pragma once

#include "lcty_device.hpp"
#include "lcty_scan.hpp"

namespace lcty {

__host__ __device__ inline uint32_t n_digits(uint64_t x) { uint32_t d = 1; while (x >= 10) { x /= 10; d++; } return d; }
__host__ __device__ inline void put_digits(char* at, uint64_t x, uint32_t d) { for (uint32_t i = d; i-- > 0;) { at[i] = char('0' + x % 10); x /= 10; } }

// sum over a workgroup of THREADS threads; every thread gets it. part: THREADS / WAVE words of LDS.
template <int THREADS> __device__ inline uint64_t block_sum(uint64_t x, uint64_t* part) {
    for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off);
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = x;
    __syncthreads();
    uint64_t t = 0;
    for (int w = 0; w < THREADS / WAVE; w++) t += part[w];
    return t;
}

// Thread t of a workgroup of THREADS threads has w bytes to write behind those of the threads before it: returns the bytes before its own,
// *all = the bytes of the whole workgroup. wsum: THREADS / WAVE words of LDS. Every thread calls it; sums stay below 2^32.
template <int THREADS> __device__ inline uint32_t block_place(uint32_t w, uint32_t* wsum, uint32_t* all) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const uint32_t incl = wave_scan_incl(w, AddOp{});
    __syncthreads();
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t k = 0; k < THREADS / WAVE; k++) { if (k < wave) before += wsum[k]; total += wsum[k]; }
    *all = total;
    return before + incl - w;
}

}  // namespace lcty
