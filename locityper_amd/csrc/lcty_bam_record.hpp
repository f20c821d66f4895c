// lcty_bam_record.hpp — a BAM record on the device, as the readers of a slice of inflated BGZF blocks see it (lcty_sample_bam.hip,
// lcty_bg_fetch.hip, lcty_aln_bam.hip): records lie at any byte of the slice, so every field is taken from two aligned dwords (ld32;
// the slice ends in SLICE_PAD zero bytes, lcty_bgzf_read.hpp). The fixed fields (rec_head, rec_fits), the file order (sort_key), the
// hash and the comparison of read names, and the two gathers every reader ends with: the CIGAR words of records dealt flat over
// the lanes (cigar_gather_kernel) and the unpack of 4-bit base codes (unpack_kernel).
#pragma once

#include "lcty_device.hpp"

namespace lcty {

constexpr uint32_t NONE32 = 0xFFFFFFFFu;

// four bytes from byte `off` of the slice (the dword behind the last one is inside SLICE_PAD)
__device__ __forceinline__ uint32_t ld32(const uint32_t* w, uint64_t off) {
    const uint64_t i = off >> 2;
    const uint64_t v = static_cast<uint64_t>(w[i]) | (static_cast<uint64_t>(w[i + 1]) << 32);
    return static_cast<uint32_t>(v >> ((off & 3u) * 8u));
}
// reference bases of a CIGAR word: M, D, N, =, X
__device__ __forceinline__ uint32_t cigar_ref_len(uint32_t w) { return ((0x18Du >> (w & 15u)) & 1u) ? (w >> 4) : 0u; }

struct RecHead { int32_t tid, pos, mtid, mpos; uint32_t l_name, n_cigar, flag, l_seq, block; };
__device__ __forceinline__ RecHead rec_head(const uint32_t* raw, uint64_t o) {
    RecHead h;
    h.block = ld32(raw, o); h.tid = static_cast<int32_t>(ld32(raw, o + 4)); h.pos = static_cast<int32_t>(ld32(raw, o + 8));
    h.l_name = ld32(raw, o + 12) & 0xFFu;
    const uint32_t nf = ld32(raw, o + 16);
    h.n_cigar = nf & 0xFFFFu; h.flag = nf >> 16;
    h.l_seq = ld32(raw, o + 20); h.mtid = static_cast<int32_t>(ld32(raw, o + 24)); h.mpos = static_cast<int32_t>(ld32(raw, o + 28));
    return h;
}
__device__ __forceinline__ bool rec_fits(const RecHead& h) {
    return 32ull + h.l_name + 4ull * h.n_cigar + (static_cast<uint64_t>(h.l_seq) + 1) / 2 + h.l_seq <= h.block;
}
// file order of two placed records; a record without coordinate (tid < 0) is behind every placed one
__device__ __forceinline__ uint64_t sort_key(int32_t tid, int32_t pos) {
    return tid < 0 ? ~0ull : (static_cast<uint64_t>(static_cast<uint32_t>(tid)) << 32) | static_cast<uint32_t>(pos + 1);
}

// FNV-1a over the name (without its NUL) of the record at byte o, then mixed
__device__ __forceinline__ uint64_t name_hash(const uint32_t* raw, uint64_t o, uint32_t l_name) {
    uint64_t x = 0xcbf29ce484222325ull;
    const uint32_t n = l_name ? l_name - 1 : 0u;
    for (uint32_t j = 0; j < n; j += 4) {
        uint32_t w = ld32(raw, o + 36 + j);
        for (uint32_t b = 0; b < 4 && j + b < n; b++) { x = (x ^ (w & 0xFFu)) * 0x100000001b3ull; w >>= 8; }
    }
    return mix64(x);
}

__device__ inline bool same_name(const uint32_t* raw, uint64_t oa, uint64_t ob) {
    const uint32_t la = ld32(raw, oa + 12) & 0xFFu, lb = ld32(raw, ob + 12) & 0xFFu;
    if (la != lb) return false;
    for (uint32_t j = 0; j < la; j += 4) {
        const uint32_t m = la - j >= 4 ? 0xFFFFFFFFu : (1u << (8 * (la - j))) - 1u;
        if ((ld32(raw, oa + 36 + j) ^ ld32(raw, ob + 36 + j)) & m) return false;
    }
    return true;
}

// CIGAR word j of the output: of the owner k of j among cigar_off[0 .. n), which is record src[k] of the records walked (src null: k)
template <typename Off>
__global__ __launch_bounds__(256) void cigar_gather_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ src,
                                                           const Off* __restrict__ cigar_off, uint32_t n, uint32_t n_words, uint32_t* __restrict__ cigar) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_words) return;
    const uint32_t k = flat_owner(cigar_off, n, j);
    const uint64_t o = rec_off[src ? src[k] : k];
    const uint32_t l_name = ld32(raw, o + 12) & 0xFFu;
    cigar[j] = ld32(raw, o + 36 + l_name + 4ull * (j - cigar_off[k]));
}

__device__ __forceinline__ uint32_t swap_nibbles(uint32_t x) { return ((x & 0x0F0F0F0Fu) << 4) | ((x >> 4) & 0x0F0F0F0Fu); }

// unit u = 32 bases of one sequence = one 64-bit word of bases2 and one word of nmask; sequence m is SEQ of record src[m], its units
// start at unit_off[m]. RESTORE: a reverse record (flag 0x10) is laid out back to front and complemented, as the sequencer gave it;
// without it the bases are those of the file. Every code but A, C, G, T ('=' included) sets the bit of nmask. A lane writes whole
// words of its own only.
template <bool RESTORE>
__global__ __launch_bounds__(256) void unpack_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ src,
                                                     const uint32_t* __restrict__ unit_off, uint32_t n_mates, uint32_t n_units,
                                                     uint64_t* __restrict__ bases2, uint32_t* __restrict__ nmask) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= n_units) return;
    const uint32_t m = flat_owner(unit_off, n_mates, u), q = u - unit_off[m];   // the mate whose units hold u
    const uint64_t o = rec_off[src[m]];
    const uint32_t l_name = ld32(raw, o + 12) & 0xFFu, nf = ld32(raw, o + 16), L = ld32(raw, o + 20);
    const bool reverse = RESTORE && ((nf >> 16) & 0x10u) != 0;
    const uint32_t n = min(32u, L - 32u * q);
    const uint32_t a = reverse ? L - 32u * q - n : 32u * q;                      // first base of the record this unit reads
    const uint64_t b0 = o + 36 + l_name + 4ull * (nf & 0xFFFFu) + (a >> 1);
    // 17 bytes at most; base a + t at bits 4 t of (lo, hi) once the nibbles of every byte are swapped and an odd start is shifted out
    const uint32_t d0 = swap_nibbles(ld32(raw, b0)), d1 = swap_nibbles(ld32(raw, b0 + 4)), d2 = swap_nibbles(ld32(raw, b0 + 8)),
                   d3 = swap_nibbles(ld32(raw, b0 + 12)), d4 = swap_nibbles(ld32(raw, b0 + 16));
    uint64_t lo = d0 | (static_cast<uint64_t>(d1) << 32), hi = d2 | (static_cast<uint64_t>(d3) << 32);
    if (a & 1u) { lo = (lo >> 4) | (hi << 60); hi = (hi >> 4) | (static_cast<uint64_t>(d4) << 60); }
    uint64_t bases = 0; uint32_t mask = 0;
#pragma unroll
    for (uint32_t t = 0; t < 32; t++) {
        if (t < n) {
            const uint32_t code = static_cast<uint32_t>((t < 16 ? lo >> (4 * t) : hi >> (4 * (t - 16))) & 15ull);
            const uint32_t e = code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : 4u;     // =ACMGRSVTWYHKDBN
            const uint32_t at = reverse ? n - 1u - t : t;
            if (e > 3u) mask |= 1u << at;
            else bases |= static_cast<uint64_t>(reverse ? 3u - e : e) << (2u * at);
        }
    }
    bases2[u] = bases; nmask[u] = mask;
}

}  // namespace lcty
