// lcty_bam_layout.hpp — from the kept records of a slice to the mates of the output, shared by the two readers of a sample's BAM file:
// lcty_sample_bam.hip (indexed: pairs by name) and lcty_bam_stream.hip (whole files in windows: single reads, or interleaved pairs).
// The kept records in file order (stream_kernel) and the mates of every read with their lengths in units of 32 bases (assemble_kernel);
// ReadChunk::place (lcty_read_chunk.hpp) makes the offsets of them, and unpack_kernel of lcty_bam_record.hpp ends both.
#pragma once

#include "lcty_bam_record.hpp"

namespace lcty {

// how assemble_kernel finds the mates of a read
enum : int { MATES_SINGLE = 0, MATES_BY_NAME = 1, MATES_INTERLEAVED = 2 };

// kept record r -> place scan[r] of the stream; the sort's input: (hash, stream ordinal)
static __global__ __launch_bounds__(256) void stream_kernel(uint32_t n_rec, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ scan,
                                                            const uint64_t* __restrict__ hash, uint32_t* __restrict__ stream, uint64_t* __restrict__ keys,
                                                            uint64_t* __restrict__ vals) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec || !kept[r]) return;
    const uint32_t s = scan[r];
    stream[s] = r;
    if (keys) { keys[s] = hash[r]; vals[s] = s; }
}

// the mates of the output: src[m] = record of mate m (NONE32: absent), its length, and its length in units of 32 bases.
// MATES_SINGLE: stream place s is read s, mate 2 absent. MATES_BY_NAME: the completing record s of a pair (mate_of[s] its mate) is
// pair pair_ix[s]; mate 1 is the first in template (info). MATES_INTERLEAVED: places 2 i and 2 i + 1 below n_stream are mates 1 and 2
// of pair i, whatever their flags.
static __global__ __launch_bounds__(256) void assemble_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ info,
                                                              const uint32_t* __restrict__ stream, uint32_t n_stream, int paired, const uint32_t* __restrict__ mate_of,
                                                              const uint32_t* __restrict__ pair_ix, uint32_t* __restrict__ src, uint32_t* __restrict__ src_stream,
                                                              uint32_t* __restrict__ mate_len, uint32_t* __restrict__ units) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_stream) return;
    uint32_t p = s, s1 = s, s2 = NONE32;
    if (paired == MATES_BY_NAME) {
        if (mate_of[s] == NONE32) return;
        p = pair_ix[s];
        s2 = mate_of[s];
        if (!(info[stream[s1]] & 0x40u)) { const uint32_t x = s1; s1 = s2; s2 = x; }     // mate 1 is the first in template
    } else if (paired == MATES_INTERLEAVED) {
        if ((s & 1u) || s + 1 >= n_stream) return;
        p = s >> 1; s2 = s + 1;
    }
    const uint32_t r1 = stream[s1], r2 = s2 != NONE32 ? stream[s2] : NONE32;
    src_stream[2 * p] = s1; src_stream[2 * p + 1] = s2;
    const uint32_t l1 = ld32(raw, rec_off[r1] + 20), l2 = r2 != NONE32 ? ld32(raw, rec_off[r2] + 20) : 0u;
    src[2 * p] = r1; src[2 * p + 1] = r2;
    mate_len[2 * p] = l1; mate_len[2 * p + 1] = l2;
    units[2 * p] = l1 / 32u + ((l1 & 31u) ? 1u : 0u); units[2 * p + 1] = l2 / 32u + ((l2 & 31u) ? 1u : 0u);
}

}  // namespace lcty
