// lcty_sample_bam_internal.hpp — what the two readers of an indexed BAM file share: lcty_sample_bam.hip
// (`genotype -a`: the reads of the target regions) and lcty_bg_fetch.hip (`preproc -a`: the alignments of the background region).
// Host: the opened file with its index, and the front half of a fetch — the chunks of the regions, pread, the BGZF split, the inflate
// (zlib, or the device with knob "sample_bam_inflate" 1) into one page-locked slice, the chain of record lengths (fetch_slice).
// Device: the fields of a record that lies at any byte of that slice (ld32, rec_head, rec_fits), the comparison and the hash of read
// names, and the unpack of 4-bit base codes (unpack_kernel).
#pragma once

#include <unistd.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "lcty_bgzf.hpp"
#include "lcty_common.hpp"
#include "lcty_device.hpp"
#include "lcty_vcf_index_parse.hpp"

namespace lcty {

constexpr uint64_t SLICE_PAD = 64;             // bytes behind the slice that the dword loads of a record's last bytes may touch
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
    uint32_t lo_m = 0, hi_m = n_mates;                                           // the mate whose units hold u: last m with unit_off[m] <= u
    while (hi_m - lo_m > 1) { const uint32_t mid = (lo_m + hi_m) / 2; if (unit_off[mid] <= u) lo_m = mid; else hi_m = mid; }
    const uint32_t m = lo_m, q = u - unit_off[m];
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

// The front half of a fetch. slice: page-locked, `total` inflated bytes + SLICE_PAD zero bytes; rec_off: the byte of every record
// walked (of its block_size field), in file order.
struct FetchedSlice {
    uint8_t* slice = nullptr;
    uint64_t total = 0;
    std::vector<uint64_t> rec_off;
    FetchedSlice() = default;
    FetchedSlice(const FetchedSlice&) = delete;
    FetchedSlice& operator=(const FetchedSlice&) = delete;
    ~FetchedSlice() { if (slice) (void)hipHostFree(slice); }
};

}  // namespace lcty

struct lcty_sample_bam {
    std::string path, index_path;
    int fd = -1;
    uint64_t fsize = 0;
    std::vector<uint32_t> lengths; std::vector<uint64_t> name_off; std::string names;
    uint64_t first_record = 0;                   // virtual offset behind the header
    int paired = -1;                             // flag 0x1 of the first record; -1: not looked at yet, -2: no record
    using Ref = lcty::IndexRef;                  // bins -> chunks, the linear index (lcty_vcf_index_parse.hpp)
    std::vector<Ref> refs;
    uint64_t tail_start = 0;                     // largest chunk end of the index
    uint64_t n_no_coor = 0; bool has_no_coor = false;
    ~lcty_sample_bam() { if (fd >= 0) close(fd); }
};

namespace lcty {

// n bytes of the file from byte `at` (LCTY_ERR_RUNTIME "read error"), and one BGZF block through a stream opened with 16 + MAX_WBITS
void pread_all(int fd, void* buf, size_t n, uint64_t at, const char* path);
void inflate_block(z_stream& zs, const uint8_t* in, uint32_t csize, uint8_t* out, uint32_t isize, const char* path);

// the blocks of a BGZF file one after the other, from its start: the header and the first record
struct BgzfSerial {
    int fd; uint64_t fsize; const char* path;
    uint64_t coff = 0, next = 0;                 // the block in `data`, the one behind it
    std::vector<uint8_t> data; size_t at = 0;
    z_stream zs;
    BgzfSerial(int fd_, uint64_t fsize_, const char* path_) : fd(fd_), fsize(fsize_), path(path_) {
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateInit2");
    }
    ~BgzfSerial() { inflateEnd(&zs); }
    bool load() {                                // the next block that holds data; false at the end of the file
        while (at == data.size()) {
            if (next >= fsize) return false;
            uint8_t buf[0x10000];
            const size_t n = static_cast<size_t>(std::min<uint64_t>(sizeof(buf), fsize - next));
            pread_all(fd, buf, n, next, path);
            const uint32_t csize = bgzf_block_size(buf, n);
            if (!csize || csize > n) fail(LCTY_ERR_INVALID_DATA, "%s: not a BGZF block at offset %llu", path, static_cast<unsigned long long>(next));
            const uint32_t isize = buf[csize - 4] | (buf[csize - 3] << 8) | (buf[csize - 2] << 16) | (static_cast<uint32_t>(buf[csize - 1]) << 24);
            if (isize > 0x10000) fail(LCTY_ERR_INVALID_DATA, "%s: a BGZF block of %u bytes", path, isize);
            data.resize(isize);
            if (isize) inflate_block(zs, buf, csize, data.data(), isize, path); else if (inflateReset(&zs) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateReset");
            coff = next; next += csize; at = 0;
        }
        return true;
    }
    bool read(void* out, size_t n) {             // false: the file ends first
        uint8_t* p = static_cast<uint8_t*>(out);
        while (n) {
            if (!load()) return false;
            const size_t take = std::min(n, data.size() - at);
            memcpy(p, data.data() + at, take);
            p += take; n -= take; at += take;
        }
        return true;
    }
    uint64_t tell() { return at == data.size() ? next << 16 : (coff << 16) | at; }
};

// a chunk's blocks as they lie in the file: blocks[first_block .. + n_blocks); of the inflated bytes the chunk's own are
// [chain_beg, chain_end), the last block's end is span_end
struct ChunkSpan { size_t first_block, n_blocks; uint64_t chain_beg, chain_end, span_end; };
// pread of the byte ranges of the merged chunks cs and their split into BGZF blocks: comp grows by the bytes read, blocks by their
// blocks (out_at from `total` on, which grows by their inflated sizes), spans by one entry per chunk that has blocks. A chunk that
// does not start or end inside its block, or bytes that are no BGZF block, are LCTY_ERR_INVALID_DATA.
void read_chunk_blocks(int fd, uint64_t fsize, const char* path, const std::vector<Chunk>& cs, std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks,
                       std::vector<ChunkSpan>& spans, uint64_t& total, uint64_t& bytes_read);

// the BGZF blocks the merged chunks cs span, by the headers of the blocks alone (what the plan entry points report)
uint64_t count_chunk_blocks(int fd, uint64_t fsize, const char* path, const std::vector<Chunk>& cs);

// The regions of a call must be inside the file's contigs, non-empty, sorted and disjoint: LCTY_ERR_INVALID_INPUT otherwise.
void check_regions(const lcty_sample_bam* b, uint32_t n, const uint32_t* tid, const uint32_t* start, const uint32_t* end);
// plan_chunks, pread, the BGZF split, the inflate and the walk of record lengths of one call, with the knobs
// "sample_bam_max_slice_bytes" and "sample_bam_inflate" and the errors lcty_sample_bam_fetch documents for them. Fills F and the
// fields of S up to ms_walk. d_raw: with the device inflate (returns true) the slice with its pad is already there; otherwise it is
// left alone and the caller uploads F.slice. Activates the context.
bool fetch_slice(lcty_ctx* ctx, lcty_sample_bam* bam, uint32_t n_regions, const uint32_t* tid, const uint32_t* start, const uint32_t* end,
                 bool with_unmapped, bool whole_file, FetchedSlice& F, DevBuf<uint8_t>& d_raw, lcty_sample_bam_stats& S);
// The inflate of fetch_slice on its own (lcty_aln_bam.hip reads a whole un-indexed file through it): `blocks` of `comp` into F.slice
// (page-locked, total + SLICE_PAD bytes, allocated here), by zlib on the host pool or, with knob "sample_bam_inflate" 1 and plain
// gzip headers, on the device: true, and d_raw holds the slice with its pad. comp is released. Activates the context.
bool inflate_slice(lcty_ctx* ctx, std::vector<uint8_t>& comp, const std::vector<BgzfBlock>& blocks, uint64_t total, FetchedSlice& F,
                   DevBuf<uint8_t>& d_raw, const char* path, double& ms_inflate);
// the name of the record at byte o of a slice
std::string record_name(const uint8_t* slice, uint64_t o);

}  // namespace lcty
