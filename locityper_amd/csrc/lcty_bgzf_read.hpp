// lcty_bgzf_read.hpp — the front half of every fetch from a BGZF file: the readers of an indexed BAM file
// (lcty_sample_bam.hip, lcty_bg_fetch.hip), of an indexed VCF file (lcty_vcf_fetch.hip) and of a locus's aln.bam (lcty_aln_bam.hip)
// all get their bytes this way. The opened file (BgzfFile), pread of the byte ranges of merged index chunks and their split into
// blocks (read_chunk_blocks), and the slice: every block inflated into its place of one page-locked buffer, by zlib on the host
// pool or, with knob "sample_bam_inflate" 1, by bgzf_inflate_kernel (lcty_inflate.hip), and the same bytes on the device (Slice).
#pragma once

#include <string>
#include <vector>

#include "lcty_bgzf.hpp"
#include "lcty_bgzf_index.hpp"
#include "lcty_common.hpp"

namespace lcty {

constexpr uint64_t SLICE_PAD = 64;             // zero bytes behind the slice that the dword loads of its last bytes may touch

// a file opened for pread; LCTY_ERR_INVALID_INPUT "cannot open", LCTY_ERR_RUNTIME "cannot stat", LCTY_ERR_UNSUPPORTED from 2^48 bytes
// on (a virtual offset has 48 bits for the byte of a block)
struct BgzfFile {
    std::string path;
    int fd = -1;
    uint64_t fsize = 0;
    BgzfFile() = default;
    BgzfFile(const BgzfFile&) = delete;
    BgzfFile& operator=(const BgzfFile&) = delete;
    ~BgzfFile() { if (fd >= 0) close(fd); }
    void open(const char* p);
};

// a chunk's blocks as they lie in the file: blocks[first_block .. + n_blocks); of the inflated bytes the chunk's own are
// [chain_beg, chain_end), the last block's end is span_end
struct ChunkSpan { size_t first_block, n_blocks; uint64_t chain_beg, chain_end, span_end; };
// pread of the byte ranges of the merged chunks cs and their split into BGZF blocks: comp grows by the bytes read, blocks by their
// blocks (out_at from `total` on, which grows by their inflated sizes), spans by one entry per chunk that has blocks. A chunk that
// does not start or end inside its block, or bytes that are no BGZF block, are LCTY_ERR_INVALID_DATA.
void read_chunk_blocks(const BgzfFile& f, const std::vector<Chunk>& cs, std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks,
                       std::vector<ChunkSpan>& spans, uint64_t& total, uint64_t& bytes_read);
// the BGZF blocks the merged chunks cs span, by the headers of the blocks alone
uint64_t count_chunk_blocks(const BgzfFile& f, const std::vector<Chunk>& cs);
// what a plan entry point reports: the number of chunks, the first chunk_cap of them, and (blocks_total not null) count_chunk_blocks
void report_plan(const BgzfFile& f, const std::vector<Chunk>& cs, uint64_t chunk_cap, uint64_t* n_chunks, uint64_t* chunk_beg, uint64_t* chunk_end,
                 uint64_t* blocks_total);

// `blocks` of d_comp inflated on the device, between device buffers, every block with its head > 0 (lcty_inflate.hip). The first
// refused block in input order is LCTY_ERR_INVALID_DATA "<what>: corrupt BGZF block at offset <named_at> (<class>)". Synchronises s.
void bgzf_inflate_device(lcty_ctx* ctx, const uint8_t* d_comp, uint64_t n_comp, const std::vector<BgzfBlock>& blocks, uint8_t* d_out,
                         uint64_t n_out, hipStream_t s, const char* what);

// knob "sample_bam_inflate": 0 host, 1 device, anything else LCTY_ERR_INVALID_INPUT
void check_inflate_knob(lcty_ctx* ctx);
// `total` bytes against the knob cap_knob (default 2^33): LCTY_ERR_UNSUPPORTED "<path>: <what> <total> bytes, more than ..."
void check_slice_cap(lcty_ctx* ctx, const char* path, uint64_t total, const char* cap_knob, const char* what);

// what the front half of a fetch reports; a caller copies it into its public statistics
struct SliceStats {
    uint64_t n_chunks, bytes_read, blocks_inflated, bytes_inflated; double ms_read, ms_inflate;
    template <typename Stats> void put(Stats& S) const {
        S.n_chunks = n_chunks; S.bytes_read = bytes_read; S.blocks_inflated = blocks_inflated; S.bytes_inflated = bytes_inflated;
        S.ms_read = ms_read; S.ms_inflate = ms_inflate;
    }
};

// The inflated bytes of a fetch. slice: page-locked, `total` bytes + SLICE_PAD zero bytes; rec_off: what the caller walked in it
// (a BAM reader: the byte of every record, of its block_size field, in file order).
struct Slice {
    uint8_t* slice = nullptr;
    uint64_t total = 0;
    std::vector<uint64_t> rec_off;
    std::vector<ChunkSpan> spans;              // of read(): the chunks' own bytes in the slice
    Slice() = default;
    Slice(const Slice&) = delete;
    Slice& operator=(const Slice&) = delete;
    ~Slice() { if (slice) (void)hipHostFree(slice); }

    // The front half, step one: the knob "sample_bam_inflate" checked, the chunks cs read and split, their inflated size against the
    // knob cap_knob (check_slice_cap's `what`: "the fetched slice has"). Fills S but ms_inflate.
    void read(lcty_ctx* ctx, const BgzfFile& f, const std::vector<Chunk>& cs, const char* cap_knob, SliceStats& S);
    // Step two (a reader of a whole file enters here with comp and blocks of its own split): the page-locked slice, and every block
    // inflated into its place, by zlib on the host pool or, with knob "sample_bam_inflate" 1 and plain gzip headers, on the device;
    // then the device has the slice already. comp is released. Activates the context; returns the time of the inflate.
    double inflate(lcty_ctx* ctx, const char* path);
    // the page-locked buffer alone, its pad zeroed, for `n` bytes the caller puts there. Activates the context. A slice may be used
    // again (a reader of windows, lcty_fastx_device.hip): alloc() and inflate() then keep the buffers of the last use where they are
    // large enough, on the host and on the device.
    void alloc(lcty_ctx* ctx, uint64_t n);
    // the slice with its pad on the device, as dwords too: uploaded now unless the inflate ran there
    const uint8_t* device(hipStream_t s);
    void release_device() { d_raw.release(); }
    // n bytes written over the front of the slice after alloc() or inflate() (a reader of windows carries the tail of the last one
    // here, lcty_fastx_window.hpp), on the device as well when the inflate left the slice there. Asynchronous on s.
    void put_front(const uint8_t* p, uint64_t n, hipStream_t s);

    std::vector<uint8_t> comp;                 // between read() and inflate(): the bytes read ...
    std::vector<BgzfBlock> blocks;             // ... and their blocks
private:
    DevBuf<uint8_t> d_raw;
    uint64_t cap = 0;                          // bytes the page-locked buffer holds in front of its pad
    bool on_device = false;
};

}  // namespace lcty
