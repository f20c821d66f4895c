// lcty_bgzf.hpp — BGZF (SAM specification, section 4.1), host code: the writer, the one definition behind write_bam (lcty_bam.hip)
// and lcty_io_write_bgzf (lcty_io.hip); the split of a run of bytes into blocks (bgzf_block_size) and the two ways a list of blocks
// is inflated: zlib on at most 16 threads (lcty_sample_bam.hip) and bgzf_inflate_kernel (lcty_inflate.hip). The writer either deflates
// block by block with zlib as the bytes come, or keeps them and deflates them all on the device when it is closed (lcty_deflate.hip).
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "lcty_common.hpp"

namespace lcty {

// len bytes as BGZF blocks of at most 0xff00 bytes take at most this many bytes (a stored block: 18 + 5 + n + 8), the end-of-file marker 28
uint64_t bgzf_deflate_bound(uint64_t len, bool with_eof);
// lcty_bgzf_deflate behind its argument checks (lcty_deflate.hip): data (host) cut every 0xff00 bytes, deflated on the device, packed and
// downloaded to out; block_off (may be null): the offset in out of every block and of the end of the last. Synchronises the context's stream.
void bgzf_deflate_device(lcty_ctx* ctx, const uint8_t* data, uint64_t len, bool with_eof, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                         uint64_t* block_off, lcty_bgzf_deflate_stats* stats);

// BGZF: gzip members of at most 64 KB with the BC extra field; virtual offset = start of the block << 16 | offset inside it
struct BgzfOut {
    FILE* f = nullptr;
    std::vector<uint8_t> block;
    uint64_t coff = 0;
    // on_device (a context, or null): the bytes are kept in `all` and deflated by one bgzf_deflate_device in close(). Until then tell()
    // is provisional, block ordinal << 16 | offset inside it, which grows with the final offset and maps one to one: final() translates
    // after close().
    lcty_ctx* on_device = nullptr;
    std::vector<uint8_t> all;
    std::vector<uint64_t> block_off;
    explicit BgzfOut(const char* path, lcty_ctx* device = nullptr) : on_device(device) {
        f = fopen(path, "wb");
        if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot create %s", path);
        block.reserve(0xff00);
    }
    ~BgzfOut() { if (f) fclose(f); }
    uint64_t tell() const { return on_device ? ((all.size() / 0xff00) << 16) | (all.size() % 0xff00) : (coff << 16) | block.size(); }
    uint64_t final(uint64_t v) const { return on_device ? (block_off[std::min<size_t>(v >> 16, block_off.size() - 1)] << 16) | (v & 0xffff) : v; }
    void flush() {
        uint8_t out[0x10000];
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: deflateInit2");
        zs.next_in = block.data(); zs.avail_in = static_cast<uInt>(block.size());
        zs.next_out = out + 18; zs.avail_out = sizeof(out) - 26;
        if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { deflateEnd(&zs); fail(LCTY_ERR_RUNTIME, "zlib: deflate"); }
        const uint32_t clen = static_cast<uint32_t>(zs.total_out);
        deflateEnd(&zs);
        const uint32_t bsize = clen + 25;                                   // total block size - 1
        const uint8_t head[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0,
                                  static_cast<uint8_t>(bsize & 255), static_cast<uint8_t>(bsize >> 8)};
        memcpy(out, head, 18);
        const uint32_t crc = static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), block.data(), static_cast<uInt>(block.size())));
        const uint32_t isize = static_cast<uint32_t>(block.size());
        uint8_t* tail = out + 18 + clen;
        for (int i = 0; i < 4; i++) { tail[i] = static_cast<uint8_t>(crc >> (8 * i)); tail[4 + i] = static_cast<uint8_t>(isize >> (8 * i)); }
        if (fwrite(out, 1, clen + 26, f) != clen + 26) fail(LCTY_ERR_RUNTIME, "write error");
        coff += clen + 26;
        block.clear();
    }
    void write(const void* p, size_t n) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        if (on_device) { all.insert(all.end(), b, b + n); return; }
        while (n) {
            const size_t take = std::min<size_t>(n, 0xff00 - block.size());
            block.insert(block.end(), b, b + take);
            b += take; n -= take;
            if (block.size() == 0xff00) flush();
        }
    }
    void close() {
        if (on_device) {
            std::vector<uint8_t> out(bgzf_deflate_bound(all.size(), true));
            block_off.assign(all.size() / 0xff00 + 2, 0);                   // at least ceil(size / 0xff00) + 1
            uint64_t n = 0;
            bgzf_deflate_device(on_device, all.data(), all.size(), true, out.data(), out.size(), &n, block_off.data(), nullptr);
            block_off.resize((all.size() + 0xff00 - 1) / 0xff00 + 1);
            const bool bad = fwrite(out.data(), 1, n, f) != n;
            if (fclose(f) != 0 || bad) { f = nullptr; fail(LCTY_ERR_RUNTIME, "write error"); }
            f = nullptr;
            return;
        }
        if (!block.empty()) flush();
        flush();                                                            // the empty block that marks the end of a BGZF file
        if (fclose(f) != 0) { f = nullptr; fail(LCTY_ERR_RUNTIME, "write error"); }
        f = nullptr;
    }
};

// the size of the BGZF block that starts at p (n bytes available, at least 18 needed); 0 = not a BGZF block
inline uint32_t bgzf_block_size(const uint8_t* p, size_t n) {
    if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    const uint32_t xlen = p[10] | (p[11] << 8);
    if (12 + xlen > n) return 0;
    uint32_t bsize = 0;
    for (size_t x = 12; x + 4 <= 12 + xlen;) {
        const uint32_t slen = p[x + 2] | (p[x + 3] << 8);
        if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) bsize = (p[x + 4] | (p[x + 5] << 8)) + 1u;
        x += 4 + slen;
    }
    return bsize < 12 + xlen + 8 ? 0 : bsize;
}
// of a block bgzf_block_size took: the bytes in front of its deflate stream when FLG is FEXTRA alone (what every BAM writer sets),
// else 0: a name, a comment or a header CRC follow the extra field, and the block is zlib's
inline uint32_t bgzf_plain_head(const uint8_t* p) { return p[3] == 4 ? 12u + (p[10] | (p[11] << 8)) : 0u; }

// one block of a run: compressed size, inflated size (its last four bytes), its place in the output and in the compressed bytes,
// the offset an error names, and bgzf_plain_head
struct BgzfBlock { uint32_t csize, isize; uint64_t out_at; size_t in_at; uint64_t named_at; uint32_t head; };
// every block with isize > 0 inflated to out + out_at by zlib, on at most 16 threads; a refused block is LCTY_ERR_INVALID_DATA
// "corrupt BGZF block" with `what` in front (lcty_sample_bam.hip)
void bgzf_inflate_host(const uint8_t* comp, const std::vector<BgzfBlock>& blocks, uint8_t* out, const char* what);
// the same on the device, between device buffers, every block with its head > 0 (lcty_inflate.hip). The first refused block in
// input order is LCTY_ERR_INVALID_DATA "<what>: corrupt BGZF block at offset <named_at> (<class>)". Synchronises s.
void bgzf_inflate_device(lcty_ctx* ctx, const uint8_t* d_comp, uint64_t n_comp, const std::vector<BgzfBlock>& blocks, uint8_t* d_out,
                         uint64_t n_out, hipStream_t s, const char* what);

}  // namespace lcty
