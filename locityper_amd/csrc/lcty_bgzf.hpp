// lcty_bgzf.hpp — the BGZF writer (SAM specification, section 4.1): the one definition behind write_bam (lcty_bam.hip) and
// lcty_io_write_bgzf (lcty_io.hip). Host code.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "lcty_common.hpp"

namespace lcty {

// BGZF: gzip members of at most 64 KB with the BC extra field; virtual offset = start of the block << 16 | offset inside it
struct BgzfOut {
    FILE* f = nullptr;
    std::vector<uint8_t> block;
    uint64_t coff = 0;
    explicit BgzfOut(const char* path) {
        f = fopen(path, "wb");
        if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot create %s", path);
        block.reserve(0xff00);
    }
    ~BgzfOut() { if (f) fclose(f); }
    uint64_t tell() const { return (coff << 16) | block.size(); }
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
        while (n) {
            const size_t take = std::min<size_t>(n, 0xff00 - block.size());
            block.insert(block.end(), b, b + take);
            b += take; n -= take;
            if (block.size() == 0xff00) flush();
        }
    }
    void close() {
        if (!block.empty()) flush();
        flush();                                                            // the empty block that marks the end of a BGZF file
        if (fclose(f) != 0) { f = nullptr; fail(LCTY_ERR_RUNTIME, "write error"); }
        f = nullptr;
    }
};

}  // namespace lcty
