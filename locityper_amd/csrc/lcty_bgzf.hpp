// lcty_bgzf.hpp — BGZF (SAM specification, section 4.1), host code without HIP (the host probes under scripts/ compile it with g++):
//   the writer    the one definition behind write_bam (lcty_bam.hip) and lcty_io_write_bgzf (lcty_io.hip). It either deflates block by
//                 block with zlib as the bytes come, or keeps them and deflates them all on the device when it is closed (lcty_deflate.hip).
//   the reader    the head of one block (bgzf_head: the one place that decodes the trailer), a list of blocks (BgzfBlock) inflated by
//                 zlib on a pool of threads (bgzf_inflate_host), a file's blocks one after the other (BgzfSerial), and the small file
//                 helpers every reader needs (read_whole_file, is_regular_file, has_suffix, pread_all).
// The device inflate of the same block list and the front half of a fetch are in lcty_bgzf_read.hpp.
#pragma once

#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "lcty_host.hpp"

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

// ---- files ----------------------------------------------------------------------------------------------------------------------

inline bool is_regular_file(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
inline bool has_suffix(const std::string& s, const char* suffix) {
    const size_t n = strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}
// the bytes of a file: what its size announces in one read, and whatever follows (a pipe announces nothing) 64 KiB at a time
inline std::vector<uint8_t> read_whole_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot open %s", path);
    std::vector<uint8_t> buf;
    if (fseek(f, 0, SEEK_END) == 0) {
        const long size = ftell(f);
        rewind(f);
        if (size > 0) { buf.resize(static_cast<size_t>(size)); buf.resize(fread(buf.data(), 1, buf.size(), f)); }
    }
    uint8_t chunk[1 << 16];
    size_t n;
    while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) fail(LCTY_ERR_RUNTIME, "read error on %s", path);
    return buf;
}
// n bytes of the file from byte `at` (LCTY_ERR_RUNTIME "read error")
inline void pread_all(int fd, void* buf, size_t n, uint64_t at, const char* path) {
    uint8_t* p = static_cast<uint8_t*>(buf);
    while (n) {
        const ssize_t got = pread(fd, p, n, static_cast<off_t>(at));
        if (got <= 0) fail(LCTY_ERR_RUNTIME, "read error on %s", path);
        p += got; n -= static_cast<size_t>(got); at += static_cast<uint64_t>(got);
    }
}

// ---- blocks ---------------------------------------------------------------------------------------------------------------------

// the size of the BGZF block that starts at p (n bytes available, at least 18 needed; the block may be longer than n); 0 = not a BGZF block
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

// The block that starts at p and lies whole inside the n bytes: its compressed size, its inflated size (the last four bytes) and
// bgzf_plain_head. BGZF_NOT_A_BLOCK: no BGZF header, or the block ends behind n (h is not filled); BGZF_TOO_LARGE: it claims more
// than 64 KiB (h is filled). Every walk of a run of blocks takes its fields from here and words its own verdict.
enum BgzfVerdict : uint32_t { BGZF_OK = 0, BGZF_NOT_A_BLOCK = 1, BGZF_TOO_LARGE = 2 };
struct BgzfHead { uint32_t csize, isize, head; };
inline BgzfVerdict bgzf_head(const uint8_t* p, size_t n, BgzfHead& h) {
    h.csize = bgzf_block_size(p, n);
    if (!h.csize || h.csize > n) return BGZF_NOT_A_BLOCK;
    const uint8_t* t = p + h.csize - 4;
    h.isize = t[0] | (t[1] << 8) | (t[2] << 16) | (static_cast<uint32_t>(t[3]) << 24);
    h.head = bgzf_plain_head(p);
    return h.isize > 0x10000 ? BGZF_TOO_LARGE : BGZF_OK;
}

// one block of a run: compressed size, inflated size, its place in the output and in the compressed bytes, the offset an error
// names, and bgzf_plain_head
struct BgzfBlock { uint32_t csize, isize; uint64_t out_at; size_t in_at; uint64_t named_at; uint32_t head; };

// one BGZF block through a stream opened with 16 + MAX_WBITS. A stream that ends before isize bytes, or has more, is reported with
// zlib's error codes (Z_DATA_ERROR, Z_BUF_ERROR), not with its success codes.
inline void inflate_block(z_stream& zs, const uint8_t* in, uint32_t csize, uint8_t* out, uint32_t isize, const char* path) {
    zs.next_in = const_cast<Bytef*>(in); zs.avail_in = csize;
    zs.next_out = out; zs.avail_out = isize;
    const int rc = inflate(&zs, Z_FINISH);
    if (rc != Z_STREAM_END || zs.avail_out != 0)
        fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BGZF block (zlib %d)", path, rc == Z_STREAM_END ? Z_DATA_ERROR : rc == Z_OK ? Z_BUF_ERROR : rc);
    if (inflateReset(&zs) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateReset");
}

// every block with isize > 0 inflated to out + out_at by zlib, on at most max_threads threads (the members are independent; htslib
// does the same with its pool); a refused block is LCTY_ERR_INVALID_DATA "<what>: corrupt BGZF block (zlib <rc>)". A thread that
// cannot be started: its share is inflated here (every thread that did start is joined).
inline void bgzf_inflate_host(const uint8_t* comp, const std::vector<BgzfBlock>& blocks, uint8_t* out, const char* what, size_t max_threads = 16) {
    const uint32_t n_threads = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>({blocks.size() / 64 + 1, max_threads, std::thread::hardware_concurrency()})));
    std::vector<std::string> failed(n_threads);
    auto work = [&](uint32_t id) {
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) { failed[id] = "zlib: inflateInit2"; return; }
        try {
            for (size_t k = id; k < blocks.size(); k += n_threads)
                if (blocks[k].isize) inflate_block(zs, comp + blocks[k].in_at, blocks[k].csize, out + blocks[k].out_at, blocks[k].isize, what);
        } catch (const Error& e) { failed[id] = e.what(); }
        inflateEnd(&zs);
    };
    std::vector<std::thread> th;
    std::vector<uint32_t> here;
    for (uint32_t id = 1; id < n_threads; id++) {
        try { th.emplace_back(work, id); } catch (const std::system_error&) { here.push_back(id); }
    }
    work(0);
    for (uint32_t id : here) work(id);
    for (auto& x : th) x.join();
    for (const std::string& f : failed) if (!f.empty()) fail(LCTY_ERR_INVALID_DATA, "%s", f.c_str());
}

// the blocks of a BGZF file one after the other, from its start: a header and what follows it, an index
struct BgzfSerial {
    int fd; uint64_t fsize; const char* path;
    uint64_t coff = 0, next = 0;                 // the block in `data`, the one behind it
    std::vector<uint8_t> data; size_t at = 0;
    z_stream zs;
    BgzfSerial(int fd_, uint64_t fsize_, const char* path_) : fd(fd_), fsize(fsize_), path(path_) {
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateInit2");
    }
    BgzfSerial(const BgzfSerial&) = delete;
    BgzfSerial& operator=(const BgzfSerial&) = delete;
    ~BgzfSerial() { inflateEnd(&zs); }
    bool load() {                                // the next block that holds data; false at the end of the file
        while (at == data.size()) {
            if (next >= fsize) return false;
            uint8_t buf[0x10000];
            const size_t n = static_cast<size_t>(std::min<uint64_t>(sizeof(buf), fsize - next));
            pread_all(fd, buf, n, next, path);
            BgzfHead h;
            const BgzfVerdict v = bgzf_head(buf, n, h);
            if (v == BGZF_NOT_A_BLOCK) fail(LCTY_ERR_INVALID_DATA, "%s: not a BGZF block at offset %llu", path, static_cast<unsigned long long>(next));
            if (v == BGZF_TOO_LARGE) fail(LCTY_ERR_INVALID_DATA, "%s: a BGZF block of %u bytes", path, h.isize);
            data.resize(h.isize);
            if (h.isize) inflate_block(zs, buf, h.csize, data.data(), h.isize, path); else if (inflateReset(&zs) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateReset");
            coff = next; next += h.csize; at = 0;
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
    bool append_block(std::vector<uint8_t>& out) {   // the rest of the current block (the next one, when it is used up) behind out; false at the end
        if (!load()) return false;
        out.insert(out.end(), data.begin() + static_cast<ptrdiff_t>(at), data.end());
        at = data.size();
        return true;
    }
    uint64_t tell() { return at == data.size() ? next << 16 : (coff << 16) | at; }
};

}  // namespace lcty
