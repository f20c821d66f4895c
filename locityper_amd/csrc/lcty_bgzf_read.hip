// lcty_bgzf_read.hip — the front half of every fetch from a BGZF file (lcty_bgzf_read.hpp). Host code.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "lcty_bgzf_read.hpp"
#include "lcty_objects.hpp"

namespace lcty {

void BgzfFile::open(const char* p) {
    path = p;
    fd = ::open(p, O_RDONLY | O_CLOEXEC);
    if (fd < 0) fail(LCTY_ERR_INVALID_INPUT, "cannot open %s", p);
    struct stat st;
    if (fstat(fd, &st) != 0) fail(LCTY_ERR_RUNTIME, "cannot stat %s", p);
    fsize = static_cast<uint64_t>(st.st_size);
    if (fsize >= (1ull << 48)) fail(LCTY_ERR_UNSUPPORTED, "%s: a file of 2^48 bytes or more", p);
}

void read_chunk_blocks(const BgzfFile& f, const std::vector<Chunk>& cs, std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks,
                       std::vector<ChunkSpan>& spans, uint64_t& total, uint64_t& bytes_read) {
    const int fd = f.fd;
    const uint64_t fsize = f.fsize;
    const char* path = f.path.c_str();
    for (const Chunk& c : cs) {
        const uint64_t cbeg = c.beg >> 16, cend = c.end >> 16;
        const uint32_t uend = static_cast<uint32_t>(c.end & 0xFFFF);
        if (cbeg >= fsize) continue;
        uint64_t rend = cend;                                              // ... and the block the chunk ends in, when it reaches into it
        if (uend && cend < fsize) {
            uint8_t hd[512];
            const size_t n = static_cast<size_t>(std::min<uint64_t>(sizeof(hd), fsize - cend));
            pread_all(fd, hd, n, cend, path);
            const uint32_t csize = bgzf_block_size(hd, n);
            if (!csize) fail(LCTY_ERR_INVALID_DATA, "%s: not a BGZF block at offset %llu (an index of another file?)", path, static_cast<unsigned long long>(cend));
            rend = std::min<uint64_t>(fsize, cend + csize);
        }
        rend = std::min<uint64_t>(rend, fsize);
        const size_t in0 = comp.size();
        comp.resize(in0 + (rend - cbeg));
        pread_all(fd, comp.data() + in0, rend - cbeg, cbeg, path);
        bytes_read += rend - cbeg;
        ChunkSpan sp{blocks.size(), 0, total + (c.beg & 0xFFFF), 0, 0};
        bool end_seen = false;
        uint64_t at = cbeg;
        while (at < rend && (at < cend || (at == cend && uend))) {
            const uint8_t* p = comp.data() + in0 + (at - cbeg);
            BgzfHead h;
            const BgzfVerdict v = bgzf_head(p, rend - at, h);
            if (v == BGZF_NOT_A_BLOCK) {
                if (at + 0x10000 >= fsize) fail(LCTY_ERR_INVALID_DATA, "%s: truncated or corrupt BGZF block at offset %llu", path, static_cast<unsigned long long>(at));
                fail(LCTY_ERR_INVALID_DATA, "%s: not a BGZF block at offset %llu (an index of another file?)", path, static_cast<unsigned long long>(at));
            }
            if (v == BGZF_TOO_LARGE) fail(LCTY_ERR_INVALID_DATA, "%s: a BGZF block of %u bytes", path, h.isize);
            if (at == cbeg && (c.beg & 0xFFFF) > h.isize) fail(LCTY_ERR_INVALID_DATA, "%s: a chunk of the index starts behind its block", path);
            if (at == cend) { if (uend > h.isize) fail(LCTY_ERR_INVALID_DATA, "%s: a chunk of the index ends behind its block", path); sp.chain_end = total + uend; end_seen = true; }
            blocks.push_back(BgzfBlock{h.csize, h.isize, total, in0 + static_cast<size_t>(at - cbeg), at, h.head});
            total += h.isize; at += h.csize;
        }
        sp.n_blocks = blocks.size() - sp.first_block; sp.span_end = total;
        if (!end_seen) sp.chain_end = total;
        if (sp.n_blocks) spans.push_back(sp);
    }
}

uint64_t count_chunk_blocks(const BgzfFile& f, const std::vector<Chunk>& cs) {
    uint64_t blocks = 0;
    for (const Chunk& c : cs) {
        uint64_t at = c.beg >> 16;
        const uint64_t last = c.end >> 16;
        while (at < f.fsize && (at < last || (at == last && (c.end & 0xFFFF)))) {
            uint8_t hd[512];
            const size_t n = static_cast<size_t>(std::min<uint64_t>(sizeof(hd), f.fsize - at));
            pread_all(f.fd, hd, n, at, f.path.c_str());
            const uint32_t csize = bgzf_block_size(hd, n);
            if (!csize) fail(LCTY_ERR_INVALID_DATA, "%s: not a BGZF block at offset %llu", f.path.c_str(), static_cast<unsigned long long>(at));
            blocks++; at += csize;
        }
    }
    return blocks;
}

void report_plan(const BgzfFile& f, const std::vector<Chunk>& cs, uint64_t chunk_cap, uint64_t* n_chunks, uint64_t* chunk_beg, uint64_t* chunk_end,
                 uint64_t* blocks_total) {
    *n_chunks = cs.size();
    for (size_t i = 0; i < cs.size() && i < chunk_cap; i++) { chunk_beg[i] = cs[i].beg; chunk_end[i] = cs[i].end; }
    if (blocks_total) *blocks_total = count_chunk_blocks(f, cs);
}

void check_inflate_knob(lcty_ctx* ctx) {
    const int64_t v = ctx->knob("sample_bam_inflate", 0);
    if (v > 1) fail(LCTY_ERR_INVALID_INPUT, "sample_bam_inflate = %lld (0: host, 1: device)", static_cast<long long>(v));
}

void check_slice_cap(lcty_ctx* ctx, const char* path, uint64_t total, const char* cap_knob, const char* what) {
    const uint64_t cap = static_cast<uint64_t>(ctx->knob(cap_knob, 1ll << 33));
    if (total > cap)
        fail(LCTY_ERR_UNSUPPORTED, "%s: %s %llu bytes, more than %llu (knob %s)", path, what, static_cast<unsigned long long>(total),
             static_cast<unsigned long long>(cap), cap_knob);
}

void Slice::read(lcty_ctx* ctx, const BgzfFile& f, const std::vector<Chunk>& cs, const char* cap_knob, SliceStats& S) {
    check_inflate_knob(ctx);
    S.n_chunks = cs.size();
    const double t0 = now_ms();
    read_chunk_blocks(f, cs, comp, blocks, spans, total, S.bytes_read);
    S.ms_read = now_ms() - t0;
    S.blocks_inflated = blocks.size(); S.bytes_inflated = total;
    check_slice_cap(ctx, f.path.c_str(), total, cap_knob, "the fetched slice has");
}

void Slice::alloc(lcty_ctx* ctx, uint64_t n) {
    ctx->activate();
    if (!slice || n > cap) {                                                // a slice that is used again keeps a buffer that is large enough
        if (slice) { (void)hipHostFree(slice); slice = nullptr; }
        LCTY_HIP(hipHostMalloc(reinterpret_cast<void**>(&slice), n + SLICE_PAD, hipHostMallocDefault));
        cap = n;
    }
    total = n; on_device = false;
    memset(slice + total, 0, SLICE_PAD);
}

double Slice::inflate(lcty_ctx* ctx, const char* path) {
    alloc(ctx, total);
    hipStream_t s = ctx->stream;
    const double t0 = now_ms();
    // knob "sample_bam_inflate" 1: on the device, straight into the buffer the kernels read, and from there to the page-locked
    // slice for the host's walk; blocks with more in their gzip header than the extra field leave the call to zlib
    on_device = ctx->knob("sample_bam_inflate", 0) == 1 && total > 0;
    for (const BgzfBlock& b : blocks) if (b.isize && (!b.head || b.head + 8u > b.csize)) on_device = false;
    if (on_device) {
        DevBuf<uint8_t> d_comp;
        d_comp.alloc(comp.size()); d_raw.ensure(total + SLICE_PAD);
        d_comp.upload(comp.data(), comp.size(), s);
        LCTY_HIP(hipMemsetAsync(d_raw.p + total, 0, SLICE_PAD, s));
        bgzf_inflate_device(ctx, d_comp.p, comp.size(), blocks, d_raw.p, total, s, path);
        d_raw.download(slice, total, s);
        LCTY_HIP(hipStreamSynchronize(s));
    } else bgzf_inflate_host(comp.data(), blocks, slice, path);
    const double ms = now_ms() - t0;
    std::vector<uint8_t>().swap(comp);
    std::vector<BgzfBlock>().swap(blocks);
    return ms;
}

void Slice::put_front(const uint8_t* p, uint64_t n, hipStream_t s) {
    if (n > total) fail(LCTY_ERR_RUNTIME, "slice overflow (%llu > %llu)", static_cast<unsigned long long>(n), static_cast<unsigned long long>(total));
    memcpy(slice, p, n);
    if (on_device && n) LCTY_HIP(hipMemcpyAsync(d_raw.p, slice, n, hipMemcpyHostToDevice, s));
}

const uint8_t* Slice::device(hipStream_t s) {
    if (!on_device) { d_raw.ensure(total + SLICE_PAD); d_raw.upload(slice, total + SLICE_PAD, s); on_device = true; }
    return d_raw.p;
}

}  // namespace lcty
