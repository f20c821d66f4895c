// lcty_deflate.hip — BGZF blocks deflated on the device: bgzf_deflate_kernel, bgzf_pack_kernel, lcty_bgzf_deflate and
// lcty_io_write_bgzf_device.
//   SAM specification 4.1 (BGZF), RFC 1952 (the gzip member), RFC 1951 (DEFLATE); the encoder is lcty_deflate.hpp, which the host tests
//   compile as it is and which emits the same bytes there.
// The input is cut every 0xff00 bytes, where BgzfOut cuts it. One wavefront, alone in its workgroup, encodes one block at a time, the
// blocks grid-strided: State (head table, histograms, codes: 22.9 KiB) lies in LDS, six workgroups per compute unit; the block's bytes
// are read from global memory, its tokens (one word per input byte) go to a scratch of the workgroup, its stream to the block's own slot
// of SLOT_WORDS words. The sizes of the blocks are scanned (exclusive_scan) and bgzf_pack_kernel copies header, stream and trailer of
// every block to its place; one download follows. An input above knob "bgzf_deflate_max_bytes" goes slice by slice, whole blocks each:
// a block's bytes do not depend on the blocks around it, so a seam changes nothing.
#include "lcty_bgzf.hpp"
#include "lcty_common.hpp"
#include "lcty_deflate.hpp"
#include "lcty_objects.hpp"
#include "lcty_scan.hpp"

namespace lcty {

namespace {

constexpr uint32_t SLOT_WORDS = (deflate::MAX_IN + 5 + 3) / 4;     // a block's stream, at most n + 5 bytes
constexpr uint32_t LDS_PER_CU = 160u * 1024u;                       // gfx950
constexpr uint64_t MAX_SLICE_BLOCKS = 32768;                        // 32-bit offsets inside a slice: 32 768 * (0xff00 + 31) < 2^31
const uint8_t EOF_MARKER[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t* __restrict__ in, uint64_t n_in, uint32_t n_tasks, uint32_t* slots,
                                                          uint32_t* tok, uint32_t* size, uint32_t* crc, uint32_t* form) {
    __shared__ deflate::State st;
    uint32_t* my_tok = tok + static_cast<uint64_t>(blockIdx.x) * deflate::MAX_IN;
    for (uint32_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const uint64_t at = static_cast<uint64_t>(t) * deflate::MAX_IN;
        uint32_t len = deflate::REFUSED, c = 0, f = 0;
        if (at < n_in) {
            const uint32_t n = static_cast<uint32_t>(n_in - at < deflate::MAX_IN ? n_in - at : deflate::MAX_IN);
            len = deflate::deflate_block(&st, my_tok, in + at, n, slots + static_cast<uint64_t>(t) * SLOT_WORDS, SLOT_WORDS, &c, &f);
        }
        // the block's size in the file (header 18, trailer 8); 0: refused
        if (threadIdx.x == 0) { size[t] = len == deflate::REFUSED ? 0u : len + 26u; crc[t] = c; form[t] = f; }
        __syncthreads();
    }
}

// block t of the slice to packed[off[t], off[t + 1]): the header BgzfOut writes, the stream of its slot, CRC-32 and ISIZE
__global__ __launch_bounds__(256) void bgzf_pack_kernel(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ off, const uint32_t* __restrict__ crc,
                                                        uint64_t n_in, uint32_t n_tasks, uint8_t* packed, uint64_t n_packed) {
    const uint32_t t = blockIdx.x;
    if (t >= n_tasks) return;
    const uint32_t at = off[t], size = off[t + 1] - at;
    if (size < 26 || size > deflate::MAX_IN + 31 || static_cast<uint64_t>(at) + size > n_packed) return;
    const uint64_t in_at = static_cast<uint64_t>(t) * deflate::MAX_IN;
    const uint32_t isize = static_cast<uint32_t>(n_in - in_at < deflate::MAX_IN ? n_in - in_at : deflate::MAX_IN), len = size - 26, bsize = size - 1, c = crc[t];
    uint8_t* dst = packed + at;
    if (threadIdx.x < 18) {
        const uint8_t head[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, static_cast<uint8_t>(bsize & 255u), static_cast<uint8_t>(bsize >> 8)};
        dst[threadIdx.x] = head[threadIdx.x];
    } else if (threadIdx.x < 26) {
        const uint32_t k = threadIdx.x - 18;
        dst[18 + len + k] = static_cast<uint8_t>((k < 4 ? c : isize) >> (8 * (k & 3u)));
    }
    const uint8_t* src = reinterpret_cast<const uint8_t*>(slots + static_cast<uint64_t>(t) * SLOT_WORDS);
    for (uint32_t i = threadIdx.x; i < len; i += 256) dst[18 + i] = src[i];
}

// the device buffers of lcty_bgzf_deflate, kept with the context (lcty_ctx::deflate_scratch)
struct DeflateRun {
    DevBuf<uint8_t> in, packed;
    DevBuf<uint32_t> slots, tok, size, off, crc, form, scan;
};

}  // namespace

uint64_t bgzf_deflate_bound(uint64_t len, bool with_eof) { return len + 31 * ((len + deflate::MAX_IN - 1) / deflate::MAX_IN) + (with_eof ? 28 : 0); }

void bgzf_deflate_device(lcty_ctx* ctx, const uint8_t* data, uint64_t len, bool with_eof, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                         uint64_t* block_off, lcty_bgzf_deflate_stats* stats) {
    const double t_start = now_ms();
    const int64_t knob = ctx->knob("bgzf_deflate_max_bytes", 256ll << 20);
    if (knob < static_cast<int64_t>(deflate::MAX_IN))
        fail(LCTY_ERR_INVALID_INPUT, "bgzf_deflate_max_bytes = %lld: a slice holds at least one block of %u bytes", static_cast<long long>(knob), deflate::MAX_IN);
    if (out_cap < bgzf_deflate_bound(len, with_eof))
        fail(LCTY_ERR_INVALID_INPUT, "%llu bytes may deflate to %llu, the buffer has %llu", static_cast<unsigned long long>(len),
             static_cast<unsigned long long>(bgzf_deflate_bound(len, with_eof)), static_cast<unsigned long long>(out_cap));
    const uint64_t n_blocks = (len + deflate::MAX_IN - 1) / deflate::MAX_IN;
    const uint64_t slice_blocks = std::min<uint64_t>(static_cast<uint64_t>(knob) / deflate::MAX_IN, MAX_SLICE_BLOCKS);
    lcty_bgzf_deflate_stats S{};
    S.n_blocks = n_blocks; S.bytes_in = len;
    uint64_t written = 0;
    if (n_blocks) {
        ctx->activate();
        hipStream_t s = ctx->stream;
        std::lock_guard<std::mutex> one_at_a_time(ctx->deflate_mutex);
        std::shared_ptr<DeflateRun> held;
        {
            std::lock_guard<std::mutex> lock(ctx->scratch_mutex);
            held = std::static_pointer_cast<DeflateRun>(ctx->deflate_scratch);
            if (!held) { held = std::make_shared<DeflateRun>(); ctx->deflate_scratch = held; }
        }
        DeflateRun& X = *held;
        const uint32_t per_cu = std::max<uint32_t>(1, LDS_PER_CU / static_cast<uint32_t>(sizeof(deflate::State)));
        std::vector<uint32_t> h_off, h_form;
        for (uint64_t b0 = 0; b0 < n_blocks; b0 += slice_blocks) {
            const uint32_t nb = static_cast<uint32_t>(std::min<uint64_t>(slice_blocks, n_blocks - b0));
            const uint64_t in_at = b0 * deflate::MAX_IN, n_in = std::min<uint64_t>(len - in_at, static_cast<uint64_t>(nb) * deflate::MAX_IN);
            const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(nb, static_cast<uint64_t>(per_cu) * static_cast<uint32_t>(ctx->props.multiProcessorCount)));
            double t0 = now_ms();
            X.in.ensure(n_in); X.slots.ensure(static_cast<size_t>(nb) * SLOT_WORDS); X.tok.ensure(static_cast<size_t>(grid) * deflate::MAX_IN);
            X.size.ensure(nb + 1u); X.off.ensure(nb + 1u); X.crc.ensure(nb); X.form.ensure(nb); X.scan.ensure(scan_scratch_words(nb + 1u));
            X.in.upload(data + in_at, n_in, s);
            LCTY_HIP(hipStreamSynchronize(s));
            S.ms_upload += now_ms() - t0;
            t0 = now_ms();
            LCTY_HIP(hipMemsetAsync(X.size.p, 0, (nb + 1u) * sizeof(uint32_t), s));
            hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(grid), dim3(64), 0, s, X.in.p, n_in, nb, X.slots.p, X.tok.p, X.size.p, X.crc.p, X.form.p);
            LCTY_HIP(hipGetLastError());
            exclusive_scan(X.size.p, X.off.p, nb + 1u, X.scan.p, s);
            h_off.resize(nb + 1u); h_form.resize(nb);
            X.off.download(h_off.data(), nb + 1u, s); X.form.download(h_form.data(), nb, s);
            LCTY_HIP(hipStreamSynchronize(s));
            const uint64_t total = h_off[nb];
            for (uint32_t t = 0; t < nb; t++) {
                const uint32_t size = h_off[t + 1] - h_off[t];
                if (size < 26 || size > deflate::MAX_IN + 31 || h_form[t] > deflate::DYNAMIC) fail(LCTY_ERR_RUNTIME, "lcty_bgzf_deflate: block %llu was not encoded", static_cast<unsigned long long>(b0 + t));
            }
            if (written + total + (with_eof ? 28 : 0) > out_cap) fail(LCTY_ERR_RUNTIME, "lcty_bgzf_deflate: the blocks take more than their bound");
            X.packed.ensure(total);
            hipLaunchKernelGGL(bgzf_pack_kernel, dim3(nb), dim3(256), 0, s, X.slots.p, X.off.p, X.crc.p, n_in, nb, X.packed.p, total);
            LCTY_HIP(hipGetLastError());
            LCTY_HIP(hipStreamSynchronize(s));
            S.ms_kernel += now_ms() - t0;
            t0 = now_ms();
            X.packed.download(out + written, total, s);
            LCTY_HIP(hipStreamSynchronize(s));
            S.ms_download += now_ms() - t0;
            for (uint32_t t = 0; t < nb; t++) {
                if (block_off) block_off[b0 + t] = written + h_off[t];
                (h_form[t] == deflate::STORED ? S.n_stored : h_form[t] == deflate::FIXED ? S.n_fixed : S.n_dynamic)++;
            }
            written += total;
        }
    }
    if (block_off) block_off[n_blocks] = written;
    if (with_eof) { memcpy(out + written, EOF_MARKER, 28); written += 28; }
    *out_len = written;
    S.bytes_out = written;
    S.ms_total = now_ms() - t_start;
    if (stats) *stats = S;
}

}  // namespace lcty

using namespace lcty;

uint64_t lcty_bgzf_deflate_bound(uint64_t len, int32_t with_eof) { return bgzf_deflate_bound(len, with_eof != 0); }

int32_t lcty_bgzf_deflate(lcty_ctx* ctx, const uint8_t* data, uint64_t len, int32_t with_eof, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                          uint64_t* block_off, lcty_bgzf_deflate_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return guarded([&] {
        if (!ctx || (len && !data) || !out_len || (!out && (len || with_eof))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        bgzf_deflate_device(ctx, data, len, with_eof != 0, out, out_cap, out_len, block_off, stats);
    });
}

int32_t lcty_io_write_bgzf_device(lcty_ctx* ctx, const char* path, const uint8_t* data, uint64_t len, lcty_bgzf_deflate_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return guarded([&] {
        if (!ctx || !path || (len && !data)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<uint8_t> out(bgzf_deflate_bound(len, true));
        uint64_t n = 0;
        bgzf_deflate_device(ctx, data, len, true, out.data(), out.size(), &n, nullptr, stats);
        FILE* f = fopen(path, "wb");
        if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot create %s", path);
        const bool bad = fwrite(out.data(), 1, n, f) != n;
        if (fclose(f) != 0 || bad) fail(LCTY_ERR_RUNTIME, "write error on %s", path);
    });
}
