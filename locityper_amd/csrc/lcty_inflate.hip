// lcty_inflate.hip — BGZF blocks inflated on the device: bgzf_inflate_kernel and lcty_bgzf_inflate.
//   SAM specification 4.1 (BGZF), RFC 1952 (the gzip member), RFC 1951 (DEFLATE); the decoder is lcty_inflate.hpp, which the host
//   tests compile as it is.
// One wavefront, alone in its workgroup, takes one block at a time, the blocks grid-strided. The symbol decode is one chain: every
// lane walks it with the same values, and what comes out of LDS goes through readfirstlane so that the bit buffer, the positions and
// the branches stay scalar. The lanes share the byte work: the input window (256 bytes a load), the copies of matches and stored
// blocks, the flush and the CRC. The output window is a ring of 32 KiB in LDS, the farthest distance of the format, flushed to the
// block's place with byte stores of neighbouring lanes whenever the next symbol would overwrite a byte not yet flushed, and the CRC
// of the flushed bytes is taken from the ring on the way. State is 38.4 KiB: four blocks in flight per compute unit.
#include "lcty_bgzf_read.hpp"
#include "lcty_device.hpp"
#include "lcty_inflate.hpp"
#include "lcty_objects.hpp"

namespace lcty {

struct InflateTask { uint64_t in_at, out_at; uint32_t n_in, isize; };      // deflate stream + trailer in comp; the block's place in out

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, uint64_t n_comp, uint8_t* out, uint64_t n_out,
                                                          const InflateTask* __restrict__ tasks, uint32_t n_tasks, unsigned long long* err) {
    __shared__ inflate::State st;
    for (uint32_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
        const InflateTask k = tasks[t];
        uint32_t rc = inflate::E_TASK;
        if (k.in_at <= n_comp && k.n_in <= n_comp - k.in_at && k.out_at <= n_out && k.isize <= n_out - k.out_at)
            rc = inflate::inflate_block(&st, comp + k.in_at, k.n_in, out + k.out_at, k.isize, true, nullptr);
        // (block ordinal, class): the first refused block in input order decides, as record_kernel's errors do
        if (rc != inflate::OK && threadIdx.x == 0) refuse(err, t, rc);
        __syncthreads();
    }
}

void bgzf_inflate_device(lcty_ctx* ctx, const uint8_t* d_comp, uint64_t n_comp, const std::vector<BgzfBlock>& blocks, uint8_t* d_out,
                         uint64_t n_out, hipStream_t s, const char* what) {
    std::vector<InflateTask> tasks;
    std::vector<size_t> block_of;
    for (size_t i = 0; i < blocks.size(); i++) {
        const BgzfBlock& b = blocks[i];
        if (!b.isize) continue;
        if (!b.head || b.head + 8u > b.csize) fail(LCTY_ERR_RUNTIME, "bgzf_inflate_device: block %zu is not the device's", i);
        tasks.push_back(InflateTask{b.in_at + b.head, b.out_at, b.csize - b.head, b.isize});
        block_of.push_back(i);
    }
    if (tasks.empty()) return;
    if (tasks.size() >= (1ull << 32)) fail(LCTY_ERR_UNSUPPORTED, "%s: %zu BGZF blocks in one call", what, tasks.size());
    DevBuf<InflateTask> d_tasks; ErrWord err;
    d_tasks.alloc(tasks.size()); d_tasks.upload(tasks.data(), tasks.size(), s);
    unsigned long long* d_err = err.reset(s);
    // four workgroups of 38.4 KiB fit the LDS of a compute unit
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(tasks.size(), 4ull * static_cast<uint32_t>(ctx->props.multiProcessorCount)));
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(grid), dim3(64), 0, s, d_comp, n_comp, d_out, n_out, d_tasks.p, static_cast<uint32_t>(tasks.size()), d_err);
    LCTY_HIP(hipGetLastError());
    uint64_t t; uint32_t cls;
    if (!err.take(s, t, cls)) return;
    const BgzfBlock& b = blocks[block_of[std::min<size_t>(t, block_of.size() - 1)]];
    fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BGZF block at offset %llu (%s)", what, static_cast<unsigned long long>(b.named_at), inflate::class_name(cls));
}

}  // namespace lcty

using namespace lcty;

int32_t lcty_bgzf_inflate(lcty_ctx* ctx, const uint8_t* comp, uint64_t n_comp, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                          lcty_bgzf_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return guarded([&] {
        if (!ctx || (n_comp && !comp) || !out_len) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double t_start = now_ms();
        std::vector<BgzfBlock> blocks;
        uint64_t total = 0;
        bool plain = true;
        for (uint64_t at = 0; at < n_comp;) {
            BgzfHead h;
            const BgzfVerdict v = bgzf_head(comp + at, n_comp - at, h);
            if (v == BGZF_NOT_A_BLOCK) fail(LCTY_ERR_INVALID_DATA, "not a BGZF block at offset %llu", static_cast<unsigned long long>(at));
            if (v == BGZF_TOO_LARGE) fail(LCTY_ERR_INVALID_DATA, "a BGZF block of %u bytes at offset %llu", h.isize, static_cast<unsigned long long>(at));
            if (h.isize && (!h.head || h.head + 8u > h.csize)) plain = false;
            blocks.push_back(BgzfBlock{h.csize, h.isize, total, static_cast<size_t>(at), at, h.head});
            total += h.isize; at += h.csize;
        }
        *out_len = total;
        if (!out) return;
        if (out_cap < total) fail(LCTY_ERR_INVALID_INPUT, "the blocks inflate to %llu bytes, the buffer has %llu", static_cast<unsigned long long>(total), static_cast<unsigned long long>(out_cap));
        lcty_bgzf_stats S{};
        S.n_blocks = blocks.size(); S.bytes_in = n_comp; S.bytes_out = total;
        if (!plain) {                                                        // a gzip header with more than the extra field: zlib's
            bgzf_inflate_host(comp, blocks, out, "lcty_bgzf_inflate");
        } else if (total) {
            ctx->activate();
            hipStream_t s = ctx->stream;
            double t0 = now_ms();
            DevBuf<uint8_t> d_comp, d_out;
            d_comp.alloc(n_comp); d_out.alloc(total);
            d_comp.upload(comp, n_comp, s);
            LCTY_HIP(hipStreamSynchronize(s));
            S.ms_upload = now_ms() - t0;
            t0 = now_ms();
            bgzf_inflate_device(ctx, d_comp.p, n_comp, blocks, d_out.p, total, s, "lcty_bgzf_inflate");
            S.ms_kernel = now_ms() - t0;
            t0 = now_ms();
            d_out.download(out, total, s);
            LCTY_HIP(hipStreamSynchronize(s));
            S.ms_download = now_ms() - t0;
        }
        S.ms_total = now_ms() - t_start;
        if (stats) *stats = S;
    });
}
