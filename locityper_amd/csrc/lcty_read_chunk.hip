// lcty_read_chunk.hip — the bodies of lcty_read_chunk.hpp.
#include "lcty_read_chunk.hpp"

#include "lcty_objects.hpp"

namespace lcty {

// a mate's first unit -> its offset in bases (n counts the closing entry)
static __global__ __launch_bounds__(256) void offsets_kernel(const uint32_t* __restrict__ unit_off, uint64_t n, uint64_t* __restrict__ mate_off) {
    const uint64_t m = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (m < n) mate_off[m] = 32ull * unit_off[m];
}

void ReadChunk::size_units(uint64_t units) {
    hipStream_t s = ctx->stream;
    n_units = units;
    size(d_bases, units + CHUNK_PAD_UNITS); size(d_nm, units + CHUNK_PAD_UNITS);
    LCTY_HIP(hipMemsetAsync(d_bases.p + units, 0, CHUNK_PAD_UNITS * sizeof(uint64_t), s));
    LCTY_HIP(hipMemsetAsync(d_nm.p + units, 0, CHUNK_PAD_UNITS * sizeof(uint32_t), s));
}

uint32_t ReadChunk::place(const DevBuf<uint32_t>& d_units, uint64_t M, ScanTotal& scan) {
    hipStream_t s = ctx->stream;
    const uint32_t units = scan.run(d_units, d_unit_off, M, ctx);
    hipLaunchKernelGGL(offsets_kernel, dim3(blocks_of(M + 1, 256)), dim3(256), 0, s, d_unit_off.p, M + 1, d_off.p);
    LCTY_HIP(hipGetLastError());
    size_units(units);
    len_store.resize(M); h_len = len_store.data();
    d_len.download(len_store.data(), M, s);
    return units;
}

void ReadChunk::upload(const lcty_reads_host* h) {
    if (!h) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    clear();
    const uint64_t k = h->n_pairs;
    if (k == 0) return;
    if (!h->mate_len || !h->mate_off || !h->bases2 || !h->nmask) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    for (uint64_t m = 0; m < 2 * k; m++) {
        if (h->mate_off[m] % 32) fail(LCTY_ERR_INVALID_INPUT, "mate offsets must be multiples of 32 bases");
        if (h->mate_off[m + 1] < h->mate_off[m] + h->mate_len[m]) fail(LCTY_ERR_INVALID_INPUT, "mate offsets overlap");
    }
    hipStream_t s = ctx->stream;
    const uint64_t units = h->mate_off[2 * k] / 32;
    reserve_mates(k); size_units(units); h_len = h->mate_len;
    d_len.upload(h->mate_len, 2 * k, s); d_off.upload(h->mate_off, 2 * k + 1, s);
    if (units) LCTY_HIP(hipMemcpyAsync(d_bases.p, h->bases2, units * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    d_nm.upload(h->nmask, units, s);
}

void ReadChunk::view(lcty_reads_host* view) {
    if (!have_view) {
        h_off.assign(2 * n + 1, 0); zero_off.assign(n + 1, 0); h_bases.assign(2 * n_units + 2, 0); h_nm.assign(n_units + 1, 0);
        if (n) {
            ctx->activate();
            hipStream_t s = ctx->stream;
            d_off.download(h_off.data(), 2 * n + 1, s);
            if (n_units) LCTY_HIP(hipMemcpyAsync(h_bases.data(), d_bases.p, n_units * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            d_nm.download(h_nm.data(), n_units, s);
            LCTY_HIP(hipStreamSynchronize(s));
        }
        have_view = true;
    }
    memset(view, 0, sizeof(*view)); view->n_pairs = n;
    view->mate_len = h_len; view->mate_off = h_off.data(); view->bases2 = h_bases.data(); view->nmask = h_nm.data();
    view->aln_off = zero_off.data(); view->cigar_off = zero_off.data();
}

void ReadChunk::recruit(lcty_targets* targets, uint32_t max_out, uint32_t* out_cnt, uint32_t* out_loci) const {
    if (targets_ctx(targets) != ctx) fail(LCTY_ERR_INVALID_INPUT, "the targets and the reads belong to different contexts");
    if (n == 0) return;
    ctx->activate();
    recruit_device_view(targets, n, h_len, d_len.p, d_off.p, reinterpret_cast<const uint32_t*>(d_bases.p), d_nm.p, paired ? 1 : 0, max_out, out_cnt, out_loci);
}

}  // namespace lcty
