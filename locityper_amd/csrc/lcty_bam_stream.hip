// lcty_bam_stream.hip — whole BAM files without an index, streamed through the device in windows:
// `locityper genotype|recruit -a reads.bam [-a ...] --no-index [-^]`,
//   src/seq/fastx.rs:1029-1043 process_readers!, 692-729 DirectBamReader, 423-453 PairedEndInterleaved, 587-611 BamRecord::read_from,
//   104-110 equal_names_fast
// Host (lcty_bam_stream_window.hpp): the files and their headers, windows of whole BGZF blocks inflated into one slice that is used
// again window after window (lcty_bgzf_read.hpp: zlib, or with knob "sample_bam_inflate" 1 the device), the chain of record lengths,
// the carried tail, the enlarging, the change of file, the order of errors.
// Device, on the raw bytes of the window (records lie at any byte: every field is taken from two aligned dwords, ld32):
//   stream_record_kernel  a lane per record: the fixed fields, kept iff (flag & 0x900) == 0, the classes "shorter than its fields"
//                         and "no sequence"; the primaries are counted with one atomic per wavefront
//   exclusive_scan        over the kept flags -> the window's stream (stream_kernel); a carried first mate is its record 0
//   stream_pair_kernel    a lane per pair (places 2 i, 2 i + 1): equal_names_fast on the two names, refused at the second mate's
//                         record; an odd last place is reported as waiting
//   assemble_kernel (lcty_bam_layout.hpp), ReadChunk::place (lcty_read_chunk.hpp), unpack_kernel<true> (lcty_bam_record.hpp): the mates
//                         and their bases, as lcty_sample_bam_fetch lays them out, in one chunk whose buffers serve every window
// Every lane writes words of its own only; the one atomic beside the count is the minimum of the error word: two runs give the same bytes.
#include <memory>
#include <string>
#include <vector>

#include "lcty_bam_layout.hpp"
#include "lcty_bam_stream_window.hpp"
#include "lcty_objects.hpp"
#include "lcty_sample_bam.hpp"
#include "lcty_scan.hpp"

using namespace lcty;
namespace bs = lcty::bam_stream;

namespace {

__global__ __launch_bounds__(256) void stream_record_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, uint32_t n_rec,
                                                            uint32_t* __restrict__ kept, uint32_t* __restrict__ n_primary, unsigned long long* err) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool primary = false;
    if (r < n_rec) {
        const RecHead h = rec_head(raw, rec_off[r]);
        const bool fits = rec_fits(h);
        primary = fits && (h.flag & 0x900u) == 0;                                // read_from: min_start is i64::MIN, nothing else matters
        kept[r] = primary ? 1u : 0u;
        if (!fits) refuse(err, r, bs::E_SHORT);
        else if (primary && h.l_seq == 0) refuse(err, r, bs::E_NOSEQ);           // fastx.rs:599-602
    }
    const unsigned long long prim = __ballot(primary);
    if (lane == 0 && prim) atomicAdd(n_primary, static_cast<uint32_t>(__popcll(prim)));
}

// equal_names_fast (fastx.rs:104-110) on the names, without their NUL, of the records at places 2 i and 2 i + 1 of the stream
__global__ __launch_bounds__(256) void stream_pair_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ stream,
                                                          uint32_t n_stream, uint32_t* __restrict__ wait_rec, unsigned long long* err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (2ull * i >= n_stream) return;
    const uint32_t ra = stream[2 * i];
    if (2 * i + 1 == n_stream) { *wait_rec = ra; return; }                       // waits: the host decides at the end of the input
    const uint32_t rb = stream[2 * i + 1];
    const uint64_t oa = rec_off[ra], ob = rec_off[rb];
    const uint32_t la = ld32(raw, oa + 12) & 0xFFu, lb = ld32(raw, ob + 12) & 0xFFu;
    const uint32_t n = la ? la - 1u : 0u;
    bool ok = la == lb;
    if (ok && n > 3u) ok = (ld32(raw, oa + 36 + n - 3u) & 0xFFu) == (ld32(raw, ob + 36 + n - 3u) & 0xFFu);
    if (!ok) refuse(err, rb, bs::E_MISMATCH);
}

// ---- the executor of lcty_bam_stream_window.hpp on the device
struct DevExec {
    lcty_ctx* ctx;
    lcty_sample_reads R;                             // the current chunk, its buffers and its slice F (the window) used again window after window
    DevBuf<uint64_t> d_rec_off;
    DevBuf<uint32_t> d_kept, d_scan, d_stream, d_words, d_units, d_src, d_src_stream;     // d_words: [0] primaries, [1] the waiting record
    ErrWord err; ScanTotal scan_total;
    const uint32_t* raw = nullptr;
    uint32_t n_rec = 0, n_stream = 0;
    double ms_upload = 0, ms_record = 0, ms_pair = 0, ms_unpack = 0;
    explicit DevExec(lcty_ctx* c) : ctx(c), R(c, ReadChunk::Buffers::Reused) {}

    uint8_t* alloc(uint64_t n) { R.clear(); R.F.alloc(ctx, n); return R.F.slice; }
    uint8_t* inflate(std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks, uint64_t total, const char* path) {
        R.clear();
        check_inflate_knob(ctx);
        R.F.comp.swap(comp); R.F.blocks.swap(blocks); R.F.total = total;
        R.F.inflate(ctx, path);
        return R.F.slice;
    }
    void put_front(const uint8_t* p, uint64_t n) { R.F.put_front(p, n, ctx->stream); }
    std::vector<uint64_t>& rec_off() { return R.F.rec_off; }

    void scan(bool interleaved, bs::Scanned& S) {
        ctx->activate();
        hipStream_t s = ctx->stream;
        const std::vector<uint64_t>& ro = R.F.rec_off;
        n_rec = static_cast<uint32_t>(ro.size());
        double t0 = now_ms();
        raw = reinterpret_cast<const uint32_t*>(R.F.device(s));
        d_rec_off.ensure_slack(n_rec); d_rec_off.upload(ro.data(), n_rec, s);
        LCTY_HIP(hipStreamSynchronize(s));
        ms_upload += now_ms() - t0;

        t0 = now_ms();
        d_kept.alloc(n_rec); d_words.ensure(2);
        static const uint32_t init[2] = {0u, NONE32};
        d_words.upload(init, 2, s);
        unsigned long long* d_err = err.reset(s);
        hipLaunchKernelGGL(stream_record_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, raw, d_rec_off.p, n_rec, d_kept.p, d_words.p, d_err);
        LCTY_HIP(hipGetLastError());
        n_stream = scan_total.run(d_kept, d_scan, n_rec, ctx);
        d_stream.ensure_slack(std::max<uint32_t>(n_stream, 1));
        hipLaunchKernelGGL(stream_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, n_rec, d_kept.p, d_scan.p, static_cast<const uint64_t*>(nullptr), d_stream.p,
                           static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr));
        LCTY_HIP(hipGetLastError());
        LCTY_HIP(hipStreamSynchronize(s));
        ms_record += now_ms() - t0;

        t0 = now_ms();
        if (interleaved && n_stream) {
            hipLaunchKernelGGL(stream_pair_kernel, dim3(blocks_of((static_cast<uint64_t>(n_stream) + 1) / 2, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_stream.p,
                               n_stream, d_words.p + 1, d_err);
            LCTY_HIP(hipGetLastError());
        }
        uint32_t words[2] = {0, NONE32};
        d_words.download(words, 2, s);
        uint64_t r; uint32_t cls;
        const bool any = err.take(s, r, cls);                                    // synchronises
        S.n_kept = n_stream; S.n_primary = words[0]; S.wait_rec = words[1];
        if (any) {
            S.ev_rec = static_cast<uint32_t>(r); S.ev_cls = cls;
            d_scan.download(&S.kept_before_ev, 1, s, S.ev_rec);
            if (cls == bs::E_MISMATCH) {
                LCTY_HIP(hipStreamSynchronize(s));
                d_stream.download(&S.ev_first, 1, s, S.kept_before_ev - 1);       // the second mate sits at an odd place: there is one in front
            }
            LCTY_HIP(hipStreamSynchronize(s));
        }
        ms_pair += now_ms() - t0;
    }

    uint64_t emit(uint32_t n_lim, uint32_t n_out, bool interleaved) {
        ctx->activate();
        hipStream_t s = ctx->stream;
        const double t0 = now_ms();
        const uint64_t M = 2ull * n_out;
        ReadChunk& C = R.chunk; C.reserve_mates(n_out);
        d_src_stream.ensure_slack(M); d_src.ensure_slack(M); d_units.alloc(M);
        hipLaunchKernelGGL(assemble_kernel, dim3(blocks_of(n_lim, 256)), dim3(256), 0, s, raw, d_rec_off.p, static_cast<const uint32_t*>(nullptr), d_stream.p, n_lim,
                           interleaved ? MATES_INTERLEAVED : MATES_SINGLE, static_cast<const uint32_t*>(nullptr), static_cast<const uint32_t*>(nullptr), d_src.p,
                           d_src_stream.p, C.d_len.p, d_units.p);
        LCTY_HIP(hipGetLastError());
        const uint32_t n_units = C.place(d_units, M, scan_total);
        if (n_units)
            hipLaunchKernelGGL(unpack_kernel<true>, dim3(blocks_of(n_units, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_src.p, C.d_unit_off.p, static_cast<uint32_t>(M),
                               n_units, C.d_bases.p, C.d_nm.p);
        LCTY_HIP(hipGetLastError());
        R.h_src.resize(M); R.h_src_stream.resize(M);
        d_src_stream.download(R.h_src_stream.data(), M, s); d_src.download(R.h_src.data(), M, s);
        LCTY_HIP(hipStreamSynchronize(s));
        uint64_t bases = 0;
        for (uint64_t m = 0; m < M; m++) bases += C.h_len[m];
        ms_unpack += now_ms() - t0;
        return bases;
    }
};

}  // namespace

struct lcty_bam_stream {
    lcty_ctx* ctx;
    DevExec exec;
    bs::Stream<DevExec> st;
    double ms_total = 0;
    explicit lcty_bam_stream(lcty_ctx* c) : ctx(c), exec(c), st(exec) {}
};

namespace {

void fill_stats(const lcty_bam_stream* b, lcty_bam_stream_stats* S) {
    const bs::Counters& C = b->st.C;
    S->files = C.files; S->file_bytes = C.file_bytes; S->bytes_read = C.bytes_read; S->blocks_inflated = C.blocks_inflated; S->bytes_inflated = C.bytes_inflated;
    S->windows = C.windows; S->windows_enlarged = C.windows_enlarged; S->bytes_carried = C.bytes_carried;
    S->records_walked = C.records_walked; S->records_primary = C.records_primary; S->records_kept = C.records_kept; S->bases_kept = C.bases_kept;
    S->reads = C.reads; S->first_kept = C.first_kept;
    S->ms_read = C.ms_read; S->ms_inflate = C.ms_inflate; S->ms_walk = C.ms_walk;
    S->ms_upload = b->exec.ms_upload; S->ms_record = b->exec.ms_record; S->ms_pair = b->exec.ms_pair; S->ms_unpack = b->exec.ms_unpack; S->ms_total = b->ms_total;
}

}  // namespace

extern "C" {

int32_t lcty_bam_stream_open(lcty_ctx* ctx, const char* const* paths, uint32_t n_paths, int32_t interleaved, lcty_bam_stream** out) {
    if (out) *out = nullptr;
    return guarded([&] {
        if (!ctx || !paths || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_paths == 0) fail(LCTY_ERR_INVALID_INPUT, "no input file");
        check_inflate_knob(ctx);
        std::unique_ptr<lcty_bam_stream> b(new lcty_bam_stream(ctx));
        b->exec.R.chunk.paired = interleaved != 0;
        b->st.open(paths, n_paths, interleaved != 0, ctx->knob("bam_stream_window_bytes", static_cast<int64_t>(bs::WINDOW_DEFAULT)),
                   ctx->knob("bam_stream_window_limit", static_cast<int64_t>(bs::LIMIT_DEFAULT)));
        *out = b.release();
    });
}

void lcty_bam_stream_close(lcty_bam_stream* s) { delete s; }

int32_t lcty_bam_stream_next(lcty_bam_stream* b, lcty_sample_reads** reads, uint64_t* n, lcty_bam_stream_stats* stats) {
    if (n) *n = 0;
    if (reads) *reads = nullptr;
    return guarded([&] {
        if (!b || !reads || !n) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double t0 = now_ms();
        b->ctx->activate();
        b->exec.R.clear();
        try {
            const bs::Chunk c = b->st.next();
            if (!c.n) b->exec.R.clear();
            *n = c.n;
        } catch (...) {
            b->exec.R.clear();
            b->ms_total += now_ms() - t0;
            if (stats) fill_stats(b, stats);
            throw;
        }
        b->ms_total += now_ms() - t0;
        if (stats) fill_stats(b, stats);
        *reads = &b->exec.R;
    });
}

}  // extern "C"
