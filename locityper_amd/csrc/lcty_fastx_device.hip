// lcty_fastx_device.hip — FASTA / FASTQ text parsed on the device, ahead of recruitment: the route beside lcty_fastx.hip
// for `locityper genotype -i reads_1.fq.gz reads_2.fq.gz`. The host reads windows of text into a page-locked slice (containers,
// carried tails, cursors and the order of errors: lcty_fastx_window.hpp); the kernels here make of one window
//   lines     the positions of its '\n' bytes, compacted in order (nl_count_kernel, exclusive scan, nl_place_kernel)
//   records   a 16-byte row and a class per record by the rules of lcty_fastx_parse.hpp, the smallest (record, class) in one word
//             (fastq_record_kernel; FASTA: fasta_line_kernel, two scans, fasta_header_kernel, fasta_record_kernel; names_kernel for pairs)
// and of the records of one call a chunk of reads resident on the device (ReadChunk, lcty_read_chunk.hpp), used again call after call:
//   layout    mate_len and every mate's units of 32 bases (layout_kernel); ReadChunk::place makes mate_off of them: the layout of
//             pack() in lcty_fastx.hip
//   pack      bases2 / nmask through base_bits (lcty_seq.hpp), one lane per 32 bases of a mate: it owns one nmask word and two
//             bases2 words and writes them whole, so nothing is zeroed first and no two lanes meet (pack_kernel)
// which view, recruit and lcty_recruited_add_fastx take as it lies. No kernel uses LDS or depends on timing: the only atomic is the error word's minimum.
#include <memory>
#include <string>
#include <vector>

#include "lcty_bgzf_read.hpp"
#include "lcty_common.hpp"
#include "lcty_device.hpp"
#include "lcty_fastx_parse.hpp"
#include "lcty_fastx_window.hpp"
#include "lcty_read_chunk.hpp"
#include "lcty_scan.hpp"
#include "lcty_seq.hpp"
#include "lcty_writers.hpp"

using namespace lcty;
using fastx::Row;
using fastx::Text;

namespace {

constexpr uint32_t THREADS = 256;

// ---- lines: 16 bytes a lane, read as four dwords (the slice is padded by SLICE_PAD bytes; bytes from n on do not count)
__device__ __forceinline__ uint32_t newlines_of(const uint4* __restrict__ text, uint32_t i, uint32_t n, uint32_t (&w)[4]) {
    const uint4 v = text[i];
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    uint32_t mask = 0;                                                     // bit k: byte 16 i + k is '\n'
    for (uint32_t d = 0; d < 4; d++)
        for (uint32_t b = 0; b < 4; b++)
            if (((w[d] >> (8 * b)) & 0xFFu) == '\n' && 16ull * i + 4 * d + b < n) mask |= 1u << (4 * d + b);
    return mask;
}
__global__ __launch_bounds__(THREADS) void nl_count_kernel(const uint4* __restrict__ text, uint32_t n, uint32_t n16, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n16) return;
    uint32_t w[4];
    cnt[i] = __popc(newlines_of(text, i, n, w));
}
__global__ __launch_bounds__(THREADS) void nl_place_kernel(const uint4* __restrict__ text, uint32_t n, uint32_t n16, const uint32_t* __restrict__ off,
                                                           uint32_t n_nl, uint32_t* __restrict__ nl) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n16) return;
    uint32_t w[4];
    uint32_t mask = newlines_of(text, i, n, w), at = off[i];
    while (mask && at < n_nl) {
        const uint32_t k = __ffs(mask) - 1;
        nl[at++] = 16 * i + k;
        mask &= mask - 1;
    }
}

// ---- records
__global__ __launch_bounds__(THREADS) void fastq_record_kernel(Text T, uint32_t n_rec, Row* __restrict__ rows, unsigned long long* err) {
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_rec) return;
    Row row;
    const uint32_t cls = fastx::fastq_record(T, r, row);
    rows[r] = row;
    if (cls) refuse(err, r, cls);
}
__global__ __launch_bounds__(THREADS) void fasta_line_kernel(Text T, uint32_t* __restrict__ is_header, uint32_t* __restrict__ bases) {
    const uint32_t j = blockIdx.x * THREADS + threadIdx.x;
    if (j >= T.n_lines) return;
    uint32_t h, b;
    fastx::fasta_line(T, j, h, b);
    is_header[j] = h; bases[j] = b;
}
__global__ __launch_bounds__(THREADS) void fasta_header_kernel(uint32_t n_lines, const uint32_t* __restrict__ is_header, const uint32_t* __restrict__ rank,
                                                               uint32_t n_hdr, uint32_t* __restrict__ hdr_line) {
    const uint32_t j = blockIdx.x * THREADS + threadIdx.x;
    if (j < n_lines && is_header[j] && rank[j] < n_hdr) hdr_line[rank[j]] = j;
}
__global__ __launch_bounds__(THREADS) void fasta_record_kernel(Text T, const uint32_t* __restrict__ hdr_line, const uint32_t* __restrict__ cum, uint32_t n_hdr,
                                                               uint32_t n_rec, bool final, Row* __restrict__ rows, unsigned long long* err) {
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_hdr) return;
    Row row;
    const uint32_t cls = fastx::fasta_record(T, r, hdr_line, cum, n_hdr, final, row);
    rows[r] = row;
    if (cls && r < n_rec) refuse(err, r, cls);
}
// pair i < n: records ra + sa i of one window and rb + sb i of another (or the same)
__global__ __launch_bounds__(THREADS) void names_kernel(const uint8_t* __restrict__ ta, const Row* __restrict__ rows_a, uint32_t ra, uint32_t sa,
                                                        const uint8_t* __restrict__ tb, const Row* __restrict__ rows_b, uint32_t rb, uint32_t sb, uint32_t n,
                                                        unsigned long long* err) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    if (!fastx::equal_names_fast(ta, rows_a[ra + sa * i], tb, rows_b[rb + sb * i])) refuse(err, i, fastx::C_MISMATCH);
}

// ---- the records of one call
struct MateSrc {                         // mate e of unit i: row rec0 + stride i of a window
    const uint8_t* text; const Row* rows; const uint32_t* cum; uint32_t rec0, n_lines, n_nl, n; const uint32_t* nl; bool fasta;
};
struct ChunkView { MateSrc src[2]; uint32_t k, per, stride; };

__global__ __launch_bounds__(THREADS) void layout_kernel(ChunkView V, uint32_t* __restrict__ mate_len, uint32_t* __restrict__ units) {
    const uint32_t m = blockIdx.x * THREADS + threadIdx.x;
    if (m >= 2 * V.k) return;
    const uint32_t e = m & 1u, i = m >> 1;
    const uint32_t len = e < V.per ? V.src[e].rows[V.src[e].rec0 + V.stride * i].len : 0u;
    mate_len[m] = len; units[m] = (len + 31) / 32;
}
// One lane per 32 bases. FASTQ: the bases are one run of bytes, read as nine dwords around them. FASTA: a unit may span lines; its
// owner gathers the bytes from them (no lane writes a word another lane writes, so no atomic OR and no zeroed output are needed).
__global__ __launch_bounds__(THREADS) void pack_kernel(ChunkView V, const uint32_t* __restrict__ unit_off, uint32_t n_units, uint64_t* __restrict__ bases64,
                                                       uint32_t* __restrict__ nmask) {
    const uint32_t u = blockIdx.x * THREADS + threadIdx.x;
    if (u >= n_units) return;
    const uint32_t m = flat_owner(unit_off, 2 * V.k, u);
    const MateSrc& S = V.src[m & 1u];
    const Row row = S.rows[S.rec0 + V.stride * (m >> 1)];
    const uint32_t k0 = 32 * (u - unit_off[m]), cnt = min(32u, row.len - k0);
    uint64_t two = 0; uint32_t nm = 0;
    if (!S.fasta) {
        const uint32_t p = row.seq + k0, sh = (p & 3u) * 8u;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(S.text) + (p >> 2);
        uint32_t prev = w[0];
        for (uint32_t d = 0; d < 8; d++) {
            const uint32_t next = w[d + 1];
            const uint32_t v = sh ? (prev >> sh) | (next << (32u - sh)) : prev;
            prev = next;
            for (uint32_t b = 0; b < 4; b++) {
                uint32_t t, x;
                base_bits(static_cast<uint8_t>(v >> (8 * b)), t, x);
                const uint32_t at = 4 * d + b;
                if (at < cnt) { two |= static_cast<uint64_t>(t) << (2 * at); nm |= x << at; }
            }
        }
    } else {
        Text T{S.text, S.n, S.nl, S.n_nl, S.n_lines};
        uint32_t j = fastx::fasta_line_of(S.cum, row, S.n_lines, k0), b, e;
        fastx::line_span(T, j, b, e);
        uint32_t p = b + (S.cum[row.seq] + k0 - S.cum[j]);
        for (uint32_t at = 0; at < cnt; at++) {
            while (p >= e) { j++; fastx::line_span(T, j, b, e); p = b; }
            uint32_t t, x;
            base_bits(S.text[p++], t, x);
            two |= static_cast<uint64_t>(t) << (2 * at); nm |= x << at;
        }
    }
    bases64[u] = two; nmask[u] = nm;
}

// ---- the executor of lcty_fastx_window.hpp on the device
struct DevExec {
    // the slice of a window; when the window is done with, it goes back to its executor, whose next window takes it again: one
    // page-locked buffer and one device buffer per file and role for the life of the handle, not one of each per window
    struct Buffer {
        std::unique_ptr<Slice> s;
        DevExec* home = nullptr;
        Buffer() = default;
        Buffer(const Buffer&) = delete;
        Buffer& operator=(const Buffer&) = delete;
        Buffer& operator=(Buffer&& o) noexcept {
            if (this != &o) { give_back(); s = std::move(o.s); home = o.home; }
            return *this;
        }
        ~Buffer() { give_back(); }
        void give_back() noexcept {
            if (!s || !home) return;
            try { home->spare.push_back(std::move(s)); } catch (...) { s.reset(); }
        }
        uint8_t* data() const { return s ? s->slice : nullptr; }
    };
    std::vector<std::unique_ptr<Slice>> spare;
    void take(Buffer& b) {
        b.give_back();
        if (spare.empty()) b.s.reset(new Slice());
        else { b.s = std::move(spare.back()); spare.pop_back(); }
        b.home = this;
    }
    struct FileDev {
        const uint8_t* text = nullptr; uint32_t n = 0, n_nl = 0, n_lines = 0; bool fasta = false;
        DevBuf<uint32_t> nl, cum, hdr_line; DevBuf<Row> rows;
    };
    lcty_ctx* ctx = nullptr;
    FileDev fd[2];
    ErrWord err; ScanTotal scan;
    double ms_upload = 0, ms_lines = 0, ms_records = 0;

    void alloc(Buffer& b, uint64_t n) { take(b); b.s->alloc(ctx, n); }
    void inflate(Buffer& b, std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks, uint64_t total, const char* path) {
        check_inflate_knob(ctx);
        take(b);
        b.s->comp.swap(comp); b.s->blocks.swap(blocks); b.s->total = total;
        b.s->inflate(ctx, path);
    }
    void put_front(Buffer& b, const uint8_t* p, uint64_t n) { b.s->put_front(p, n, ctx->stream); }

    void parse(int fi, Buffer& buf, uint32_t n, bool final, bool fasta, fastx::Parsed& P) {
        ctx->activate();
        hipStream_t s = ctx->stream;
        FileDev& F = fd[fi];
        double t0 = now_ms();
        F.text = buf.s->device(s); F.n = n; F.fasta = fasta;
        LCTY_HIP(hipStreamSynchronize(s));
        ms_upload += now_ms() - t0;

        // ---- lines
        t0 = now_ms();
        const uint32_t n16 = (n + 15) / 16;
        const uint4* text16 = reinterpret_cast<const uint4*>(F.text);
        DevBuf<uint32_t> d_cnt, d_off;
        d_cnt.alloc(std::max<uint32_t>(n16, 1));
        if (n16) hipLaunchKernelGGL(nl_count_kernel, dim3(blocks_of(n16, THREADS)), dim3(THREADS), 0, s, text16, n, n16, d_cnt.p);
        LCTY_HIP(hipGetLastError());
        F.n_nl = scan.run(d_cnt, d_off, n16, ctx);
        F.nl.alloc(std::max<uint32_t>(F.n_nl, 1));
        uint32_t last_nl = 0;
        if (F.n_nl) {
            hipLaunchKernelGGL(nl_place_kernel, dim3(blocks_of(n16, THREADS)), dim3(THREADS), 0, s, text16, n, n16, d_off.p, F.n_nl, F.nl.p);
            LCTY_HIP(hipGetLastError());
            F.nl.download(&last_nl, 1, s, F.n_nl - 1);
        }
        LCTY_HIP(hipStreamSynchronize(s));
        F.n_lines = fastx::n_lines_of(n, F.n_nl, last_nl, final);
        ms_lines += now_ms() - t0;

        // ---- records
        t0 = now_ms();
        const Text T{F.text, n, F.nl.p, F.n_nl, F.n_lines};
        unsigned long long* d_err = err.reset(s);
        uint32_t n_rows = 0;
        if (!fasta) {
            P.n_rec = final ? (F.n_lines + 3) / 4 : F.n_nl / 4;
            n_rows = P.n_rec;
            F.rows.alloc(std::max<uint32_t>(n_rows, 1));
            uint32_t end_nl = 0;
            if (P.n_rec) {
                hipLaunchKernelGGL(fastq_record_kernel, dim3(blocks_of(P.n_rec, THREADS)), dim3(THREADS), 0, s, T, P.n_rec, F.rows.p, d_err);
                LCTY_HIP(hipGetLastError());
                if (!final) F.nl.download(&end_nl, 1, s, 4ull * P.n_rec - 1);
            }
            P.rows.resize(n_rows);
            F.rows.download(P.rows.data(), n_rows, s);
            LCTY_HIP(hipStreamSynchronize(s));
            P.covered = final ? n : P.n_rec ? end_nl + 1 : 0;
        } else {
            DevBuf<uint32_t> d_hdr, d_bases, d_rank;
            d_hdr.alloc(std::max<uint32_t>(F.n_lines, 1)); d_bases.alloc(std::max<uint32_t>(F.n_lines, 1));
            if (F.n_lines) hipLaunchKernelGGL(fasta_line_kernel, dim3(blocks_of(F.n_lines, THREADS)), dim3(THREADS), 0, s, T, d_hdr.p, d_bases.p);
            LCTY_HIP(hipGetLastError());
            const uint32_t n_hdr = scan.run(d_hdr, d_rank, F.n_lines, ctx);
            scan.run(d_bases, F.cum, F.n_lines, ctx);
            F.hdr_line.alloc(std::max<uint32_t>(n_hdr, 1));
            n_rows = n_hdr;
            P.n_rec = final ? n_hdr : n_hdr ? n_hdr - 1 : 0;
            F.rows.alloc(std::max<uint32_t>(n_rows, 1));
            if (n_hdr) {
                hipLaunchKernelGGL(fasta_header_kernel, dim3(blocks_of(F.n_lines, THREADS)), dim3(THREADS), 0, s, F.n_lines, d_hdr.p, d_rank.p, n_hdr, F.hdr_line.p);
                hipLaunchKernelGGL(fasta_record_kernel, dim3(blocks_of(n_hdr, THREADS)), dim3(THREADS), 0, s, T, F.hdr_line.p, F.cum.p, n_hdr, P.n_rec, final,
                                   F.rows.p, d_err);
                LCTY_HIP(hipGetLastError());
            }
            P.rows.resize(n_rows); P.nl.resize(F.n_nl); P.cum.resize(F.n_lines + 1);
            F.rows.download(P.rows.data(), n_rows, s);
            F.nl.download(P.nl.data(), F.n_nl, s);
            F.cum.download(P.cum.data(), F.n_lines + 1, s);
            LCTY_HIP(hipStreamSynchronize(s));
            P.covered = final ? n : n_hdr ? P.rows[n_hdr - 1].name_beg - 1 : 0;
        }
        uint64_t r; uint32_t cls;
        if (err.take(s, r, cls)) { P.ev_rec = static_cast<uint32_t>(r); P.ev_cls = cls; }
        ms_records += now_ms() - t0;
    }

    uint32_t mismatch(int fa, uint32_t ra, uint32_t sa, int fb, uint32_t rb, uint32_t sb, uint32_t n) {
        if (!n) return 0;
        ctx->activate();
        hipStream_t s = ctx->stream;
        const double t0 = now_ms();
        unsigned long long* d_err = err.reset(s);
        hipLaunchKernelGGL(names_kernel, dim3(blocks_of(n, THREADS)), dim3(THREADS), 0, s, fd[fa].text, fd[fa].rows.p, ra, sa, fd[fb].text, fd[fb].rows.p, rb, sb, n,
                           d_err);
        LCTY_HIP(hipGetLastError());
        uint64_t r; uint32_t cls;
        const bool any = err.take(s, r, cls);
        ms_records += now_ms() - t0;
        return any ? static_cast<uint32_t>(r) : n;
    }
};

}  // namespace

struct lcty_fastx_device {
    lcty_ctx* ctx;
    DevExec exec;
    fastx::Stream<DevExec> st;
    fastx::Chunk chunk;
    ReadChunk reads;                          // the current chunk on the device
    DevBuf<uint32_t> d_units;
    double ms_pack = 0, ms_total = 0;
    explicit lcty_fastx_device(lcty_ctx* c) : ctx(c), st(exec), reads(c, ReadChunk::Buffers::Reused) { exec.ctx = c; }
};

namespace {

void fill_stats(const lcty_fastx_device* f, lcty_fastx_device_stats* S) {
    const fastx::Counters& C = f->st.C;
    S->bytes_read = C.bytes_read; S->bytes_inflated = C.bytes_inflated; S->windows = C.windows; S->windows_enlarged = C.windows_enlarged;
    S->records = C.records; S->ms_read = C.ms_read; S->ms_inflate = C.ms_inflate;
    S->ms_upload = f->exec.ms_upload; S->ms_lines = f->exec.ms_lines; S->ms_records = f->exec.ms_records; S->ms_pack = f->ms_pack; S->ms_total = f->ms_total;
}

// layout and pack of the chunk the stream just handed out
void emit(lcty_fastx_device* f) {
    const fastx::Chunk& c = f->chunk;
    hipStream_t s = f->ctx->stream;
    const uint32_t k = c.k, M = 2 * k;
    ReadChunk& R = f->reads;
    R.clear(); R.paired = f->st.paired;
    if (!k) return;
    if (k >= (1u << 30)) fail(LCTY_ERR_UNSUPPORTED, "more than 2^30 records in one call");
    const double t0 = now_ms();
    ChunkView V{};
    V.k = k; V.per = static_cast<uint32_t>(c.per); V.stride = c.stride;
    for (int e = 0; e < 2; e++) {
        const DevExec::FileDev& F = f->exec.fd[c.file[e]];
        V.src[e] = MateSrc{F.text, F.rows.p, F.cum.p, c.rec0[e], F.n_lines, F.n_nl, F.n, F.nl.p, F.fasta};
    }
    R.reserve_mates(k); f->d_units.ensure_slack(M);
    hipLaunchKernelGGL(layout_kernel, dim3(blocks_of(M, THREADS)), dim3(THREADS), 0, s, V, R.d_len.p, f->d_units.p);
    LCTY_HIP(hipGetLastError());
    const uint32_t n_units = R.place(f->d_units, M, f->exec.scan);
    if (n_units) hipLaunchKernelGGL(pack_kernel, dim3(blocks_of(n_units, THREADS)), dim3(THREADS), 0, s, V, R.d_unit_off.p, n_units, R.d_bases.p, R.d_nm.p);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));
    f->ms_pack += now_ms() - t0;
}

}  // namespace

namespace lcty {

const ReadChunk& fastx_device_reads(const lcty_fastx_device* f) { return f->reads; }
// the name lcty_fastx_device_write_recruited writes for unit i: the header of its first record up to the first blank
std::string fastx_device_name(lcty_fastx_device* f, uint64_t i) {
    const fastx::Chunk& c = f->chunk;
    return f->st.name_of(f->st.f[c.file[0]], c.rec0[0] + c.stride * static_cast<uint32_t>(i));
}

}  // namespace lcty

extern "C" {

int32_t lcty_fastx_device_open(lcty_ctx* ctx, const char* path1, const char* path2, int32_t interleaved, lcty_fastx_device** out) {
    if (out) *out = nullptr;
    return guarded([&] {
        if (!ctx || !path1 || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (path2 && interleaved) fail(LCTY_ERR_INVALID_INPUT, "two input files cannot be interleaved as well");
        std::unique_ptr<lcty_fastx_device> f(new lcty_fastx_device(ctx));
        f->st.open(path1, path2, interleaved != 0, static_cast<uint64_t>(ctx->knob("fastx_window_bytes", static_cast<int64_t>(fastx::WINDOW_DEFAULT))),
                   static_cast<uint64_t>(ctx->knob("fastx_window_limit", static_cast<int64_t>(fastx::WINDOW_LIMIT))));
        *out = f.release();
    });
}

void lcty_fastx_device_close(lcty_fastx_device* f) { delete f; }

int32_t lcty_fastx_device_is_paired(const lcty_fastx_device* f, int32_t* paired) {
    return guarded([&] {
        if (!f || !paired) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *paired = f->st.paired ? 1 : 0;
    });
}

int32_t lcty_fastx_device_next(lcty_fastx_device* f, uint64_t max_records, uint64_t* n, lcty_fastx_device_stats* stats) {
    if (n) *n = 0;
    return guarded([&] {
        if (!f || !n) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double t0 = now_ms();
        f->ctx->activate();
        f->chunk = fastx::Chunk();
        f->reads.clear();
        try {
            f->chunk = f->st.next(max_records);
            emit(f);
        } catch (...) {
            f->chunk = fastx::Chunk();
            f->reads.clear();
            f->ms_total += now_ms() - t0;
            if (stats) fill_stats(f, stats);
            throw;
        }
        f->ms_total += now_ms() - t0;
        if (stats) fill_stats(f, stats);
        *n = f->chunk.k;
    });
}

int32_t lcty_fastx_device_view(lcty_fastx_device* f, lcty_reads_host* view) {
    return guarded([&] {
        if (!f || !view) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        f->reads.view(view);
    });
}

int32_t lcty_fastx_device_recruit(lcty_targets* targets, lcty_fastx_device* f, uint32_t max_out, uint32_t* out_cnt, uint32_t* out_loci) {
    return guarded([&] {
        if (!targets || !f || !out_cnt || !out_loci || max_out == 0) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        f->reads.recruit(targets, max_out, out_cnt, out_loci);
    });
}

int32_t lcty_fastx_device_write_recruited(lcty_fastx_device* f, lcty_fastx_writers* w, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci,
                                          uint64_t* n_written) {
    return guarded([&] {
        if (!f || !w || !out_cnt || !out_loci || max_out == 0) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const fastx::Chunk& c = f->chunk;
        const uint64_t written = write_recruited_units(w, c.k, max_out, out_cnt, out_loci, [&](uint64_t i, std::string& text) {
            for (int e = 0; e < c.per; e++) f->st.record_text(f->st.f[c.file[e]], c.rec0[e] + c.stride * static_cast<uint32_t>(i), text);      // [T; 2]::write_to: the mates one after the other
        });
        if (n_written) *n_written = written;
    });
}

}  // extern "C"
