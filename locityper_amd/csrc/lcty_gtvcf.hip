// lcty_gtvcf.hip — a cohort's genotypes as a phased VCF (extra/into_vcf.py): for one locus, the calls of every sample's predicted
// haplotypes in every record of the locus's window (copy_genotype 99-114, process_locus 126-142) and the text of the file; for all loci
// of a set, the merged file (merge_vcfs 167-196). The contract of every entry point is stated in the header and in DESIGN.md 5x; the
// host half (names, fixed point, header, tabix writer) is lcty_gtvcf_host.hpp. The text stage has the shape of lcty_pafvcf.hip's and
// shares its helpers (lcty_text.hpp); the sort is the shared one (lcty_sort.hpp).
#include <memory>
#include <string>
#include <vector>

#include "lcty_common.hpp"
#include "lcty_device.hpp"
#include "lcty_gtvcf_host.hpp"
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"
#include "lcty_text.hpp"

namespace {

using namespace lcty;
using namespace lcty::gtvcf;

constexpr int WG = 256;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t MAX_PLOIDY = 255, MAX_WARN = 65535;                   // keep the field widths of 256 samples inside 32 bits
constexpr uint32_t MAX_SAMPLES = 65535u * WG;                            // the join takes the samples in blocks of WG along grid.y
// the most bytes of ":value" for the four numbers of a sample (a sign, 19 digits and a point each) and the ":" of the warning or its `.`
constexpr uint64_t MAX_NUM_SUFFIX = 4 * (1 + 21) + 2;
// the first record / sample / record / position of every kind of failure
enum { F_BADCELL = 0, F_BADWARN = 1, F_LONGLINE = 2, F_LONGRUN = 3, F_COUNT = 4 };

struct Recs {
    const uint32_t* pos; const uint32_t* ref_len; const uint32_t* rec_allele; const uint64_t* allele_off; const uint8_t* allele_bytes;
    const uint64_t* id_off; const uint8_t* id_bytes;                     // id_off null: every ID is `.`
    uint32_t n_recs, n_haps;
};
struct Feats { const int64_t* num[4]; const uint64_t* warn_off; const char* warn; uint32_t mask; };   // a null array: absent for everyone
struct Cols {
    const uint32_t* pred_off; const int16_t* calls; const uint32_t* suf_off; const char* suf;
    uint32_t n_samples, n_slots;
};
struct Tail { char s[48]; uint32_t len; };                               // "\t.\t.\t.\t" + FORMAT
// one locus of a set as the kernels see it
struct LocusDev { Recs R; Cols C; const int64_t* qual10; const char* chrom; uint32_t chrom_len, contig_ix; };
// The lines of a file: line r restates record line_rec[r] (null: record r), and the field of sample s in it comes from record
// choice[r][s] (null: the line's own record). Records are numbered through the loci, locus l from rec0[l] on.
struct Lines { const LocusDev* loci; const uint32_t* rec0; const uint32_t* line_rec; const uint32_t* choice; uint32_t n_loci, n_samples; };
struct Src { const LocusDev* L; uint32_t r; };
__device__ inline Src src_of(const Lines& X, uint32_t g) {
    const uint32_t l = X.n_loci == 1 ? 0u : flat_owner(X.rec0, X.n_loci, g);
    return Src{X.loci + l, g - X.rec0[l]};
}

__device__ inline uint32_t feature_decimals(uint32_t f) { return f == 0 ? QUAL_DECIMALS : f == 3 ? WDIST_DECIMALS : 0; }

// ---- device: cells --------------------------------------------------------------------------------------------------------------------

// copy_genotype (99-114), one lane per (record, slot); consecutive lanes take consecutive slots of one record
__global__ __launch_bounds__(WG) void gtvcf_cells_kernel(Recs R, uint32_t n_slots, const uint32_t* __restrict__ pred_col, const int16_t* __restrict__ gt,
                                                         int16_t* __restrict__ calls, uint32_t* __restrict__ flags) {
    const uint32_t r = blockIdx.x, k = blockIdx.y * WG + threadIdx.x;
    if (k >= n_slots) return;
    const uint32_t col = pred_col[k];
    int32_t v = col == LCTY_GTVCF_REF ? 0 : gt[uint64_t(r) * R.n_haps + col];
    if (v < 0) v = -1;
    if (v >= int32_t(R.rec_allele[r + 1] - R.rec_allele[r])) atomicMin(&flags[F_BADCELL], r);
    calls[uint64_t(r) * n_slots + k] = int16_t(v);
}

// ---- device: the features of a sample, the same text in every record ------------------------------------------------------------------

__device__ inline bool warn_byte_ok(char c) { return c != '\t' && c != ' ' && c != '\n' && c != ':'; }

// one lane per sample: the bytes of ":value" for every selected feature, 0 for a sample without a prediction
__global__ __launch_bounds__(WG) void gtvcf_sufwidth_kernel(Feats F, uint32_t n_samples, const uint32_t* __restrict__ pred_off, uint32_t* __restrict__ width,
                                                            uint32_t* __restrict__ flags) {
    const uint32_t s = blockIdx.x * WG + threadIdx.x;
    if (s >= n_samples) return;
    uint32_t w = 0;
    if (pred_off[s] != pred_off[s + 1]) {
        for (uint32_t f = 0; f < 4; f++)
            if (F.mask >> f & 1) w += 1 + fixed_width(F.num[f] ? F.num[f][s] : LCTY_GTVCF_ABSENT, feature_decimals(f), false);
        if (F.mask >> 4 & 1) {
            const uint64_t w0 = F.warn_off ? F.warn_off[s] : 0, w1 = F.warn_off ? F.warn_off[s + 1] : 0;
            for (uint64_t x = w0; x < w1; x++) if (!warn_byte_ok(F.warn[x])) { atomicMin(&flags[F_BADWARN], s); break; }
            w += 1 + (w1 == w0 ? 1u : uint32_t(w1 - w0));
        }
    }
    width[s] = w;
}

__global__ __launch_bounds__(WG) void gtvcf_sufwrite_kernel(Feats F, uint32_t n_samples, const uint32_t* __restrict__ suf_off, char* __restrict__ suf) {
    const uint32_t s = blockIdx.x * WG + threadIdx.x;
    if (s >= n_samples || suf_off[s] == suf_off[s + 1]) return;
    char* at = suf + suf_off[s];
    for (uint32_t f = 0; f < 4; f++)
        if (F.mask >> f & 1) {
            const int64_t v = F.num[f] ? F.num[f][s] : LCTY_GTVCF_ABSENT;
            *at++ = ':';
            fixed_put(at, v, feature_decimals(f), false);
            at += fixed_width(v, feature_decimals(f), false);
        }
    if (F.mask >> 4 & 1) {
        const uint64_t w0 = F.warn_off ? F.warn_off[s] : 0, w1 = F.warn_off ? F.warn_off[s + 1] : 0;
        *at++ = ':';
        if (w0 == w1) *at = '.';
        for (uint64_t x = w0; x < w1; x++) at[x - w0] = F.warn[x];
    }
}

// ---- device: lines --------------------------------------------------------------------------------------------------------------------

// the record whose calls and features sample s shows in line r, whose own record is `own`
__device__ inline Src field_src(const Lines& X, uint32_t r, const Src& own, uint32_t g, uint32_t s) {
    if (!X.choice) return own;
    const uint32_t gs = X.choice[uint64_t(r) * X.n_samples + s];
    return gs == g ? own : src_of(X, gs);
}

// the tab and the field of sample s in record r of C (into_vcf.py:132-141)
__device__ inline uint32_t field_width(const Cols& C, uint32_t r, uint32_t s) {
    const uint32_t p0 = C.pred_off[s], p1 = C.pred_off[s + 1];
    if (p0 == p1) return 2;
    uint32_t w = 1 + (p1 - p0 - 1) + (C.suf_off[s + 1] - C.suf_off[s]);
    for (uint32_t k = p0; k < p1; k++) { const int32_t v = C.calls[uint64_t(r) * C.n_slots + k]; w += v < 0 ? 1u : n_digits(uint64_t(v)); }
    return w;
}

// the length of one line; one workgroup per line
__global__ __launch_bounds__(WG) void gtvcf_linelen_kernel(Lines X, uint32_t tail_len, uint64_t* __restrict__ line_len, uint32_t* __restrict__ flags) {
    __shared__ uint64_t part[WG / WAVE];
    const uint32_t r = blockIdx.x, g = X.line_rec ? X.line_rec[r] : r;
    const Src own = src_of(X, g);
    const Recs& R = own.L->R;
    const uint32_t ra = R.rec_allele[own.r], na = R.rec_allele[own.r + 1] - ra;
    uint64_t mine = 0;
    for (uint32_t a = 1 + threadIdx.x; a < na; a += WG) mine += 1 + (R.allele_off[ra + a + 1] - R.allele_off[ra + a]);
    for (uint32_t s = threadIdx.x; s < X.n_samples; s += WG) { const Src f = field_src(X, r, own, g, s); mine += field_width(f.L->C, f.r, s); }
    const uint64_t sum = block_sum<WG>(mine, part);
    if (threadIdx.x == 0) {
        const uint64_t id_len = R.id_off ? R.id_off[own.r + 1] - R.id_off[own.r] : 0;
        const uint64_t len = own.L->chrom_len + 1 + n_digits(uint64_t(R.pos[own.r]) + 1) + 1 + (id_len ? id_len : 1) + 1 + (R.allele_off[ra + 1] - R.allele_off[ra]) +
                             (na == 1 ? 2 : 0) + tail_len + sum + 1;
        line_len[r + 1] = len;
        if (len > 0xFFFFFFFFull) atomicMin(&flags[F_LONGLINE], r);
    }
}

// one line at its offset; one workgroup per line. The alleles lie back to back in the pool and go out in one pass over their bytes, the
// fields take a scan of their widths per 256 samples.
__global__ __launch_bounds__(WG) void gtvcf_write_kernel(Lines X, Tail T, const uint64_t* __restrict__ line_off, char* __restrict__ out) {
    __shared__ uint32_t wsum[WG / WAVE];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, g = X.line_rec ? X.line_rec[r] : r;
    const Src own = src_of(X, g);
    const Recs& R = own.L->R;
    char* line = out + line_off[r];
    uint64_t at = 0;
    const uint32_t chrom_len = own.L->chrom_len;
    for (uint32_t x = tid; x < chrom_len; x += WG) line[x] = own.L->chrom[x];
    at += chrom_len;
    const uint64_t pos = uint64_t(R.pos[own.r]) + 1;
    const uint32_t pd = n_digits(pos);
    if (tid == 0) { line[at] = '\t'; put_digits(line + at + 1, pos, pd); line[at + 1 + pd] = '\t'; }
    at += 2 + pd;
    const uint64_t i0 = R.id_off ? R.id_off[own.r] : 0, id_len = R.id_off ? R.id_off[own.r + 1] - i0 : 0;
    if (id_len == 0 && tid == 0) line[at] = '.';
    for (uint64_t x = tid; x < id_len; x += WG) line[at + x] = char(R.id_bytes[i0 + x]);
    at += id_len ? id_len : 1;
    const uint32_t ra = R.rec_allele[own.r], na = R.rec_allele[own.r + 1] - ra;
    const uint64_t o0 = R.allele_off[ra], total = R.allele_off[ra + na] - o0;
    for (uint32_t a = tid; a < na; a += WG) line[at + (R.allele_off[ra + a] - o0) + a] = a <= 1 ? '\t' : ',';
    for (uint64_t x = tid; x < total; x += WG) {
        const uint32_t a = flat_owner(R.allele_off + ra, na, o0 + x);
        line[at + x + a + 1] = char(R.allele_bytes[o0 + x]);
    }
    at += total + na;
    if (na == 1) { if (tid == 0) { line[at] = '\t'; line[at + 1] = '.'; } at += 2; }
    if (tid < T.len) line[at + tid] = T.s[tid];
    at += T.len;
    for (uint32_t s0 = 0; s0 < X.n_samples; s0 += WG) {
        const uint32_t s = s0 + tid;
        Src f = own;
        if (s < X.n_samples) f = field_src(X, r, own, g, s);
        const Cols& C = f.L->C;
        const uint32_t w = s < X.n_samples ? field_width(C, f.r, s) : 0u;
        uint32_t all = 0;
        const uint32_t before = block_place<WG>(w, wsum, &all);
        if (s < X.n_samples) {
            char* c = line + at + before;
            *c++ = '\t';
            const uint32_t p0 = C.pred_off[s], p1 = C.pred_off[s + 1];
            if (p0 == p1) *c = '.';
            for (uint32_t k = p0; k < p1; k++) {
                if (k > p0) *c++ = '|';
                const int32_t v = C.calls[uint64_t(f.r) * C.n_slots + k];
                if (v < 0) *c++ = '.';
                else { const uint32_t d = n_digits(uint64_t(v)); put_digits(c, uint64_t(v), d); c += d; }
            }
            const uint32_t f0 = C.suf_off[s], f1 = C.suf_off[s + 1];
            for (uint32_t x = f0; x < f1; x++) c[x - f0] = C.suf[x];
        }
        at += all;
    }
    if (tid == 0) line[at] = '\n';
}

// ---- device: the merge ----------------------------------------------------------------------------------------------------------------

// the key (contig, pos) of every record of every locus, and its number
__global__ __launch_bounds__(WG) void gtvcf_keys_kernel(Lines X, uint32_t n, uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
    const uint32_t g = blockIdx.x * WG + threadIdx.x;
    if (g >= n) return;
    const Src a = src_of(X, g);
    keys[g] = uint64_t(a.L->contig_ix) << 32 | a.L->R.pos[a.r];
    vals[g] = g;
}
__global__ __launch_bounds__(WG) void gtvcf_head_kernel(uint32_t n, const uint64_t* __restrict__ keys, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) head[i] = i == 0 || keys[i] != keys[i - 1];
}
// start[k] = the first item of group k (head: its flags, rank: their exclusive scan); start[n_groups] = n
__global__ __launch_bounds__(WG) void gtvcf_starts_kernel(uint32_t n, uint32_t n_groups, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank,
                                                          uint32_t* __restrict__ start) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n && head[i]) start[rank[i]] = i;
    if (i == 0) start[n_groups] = n;
}

// the allele tuples of two records as Python compares tuples of bytes (into_vcf.py:181, 192): element by element, bytewise, a proper
// prefix first. < 0, 0, > 0.
__device__ inline int compare_alleles(const Src& a, const Src& b) {
    const Recs& A = a.L->R; const Recs& B = b.L->R;
    const uint32_t ra = A.rec_allele[a.r], na = A.rec_allele[a.r + 1] - ra, rb = B.rec_allele[b.r], nb = B.rec_allele[b.r + 1] - rb;
    for (uint32_t e = 0; e < na && e < nb; e++) {
        const uint64_t a0 = A.allele_off[ra + e], la = A.allele_off[ra + e + 1] - a0, b0 = B.allele_off[rb + e], lb = B.allele_off[rb + e + 1] - b0;
        for (uint64_t x = 0; x < la && x < lb; x++) {
            const int d = int(A.allele_bytes[a0 + x]) - int(B.allele_bytes[b0 + x]);
            if (d) return d;
        }
        if (la != lb) return la < lb ? -1 : 1;
    }
    return na == nb ? 0 : na < nb ? -1 : 1;
}

// One wavefront per run of equal (contig, pos), a lane per record: the rank of a record is the number of records of the run before it in
// the order (allele tuple, order of arrival), which the stable sort left as the order of the loci. order: the records in output order;
// first: whether a record opens a key (the others are joined to it).
__global__ __launch_bounds__(WG) void gtvcf_run_kernel(Lines X, uint32_t n_runs, const uint32_t* __restrict__ run_start, const uint64_t* __restrict__ vals,
                                                       uint32_t* __restrict__ order, uint32_t* __restrict__ first, uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t run = blockIdx.x * (WG / WAVE) + threadIdx.x / WAVE;
    if (run >= n_runs) return;                                          // whole wavefronts leave
    const uint32_t i0 = run_start[run], len = run_start[run + 1] - i0;
    if (len > WAVE) { if (lane == 0) atomicMin(&flags[F_LONGRUN], i0); return; }
    const uint32_t g = lane < len ? uint32_t(vals[i0 + lane]) : 0u;
    const Src me = src_of(X, g);
    uint32_t rank = 0; bool opens = true;
    for (uint32_t m = 0; m < len; m++) {
        const uint32_t gm = __shfl(g, m);
        if (lane >= len || m == lane) continue;
        const int c = compare_alleles(src_of(X, gm), me);
        if (c < 0 || (c == 0 && m < lane)) rank++;
        if (c == 0 && m < lane) opens = false;
    }
    if (lane < len) { order[i0 + rank] = g; first[i0 + rank] = opens; }
}

__device__ inline int64_t floor_units(int64_t tenths) {                  // an absent quality is the lowest
    if (tenths == LCTY_GTVCF_ABSENT) return tenths;
    return tenths >= 0 ? tenths / 10 : -((-tenths + 9) / 10);
}

// The join of the records of one key, one lane per (line, sample): the first record in order keeps the sample's field; a later record
// replaces it iff the sample has a prediction there and either had none so far, or the GTs differ and the later record's quality in whole
// units is strictly larger. line_rec: the first record of every line.
__global__ __launch_bounds__(WG) void gtvcf_join_kernel(Lines X, const uint32_t* __restrict__ line_start, const uint32_t* __restrict__ order,
                                                        uint32_t* __restrict__ line_rec, uint32_t* __restrict__ choice) {
    const uint32_t line = blockIdx.x, s = blockIdx.y * WG + threadIdx.x;
    const uint32_t i0 = line_start[line], i1 = line_start[line + 1];
    if (s == 0) line_rec[line] = order[i0];
    if (s >= X.n_samples) return;
    uint32_t cur_g = order[i0];
    Src cur = src_of(X, cur_g);
    for (uint32_t i = i0 + 1; i < i1; i++) {
        const uint32_t g = order[i];
        const Src nxt = src_of(X, g);
        const Cols& A = cur.L->C; const Cols& B = nxt.L->C;
        const uint32_t a0 = A.pred_off[s], an = A.pred_off[s + 1] - a0, b0 = B.pred_off[s], bn = B.pred_off[s + 1] - b0;
        if (!bn) continue;
        bool take = an == 0;
        if (!take) {
            bool differ = an != bn;
            for (uint32_t k = 0; k < an && !differ; k++) differ = A.calls[uint64_t(cur.r) * A.n_slots + a0 + k] != B.calls[uint64_t(nxt.r) * B.n_slots + b0 + k];
            const int64_t qa = floor_units(cur.L->qual10 ? cur.L->qual10[s] : LCTY_GTVCF_ABSENT), qb = floor_units(nxt.L->qual10 ? nxt.L->qual10[s] : LCTY_GTVCF_ABSENT);
            take = differ && qb > qa;
        }
        if (take) { cur = nxt; cur_g = g; }
    }
    choice[uint64_t(line) * X.n_samples + s] = cur_g;
}

// what a tabix writer needs of every line; header_ix[l]: the place of locus l's contig among the contigs of the header
__global__ __launch_bounds__(WG) void gtvcf_lineinfo_kernel(Lines X, uint32_t n_lines, const uint32_t* __restrict__ header_ix, uint32_t* __restrict__ contig,
                                                            uint32_t* __restrict__ pos, uint32_t* __restrict__ ref_len) {
    const uint32_t r = blockIdx.x * WG + threadIdx.x;
    if (r >= n_lines) return;
    const Src a = src_of(X, X.line_rec[r]);
    contig[r] = header_ix[a.L - X.loci]; pos[r] = a.L->R.pos[a.r]; ref_len[r] = a.L->R.ref_len[a.r];
}

#define LAUNCH(kernel, grid, ...) do { hipLaunchKernelGGL(kernel, dim3 grid, dim3(WG), 0, s, __VA_ARGS__); LCTY_HIP(hipGetLastError()); } while (0)

template <typename T> void put(DevBuf<T>& d, const T* host, size_t n, hipStream_t s, uint64_t* bytes) {
    d.ensure(std::max<size_t>(n, 1));
    d.upload(host, n, s);
    *bytes += n * sizeof(T);
}

// offsets of a CSR array as the C interface takes them: ascending from 0
template <typename T> void check_off(const T* off, uint64_t n, const char* what) {
    if (off[0] != 0) fail(LCTY_ERR_INVALID_INPUT, "%s does not start at 0", what);
    for (uint64_t i = 0; i < n; i++) if (off[i + 1] < off[i]) fail(LCTY_ERR_INVALID_INPUT, "%s decreases at %llu", what, static_cast<unsigned long long>(i));
}

// what the set keeps of a locus: its records, the calls and the feature text of every sample
struct GtLocus {
    std::string name, chrom;
    uint32_t contig_ix = 0, start = 0, end = 0, n_recs = 0, n_haps = 0, n_samples = 0, n_slots = 0;
    uint64_t contig_len = 0;
    bool with_ids = false, with_qual = false;
    DevBuf<uint32_t> pos, ref_len, rec_allele, pred_off, suf_off;
    DevBuf<uint64_t> allele_off, id_off;
    DevBuf<uint8_t> allele_bytes, id_bytes;
    DevBuf<int16_t> calls;
    DevBuf<int64_t> qual10;
    DevBuf<char> suf, chrom_d;
    LocusDev view() const {
        return LocusDev{Recs{pos.p, ref_len.p, rec_allele.p, allele_off.p, allele_bytes.p, with_ids ? id_off.p : nullptr, id_bytes.p, n_recs, n_haps},
                        Cols{pred_off.p, calls.p, suf_off.p, suf.p, n_samples, n_slots}, with_qual ? qual10.p : nullptr, chrom_d.p, uint32_t(chrom.size()), contig_ix};
    }
};

}  // namespace

struct lcty_gtvcf {
    lcty_ctx* ctx = nullptr;
    std::vector<std::string> samples;
    uint32_t field_mask = 0;
    Tail tail{};
    std::vector<std::unique_ptr<GtLocus>> loci;
    // scratch of a call, grow-only
    DevBuf<uint32_t> pred_col, suf_w, flags, rec0;
    DevBuf<uint64_t> warn_off, line_len, line_off;
    DevBuf<int16_t> gt;
    DevBuf<int64_t> num[4];
    DevBuf<char> warn, text;
    DevBuf<LocusDev> views;
    // scratch of lcty_gtvcf_merge, grow-only as well
    DevBuf<uint64_t> ka, kb, va, vb;
    DevBuf<uint32_t> head, rank, run_start, order, first, line_start, line_rec, choice, header_ix, l_contig, l_pos, l_len;
    ScanTotal scan;
    RadixSort sorter;
};

namespace {

// The text stage over `n_lines` lines of X behind `header`: lengths, a 64-bit scan, every line at its offset, one download.
void text_stage(lcty_gtvcf& S, const Lines& X, uint32_t n_lines, const std::string& header, Handoff& h, lcty_gtvcf_out* o, lcty_gtvcf_stats* st, double* t) {
    lcty_ctx* ctx = S.ctx;
    hipStream_t s = ctx->stream;
    auto lap = [&](double* ms) { LCTY_HIP(hipStreamSynchronize(s)); const double now = now_ms(); *ms += now - *t; *t = now; };
    // line_len[0] is the header: the exclusive scan of n_lines + 1 lengths gives the header's 0, every line's offset and the end of the text
    S.line_len.ensure(size_t(n_lines) + 1); S.line_off.ensure(size_t(n_lines) + 2);
    const uint64_t header_len = header.size();
    S.line_len.upload(&header_len, 1, s);
    if (n_lines) LAUNCH(gtvcf_linelen_kernel, (n_lines), X, S.tail.len, S.line_len.p, S.flags.p);
    launch_scan<uint64_t>(s, uint64_t(n_lines) + 1, LoadU64{S.line_len.p}, AddOp{}, uint64_t(0), S.line_off.p, true);
    uint64_t text_len = 0; uint32_t flags[F_COUNT];
    S.line_off.download(&text_len, 1, s, size_t(n_lines) + 1);
    S.flags.download(flags, F_COUNT, s);
    lap(&st->widths_ms);
    if (flags[F_BADCELL] != NONE) fail(LCTY_ERR_INVALID_DATA, "record %u: a genotype names an allele the record does not have", flags[F_BADCELL]);
    if (flags[F_BADWARN] != NONE) fail(LCTY_ERR_INVALID_DATA, "sample `%s`: a warning text with a tab, a space, a newline or `:`", S.samples[flags[F_BADWARN]].c_str());
    if (flags[F_LONGLINE] != NONE) fail(LCTY_ERR_UNSUPPORTED, "line %u has 2^32 bytes or more", flags[F_LONGLINE]);
    S.text.ensure(text_len);
    S.text.upload(header.data(), header.size(), s);
    if (n_lines) LAUNCH(gtvcf_write_kernel, (n_lines), X, S.tail, S.line_off.p + 1, S.text.p);
    lap(&st->write_ms);
    o->text = static_cast<char*>(h.raw(text_len));
    S.text.download(o->text, text_len, s);
    o->text_len = text_len; o->n_lines = n_lines;
    o->line_off = static_cast<uint64_t*>(h.raw((size_t(n_lines) + 1) * 8));
    S.line_off.download(o->line_off, size_t(n_lines) + 1, s, 1);
    st->bytes_d2h += text_len + (uint64_t(n_lines) + 1) * 8;
    lap(&st->download_ms);
    st->header_bytes = header.size(); st->text_bytes = text_len;
}

void reset_flags(lcty_gtvcf& S, hipStream_t s, uint64_t* bytes) {
    static const uint32_t flags0[F_COUNT] = {NONE, NONE, NONE, NONE};
    put(S.flags, flags0, F_COUNT, s, bytes);
}

}  // namespace

extern "C" {

int32_t lcty_gtvcf_columns(const lcty_vcf_view* view, const char* genome_name, uint32_t n_names, const char* names, uint32_t* cols) {
    return guarded([&] {
        if (!view || !genome_name || (n_names && (!names || !cols))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const SampleIndex ix = sample_index(*view);
        const std::string genome(genome_name);
        std::vector<uint32_t> got(n_names);
        const char* p = names;
        for (uint32_t i = 0; i < n_names; i++) { const std::string name(p); p += name.size() + 1; got[i] = resolve_column(*view, ix, genome, name); }
        if (n_names) memcpy(cols, got.data(), 4 * size_t(n_names));           // all or nothing
    });
}

int32_t lcty_gtvcf_fixed_print(int64_t value, uint32_t decimals, int32_t pad, char* out, uint64_t cap, uint64_t* len) {
    return guarded([&] {
        if (!len) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (decimals > MAX_DECIMALS) fail(LCTY_ERR_INVALID_INPUT, "%u decimals (at most %u)", decimals, MAX_DECIMALS);
        const std::string s = fixed_text(value, decimals, pad != 0);
        *len = s.size();
        if (!out) return;
        if (cap < s.size()) fail(LCTY_ERR_INVALID_INPUT, "output buffer too small (%zu bytes)", s.size());
        memcpy(out, s.data(), s.size());
    });
}

int32_t lcty_gtvcf_fixed_parse(const char* text, uint32_t decimals, int64_t* value) {
    return guarded([&] {
        if (!text || !value) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (decimals > MAX_DECIMALS) fail(LCTY_ERR_INVALID_INPUT, "%u decimals (at most %u)", decimals, MAX_DECIMALS);
        *value = fixed_parse(text, decimals);
    });
}

int32_t lcty_gtvcf_header(uint32_t n_contigs, const char* contigs, const uint64_t* contig_len, uint32_t n_samples, const char* samples, char* out,
                          uint64_t cap, uint64_t* len) {
    return guarded([&] {
        if (!len || (n_contigs && !contigs) || (n_samples && !samples)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const std::string s = header_text(split_names(contigs ? contigs : "", n_contigs), contig_len, split_names(samples ? samples : "", n_samples));
        *len = s.size();
        if (!out) return;
        if (cap < s.size()) fail(LCTY_ERR_INVALID_INPUT, "output buffer too small (%zu bytes)", s.size());
        memcpy(out, s.data(), s.size());
    });
}

int32_t lcty_tbi_write(const char* path, uint32_t n_contigs, const char* contigs, uint64_t n_records, const uint32_t* contig_ix, const uint32_t* pos,
                       const uint32_t* ref_len, const uint64_t* line_off, const uint64_t* block_off, uint64_t n_blocks) {
    return guarded([&] {
        if (!path || (n_contigs && !contigs) || !line_off || !block_off || (n_records && (!contig_ix || !pos || !ref_len))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const std::string plain = tbi_plain(split_names(contigs ? contigs : "", n_contigs), n_records, contig_ix, pos, ref_len, line_off, block_off, n_blocks);
        const int32_t rc = lcty_io_write_bgzf(path, reinterpret_cast<const uint8_t*>(plain.data()), plain.size());
        if (rc != LCTY_OK) throw Error(rc, lcty_last_error());
    });
}

int32_t lcty_gtvcf_create(lcty_ctx* ctx, const char* samples, uint32_t n_samples, uint32_t field_mask, lcty_gtvcf** out) {
    if (out) *out = nullptr;
    return guarded([&] {
        if (!ctx || !out || (n_samples && !samples)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (field_mask & ~LCTY_GTVCF_ALL) fail(LCTY_ERR_INVALID_INPUT, "field_mask %u has bits beyond LCTY_GTVCF_ALL", field_mask);
        if (n_samples > MAX_SAMPLES) fail(LCTY_ERR_UNSUPPORTED, "%u samples (at most %u)", n_samples, MAX_SAMPLES);
        std::unique_ptr<lcty_gtvcf> S(new lcty_gtvcf());
        S->ctx = ctx; S->field_mask = field_mask;
        S->samples = split_names(samples ? samples : "", n_samples);
        for (uint32_t i = 0; i < n_samples; i++)
            if (S->samples[i].empty() || S->samples[i].find_first_of("\t\n") != std::string::npos) fail(LCTY_ERR_INVALID_INPUT, "sample %u: not a name of a VCF column", i);
        const std::string tail = "\t.\t.\t.\t" + format_key(field_mask);
        static_assert(sizeof("\t.\t.\t.\tGT:qual:reads:unexpl:wdist:warn") <= sizeof(Tail::s), "Tail holds the longest FORMAT key");
        memcpy(S->tail.s, tail.data(), tail.size()); S->tail.len = uint32_t(tail.size());
        *out = S.release();
    });
}

void lcty_gtvcf_destroy(lcty_gtvcf* set) { delete set; }

int32_t lcty_gtvcf_add_locus(lcty_gtvcf* set, const lcty_gtvcf_locus_in* in, lcty_gtvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!set || !in || !out || !in->chrom || !in->locus) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_gtvcf& S = *set;
        lcty_ctx* ctx = S.ctx;
        const uint32_t n_recs = in->n_recs, n_samples = uint32_t(S.samples.size());
        // ---- the arguments: every offset the kernels follow is checked here
        if (n_recs >= 0x7FFFFFF0u) fail(LCTY_ERR_UNSUPPORTED, "%u records", n_recs);
        if (n_recs && (!in->pos || !in->ref_len || !in->rec_allele || !in->allele_off)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_samples && !in->pred_off) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (in->end < in->start) fail(LCTY_ERR_INVALID_INPUT, "locus %s: the interval ends before it starts", in->locus);
        const size_t chrom_len = strlen(in->chrom);
        if (chrom_len == 0 || chrom_len > 0xFFFFu) fail(LCTY_ERR_INVALID_INPUT, "a contig name of %zu bytes", chrom_len);
        for (const auto& L : S.loci) {
            if (L->name == in->locus) fail(LCTY_ERR_INVALID_INPUT, "locus %s is in the set already", in->locus);
            if (L->contig_ix == in->contig_ix && (L->chrom != in->chrom || L->contig_len != in->contig_len))
                fail(LCTY_ERR_INVALID_INPUT, "locus %s: contig %u is %s (length %llu) in locus %s", in->locus, in->contig_ix, L->chrom.c_str(),
                     static_cast<unsigned long long>(L->contig_len), L->name.c_str());
        }
        uint64_t n_alleles = 0, pool = 0, id_len = 0;
        if (n_recs) {
            check_off(in->rec_allele, n_recs, "rec_allele");
            for (uint32_t r = 0; r < n_recs; r++) if (in->rec_allele[r + 1] == in->rec_allele[r]) fail(LCTY_ERR_INVALID_INPUT, "record %u has no allele", r);
            n_alleles = in->rec_allele[n_recs];
            check_off(in->allele_off, n_alleles, "allele_off");
            pool = in->allele_off[n_alleles];
            if (pool && !in->allele_bytes) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            if (in->id_off) {
                check_off(in->id_off, n_recs, "id_off");
                id_len = in->id_off[n_recs];
                if (id_len && !in->id_bytes) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            }
        }
        uint32_t n_slots = 0; uint64_t n_predicted = 0, warn_len = 0;
        if (n_samples) {
            check_off(in->pred_off, n_samples, "pred_off");
            if (in->pred_off[n_samples] > 65535u * WG) fail(LCTY_ERR_UNSUPPORTED, "%u predicted alleles", in->pred_off[n_samples]);   // the cells kernel's grid
            n_slots = in->pred_off[n_samples];
            if (n_slots && !in->pred_col) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            for (uint32_t i = 0; i < n_samples; i++) {
                const uint32_t p = in->pred_off[i + 1] - in->pred_off[i];
                if (p > MAX_PLOIDY) fail(LCTY_ERR_UNSUPPORTED, "sample `%s`: %u predicted alleles (at most %u)", S.samples[i].c_str(), p, MAX_PLOIDY);
                n_predicted += p != 0;
            }
            for (uint32_t k = 0; k < n_slots; k++)
                if (in->pred_col[k] != LCTY_GTVCF_REF && in->pred_col[k] >= in->n_haps) fail(LCTY_ERR_INVALID_INPUT, "slot %u reads column %u of %u", k, in->pred_col[k], in->n_haps);
            if (in->warn_off && (S.field_mask & LCTY_GTVCF_WARN)) {
                check_off(in->warn_off, n_samples, "warn_off");
                warn_len = in->warn_off[n_samples];
                if (warn_len && !in->warn) fail(LCTY_ERR_INVALID_INPUT, "null argument");
                for (uint32_t i = 0; i < n_samples; i++)
                    if (in->warn_off[i + 1] - in->warn_off[i] > MAX_WARN)
                        fail(LCTY_ERR_UNSUPPORTED, "sample `%s`: a warning text of %llu bytes (at most %u)", S.samples[i].c_str(),
                             static_cast<unsigned long long>(in->warn_off[i + 1] - in->warn_off[i]), MAX_WARN);
            }
        }
        // the feature texts of all samples are placed by a 32-bit scan
        if (warn_len + MAX_NUM_SUFFIX * n_predicted >= 0x7FFFFFF0ull)
            fail(LCTY_ERR_UNSUPPORTED, "the feature texts of %llu samples with %llu bytes of warnings may reach 2^31 bytes", static_cast<unsigned long long>(n_predicted),
                 static_cast<unsigned long long>(warn_len));
        if (n_recs && n_slots && in->n_haps && !in->gt) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<std::string> contig(1, in->chrom);
        const std::string header = header_text(contig, &in->contig_len, S.samples);

        ctx->activate();
        hipStream_t s = ctx->stream;
        lcty_gtvcf_stats st{};
        st.n_records = n_recs; st.n_samples = n_samples; st.n_slots = n_slots; st.n_predicted = n_predicted;
        const double t0 = now_ms();
        double t = t0;
        auto lap = [&](double* ms) { LCTY_HIP(hipStreamSynchronize(s)); const double now = now_ms(); *ms += now - t; t = now; };
        // ---- upload: what the set keeps goes into buffers of the locus, the rest into the set's scratch
        std::unique_ptr<GtLocus> own(new GtLocus());
        GtLocus& L = *own;
        L.name = in->locus; L.chrom = in->chrom; L.contig_ix = in->contig_ix; L.start = in->start; L.end = in->end; L.contig_len = in->contig_len;
        L.n_recs = n_recs; L.n_haps = in->n_haps; L.n_samples = n_samples; L.n_slots = n_slots;
        reset_flags(S, s, &st.bytes_h2d);
        put(L.chrom_d, in->chrom, chrom_len, s, &st.bytes_h2d);
        put(L.pos, in->pos, n_recs, s, &st.bytes_h2d);
        put(L.ref_len, in->ref_len, n_recs, s, &st.bytes_h2d);
        const uint32_t zero32 = 0; const uint64_t zero64 = 0;
        put(L.rec_allele, n_recs ? in->rec_allele : &zero32, size_t(n_recs) + 1, s, &st.bytes_h2d);
        put(L.allele_off, n_recs ? in->allele_off : &zero64, n_alleles + 1, s, &st.bytes_h2d);
        put(L.allele_bytes, in->allele_bytes, pool, s, &st.bytes_h2d);
        L.with_ids = n_recs && in->id_off;
        if (L.with_ids) { put(L.id_off, in->id_off, size_t(n_recs) + 1, s, &st.bytes_h2d); put(L.id_bytes, in->id_bytes, id_len, s, &st.bytes_h2d); }
        put(L.pred_off, n_samples ? in->pred_off : &zero32, size_t(n_samples) + 1, s, &st.bytes_h2d);
        put(S.pred_col, in->pred_col, n_slots, s, &st.bytes_h2d);
        const uint64_t n_gt = n_slots ? uint64_t(n_recs) * in->n_haps : 0;
        put(S.gt, in->gt, n_gt, s, &st.bytes_h2d);
        Feats F{};
        F.mask = S.field_mask;
        L.with_qual = in->qual10 && n_samples;                           // the merge reads the quality whatever field_mask says
        if (L.with_qual) put(L.qual10, in->qual10, n_samples, s, &st.bytes_h2d);
        const int64_t* const num[4] = {in->qual10, in->reads, in->unexpl, in->wdist5};
        for (uint32_t f = 0; f < 4; f++)
            if (num[f] && (S.field_mask >> f & 1) && n_samples) {
                if (f == 0) { F.num[0] = L.qual10.p; continue; }
                put(S.num[f], num[f], n_samples, s, &st.bytes_h2d); F.num[f] = S.num[f].p;
            }
        if (in->warn_off && (S.field_mask & LCTY_GTVCF_WARN) && n_samples) {
            put(S.warn_off, in->warn_off, size_t(n_samples) + 1, s, &st.bytes_h2d); put(S.warn, in->warn, warn_len, s, &st.bytes_h2d);
            F.warn_off = S.warn_off.p; F.warn = S.warn.p;
        }
        lap(&st.upload_ms);
        // ---- cells
        const uint64_t n_cells = uint64_t(n_recs) * n_slots;
        L.calls.alloc(std::max<uint64_t>(n_cells, 1));
        if (n_cells) LAUNCH(gtvcf_cells_kernel, (n_recs, blocks_of(n_slots, WG)), L.view().R, n_slots, S.pred_col.p, S.gt.p, L.calls.p, S.flags.p);
        lap(&st.cells_ms);
        // ---- widths: the features of every sample, then the lines
        S.suf_w.ensure(std::max(n_samples, 1u));
        if (n_samples) {
            LAUNCH(gtvcf_sufwidth_kernel, (blocks_of(n_samples, WG)), F, n_samples, L.pred_off.p, S.suf_w.p, S.flags.p);
            const uint32_t suf_total = S.scan.run(S.suf_w, L.suf_off, n_samples, ctx);
            L.suf.alloc(std::max(suf_total, 1u));
            LAUNCH(gtvcf_sufwrite_kernel, (blocks_of(n_samples, WG)), F, n_samples, L.suf_off.p, L.suf.p);
        } else put(L.suf_off, &zero32, 1, s, &st.bytes_h2d);
        const LocusDev view = L.view();
        const uint32_t rec0[2] = {0, n_recs};
        put(S.views, &view, 1, s, &st.bytes_h2d);
        put(S.rec0, rec0, 2, s, &st.bytes_h2d);
        const Lines X{S.views.p, S.rec0.p, nullptr, nullptr, 1, n_samples};
        lcty_gtvcf_out o{}; Handoff h;
        text_stage(S, X, n_recs, header, h, &o, &st, &t);
        o.n_slots = n_slots;
        if (in->want_calls) {
            o.calls = from(h, L.calls, n_cells, s); st.bytes_d2h += n_cells * 2;
            lap(&st.download_ms);
        }
        st.total_ms = now_ms() - t0;
        o.stats = st;
        S.loci.push_back(std::move(own));
        *out = o; h.commit();
    });
}

int32_t lcty_gtvcf_merge(lcty_gtvcf* set, lcty_gtvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!set || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_gtvcf& S = *set;
        lcty_ctx* ctx = S.ctx;
        const uint32_t n_loci = uint32_t(S.loci.size()), n_samples = uint32_t(S.samples.size());
        // merge_vcfs 169-176: the contigs in index order, the loci by (contig index, start, end)
        std::vector<uint32_t> by(n_loci);
        for (uint32_t i = 0; i < n_loci; i++) by[i] = i;
        std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) {
            const GtLocus& A = *S.loci[a]; const GtLocus& B = *S.loci[b];
            return A.contig_ix != B.contig_ix ? A.contig_ix < B.contig_ix : A.start != B.start ? A.start < B.start : A.end < B.end;
        });
        std::vector<std::string> contigs; std::vector<uint64_t> contig_len;
        std::vector<LocusDev> views(std::max(n_loci, 1u)); std::vector<uint32_t> rec0(size_t(n_loci) + 1, 0);
        std::vector<uint32_t> header_ix(std::max(n_loci, 1u), 0);
        uint64_t total = 0; uint32_t max_contig = 0;
        for (uint32_t k = 0; k < n_loci; k++) {
            const GtLocus& L = *S.loci[by[k]];
            if (k == 0 || L.contig_ix != S.loci[by[k - 1]]->contig_ix) { contigs.push_back(L.chrom); contig_len.push_back(L.contig_len); }
            header_ix[k] = uint32_t(contigs.size() - 1);
            views[k] = L.view();
            total += L.n_recs;
            if (total >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%llu records in the set", static_cast<unsigned long long>(total));
            rec0[k + 1] = uint32_t(total);
            max_contig = std::max(max_contig, L.contig_ix);
        }
        const uint32_t N = uint32_t(total);
        const std::string header = header_text(contigs, contig_len.data(), S.samples);

        ctx->activate();
        hipStream_t s = ctx->stream;
        lcty_gtvcf_stats st{};
        st.n_records = N; st.n_samples = n_samples;
        const double t0 = now_ms();
        double t = t0;
        auto lap = [&](double* ms) { LCTY_HIP(hipStreamSynchronize(s)); const double now = now_ms(); *ms += now - t; t = now; };
        reset_flags(S, s, &st.bytes_h2d);
        put(S.views, views.data(), n_loci, s, &st.bytes_h2d);
        put(S.rec0, rec0.data(), rec0.size(), s, &st.bytes_h2d);
        put(S.header_ix, header_ix.data(), n_loci, s, &st.bytes_h2d);
        lap(&st.upload_ms);
        Lines X{S.views.p, S.rec0.p, nullptr, nullptr, std::max(n_loci, 1u), n_samples};
        DevBuf<uint64_t>&ka = S.ka, &kb = S.kb, &va = S.va, &vb = S.vb;
        DevBuf<uint32_t>&head = S.head, &rank = S.rank, &run_start = S.run_start, &order = S.order, &first = S.first, &line_start = S.line_start, &line_rec = S.line_rec,
                        &choice = S.choice, &l_contig = S.l_contig, &l_pos = S.l_pos, &l_len = S.l_len;
        uint32_t n_lines = 0;
        if (N) {
            // a stable sort by (contig, pos); one wavefront per run of equal keys orders it by alleles and finds the records to join
            ka.ensure(N); kb.ensure(N); va.ensure(N); vb.ensure(N);
            LAUNCH(gtvcf_keys_kernel, (blocks_of(N, WG)), X, N, ka.p, va.p);
            std::vector<uint32_t> shifts;
            for (uint32_t b = 0; b < 4; b++) shifts.push_back(8 * b);
            for (uint32_t b = 0; b < 4 && (b == 0 || (max_contig >> (8 * b))); b++) shifts.push_back(32 + 8 * b);
            const int side = S.sorter.run(ka.p, va.p, kb.p, vb.p, N, shifts, s);
            const uint64_t* keys = side ? kb.p : ka.p; const uint64_t* vals = side ? vb.p : va.p;
            head.ensure(N);
            LAUNCH(gtvcf_head_kernel, (blocks_of(N, WG)), N, keys, head.p);
            const uint32_t n_runs = S.scan.run(head, rank, N, ctx);
            run_start.ensure(size_t(n_runs) + 1);
            LAUNCH(gtvcf_starts_kernel, (blocks_of(N, WG)), N, n_runs, head.p, rank.p, run_start.p);
            order.ensure(N); first.ensure(N);
            LAUNCH(gtvcf_run_kernel, (blocks_of(n_runs, WG / WAVE)), X, n_runs, run_start.p, vals, order.p, first.p, S.flags.p);
            uint32_t flags[F_COUNT];
            S.flags.download(flags, F_COUNT, s);
            LCTY_HIP(hipStreamSynchronize(s));
            if (flags[F_LONGRUN] != NONE) {
                uint64_t key = 0;
                LCTY_HIP(hipMemcpy(&key, keys + flags[F_LONGRUN], 8, hipMemcpyDeviceToHost));
                fail(LCTY_ERR_UNSUPPORTED, "more than %d records at position %llu of contig %llu", WAVE, static_cast<unsigned long long>((key & 0xFFFFFFFFull) + 1),
                     static_cast<unsigned long long>(key >> 32));
            }
            n_lines = S.scan.run(first, rank, N, ctx);
            line_start.ensure(size_t(n_lines) + 1);
            LAUNCH(gtvcf_starts_kernel, (blocks_of(N, WG)), N, n_lines, first.p, rank.p, line_start.p);
            line_rec.ensure(n_lines); choice.ensure(std::max<uint64_t>(uint64_t(n_lines) * n_samples, 1));
            LAUNCH(gtvcf_join_kernel, (n_lines, std::max(blocks_of(n_samples, WG), 1u)), X, line_start.p, order.p, line_rec.p, choice.p);
            X.line_rec = line_rec.p; X.choice = choice.p;
        }
        lap(&st.merge_ms);
        lcty_gtvcf_out o{}; Handoff h;
        text_stage(S, X, n_lines, header, h, &o, &st, &t);
        l_contig.ensure(std::max(n_lines, 1u)); l_pos.ensure(std::max(n_lines, 1u)); l_len.ensure(std::max(n_lines, 1u));
        if (n_lines) LAUNCH(gtvcf_lineinfo_kernel, (blocks_of(n_lines, WG)), X, n_lines, S.header_ix.p, l_contig.p, l_pos.p, l_len.p);
        o.line_contig = from(h, l_contig, n_lines, s); o.line_pos = from(h, l_pos, n_lines, s); o.line_ref_len = from(h, l_len, n_lines, s);
        st.bytes_d2h += 12ull * n_lines;
        lap(&st.download_ms);
        o.n_joined = N - n_lines;
        std::string blob;
        for (const std::string& c : contigs) { blob += c; blob.push_back('\0'); }
        o.contigs = reinterpret_cast<char*>(h.bytes(blob)); o.contigs_len = blob.size(); o.n_contigs = uint32_t(contigs.size());
        o.contig_ix = static_cast<uint32_t*>(h.raw(std::max<size_t>(contigs.size(), 1) * 4));
        for (uint32_t k = 0; k < n_loci; k++) o.contig_ix[header_ix[k]] = S.loci[by[k]]->contig_ix;
        st.total_ms = now_ms() - t0;
        o.stats = st;
        *out = o; h.commit();
    });
}

void lcty_gtvcf_out_free(lcty_gtvcf_out* out) {
    if (!out) return;
    free(out->text); free(out->line_off); free(out->calls); free(out->line_contig); free(out->line_pos); free(out->line_ref_len); free(out->contigs); free(out->contig_ix);
    memset(out, 0, sizeof(*out));
}

}  // extern "C"
