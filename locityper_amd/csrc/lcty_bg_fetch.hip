// lcty_bg_fetch.hip — the alignments of a sample's background region read through the index of its whole-genome BAM file, the input
// of `locityper preproc -a`: IndexedReader::fetch + load_alns (src/command/preproc.rs:988-1028, 1174-1192), group_mates
// (src/bg/insertsz.rs:25-37). What lcty_bg_reads_load (lcty_io.hip) does record by record on the host over a whole file, here on the
// device over the slice that fetch_slice (lcty_sample_bam.hip) read for the one region:
//   bg_record_kernel   a lane per walked record: region membership, the load_alns filter (flags, MAPQ, clipping rate), the drop of
//                      infer_ext_cigar, the operations and the query length of the records still alive, the hash of the name; a
//                      CIGAR of more than 64 operations is walked by the whole wavefront, 64 words a step
//   exclusive_scan     over the kept flags, the CIGAR lengths and the 32-base units -> record order, cigar_off, seq_off
//   bg_compact_kernel  the kept records side by side, and the sort's input (hash of the name, kept ordinal)
//   RadixSort + bg_mate_kernel (paired data)   a lane per record walks the run of its hash, names compared byte for byte
//   cigar_gather_kernel   the CIGAR words, dealt flat over the lanes;   unpack_kernel<false>   SEQ as it lies in the file (lcty_bam_record.hpp)
// The arrays stay on the device with the handle (lcty_bg_estimate on the same context reads them there) and are downloaded once.
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "lcty_bg_reads.hpp"
#include "lcty_sample_bam.hpp"
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"

namespace lcty {
namespace {

// error classes, by rank at one record (refuse, lcty_device.hpp): the first offending record in file order decides, as in the loop
// of lcty_bg_reads_load
enum : uint32_t { B_SHORT = 1, B_UNSORTED = 2, B_NO_CIGAR = 3, B_BAD_OP = 4, B_QLEN = 5, B_MATES = 6 };
enum : uint32_t { C_IGNORED = 0, C_WO_CIGAR = 1, C_UNPAIRED = 2, C_PAIRED = 3, C_PRIMARY = 4, N_COUNTS = 5 };

struct BgView {
    const uint32_t* raw;                        // the slice as dwords
    const uint64_t* rec_off; uint32_t n_rec;
    int32_t tid; uint32_t start, end;           // the background interval
    uint64_t padded_start, padded_end;
    uint32_t min_mapq; double max_clipping;
    uint64_t hash_mask;
    uint32_t* kept;                             // 0 / 1
    uint32_t* pos; uint32_t* endpos; uint32_t* qlen; uint8_t* flags;
    uint32_t* n_cigar; uint32_t* units;         // 0 for a record that is not kept
    uint64_t* hash; uint8_t* paired;
    unsigned long long* err; uint32_t* counts;
};

// an operation that consumes the reference: M, D, N, =, X;   query bases of a CIGAR word: M, I, S, =, X;   an operation
// lcty_bg_estimate counts: M, I, D, S, =, X
__device__ __forceinline__ bool cigar_consumes_ref(uint32_t w) { return ((0x18Du >> (w & 15u)) & 1u) != 0; }
__device__ __forceinline__ uint32_t cigar_query_len(uint32_t w) { return ((0x193u >> (w & 15u)) & 1u) ? (w >> 4) : 0u; }
__device__ __forceinline__ bool cigar_op_known(uint32_t w) { return ((0x197u >> (w & 15u)) & 1u) != 0; }
// Cigar::infer_ext_cigar (seq/cigar.rs:446-448): an M run that starts before the padded sequence or ends at or past its end
__device__ __forceinline__ bool m_run_outside(uint32_t w, uint64_t ref_at, uint64_t padded_start, uint64_t padded_end) {
    return (w & 15u) == 0u && (ref_at < padded_start || ref_at + (w >> 4) >= padded_end);
}

__global__ __launch_bounds__(256) void bg_record_kernel(const BgView V) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = r < V.n_rec;
    const uint64_t o = valid ? V.rec_off[r] : 0ull;
    RecHead h{};
    bool fits = false;
    if (valid) { h = rec_head(V.raw, o); fits = rec_fits(h); }
    const uint64_t cig = o + 36 + h.l_name;
    // the records whose CIGAR is looked at: on the contig, placed, starting before the interval's end
    const bool cand = fits && h.tid == V.tid && h.pos >= 0 && static_cast<uint32_t>(h.pos) < V.end;
    const uint64_t pos = static_cast<uint64_t>(static_cast<uint32_t>(h.pos));
    // ---- the sums of the CIGAR: up to 64 operations by the lane, more by the wavefront
    unsigned long long rl = 0, ql = 0;
    bool dropped = false, bad_op = false;
    const bool long_cigar = cand && h.n_cigar > 64u;
    if (cand && !long_cigar)
        for (uint32_t j = 0; j < h.n_cigar; j++) {
            const uint32_t w = ld32(V.raw, cig + 4ull * j);
            dropped |= m_run_outside(w, pos + rl, V.padded_start, V.padded_end);
            rl += cigar_ref_len(w); ql += cigar_query_len(w);
            bad_op |= !cigar_op_known(w);
        }
    unsigned long long pending = __ballot(long_cigar);
    while (pending) {
        const int src = __ffsll(pending) - 1;
        pending &= pending - 1;
        const uint64_t c0 = __shfl(static_cast<unsigned long long>(cig), src), p0 = __shfl(static_cast<unsigned long long>(pos), src);
        const uint32_t nc = __shfl(h.n_cigar, src);
        unsigned long long carry = 0, q_part = 0;
        bool d_part = false, b_part = false;
        for (uint32_t base = 0; base < nc; base += 64u) {                        // nc is the same in every lane: they all take every step
            const uint32_t j = base + lane;
            const bool in = j < nc;
            const uint32_t w = in ? ld32(V.raw, c0 + 4ull * j) : 0u;
            const unsigned long long ref = in ? cigar_ref_len(w) : 0u;
            const unsigned long long incl = wave_scan_incl(ref, AddOp{});
            if (in) {
                d_part |= m_run_outside(w, p0 + carry + incl - ref, V.padded_start, V.padded_end);
                q_part += cigar_query_len(w);
                b_part |= !cigar_op_known(w);
            }
            carry += __shfl(incl, 63);
        }
        q_part = wave_reduce(q_part, AddOp{});
        const bool d_any = __ballot(d_part) != 0ull, b_any = __ballot(b_part) != 0ull;
        if (static_cast<int>(lane) == src) { rl = carry; ql = q_part; dropped = d_any; bad_op = b_any; }
    }
    // ---- the tests, in the order of lcty_bg_reads_load
    bool kept = false, ignored = false, wo_cigar = false;
    uint32_t err = 0;
    if (valid && !fits) err = B_SHORT;
    if (cand) {
        const uint64_t rec_end = pos + (((h.flag & 4u) || rl == 0) ? 1ull : rl);            // bam_endpos
        if (rec_end > V.start) {
            const uint32_t mapq = (ld32(V.raw, o + 12) >> 8) & 0xFFu;
            bool keep = (h.flag & 3844u) == 0 && mapq >= V.min_mapq;                         // preproc.rs:1006
            if (keep) {
                if (h.n_cigar == 0) err = B_NO_CIGAR;
                else {                                                                       // clipping_rate (seq/cigar.rs:944-966)
                    const uint32_t first = ld32(V.raw, cig), last = ld32(V.raw, cig + 4ull * (h.n_cigar - 1));
                    const uint32_t clip = (cigar_consumes_ref(first) ? 0u : first >> 4) + (cigar_consumes_ref(last) ? 0u : last >> 4);
                    const double rate = clip == 0 ? 0.0 : static_cast<double>(clip) / static_cast<double>(h.l_seq);
                    keep = rate <= V.max_clipping;
                }
            }
            if (!err) {
                if (!keep) ignored = true;
                else if (dropped) wo_cigar = true;
                else if (bad_op) err = B_BAD_OP;
                else if (ql != h.l_seq) err = B_QLEN;
                else kept = true;
            }
        }
    }
    if (fits && r > 0) {
        const uint64_t op = V.rec_off[r - 1];
        const uint64_t before = sort_key(static_cast<int32_t>(ld32(V.raw, op + 4)), static_cast<int32_t>(ld32(V.raw, op + 8)));
        if (before > sort_key(h.tid, h.pos) && (!err || err > B_UNSORTED)) { err = B_UNSORTED; kept = ignored = wo_cigar = false; }
    }
    const bool paired = (h.flag & 1u) != 0;
    if (valid) {
        V.kept[r] = kept ? 1u : 0u;
        V.pos[r] = static_cast<uint32_t>(h.pos); V.endpos[r] = static_cast<uint32_t>(pos + rl); V.qlen[r] = h.l_seq;
        V.flags[r] = static_cast<uint8_t>(((h.flag & 0x10u) ? LCTY_BG_REVERSE : 0u) | ((h.flag & 0x80u) ? LCTY_BG_SECOND : 0u));
        V.n_cigar[r] = kept ? h.n_cigar : 0u;
        V.units[r] = kept ? h.l_seq / 32u + ((h.l_seq & 31u) ? 1u : 0u) : 0u;
        V.hash[r] = kept ? name_hash(V.raw, o, h.l_name) & V.hash_mask : 0ull;
        V.paired[r] = paired ? 1 : 0;
        if (err) refuse(V.err, r, err);
    }
    const unsigned long long b_ign = __ballot(ignored), b_wo = __ballot(wo_cigar), b_un = __ballot(kept && !paired), b_pa = __ballot(kept && paired),
                             b_prim = __ballot(fits && (h.flag & 0x900u) == 0);
    if (lane == 0) {
        if (b_ign) atomicAdd(V.counts + C_IGNORED, static_cast<uint32_t>(__popcll(b_ign)));
        if (b_wo) atomicAdd(V.counts + C_WO_CIGAR, static_cast<uint32_t>(__popcll(b_wo)));
        if (b_un) atomicAdd(V.counts + C_UNPAIRED, static_cast<uint32_t>(__popcll(b_un)));
        if (b_pa) atomicAdd(V.counts + C_PAIRED, static_cast<uint32_t>(__popcll(b_pa)));
        if (b_prim) atomicAdd(V.counts + C_PRIMARY, static_cast<uint32_t>(__popcll(b_prim)));
    }
}

// the compact arrays of the handle, every one with n_kept (+ 1) entries, and the sort's input
struct BgCompact {
    uint32_t* src;                              // kept ordinal -> record among the records walked
    uint32_t* pos; uint32_t* endpos; uint32_t* qlen; uint8_t* flags;
    uint64_t* cigar_off; uint64_t* seq_off;
    uint32_t* cigar_off32; uint32_t* unit_off;  // the same offsets as the searches of the gather and the unpack take them
    uint64_t* keys; uint64_t* vals;             // null: single-end data
};

__global__ __launch_bounds__(256) void bg_compact_kernel(const BgView V, const uint32_t* __restrict__ scan_kept, const uint32_t* __restrict__ scan_cigar,
                                                         const uint32_t* __restrict__ scan_units, uint32_t n_kept, const BgCompact C) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r == 0) {
        const uint32_t nc = scan_cigar[V.n_rec], nu = scan_units[V.n_rec];
        C.cigar_off[n_kept] = nc; C.cigar_off32[n_kept] = nc; C.seq_off[n_kept] = 32ull * nu; C.unit_off[n_kept] = nu;
    }
    if (r >= V.n_rec || !V.kept[r]) return;
    const uint32_t k = scan_kept[r];
    C.src[k] = r;
    C.pos[k] = V.pos[r]; C.endpos[k] = V.endpos[r]; C.qlen[k] = V.qlen[r]; C.flags[k] = V.flags[r];
    C.cigar_off[k] = scan_cigar[r]; C.cigar_off32[k] = scan_cigar[r];
    C.seq_off[k] = 32ull * scan_units[r]; C.unit_off[k] = scan_units[r];
    if (C.keys) { C.keys[k] = V.hash[r]; C.vals[k] = k; }
}

// group_mates (bg/insertsz.rs:25-37) for the record at place i of the sorted list: the records of its hash lie side by side in kept
// order. One of its name and its end before it: "several first / second mates" at this record (the smallest such record is the one
// the host loop names). One of its name and the other end: its mate.
__global__ __launch_bounds__(256) void bg_mate_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ src,
                                                      const uint8_t* __restrict__ flags, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                      uint32_t n, uint32_t* __restrict__ mate, unsigned long long* err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    const uint32_t s = static_cast<uint32_t>(vals[i]);
    const uint64_t o = rec_off[src[s]];
    const uint32_t second = flags[s] & LCTY_BG_SECOND;
    uint32_t m = NONE32;
    for (uint32_t t = i; t > 0 && keys[t - 1] == key; t--) {
        const uint32_t st = static_cast<uint32_t>(vals[t - 1]);
        if (!same_name(raw, rec_off[src[st]], o)) continue;
        if ((flags[st] & LCTY_BG_SECOND) == second) refuse(err, src[s], B_MATES);
        else m = st;
    }
    for (uint32_t t = i + 1; t < n && keys[t] == key; t++) {
        const uint32_t st = static_cast<uint32_t>(vals[t]);
        if ((flags[st] & LCTY_BG_SECOND) != second && same_name(raw, rec_off[src[st]], o)) m = st;
    }
    mate[s] = m;
}

}  // namespace
}  // namespace lcty

using namespace lcty;

extern "C" {

int32_t lcty_bg_reads_fetch(lcty_ctx* ctx, lcty_sample_bam* bam, const char* contig, uint32_t start, uint32_t end, uint32_t padded_start,
                            uint32_t padded_len, const lcty_bg_params* params, lcty_bg_reads** out, lcty_sample_bam_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return guarded([&] {
        if (!ctx || !bam || !contig || !params || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double t_start = now_ms();
        const char* path = bam->file.path.c_str();
        if (start >= end || padded_start > start || static_cast<uint64_t>(padded_start) + padded_len < end)
            fail(LCTY_ERR_INVALID_INPUT, "background interval [%u, %u) is not inside the padded sequence [%u, +%u)", start, end, padded_start, padded_len);
        uint32_t tid = NONE32;
        for (size_t r = 0; r < bam->lengths.size() && tid == NONE32; r++)
            if (strcmp(bam->names.c_str() + bam->name_off[r], contig) == 0) tid = static_cast<uint32_t>(r);
        if (tid == NONE32) fail(LCTY_ERR_INVALID_INPUT, "%s: no reference sequence %s in the BAM header", path, contig);
        const int64_t hash_bits = ctx->knob("sample_bam_hash_bits", 64);
        if (hash_bits > 64) fail(LCTY_ERR_INVALID_INPUT, "sample_bam_hash_bits = %lld (0 .. 64)", static_cast<long long>(hash_bits));
        const uint64_t hash_mask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1;
        const uint64_t padded_end = static_cast<uint64_t>(padded_start) + padded_len;
        lcty_sample_bam_stats S{};
        S.n_regions = 1; S.file_bytes = bam->file.fsize;

        // ---- the front half of lcty_sample_bam_fetch for the one region, without the unmapped tail
        Slice F;
        fetch_slice(ctx, bam, 1, &tid, &start, &end, false, false, F, S);
        hipStream_t s = ctx->stream;
        const std::vector<uint64_t>& rec_off = F.rec_off;
        const uint64_t n_rec = rec_off.size();
        if (n_rec == 0) fail(LCTY_ERR_INVALID_DATA, "BAM file contains no reads in the target region");

        // ---- upload, the record stage
        double t0 = now_ms();
        DevBuf<uint64_t> d_rec_off, d_hash; DevBuf<uint32_t> d_kept, d_pos, d_end, d_qlen, d_ncig, d_units, d_counts; DevBuf<uint8_t> d_flags, d_paired;
        ErrWord err;
        const uint32_t* raw = reinterpret_cast<const uint32_t*>(F.device(s));
        d_rec_off.alloc(n_rec); d_rec_off.upload(rec_off.data(), n_rec, s);
        d_kept.alloc(n_rec); d_pos.alloc(n_rec); d_end.alloc(n_rec); d_qlen.alloc(n_rec); d_ncig.alloc(n_rec); d_units.alloc(n_rec);
        d_hash.alloc(n_rec); d_flags.alloc(n_rec); d_paired.alloc(n_rec); d_counts.alloc(N_COUNTS);
        d_counts.zero(s);
        unsigned long long* d_err = err.reset(s);
        LCTY_HIP(hipStreamSynchronize(s));
        S.ms_upload = now_ms() - t0;
        t0 = now_ms();
        BgView V{};
        V.raw = raw; V.rec_off = d_rec_off.p; V.n_rec = static_cast<uint32_t>(n_rec);
        V.tid = static_cast<int32_t>(tid); V.start = start; V.end = end; V.padded_start = padded_start; V.padded_end = padded_end;
        V.min_mapq = params->min_mapq; V.max_clipping = params->max_clipping; V.hash_mask = hash_mask;
        V.kept = d_kept.p; V.pos = d_pos.p; V.endpos = d_end.p; V.qlen = d_qlen.p; V.flags = d_flags.p; V.n_cigar = d_ncig.p; V.units = d_units.p;
        V.hash = d_hash.p; V.paired = d_paired.p; V.err = d_err; V.counts = d_counts.p;
        hipLaunchKernelGGL(bg_record_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, V);
        LCTY_HIP(hipGetLastError());
        auto check_err = [&]() {
            uint64_t r; uint32_t cls;
            if (!err.take(s, r, cls)) return;
            const uint8_t* rec = F.slice + rec_off[r];
            if (cls == B_SHORT) fail(LCTY_ERR_INVALID_DATA, "%s: record %llu of the fetched slice is shorter than its fields", path, static_cast<unsigned long long>(r));
            const std::string name = record_name(F.slice, rec_off[r]);
            if (cls == B_UNSORTED) fail(LCTY_ERR_INVALID_DATA, "%s: coordinates run backwards at read %s: the file is not sorted", path, name.c_str());
            if (cls == B_NO_CIGAR) fail(LCTY_ERR_INVALID_DATA, "%s: mapped record without a CIGAR (read %s)", path, name.c_str());
            uint16_t n_cigar, flag; uint32_t l_seq;
            memcpy(&n_cigar, rec + 16, 2); memcpy(&flag, rec + 18, 2); memcpy(&l_seq, rec + 20, 4);
            const uint8_t* cg = rec + 36 + rec[12];
            if (cls == B_BAD_OP)
                for (uint32_t k = 0; k < n_cigar; k++) {
                    uint32_t w; memcpy(&w, cg + 4 * k, 4);
                    const uint32_t op = w & 15u;
                    if (op == 3 || op == 5 || op == 6 || op > 8)
                        fail(LCTY_ERR_INVALID_DATA, "Read %s: unsupported CIGAR operation %c in a background alignment", name.c_str(), "MIDNSHP=X???????"[op]);
                }
            if (cls == B_QLEN) {
                uint64_t ql = 0;
                for (uint32_t k = 0; k < n_cigar; k++) {
                    uint32_t w; memcpy(&w, cg + 4 * k, 4);
                    const uint32_t op = w & 15u;
                    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ql += w >> 4;
                }
                fail(LCTY_ERR_INVALID_DATA, "Failed to convert CIGAR for read \"%s\" (query length %llu, SEQ length %u)", name.c_str(),
                     static_cast<unsigned long long>(ql), l_seq);
            }
            if (cls == B_MATES) fail(LCTY_ERR_INVALID_DATA, "Read %s has several %s mates", name.c_str(), (flag & 0x80) ? "second" : "first");
            fail(LCTY_ERR_RUNTIME, "%s: unknown device error %u", path, cls);
        };
        check_err();
        uint32_t counts[N_COUNTS];
        d_counts.download(counts, N_COUNTS, s);
        LCTY_HIP(hipStreamSynchronize(s));
        S.records_primary = counts[C_PRIMARY];
        // the host remainder of the loop, in its order
        if (counts[C_UNPAIRED] > 0 && counts[C_PAIRED] > 0) fail(LCTY_ERR_INVALID_DATA, "BAM file contains both paired and unpaired reads");
        if (counts[C_UNPAIRED] + counts[C_PAIRED] == 0) fail(LCTY_ERR_INVALID_DATA, "BAM file contains no reads in the target region");
        const bool paired = counts[C_PAIRED] > 0;
        if (paired && params->technology != LCTY_TECH_ILLUMINA) fail(LCTY_ERR_INVALID_INPUT, "Paired end reads are not supported by this technology");

        // ---- record order, cigar_off, seq_off; the kept records side by side
        ScanTotal scan;
        DevBuf<uint32_t> d_scan_kept, d_scan_cigar, d_scan_units;
        const uint32_t n = scan.run(d_kept, d_scan_kept, n_rec, ctx);
        const uint32_t n_words = scan.run(d_ncig, d_scan_cigar, n_rec, ctx);
        const uint32_t n_units = scan.run(d_units, d_scan_units, n_rec, ctx);
        auto T = std::make_unique<lcty_bg_reads>();
        DevBuf<uint32_t> d_src, d_coff32, d_unit_off;
        DevBuf<uint64_t> d_ka, d_va, d_kb, d_vb;
        d_src.alloc(n); d_coff32.alloc(n + 1ull); d_unit_off.alloc(n + 1ull);
        T->d_pos.alloc(n); T->d_end.alloc(n);
        DevBuf<uint32_t> d_qlen_c;
        d_qlen_c.alloc(n); T->d_flags.alloc(n); T->d_cigar_off.alloc(n + 1ull); T->d_seq_off.alloc(n + 1ull);
        if (paired) { d_ka.alloc(n); d_va.alloc(n); d_kb.alloc(n); d_vb.alloc(n); }
        BgCompact C{};
        C.src = d_src.p; C.pos = T->d_pos.p; C.endpos = T->d_end.p; C.qlen = d_qlen_c.p; C.flags = T->d_flags.p;
        C.cigar_off = T->d_cigar_off.p; C.seq_off = T->d_seq_off.p; C.cigar_off32 = d_coff32.p; C.unit_off = d_unit_off.p;
        C.keys = paired ? d_ka.p : nullptr; C.vals = paired ? d_va.p : nullptr;
        hipLaunchKernelGGL(bg_compact_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, V, d_scan_kept.p, d_scan_cigar.p, d_scan_units.p, n, C);
        LCTY_HIP(hipGetLastError());
        LCTY_HIP(hipStreamSynchronize(s));
        S.records_kept = n;
        S.ms_record = now_ms() - t0;

        // ---- mates
        t0 = now_ms();
        T->mate.assign(n, LCTY_NONE_U32);
        if (paired) {
            RadixSort sorter;
            std::vector<uint32_t> shifts;
            for (uint32_t sh = 0; sh < static_cast<uint32_t>(hash_bits); sh += 8) shifts.push_back(sh);
            int where = 0;
            if (!shifts.empty()) where = sorter.run(d_ka.p, d_va.p, d_kb.p, d_vb.p, n, shifts, s);
            const uint64_t* keys = where ? d_kb.p : d_ka.p; const uint64_t* vals = where ? d_vb.p : d_va.p;
            DevBuf<uint32_t> d_mate;
            d_mate.alloc(n);
            hipLaunchKernelGGL(bg_mate_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_src.p, T->d_flags.p, keys, vals, n, d_mate.p, d_err);
            LCTY_HIP(hipGetLastError());
            check_err();
            d_mate.download(T->mate.data(), n, s);
            LCTY_HIP(hipStreamSynchronize(s));
        }
        S.ms_pair = now_ms() - t0;

        // ---- CIGAR words, bases, and the view's arrays on the host
        t0 = now_ms();
        T->d_cigar.alloc(std::max<uint32_t>(n_words, 1));
        T->d_bases2.alloc(2ull * n_units + 2); T->d_nmask.alloc(n_units + 1ull);
        T->d_bases2.zero(s); T->d_nmask.zero(s);
        if (n_words)
            hipLaunchKernelGGL(cigar_gather_kernel<uint32_t>, dim3(blocks_of(n_words, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_src.p, d_coff32.p, n, n_words, T->d_cigar.p);
        LCTY_HIP(hipGetLastError());
        if (n_units)
            hipLaunchKernelGGL(unpack_kernel<false>, dim3(blocks_of(n_units, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_src.p, d_unit_off.p, n, n_units,
                               reinterpret_cast<uint64_t*>(T->d_bases2.p), T->d_nmask.p);
        LCTY_HIP(hipGetLastError());
        T->pos.resize(n); T->end.resize(n); T->qlen.resize(n); T->flags.resize(n); T->cigar_off.resize(n + 1ull); T->seq_off.resize(n + 1ull);
        T->cigar.resize(n_words); T->bases2.resize(2ull * n_units + 2); T->nmask.resize(n_units + 1ull);
        T->d_pos.download(T->pos.data(), n, s); T->d_end.download(T->end.data(), n, s); d_qlen_c.download(T->qlen.data(), n, s);
        T->d_flags.download(T->flags.data(), n, s);
        T->d_cigar_off.download(T->cigar_off.data(), n + 1ull, s); T->d_seq_off.download(T->seq_off.data(), n + 1ull, s);
        T->d_cigar.download(T->cigar.data(), n_words, s);
        T->d_bases2.download(T->bases2.data(), T->bases2.size(), s); T->d_nmask.download(T->nmask.data(), T->nmask.size(), s);
        LCTY_HIP(hipStreamSynchronize(s));
        S.ms_unpack = now_ms() - t0;

        uint64_t n_pairs = 0;
        for (uint32_t a = 0; a < n; a++) n_pairs += T->mate[a] != LCTY_NONE_U32 && !(T->flags[a] & LCTY_BG_SECOND);
        S.n_pairs = n_pairs; S.n_discarded = 0;
        double sum = 0.0;                                   // read_len_from_alns (preproc.rs:1031-1037)
        const size_t m = std::min<size_t>(n, 10000);
        for (size_t a = 0; a < m; a++) sum += static_cast<double>(T->qlen[a]);
        lcty_bg_reads_view& v = T->view;
        v.n_records = n; v.n_ignored = counts[C_IGNORED]; v.n_wo_cigar = counts[C_WO_CIGAR]; v.paired = paired ? 1 : 0;
        v.read_len = sum / static_cast<double>(m);
        v.pos = T->pos.data(); v.end = T->end.data(); v.qlen = T->qlen.data(); v.flags = T->flags.data(); v.mate = T->mate.data();
        v.cigar_off = T->cigar_off.data(); v.cigar = T->cigar.data(); v.seq_off = T->seq_off.data();
        v.bases2 = T->bases2.data(); v.nmask = T->nmask.data();
        T->ctx = ctx;
        S.ms_total = now_ms() - t_start;
        if (stats) *stats = S;
        *out = T.release();
    });
}

}  // extern "C"
