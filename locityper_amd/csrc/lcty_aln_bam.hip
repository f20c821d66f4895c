// lcty_aln_bam.hip — a locus's aln.bam read on the device, straight into a batch: what lcty_bam_read (lcty_io.hip) does
// record by record on the host — AllAlignments::load over the mapper's name-grouped file (src/model/locs.rs:405-461, 502-567,
// 1116-1150) —, over the whole file as one slice:
//   host   read, BGZF split, inflate (Slice::inflate of lcty_bgzf_read.hpp: host pool, or the device with knob "sample_bam_inflate" 1),
//          the header and the chain of record lengths (lcty_aln_bam_parse.hpp)
//   aln_record_kernel   a lane per walked record: head, rec_fits, primary or not, the lcty_aln_rec fields but cigar_rel, MAPQ, n_cigar,
//                       the error classes of one record
//   exclusive scans     primary flags -> primary ordinal j; n_cigar -> the place of every record's CIGAR words
//   aln_place_kernel    primary j -> its record;   aln_primary_kernel   a lane per primary: l_seq, units, name length, the records of
//                       its read end, and for a pair's second end the comparison of its name with the first end's
//   scans               units -> mate_off, l_seq -> qual_off, name lengths -> name_off
//   aln_pair_kernel     a lane per record: cigar_rel (relative to its pair), the largest CIGAR of a record per pair
//   aln_mate_kernel     a lane per primary: the per-mate and per-pair arrays of the table
//   gathers             CIGAR words (cigar_gather_kernel), name bytes, quality bytes dealt flat over the lanes; unpack_kernel<false> for SEQ as stored
// The grouping is a pure function of the primary flags: primary j starts a read (paired == 0), or starts a pair when j is even and is
// its second end when j is odd. Errors: (record ordinal, class) through refuse (lcty_device.hpp), the first offending record in file order
// decides and at one record the order of checks of the host loop; the host words the message from the slice.
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "lcty_aln_bam.hpp"
#include "lcty_aln_bam_parse.hpp"
#include "lcty_bam_record.hpp"
#include "lcty_bgzf_read.hpp"
#include "lcty_objects.hpp"
#include "lcty_scan.hpp"

namespace lcty {
namespace {

// error classes, by rank at one record (the order of the loop of lcty_bam_read)
enum : uint32_t { A_CORRUPT = 1, A_FIRST_NOT_PRIMARY = 2, A_NO_SECOND_END = 3, A_NO_REFERENCE = 4 };

struct AlnView {
    const uint32_t* raw;                        // the slice as dwords
    const uint64_t* rec_off; uint32_t n_rec;
    const uint32_t* tid2contig; uint32_t n_ref;
    lcty_aln_rec* recs; uint8_t* mapq;
    uint32_t* prim; uint32_t* n_cigar;          // 0 / 1;   0 for a record whose fields leave its block
    unsigned long long* err;
};

__global__ __launch_bounds__(256) void aln_record_kernel(const AlnView V) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= V.n_rec) return;
    const uint64_t o = V.rec_off[r];
    const RecHead h = rec_head(V.raw, o);                                        // the 32 fixed bytes are inside the block (the walk)
    const bool fits = rec_fits(h);
    const bool primary = (h.flag & 0x900u) == 0;                                 // is_primary, locs.rs:405-407
    const bool unmapped = (h.flag & 4u) != 0;
    const bool has_ref = h.tid >= 0 && static_cast<uint32_t>(h.tid) < V.n_ref;
    uint32_t err = 0;
    if (!fits) err = A_CORRUPT;
    else if (r == 0 && !primary) err = A_FIRST_NOT_PRIMARY;
    else if (!unmapped && !has_ref) err = A_NO_REFERENCE;                        // a second end of another name ranks before it (aln_primary_kernel)
    lcty_aln_rec rec;
    rec.pos = h.pos < 0 ? 0u : static_cast<uint32_t>(h.pos);
    rec.contig = static_cast<uint16_t>(unmapped || !has_ref ? 0u : V.tid2contig[h.tid]);
    rec.flags = static_cast<uint16_t>(h.flag & (LCTY_FLAG_UNMAPPED | LCTY_FLAG_REVERSE | LCTY_FLAG_MATE2 | LCTY_FLAG_SECONDARY | LCTY_FLAG_SUPPL));
    rec.n_cigar = fits ? h.n_cigar : 0u;
    rec.cigar_rel = 0;
    V.recs[r] = rec;
    V.mapq[r] = static_cast<uint8_t>((ld32(V.raw, o + 12) >> 8) & 0xFFu);
    V.prim[r] = primary ? 1u : 0u;
    V.n_cigar[r] = fits ? h.n_cigar : 0u;
    if (err) refuse(V.err, r, err);
}

__global__ __launch_bounds__(256) void aln_place_kernel(const uint32_t* __restrict__ prim, const uint32_t* __restrict__ prim_ord, uint32_t n_rec,
                                                        uint32_t* __restrict__ prim_rec) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n_rec && prim[r]) prim_rec[prim_ord[r]] = r;
}

// the names of two records as the host loop compares them: l_read_name - 1 bytes each (both records fit their blocks)
__device__ inline bool same_qname(const uint32_t* raw, uint64_t oa, uint64_t ob) {
    const uint32_t la = ld32(raw, oa + 12) & 0xFFu, lb = ld32(raw, ob + 12) & 0xFFu;
    const uint32_t na = la ? la - 1u : 0u, nb = lb ? lb - 1u : 0u;
    if (na != nb) return false;
    for (uint32_t j = 0; j < na; j += 4) {
        const uint32_t m = na - j >= 4 ? 0xFFFFFFFFu : (1u << (8 * (na - j))) - 1u;
        if ((ld32(raw, oa + 36 + j) ^ ld32(raw, ob + 36 + j)) & m) return false;
    }
    return true;
}

// per primary j (in file order): what the scans and the per-mate arrays take
struct AlnPrimaries {
    uint32_t* l_seq; uint32_t* units; uint32_t* name_len;       // name_len: 0 for a pair's second end (a pair has the name of its first)
    uint32_t* n_recs;                                           // records of the read end: up to the next primary
};

__global__ __launch_bounds__(256) void aln_primary_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, uint32_t n_rec,
                                                          const uint32_t* __restrict__ prim_rec, uint32_t n_prim, int paired, const AlnPrimaries P,
                                                          unsigned long long* err) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_prim) return;
    const uint32_t r = prim_rec[j];
    const uint64_t o = rec_off[r];
    const RecHead h = rec_head(raw, o);
    const bool fits = rec_fits(h);                                               // before anything that depends on l_read_name
    const bool second = paired && (j & 1u);
    if (second && fits) {
        const uint64_t of = rec_off[prim_rec[j - 1]];
        if (rec_fits(rec_head(raw, of)) && !same_qname(raw, of, o)) refuse(err, r, A_NO_SECOND_END);
    }
    P.l_seq[j] = fits ? h.l_seq : 0u;
    P.units[j] = fits ? h.l_seq / 32u + ((h.l_seq & 31u) ? 1u : 0u) : 0u;
    P.name_len[j] = fits && !second && h.l_name ? h.l_name - 1u : 0u;
    P.n_recs[j] = (j + 1 < n_prim ? prim_rec[j + 1] : n_rec) - r;
}

__global__ __launch_bounds__(256) void aln_pair_kernel(const uint32_t* __restrict__ prim, const uint32_t* __restrict__ prim_ord,
                                                       const uint32_t* __restrict__ cigar_at, const uint32_t* __restrict__ prim_rec, uint32_t n_rec,
                                                       int paired, lcty_aln_rec* __restrict__ recs, uint32_t* __restrict__ pair_max_cigar) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec) return;
    const uint32_t upto = prim_ord[r] + prim[r];                                 // primaries up to and with this record: the first record is one
    if (upto == 0) return;
    const uint32_t g = upto - 1u;                                                // the group of the record = the primary in front of it
    const uint32_t pair = paired ? g >> 1 : g;
    const uint32_t first = prim_rec[paired ? g & ~1u : g];
    recs[r].cigar_rel = cigar_at[r] - cigar_at[first];
    const uint32_t nc = cigar_at[r + 1] - cigar_at[r];
    if (nc) atomicMax(pair_max_cigar + pair, nc);
}

// the table's per-mate arrays [2 P (+ 1)] and per-pair arrays [P (+ 1)]
struct AlnTable {
    uint32_t* mate_len; uint64_t* mate_off; uint64_t* qual_off; uint32_t* n_recs_mate;
    uint64_t* aln_off; uint64_t* cigar_off; uint64_t* name_off;
};

__global__ __launch_bounds__(256) void aln_mate_kernel(const uint32_t* __restrict__ prim_rec, uint32_t n_prim, uint32_t n_rec, int paired, const AlnPrimaries P,
                                                       const uint32_t* __restrict__ unit_off, const uint64_t* __restrict__ qual_at,
                                                       const uint64_t* __restrict__ name_at, const uint32_t* __restrict__ cigar_at, const AlnTable T) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_prim) return;
    const uint32_t r = prim_rec[j];
    const uint32_t m = paired ? j : 2u * j;
    T.mate_len[m] = P.l_seq[j]; T.mate_off[m] = 32ull * unit_off[j]; T.qual_off[m] = qual_at[j]; T.n_recs_mate[m] = P.n_recs[j];
    if (!paired) {                                                               // the absent second end: mate_len 0, nothing behind the first
        T.mate_len[m + 1] = 0; T.mate_off[m + 1] = 32ull * unit_off[j + 1]; T.qual_off[m + 1] = qual_at[j + 1]; T.n_recs_mate[m + 1] = 0;
    }
    if (!paired || !(j & 1u)) {
        const uint32_t p = paired ? j >> 1 : j;
        T.aln_off[p] = r; T.cigar_off[p] = cigar_at[r]; T.name_off[p] = name_at[j];
    }
    if (j == 0) {
        const uint32_t n_pairs = paired ? (n_prim + 1u) / 2u : n_prim;
        T.mate_off[2ull * n_pairs] = 32ull * unit_off[n_prim]; T.qual_off[2ull * n_pairs] = qual_at[n_prim];
        T.aln_off[n_pairs] = n_rec; T.cigar_off[n_pairs] = cigar_at[n_rec]; T.name_off[n_pairs] = name_at[n_prim];
    }
}

// byte b of the output: of the last primary j with at[j] <= b. QUAL: the qualities behind SEQ, else the name behind the fixed fields.
template <bool QUAL>
__global__ __launch_bounds__(256) void aln_bytes_kernel(const uint8_t* __restrict__ raw8, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ prim_rec,
                                                        const uint64_t* __restrict__ at, uint32_t n_prim, uint64_t n_bytes, uint8_t* __restrict__ out) {
    const uint64_t b = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (b >= n_bytes) return;
    const uint32_t j = flat_owner(at, n_prim, b);
    const uint64_t o = rec_off[prim_rec[j]];
    uint64_t from = o + 36;
    if (QUAL) {
        const uint32_t* raw = reinterpret_cast<const uint32_t*>(raw8);
        const uint32_t l_name = ld32(raw, o + 12) & 0xFFu, n_cigar = ld32(raw, o + 16) & 0xFFFFu, l_seq = ld32(raw, o + 20);
        from += l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2;
    }
    out[b] = raw8[from + (b - at[j])];
}

// the whole file, split into its BGZF blocks; false: not BGZF from end to end
bool whole_file_blocks(const std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks, uint64_t& total) {
    blocks.clear(); total = 0;
    for (uint64_t at = 0; at < comp.size();) {
        BgzfHead h;
        if (bgzf_head(comp.data() + at, comp.size() - at, h) != BGZF_OK) { blocks.clear(); return false; }
        blocks.push_back(BgzfBlock{h.csize, h.isize, total, static_cast<size_t>(at), at, h.head});
        total += h.isize; at += h.csize;
    }
    return true;
}

}  // namespace
}  // namespace lcty

using namespace lcty;

extern "C" {

int32_t lcty_bam_read_device(lcty_ctx* ctx, const char* path, const char* const* names, uint32_t n_alleles, int32_t paired_arg, int32_t host_copy,
                             lcty_bam_table** out, lcty_aln_bam_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return guarded([&] {
        if (!ctx || !path || !names || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *out = nullptr;
        const double t_start = now_ms();
        const int paired = paired_arg != 0;
        check_inflate_knob(ctx);
        lcty_aln_bam_stats S{};

        // ---- the bytes of the file, split into blocks, inflated into one page-locked slice
        double t0 = now_ms();
        Slice F;
        F.comp = read_whole_file(path);
        S.bytes_read = F.comp.size();
        const bool bgzf = whole_file_blocks(F.comp, F.blocks, F.total);
        S.ms_read = now_ms() - t0;
        if (bgzf) {
            S.blocks = F.blocks.size(); S.bytes_inflated = F.total;
            check_slice_cap(ctx, path, F.total, "aln_bam_max_slice_bytes", "the file inflates to");
            S.ms_inflate = F.inflate(ctx, path);
        } else {
            // gzip members that are not BGZF blocks: the serial inflate of the host reader, with its errors
            std::vector<uint8_t>().swap(F.comp);
            t0 = now_ms();
            uint8_t* data = nullptr; uint64_t len = 0;
            const int32_t rc = lcty_io_read_file(path, &data, &len);
            if (rc != LCTY_OK) throw Error(rc, lcty_last_error());
            struct Freed { uint8_t* p; ~Freed() { free(p); } } freed{data};
            S.bytes_inflated = len;
            check_slice_cap(ctx, path, len, "aln_bam_max_slice_bytes", "the file inflates to");
            F.alloc(ctx, len);
            if (len) memcpy(F.slice, data, len);
            S.ms_inflate = now_ms() - t0;
        }
        hipStream_t s = ctx->stream;

        // ---- the header and the chain of record lengths
        t0 = now_ms();
        const alnbam::Header H = alnbam::parse_header(F.slice, F.total, names, n_alleles, path);
        std::vector<uint64_t>& rec_off = F.rec_off;
        const alnbam::WalkStop stop = alnbam::walk_records(F.slice, F.total, H.first_record, rec_off);
        const uint64_t n_rec = rec_off.size();
        S.records = n_rec;
        S.ms_walk = now_ms() - t0;
        if (n_rec >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%s: %llu records in one file", path, static_cast<unsigned long long>(n_rec));
        // what the walk stopped at, once no record before it has an error of its own
        auto walk_error = [&] {
            if (stop == alnbam::WALK_TRUNCATED) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM", path);
            if (stop == alnbam::WALK_SHORT_BLOCK) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BAM record", path);
        };
        auto last_primary_name = [&](uint64_t before) {                          // the read whose second end is looked for
            for (uint64_t r = before; r-- > 0;) if (alnbam::is_primary_at(F.slice, rec_off[r])) return alnbam::qname_at(F.slice, rec_off[r]);
            return std::string();
        };

        auto T = std::make_unique<lcty_bam_table>();
        T->n_refs = H.n_ref; T->ctx = ctx; T->host_copy = host_copy != 0;
        uint32_t n_prim = 0, n_pairs = 0, n_words = 0, n_units = 0;
        uint64_t n_name = 0, n_qual = 0;
        DevBuf<uint8_t> d_mapq, d_names, d_quals;
        DevBuf<uint32_t> d_mate_len, d_nrm, d_pmax;
        DevBuf<uint64_t> d_mate_off, d_qual_off, d_aln_off, d_cigar_off, d_name_off;
        if (n_rec == 0) walk_error();
        if (n_rec) {
            // ---- upload, the record stage
            t0 = now_ms();
            DevBuf<uint64_t> d_rec_off; DevBuf<uint32_t> d_tid, d_prim, d_ncig; ErrWord err;
            const uint8_t* d_raw = F.device(s);
            d_rec_off.alloc(n_rec); d_rec_off.upload(rec_off.data(), n_rec, s);
            d_tid.alloc(std::max<size_t>(H.n_ref, 1)); d_tid.upload(H.tid2contig.data(), H.n_ref, s);
            T->d_recs.alloc(n_rec); d_mapq.alloc(n_rec); d_prim.alloc(n_rec); d_ncig.alloc(n_rec);
            unsigned long long* d_err = err.reset(s);
            const uint32_t* raw = reinterpret_cast<const uint32_t*>(d_raw);
            AlnView V{};
            V.raw = raw; V.rec_off = d_rec_off.p; V.n_rec = static_cast<uint32_t>(n_rec); V.tid2contig = d_tid.p; V.n_ref = H.n_ref;
            V.recs = T->d_recs.p; V.mapq = d_mapq.p; V.prim = d_prim.p; V.n_cigar = d_ncig.p; V.err = d_err;
            hipLaunchKernelGGL(aln_record_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, V);
            LCTY_HIP(hipGetLastError());
            ScanTotal scan;
            DevBuf<uint32_t> d_prim_ord, d_cigar_at, d_unit_off;
            n_prim = scan.run(d_prim, d_prim_ord, n_rec, ctx);
            n_words = scan.run(d_ncig, d_cigar_at, n_rec, ctx);
            n_pairs = paired ? (n_prim + 1u) / 2u : n_prim;
            DevBuf<uint32_t> d_prim_rec, d_lseq, d_units, d_nlen, d_nrecs;
            d_prim_rec.alloc(std::max<uint32_t>(n_prim, 1)); d_lseq.alloc(std::max<uint32_t>(n_prim, 1)); d_units.alloc(std::max<uint32_t>(n_prim, 1));
            d_nlen.alloc(std::max<uint32_t>(n_prim, 1)); d_nrecs.alloc(std::max<uint32_t>(n_prim, 1));
            const AlnPrimaries P{d_lseq.p, d_units.p, d_nlen.p, d_nrecs.p};
            hipLaunchKernelGGL(aln_place_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, d_prim.p, d_prim_ord.p, static_cast<uint32_t>(n_rec), d_prim_rec.p);
            LCTY_HIP(hipGetLastError());
            if (n_prim)
                hipLaunchKernelGGL(aln_primary_kernel, dim3(blocks_of(n_prim, 256)), dim3(256), 0, s, raw, d_rec_off.p, static_cast<uint32_t>(n_rec), d_prim_rec.p,
                                   n_prim, paired, P, d_err);
            LCTY_HIP(hipGetLastError());
            // ---- errors: of a record, of the walk behind the records, of the end of the file
            uint64_t r; uint32_t cls;
            if (err.take(s, r, cls)) {
                if (cls == A_CORRUPT) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BAM record", path);
                if (cls == A_FIRST_NOT_PRIMARY) fail(LCTY_ERR_INVALID_DATA, "First record in the BAM file is secondary/supplementary");
                if (cls == A_NO_SECOND_END) fail(LCTY_ERR_INVALID_DATA, "Read %s does not have a second read end", last_primary_name(r).c_str());
                if (cls == A_NO_REFERENCE) fail(LCTY_ERR_INVALID_DATA, "%s: mapped record without a reference", path);
                fail(LCTY_ERR_RUNTIME, "%s: unknown device error %u", path, cls);
            }
            walk_error();
            if (paired && (n_prim & 1u)) fail(LCTY_ERR_INVALID_DATA, "Read %s does not have a second read end", last_primary_name(n_rec).c_str());

            // ---- offsets: units, qualities, names; cigar_rel; the per-mate and per-pair arrays
            n_units = scan.run(d_units, d_unit_off, n_prim, ctx);
            DevBuf<uint64_t> d_qual_at, d_name_at;
            d_qual_at.alloc(n_prim + 1ull); d_name_at.alloc(n_prim + 1ull);
            launch_scan<uint64_t>(s, n_prim, LoadU32AsU64{d_lseq.p}, AddOp{}, 0ull, d_qual_at.p, true);
            launch_scan<uint64_t>(s, n_prim, LoadU32AsU64{d_nlen.p}, AddOp{}, 0ull, d_name_at.p, true);
            d_pmax.alloc(n_pairs); d_pmax.zero(s);
            hipLaunchKernelGGL(aln_pair_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, d_prim.p, d_prim_ord.p, d_cigar_at.p, d_prim_rec.p,
                               static_cast<uint32_t>(n_rec), paired, T->d_recs.p, d_pmax.p);
            LCTY_HIP(hipGetLastError());
            d_mate_len.alloc(2ull * n_pairs); d_mate_off.alloc(2ull * n_pairs + 1); d_qual_off.alloc(2ull * n_pairs + 1); d_nrm.alloc(2ull * n_pairs);
            d_aln_off.alloc(n_pairs + 1ull); d_cigar_off.alloc(n_pairs + 1ull); d_name_off.alloc(n_pairs + 1ull);
            const AlnTable A{d_mate_len.p, d_mate_off.p, d_qual_off.p, d_nrm.p, d_aln_off.p, d_cigar_off.p, d_name_off.p};
            hipLaunchKernelGGL(aln_mate_kernel, dim3(blocks_of(n_prim, 256)), dim3(256), 0, s, d_prim_rec.p, n_prim, static_cast<uint32_t>(n_rec), paired, P,
                               d_unit_off.p, d_qual_at.p, d_name_at.p, d_cigar_at.p, A);
            LCTY_HIP(hipGetLastError());
            uint64_t ends[2] = {0, 0};
            d_qual_at.download(&ends[0], 1, s, n_prim); d_name_at.download(&ends[1], 1, s, n_prim);
            LCTY_HIP(hipStreamSynchronize(s));
            n_qual = ends[0]; n_name = ends[1];
            S.ms_record = now_ms() - t0;

            // ---- gathers: CIGAR words, name bytes, quality bytes
            t0 = now_ms();
            T->d_cigar.alloc(std::max<uint32_t>(n_words, 1));
            d_names.alloc(std::max<uint64_t>(n_name, 1)); d_quals.alloc(std::max<uint64_t>(n_qual, 1));
            if (n_words)
                hipLaunchKernelGGL(cigar_gather_kernel<uint32_t>, dim3(blocks_of(n_words, 256)), dim3(256), 0, s, raw, d_rec_off.p, nullptr, d_cigar_at.p, static_cast<uint32_t>(n_rec),
                                   n_words, T->d_cigar.p);
            LCTY_HIP(hipGetLastError());
            if (n_name)
                hipLaunchKernelGGL(aln_bytes_kernel<false>, dim3(blocks_of(n_name, 256)), dim3(256), 0, s, d_raw, d_rec_off.p, d_prim_rec.p, d_name_at.p, n_prim,
                                   n_name, d_names.p);
            LCTY_HIP(hipGetLastError());
            if (n_qual && host_copy)                                             // nothing on the device reads qualities: they exist for the caller
                hipLaunchKernelGGL(aln_bytes_kernel<true>, dim3(blocks_of(n_qual, 256)), dim3(256), 0, s, d_raw, d_rec_off.p, d_prim_rec.p, d_qual_at.p, n_prim,
                                   n_qual, d_quals.p);
            LCTY_HIP(hipGetLastError());
            LCTY_HIP(hipStreamSynchronize(s));
            S.ms_gather = now_ms() - t0;

            // ---- SEQ of the primaries as stored
            t0 = now_ms();
            T->d_bases2.alloc(2ull * n_units + 2); T->d_nmask.alloc(n_units + 1ull);
            T->d_bases2.zero(s); T->d_nmask.zero(s);
            if (n_units)
                hipLaunchKernelGGL(unpack_kernel<false>, dim3(blocks_of(n_units, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_prim_rec.p, d_unit_off.p, n_prim, n_units,
                                   reinterpret_cast<uint64_t*>(T->d_bases2.p), T->d_nmask.p);
            LCTY_HIP(hipGetLastError());
            LCTY_HIP(hipStreamSynchronize(s));
            S.ms_unpack = now_ms() - t0;
        }

        // ---- the host's arrays: per pair always, everything with host_copy
        t0 = now_ms();
        T->n_recs = n_rec; T->n_cigar = n_words;
        T->mate_len.assign(2ull * n_pairs, 0); T->mate_off.assign(2ull * n_pairs + 1, 0); T->aln_off.assign(n_pairs + 1ull, 0);
        T->cigar_off.assign(n_pairs + 1ull, 0); T->name_off.assign(n_pairs + 1ull, 0); T->names.assign(n_name, '\0');
        T->n_recs_mate.assign(2ull * n_pairs, 0); T->pair_max_cigar.assign(n_pairs, 0);
        if (n_rec) {
            d_mate_len.download(T->mate_len.data(), 2ull * n_pairs, s); d_mate_off.download(T->mate_off.data(), 2ull * n_pairs + 1, s);
            d_aln_off.download(T->aln_off.data(), n_pairs + 1ull, s); d_cigar_off.download(T->cigar_off.data(), n_pairs + 1ull, s);
            d_name_off.download(T->name_off.data(), n_pairs + 1ull, s);
            d_names.download(reinterpret_cast<uint8_t*>(&T->names[0]), n_name, s);
            d_nrm.download(T->n_recs_mate.data(), 2ull * n_pairs, s); d_pmax.download(T->pair_max_cigar.data(), n_pairs, s);
        }
        if (host_copy) {
            T->recs.resize(n_rec); T->cigar.resize(n_words); T->mapq.resize(n_rec); T->quals.resize(n_qual); T->qual_off.assign(2ull * n_pairs + 1, 0);
            T->bases2.assign(std::max<uint64_t>(2ull * n_units, 2), 0); T->nmask.assign(std::max<uint64_t>(n_units, 1), 0);
            if (n_rec) {
                T->d_recs.download(T->recs.data(), n_rec, s); T->d_cigar.download(T->cigar.data(), n_words, s); d_mapq.download(T->mapq.data(), n_rec, s);
                d_quals.download(T->quals.data(), n_qual, s); d_qual_off.download(T->qual_off.data(), 2ull * n_pairs + 1, s);
                T->d_bases2.download(T->bases2.data(), 2ull * n_units, s); T->d_nmask.download(T->nmask.data(), n_units, s);
            }
        }
        LCTY_HIP(hipStreamSynchronize(s));
        S.ms_download = now_ms() - t0;
        T->view.n_pairs = n_pairs;
        if (host_copy) {
            T->view.mate_len = T->mate_len.data(); T->view.mate_off = T->mate_off.data(); T->view.bases2 = T->bases2.data(); T->view.nmask = T->nmask.data();
            T->view.aln_off = T->aln_off.data(); T->view.recs = T->recs.data(); T->view.cigar_off = T->cigar_off.data(); T->view.cigar = T->cigar.data();
        }
        S.pairs = n_pairs; S.bases = T->mate_off.back(); S.cigar_words = n_words;
        S.ms_total = now_ms() - t_start;
        if (stats) *stats = S;
        *out = T.release();
    });
}

int32_t lcty_bam_table_sizes(const lcty_bam_table* t, uint64_t* n_pairs, uint64_t* n_bases, uint64_t* n_recs, uint64_t* n_cigar, uint32_t* n_refs) {
    return guarded([&] {
        if (!t) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_pairs) *n_pairs = t->view.n_pairs;
        if (n_bases) *n_bases = t->mate_off.empty() ? 0 : t->mate_off.back();
        if (n_recs) *n_recs = t->ctx ? t->n_recs : t->recs.size();
        if (n_cigar) *n_cigar = t->ctx ? t->n_cigar : t->cigar.size();
        if (n_refs) *n_refs = t->n_refs;
    });
}

int32_t lcty_bam_table_quals(const lcty_bam_table* t, const uint64_t** qual_off, const uint8_t** quals, const uint8_t** mapq) {
    return guarded([&] {
        if (!t) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (!t->host_copy) fail(LCTY_ERR_INVALID_INPUT, "the table was read on the device without host_copy: its qualities were not downloaded");
        if (qual_off) *qual_off = t->qual_off.data();
        if (quals) *quals = t->quals.data();
        if (mapq) *mapq = t->mapq.data();
    });
}

int32_t lcty_reads_append_bam(lcty_reads* reads, const lcty_bam_table* t, uint64_t first_pair, uint64_t n) {
    lcty_reads_host h{};
    std::vector<uint64_t> mo, ao, co;
    DeviceRecords dev{};
    const int32_t rc = guarded([&] {
        if (!reads || !t) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (!t->ctx) fail(LCTY_ERR_INVALID_INPUT, "the table was read on the host (lcty_bam_read): append its view with lcty_reads_append");
        if (t->ctx != reads->ctx) fail(LCTY_ERR_INVALID_INPUT, "the table was read on another context than the batch's");
        const uint64_t P = t->view.n_pairs;
        if (first_pair > P || n > P - first_pair)
            fail(LCTY_ERR_INVALID_INPUT, "pairs [%llu, +%llu) are outside the table (%llu pairs)", static_cast<unsigned long long>(first_pair),
                 static_cast<unsigned long long>(n), static_cast<unsigned long long>(P));
        if (n == 0) return;
        // the rebased offsets of the range: mate_off is a multiple of 32 per mate, cigar_rel relative to the pair — nothing else moves
        const uint64_t b0 = t->mate_off[2 * first_pair], r0 = t->aln_off[first_pair], c0 = t->cigar_off[first_pair];
        mo.resize(2 * n + 1); ao.resize(n + 1); co.resize(n + 1);
        for (uint64_t m = 0; m <= 2 * n; m++) mo[m] = t->mate_off[2 * first_pair + m] - b0;
        for (uint64_t p = 0; p <= n; p++) { ao[p] = t->aln_off[first_pair + p] - r0; co[p] = t->cigar_off[first_pair + p] - c0; }
        h.n_pairs = n; h.mate_len = t->mate_len.data() + 2 * first_pair; h.mate_off = mo.data(); h.aln_off = ao.data(); h.cigar_off = co.data();
        dev.recs = t->d_recs.p + r0; dev.cigar = t->d_cigar.p + c0; dev.bases2 = t->d_bases2.p + b0 / 16; dev.nmask = t->d_nmask.p + b0 / 32;
        dev.n_recs_mate = t->n_recs_mate.data() + 2 * first_pair;
        dev.max_rec_cigar = *std::max_element(t->pair_max_cigar.begin() + first_pair, t->pair_max_cigar.begin() + first_pair + n);
    });
    if (rc != LCTY_OK || n == 0) return rc;
    return reads_append_device(reads, &h, &dev);
}

}  // extern "C"
