// lcty_sample_bam.hip — a sample's reads from a coordinate-sorted, indexed BAM file, the input of `locityper genotype -a`:
//   src/command/genotype.rs:776-797 postprocess_targets, 857-867 identify_pairedness, 872-907 recruit_to_targets
//   src/seq/fastx.rs:577-673 BamRecord (read_from, write_to), 692-729 DirectBamReader, 732-803 IndexedBamReader, 805-874 PairedBamReader
//   src/seq/interv.rs:74-77 add_padding, 232-247 merge
// Host: the BAI index (SAM specification 5.2: bins -> chunks, the 16 kb linear index, the pseudo-bin 37450, n_no_coor), reg2bins, the
// chunks of a call, pread of their byte ranges, inflation of their BGZF blocks into one page-locked buffer (zlib, or with knob
// "sample_bam_inflate" 1 bgzf_inflate_kernel of lcty_inflate.hip and a copy back), the chain of record lengths.
// Device, on the raw bytes of that buffer (records lie at any byte: every field is taken from two aligned dwords, ld32):
//   record_kernel   a lane per record: fixed fields, reference length of the CIGAR (a CIGAR of more than 64 operations is summed by the
//                   whole wavefront), the region / flag tests, the hash of the name, `curr <= mate`, the error classes
//   exclusive_scan  over the kept flags -> the fetched stream in file order
//   RadixSort       (hash of the name, stream ordinal): records of one hash side by side, in stream order
//   pair_kernel     a lane per record: PairedBamReader's state machine replayed over the records of ITS name before it in the run of
//                   its hash (names compared byte for byte), which says whether this record completes a pair and with whom
//   exclusive_scan  over the completing records -> the pairs in the reference's order; assemble_kernel gives every mate its record,
//                   length and units (stream_kernel, assemble_kernel: lcty_bam_layout.hpp, shared with lcty_bam_stream.hip), and
//                   ReadChunk::place (lcty_read_chunk.hpp) lays the mates out: the chunk the handle keeps, sized once
//   unpack_kernel   a lane per 32 bases of a mate: 4-bit codes -> bases2 / nmask, back to front and complemented for reverse records;
//                   a lane writes whole words of its own only
// The record on the device (lcty_bam_record.hpp) and the front half of a fetch (fetch_slice, lcty_sample_bam.hpp, over the slice of
// lcty_bgzf_read.hpp) are shared with the background route, lcty_bg_fetch.hip.
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "lcty_bam_layout.hpp"
#include "lcty_sample_bam.hpp"
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"

namespace lcty {

// error classes, by rank at one record (refuse, lcty_device.hpp)
enum : uint32_t { E_SHORT = 1, E_UNSORTED = 2, E_CG = 3, E_NOSEQ = 4, E_UNPAIRED = 5, E_TWO_ENDS = 6 };
constexpr uint32_t INFO_KEPT = 1u << 16, INFO_WAITS = 1u << 17;

struct SampleView {
    const uint32_t* raw;                        // the slice as dwords
    const uint64_t* rec_off; uint32_t n_rec;    // byte offset of every record (of its block_size field)
    const uint32_t* reg_tid; const uint32_t* reg_start; const uint32_t* reg_end; uint32_t n_reg;
    int with_unmapped, whole_file;
    uint64_t hash_mask;
    uint32_t* info;                             // flag | INFO_*
    uint64_t* hash;
    uint32_t* kept;                             // 0 / 1
    unsigned long long* err; uint32_t* n_primary;
};

__global__ __launch_bounds__(256) void record_kernel(const SampleView V) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = r < V.n_rec;
    const uint64_t o = valid ? V.rec_off[r] : 0ull;
    RecHead h{};
    bool fits = false;
    if (valid) { h = rec_head(V.raw, o); fits = rec_fits(h); }
    const uint64_t cig = o + 36 + h.l_name;
    // ---- reference length: up to 64 operations by the lane, more by the wavefront
    unsigned long long rlen = 0;
    const bool long_cigar = fits && h.n_cigar > 64u;
    if (fits && !long_cigar) for (uint32_t j = 0; j < h.n_cigar; j++) rlen += cigar_ref_len(ld32(V.raw, cig + 4ull * j));
    unsigned long long pending = __ballot(long_cigar);
    while (pending) {
        const int src = __ffsll(pending) - 1;
        pending &= pending - 1;
        const uint64_t c0 = __shfl(static_cast<unsigned long long>(cig), src);
        const uint32_t nc = __shfl(h.n_cigar, src);
        unsigned long long part = 0;
        for (uint32_t j = lane; j < nc; j += 64u) part += cigar_ref_len(ld32(V.raw, c0 + 4ull * j));
        part = wave_reduce(part, AddOp{});
        if (static_cast<int>(lane) == src) rlen = part;
    }
    // ---- the tests
    bool kept = false, primary = false;
    uint32_t err = 0, info = 0;
    if (valid && !fits) err = E_SHORT;
    if (fits) {
        primary = (h.flag & 0x900u) == 0;
        if (V.whole_file) kept = primary;
        else if (h.tid < 0) kept = primary && V.with_unmapped;
        else {
            if (h.flag & 4u) rlen = 0;
            const int64_t endpos = static_cast<int64_t>(h.pos) + static_cast<int64_t>(rlen ? rlen : 1ull);    // bam_endpos
            // the first region that ends behind pos (regions are sorted and disjoint): the only one the record can be taken by, since
            // the regions before it end at or before pos and a later one on this contig would refuse pos < its min_start
            uint32_t lo = 0, hi = V.n_reg;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) / 2;
                const uint32_t t = V.reg_tid[mid];
                const bool behind = t > static_cast<uint32_t>(h.tid) || (t == static_cast<uint32_t>(h.tid) && static_cast<int64_t>(V.reg_end[mid]) > h.pos);
                if (behind) hi = mid; else lo = mid + 1;
            }
            const bool overlaps = lo < V.n_reg && V.reg_tid[lo] == static_cast<uint32_t>(h.tid) && static_cast<int64_t>(V.reg_start[lo]) < endpos;
            kept = primary && overlaps;
            if (primary && !(h.flag & 4u) && h.n_cigar == 2u && ld32(V.raw, cig) == ((h.l_seq << 4) | 4u) && (ld32(V.raw, cig + 4) & 15u) == 3u)
                err = E_CG;
        }
        if (!err && kept && h.l_seq == 0) err = E_NOSEQ;                          // fastx.rs:599-602
        if (!V.whole_file && r > 0) {
            const uint64_t op = V.rec_off[r - 1];
            const uint64_t before = sort_key(static_cast<int32_t>(ld32(V.raw, op + 4)), static_cast<int32_t>(ld32(V.raw, op + 8)));
            if (before > sort_key(h.tid, h.pos) && (!err || err > E_UNSORTED)) err = E_UNSORTED;
        }
        const bool waits = static_cast<uint32_t>(h.tid) < static_cast<uint32_t>(h.mtid) ||
                           (h.tid == h.mtid && static_cast<uint64_t>(static_cast<int64_t>(h.pos)) <= static_cast<uint64_t>(static_cast<int64_t>(h.mpos)));
        info = h.flag | (kept ? INFO_KEPT : 0u) | (waits ? INFO_WAITS : 0u);
        if (kept) V.hash[r] = name_hash(V.raw, o, h.l_name) & V.hash_mask;
    }
    if (valid) {
        V.info[r] = info; V.kept[r] = kept ? 1u : 0u;
        if (!kept) V.hash[r] = 0;
        if (err) refuse(V.err, r, err);
    }
    const unsigned long long prim = __ballot(primary);
    if (lane == 0 && prim) atomicAdd(V.n_primary, static_cast<uint32_t>(__popcll(prim)));
}

// PairedBamReader::read_next (fastx.rs:829-869) for the record at place i of the sorted list: the records of its name before it, in
// stream order, leave a record waiting or nobody; then this record completes a pair, waits, is discarded or is an error.
__global__ __launch_bounds__(256) void pair_kernel(const uint32_t* __restrict__ raw, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ info,
                                                   const uint32_t* __restrict__ stream, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                   uint32_t n, uint32_t* __restrict__ mate_of, uint32_t* __restrict__ completes, unsigned long long* err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    uint32_t g = i;
    while (g > 0 && keys[g - 1] == key) g--;
    const uint32_t s = static_cast<uint32_t>(vals[i]), r = stream[s];
    const uint64_t o = rec_off[r];
    bool waiting = false, wait_first = false;
    uint32_t wait_s = 0, mate = NONE32;
    for (uint32_t t = g; t <= i; t++) {
        const uint32_t st = static_cast<uint32_t>(vals[t]), rt = stream[st];
        if (t < i && !same_name(raw, rec_off[rt], o)) continue;
        const uint32_t inf = info[rt];
        if ((inf & 0xC0u) == 0) {
            if (t == i) refuse(err, r, E_UNPAIRED);
            continue;
        }
        const bool first = (inf & 0x40u) != 0;
        if (waiting) {
            if (first == wait_first) { if (t == i) refuse(err, r, E_TWO_ENDS); }
            else if (t == i) mate = wait_s;
            waiting = false;                                                     // HashSet::take removed it either way
        } else if (inf & INFO_WAITS) { waiting = true; wait_first = first; wait_s = st; }
    }
    mate_of[s] = mate; completes[s] = mate != NONE32 ? 1u : 0u;
}

}  // namespace lcty

using namespace lcty;

namespace {

void load_bai(lcty_sample_bam* b) {
    const std::vector<uint8_t> x = read_whole_file(b->index_path.c_str());
    Bai B = parse_bai(x.data(), x.size(), b->lengths.size(), b->index_path.c_str());
    b->refs = std::move(B.refs);
    b->tail_start = std::max(b->first_record, B.tail_start);
    b->n_no_coor = B.n_no_coor; b->has_no_coor = B.has_no_coor;
}

// the chunks of a call: those of its regions (region_chunks) and the tail of the file, sorted and merged (merge_chunks,
// lcty_bgzf_index.hpp: the rule the tabix index of lcty_vcf_fetch.hip follows too)
std::vector<Chunk> plan_chunks(const lcty_sample_bam* b, uint32_t n, const uint32_t* tid, const uint32_t* start, const uint32_t* end, bool with_unmapped,
                               bool whole_file) {
    std::vector<Chunk> cs;
    const uint64_t file_end = b->file.fsize << 16;
    if (whole_file) { cs.push_back(Chunk{b->first_record, file_end}); return cs; }
    for (uint32_t i = 0; i < n; i++) region_chunks(b->refs[tid[i]], start[i], end[i], cs);
    if (with_unmapped && b->tail_start < file_end) cs.push_back(Chunk{b->tail_start, file_end});
    return merge_chunks(cs);
}

}  // namespace

namespace lcty {

void check_regions(const lcty_sample_bam* b, uint32_t n, const uint32_t* tid, const uint32_t* start, const uint32_t* end) {
    if (n && (!tid || !start || !end)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    for (uint32_t i = 0; i < n; i++) {
        if (tid[i] >= b->lengths.size()) fail(LCTY_ERR_INVALID_INPUT, "region %u: contig %u of %zu", i, tid[i], b->lengths.size());
        if (start[i] >= end[i]) fail(LCTY_ERR_INVALID_INPUT, "region %u is empty (%u-%u)", i, start[i], end[i]);
        if (i && (tid[i] < tid[i - 1] || (tid[i] == tid[i - 1] && start[i] < end[i - 1])))
            fail(LCTY_ERR_INVALID_INPUT, "Cannot fetch reads from BAM file: regions must be sorted (region %u)", i);       // fastx.rs:770
    }
}

void fetch_slice(lcty_ctx* ctx, lcty_sample_bam* bam, uint32_t n_regions, const uint32_t* tid, const uint32_t* start, const uint32_t* end,
                 bool with_unmapped, bool whole_file, Slice& F, lcty_sample_bam_stats& S) {
    const char* path = bam->file.path.c_str();
    SliceStats T{};
    F.read(ctx, bam->file, plan_chunks(bam, n_regions, tid, start, end, with_unmapped, whole_file), "sample_bam_max_slice_bytes", T);
    T.ms_inflate = F.inflate(ctx, path);
    T.put(S);

    // ---- the chain of record lengths
    const double t0 = now_ms();
    std::vector<uint64_t>& rec_off = F.rec_off;
    for (const ChunkSpan& sp : F.spans) {
        uint64_t p = sp.chain_beg;
        while (p < sp.chain_end) {
            uint32_t bs = 0;
            if (p + 4 <= sp.span_end) memcpy(&bs, F.slice + p, 4);
            if (p + 4 > sp.span_end || bs < 32 || p + 4 + bs > sp.span_end)
                fail(LCTY_ERR_INVALID_DATA, "%s: record %zu of the fetched slice is truncated, or its length (%u) leaves the slice", path, rec_off.size(), bs);
            rec_off.push_back(p);
            p += 4ull + bs;
        }
    }
    const uint64_t n_rec = rec_off.size();
    S.records_walked = n_rec;
    S.ms_walk = now_ms() - t0;
    if (n_rec >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%s: %llu records in one fetch", path, static_cast<unsigned long long>(n_rec));
}

}  // namespace lcty

extern "C" {

int32_t lcty_sample_bam_open(const char* path, const char* index_path, lcty_sample_bam** out) {
    return guarded([&] {
        if (!path || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *out = nullptr;
        std::unique_ptr<lcty_sample_bam> b(new lcty_sample_bam());
        b->file.open(path);
        uint8_t magic[4] = {0, 0, 0, 0};
        if (b->file.fsize >= 4) pread_all(b->file.fd, magic, 4, 0, path);
        if (memcmp(magic, "CRAM", 4) == 0) fail(LCTY_ERR_UNSUPPORTED, "%s is a CRAM file (only BAM files are read)", path);
        // ---- the header (SAM specification 4.2)
        BgzfSerial in(b->file.fd, b->file.fsize, path);
        uint8_t head[8];
        if (!in.read(head, 8) || memcmp(head, "BAM\1", 4) != 0) fail(LCTY_ERR_INVALID_DATA, "%s is not a BAM file", path);
        uint32_t l_text; memcpy(&l_text, head + 4, 4);
        std::vector<uint8_t> text(l_text);
        uint32_t n_ref = 0;
        if (!in.read(text.data(), l_text) || !in.read(&n_ref, 4)) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM header", path);
        for (uint32_t r = 0; r < n_ref; r++) {
            uint32_t l_name = 0, l_ref = 0;
            if (!in.read(&l_name, 4) || l_name == 0 || l_name > (1u << 20)) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM header", path);
            std::string nm(l_name, '\0');
            if (!in.read(&nm[0], l_name) || !in.read(&l_ref, 4)) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM header", path);
            b->name_off.push_back(b->names.size());
            b->names.append(nm.c_str()); b->names.push_back('\0');
            b->lengths.push_back(l_ref);
        }
        b->name_off.push_back(b->names.size());
        (void)in.load();
        b->first_record = in.tell();
        uint8_t rec[36];
        if (in.read(rec, 36)) { uint16_t flag; memcpy(&flag, rec + 18, 2); b->paired = flag & 1; } else b->paired = -2;
        // ---- the index
        const std::string p = path;
        if (index_path) b->index_path = index_path;
        else if (is_regular_file(p + ".bai")) b->index_path = p + ".bai";
        else if (p.size() > 4 && has_suffix(p, ".bam") && is_regular_file(p.substr(0, p.size() - 4) + ".bai")) b->index_path = p.substr(0, p.size() - 4) + ".bai";
        else if (is_regular_file(p + ".csi")) fail(LCTY_ERR_UNSUPPORTED, "%s.csi is a CSI index (only BAI indices are read)", path);
        else fail(LCTY_ERR_INVALID_INPUT, "no index for %s (%s.bai)", path, path);
        if (!is_regular_file(b->index_path)) fail(LCTY_ERR_INVALID_INPUT, "no index for %s (%s)", path, b->index_path.c_str());
        load_bai(b.get());
        *out = b.release();
    });
}

void lcty_sample_bam_close(lcty_sample_bam* bam) { delete bam; }

int32_t lcty_sample_bam_contigs(const lcty_sample_bam* bam, uint32_t* n, const char** names, const uint64_t** name_off, const uint32_t** lengths) {
    return guarded([&] {
        if (!bam || !n) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *n = static_cast<uint32_t>(bam->lengths.size());
        if (names) *names = bam->names.c_str();
        if (name_off) *name_off = bam->name_off.data();
        if (lengths) *lengths = bam->lengths.data();
    });
}

int32_t lcty_sample_bam_is_paired(lcty_sample_bam* bam, int32_t* paired) {
    return guarded([&] {
        if (!bam || !paired) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (bam->paired < 0) fail(LCTY_ERR_INVALID_DATA, "Input BAM/CRAM file is empty");              // genotype.rs:861
        *paired = bam->paired;
    });
}

int32_t lcty_recruit_fetch_regions(uint32_t n_in, const uint32_t* tid, const uint32_t* start, const uint32_t* end, uint32_t n_contigs,
                                   const uint32_t* contig_len, uint32_t padding, uint32_t alt_contig_len, uint32_t merge_distance,
                                   uint32_t* out_tid, uint32_t* out_start, uint32_t* out_end, uint32_t* n_out) {
    return guarded([&] {
        if ((n_in && (!tid || !start || !end)) || (n_contigs && !contig_len) || !out_tid || !out_start || !out_end || !n_out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        struct Iv { uint32_t tid, start, end; };
        std::vector<Iv> v;
        for (uint32_t i = 0; i < n_in; i++) {
            if (tid[i] >= n_contigs) fail(LCTY_ERR_INVALID_INPUT, "interval %u: contig %u of %u", i, tid[i], n_contigs);
            if (start[i] >= end[i]) fail(LCTY_ERR_INVALID_INPUT, "interval %u is empty (%u-%u)", i, start[i], end[i]);
            // Interval::add_padding (interv.rs:74-77)
            const uint64_t e = std::min<uint64_t>(static_cast<uint64_t>(end[i]) + padding, contig_len[tid[i]]);
            v.push_back(Iv{tid[i], start[i] > padding ? start[i] - padding : 0u, static_cast<uint32_t>(e)});
        }
        for (uint32_t c = 0; c < n_contigs; c++) if (contig_len[c] < alt_contig_len) v.push_back(Iv{c, 0, contig_len[c]});
        std::sort(v.begin(), v.end(), [](const Iv& a, const Iv& b) { return a.tid != b.tid ? a.tid < b.tid : a.start != b.start ? a.start < b.start : a.end < b.end; });
        uint32_t m = 0;
        for (const Iv& c : v) {                                                  // Interval::merge (interv.rs:232-247)
            if (m && out_tid[m - 1] == c.tid && static_cast<uint64_t>(out_end[m - 1]) + merge_distance >= c.start) out_end[m - 1] = std::max(out_end[m - 1], c.end);
            else { out_tid[m] = c.tid; out_start[m] = c.start; out_end[m] = c.end; m++; }
        }
        *n_out = m;
    });
}

int32_t lcty_sample_bam_plan(lcty_sample_bam* bam, uint32_t n_regions, const uint32_t* tid, const uint32_t* start, const uint32_t* end,
                             int32_t with_unmapped, uint64_t chunk_cap, uint64_t* n_chunks, uint64_t* chunk_beg, uint64_t* chunk_end,
                             uint64_t* blocks_total) {
    return guarded([&] {
        if (!bam || !n_chunks || (chunk_cap && (!chunk_beg || !chunk_end))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_regions(bam, n_regions, tid, start, end);
        report_plan(bam->file, plan_chunks(bam, n_regions, tid, start, end, with_unmapped != 0, false), chunk_cap, n_chunks, chunk_beg, chunk_end, blocks_total);
    });
}

int32_t lcty_sample_bam_fetch(lcty_ctx* ctx, lcty_sample_bam* bam, uint32_t n_regions, const uint32_t* tid, const uint32_t* start,
                              const uint32_t* end, int32_t with_unmapped, int32_t whole_file, int32_t paired, lcty_sample_reads** reads,
                              lcty_sample_bam_stats* stats) {
    if (reads) *reads = nullptr;
    if (stats) memset(stats, 0, sizeof(*stats));
    return guarded([&] {
        if (!ctx || !bam || !reads) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double t_start = now_ms();
        const char* path = bam->file.path.c_str();
        if (whole_file && (n_regions || with_unmapped)) fail(LCTY_ERR_INVALID_INPUT, "whole_file goes without regions and without with_unmapped");
        if (!whole_file && !n_regions && !with_unmapped) fail(LCTY_ERR_INVALID_INPUT, "nothing to fetch: no regions, no unmapped reads, not the whole file");
        if (paired < 0) {
            if (bam->paired < 0) fail(LCTY_ERR_INVALID_DATA, "Input BAM/CRAM file is empty");
            paired = bam->paired;
        }
        if (paired && whole_file) fail(LCTY_ERR_UNSUPPORTED, "paired-end reads of a BAM file are read through its index: give the regions (fastx.rs:692-729 is single-end)");
        check_regions(bam, n_regions, tid, start, end);
        const int64_t hash_bits = ctx->knob("sample_bam_hash_bits", 64);
        if (hash_bits > 64) fail(LCTY_ERR_INVALID_INPUT, "sample_bam_hash_bits = %lld (0 .. 64)", static_cast<long long>(hash_bits));
        const uint64_t hash_mask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1;
        lcty_sample_bam_stats S{};
        S.n_regions = n_regions; S.file_bytes = bam->file.fsize;
        // ---- the front half: chunks, pread, BGZF split, inflate, the chain of record lengths
        std::unique_ptr<lcty_sample_reads> R(new lcty_sample_reads(ctx, ReadChunk::Buffers::OneShot));
        ReadChunk& C = R->chunk; C.paired = paired != 0;
        fetch_slice(ctx, bam, n_regions, tid, start, end, with_unmapped != 0, whole_file != 0, R->F, S);
        hipStream_t s = ctx->stream;
        const std::vector<uint64_t>& rec_off = R->F.rec_off;
        const uint64_t n_rec = rec_off.size();
        double t0;

        auto finish = [&]() {
            R->F.release_device();                                               // the handle keeps the host's slice alone
            S.ms_total = now_ms() - t_start;
            if (stats) *stats = S;
            *reads = R.release();
        };
        if (n_rec == 0) { finish(); return; }                                    // the empty chunk

        // ---- upload, record kernel
        t0 = now_ms();
        DevBuf<uint64_t> d_rec_off, d_hash; DevBuf<uint32_t> d_reg, d_info, d_kept, d_nprim; ErrWord err;
        const uint32_t* raw = reinterpret_cast<const uint32_t*>(R->F.device(s));
        d_rec_off.alloc(n_rec); d_rec_off.upload(rec_off.data(), n_rec, s);
        std::vector<uint32_t> reg(3ull * std::max(n_regions, 1u), 0);
        for (uint32_t i = 0; i < n_regions; i++) { reg[i] = tid[i]; reg[n_regions + i] = start[i]; reg[2ull * n_regions + i] = end[i]; }
        d_reg.alloc(reg.size()); d_reg.upload(reg.data(), reg.size(), s);
        d_info.alloc(n_rec); d_kept.alloc(n_rec); d_hash.alloc(n_rec); d_nprim.alloc(1);
        d_nprim.zero(s);
        unsigned long long* d_err = err.reset(s);
        LCTY_HIP(hipStreamSynchronize(s));
        S.ms_upload = now_ms() - t0;
        t0 = now_ms();
        SampleView V{};
        V.raw = raw; V.rec_off = d_rec_off.p; V.n_rec = static_cast<uint32_t>(n_rec);
        V.reg_tid = d_reg.p; V.reg_start = d_reg.p + n_regions; V.reg_end = d_reg.p + 2ull * n_regions; V.n_reg = n_regions;
        V.with_unmapped = with_unmapped != 0; V.whole_file = whole_file != 0; V.hash_mask = hash_mask;
        V.info = d_info.p; V.hash = d_hash.p; V.kept = d_kept.p; V.err = d_err; V.n_primary = d_nprim.p;
        hipLaunchKernelGGL(record_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, V);
        LCTY_HIP(hipGetLastError());
        ScanTotal scan;
        DevBuf<uint32_t> d_scan, d_stream;
        const uint32_t n_stream = scan.run(d_kept, d_scan, n_rec, ctx);
        auto check_err = [&]() {
            uint64_t r; uint32_t cls;
            if (!err.take(s, r, cls)) return;
            const uint64_t o = rec_off[r];
            if (cls == E_SHORT) fail(LCTY_ERR_INVALID_DATA, "%s: record %llu of the fetched slice is shorter than its fields", path, static_cast<unsigned long long>(r));
            const std::string name = record_name(R->F.slice, o);
            if (cls == E_UNSORTED) fail(LCTY_ERR_INVALID_DATA, "%s: coordinates run backwards at read %s: the file is not sorted", path, name.c_str());
            if (cls == E_CG) fail(LCTY_ERR_UNSUPPORTED, "%s: the CIGAR of read %s is kept in a CG tag (more than 65 535 operations)", path, name.c_str());
            if (cls == E_NOSEQ) fail(LCTY_ERR_INVALID_DATA, "Primary alignment for read %s has no sequence", name.c_str());
            if (cls == E_UNPAIRED) fail(LCTY_ERR_INVALID_DATA, "Expected paired-end reads, but read %s is unpaired", name.c_str());
            if (cls == E_TWO_ENDS) fail(LCTY_ERR_INVALID_DATA, "Found two primary alignments for %s for the same read end", name.c_str());
            fail(LCTY_ERR_RUNTIME, "%s: unknown device error %u", path, cls);
        };
        check_err();
        uint32_t n_primary = 0;
        d_nprim.download(&n_primary, 1, s);
        LCTY_HIP(hipStreamSynchronize(s));
        S.records_primary = n_primary; S.records_kept = n_stream;
        S.ms_record = now_ms() - t0;

        // ---- the stream, and its pairs
        t0 = now_ms();
        d_stream.alloc(std::max<uint32_t>(n_stream, 1));
        DevBuf<uint64_t> d_ka, d_va, d_kb, d_vb;
        DevBuf<uint32_t> d_mate_of, d_completes, d_pair_ix;
        if (paired) { d_ka.alloc(std::max<uint32_t>(n_stream, 1)); d_va.alloc(d_ka.n); d_kb.alloc(d_ka.n); d_vb.alloc(d_ka.n); }
        hipLaunchKernelGGL(stream_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, static_cast<uint32_t>(n_rec), d_kept.p, d_scan.p, d_hash.p,
                           d_stream.p, paired ? d_ka.p : nullptr, paired ? d_va.p : nullptr);
        LCTY_HIP(hipGetLastError());
        uint64_t n_out = n_stream;
        RadixSort sorter;
        if (paired && n_stream) {
            std::vector<uint32_t> shifts;
            for (uint32_t sh = 0; sh < static_cast<uint32_t>(std::max<int64_t>(hash_bits, 0)); sh += 8) shifts.push_back(sh);
            int where = 0;
            if (!shifts.empty()) where = sorter.run(d_ka.p, d_va.p, d_kb.p, d_vb.p, n_stream, shifts, s);
            const uint64_t* keys = where ? d_kb.p : d_ka.p; const uint64_t* vals = where ? d_vb.p : d_va.p;
            d_mate_of.alloc(n_stream); d_completes.alloc(n_stream);
            hipLaunchKernelGGL(pair_kernel, dim3(blocks_of(n_stream, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_info.p, d_stream.p, keys, vals, n_stream,
                               d_mate_of.p, d_completes.p, d_err);
            LCTY_HIP(hipGetLastError());
            n_out = scan.run(d_completes, d_pair_ix, n_stream, ctx);
            check_err();
        } else if (paired) n_out = 0;
        S.n_pairs = n_out; S.n_discarded = paired ? n_stream - 2 * n_out : 0;
        S.ms_pair = now_ms() - t0;

        // ---- the mates and their bases
        t0 = now_ms();
        if (n_out == 0) { finish(); return; }
        DevBuf<uint32_t> d_units, d_src, d_src_stream;
        C.reserve_mates(n_out);
        d_src_stream.alloc(2 * n_out); d_src.alloc(2 * n_out); d_units.alloc(2 * n_out);
        hipLaunchKernelGGL(assemble_kernel, dim3(blocks_of(n_stream, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_info.p, d_stream.p, n_stream, paired ? 1 : 0,
                           d_mate_of.p, d_pair_ix.p, d_src.p, d_src_stream.p, C.d_len.p, d_units.p);
        LCTY_HIP(hipGetLastError());
        const uint32_t n_units = C.place(d_units, 2 * n_out, scan);
        if (n_units)
            hipLaunchKernelGGL(unpack_kernel<true>, dim3(blocks_of(n_units, 256)), dim3(256), 0, s, raw, d_rec_off.p, d_src.p, C.d_unit_off.p,
                               static_cast<uint32_t>(2 * n_out), n_units, C.d_bases.p, C.d_nm.p);
        LCTY_HIP(hipGetLastError());
        R->h_src.resize(2 * n_out); R->h_src_stream.resize(2 * n_out);
        d_src_stream.download(R->h_src_stream.data(), 2 * n_out, s); d_src.download(R->h_src.data(), 2 * n_out, s);
        LCTY_HIP(hipStreamSynchronize(s));
        C.d_unit_off.release();                                                  // nothing reads it behind the unpack: the handle keeps the chunk alone
        S.ms_unpack = now_ms() - t0;
        finish();
    });
}

int32_t lcty_sample_reads_view(lcty_sample_reads* R, lcty_reads_host* view, const uint32_t** src_record, int32_t* paired) {
    return guarded([&] {
        if (!R || !view) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        R->chunk.view(view);
        if (src_record) *src_record = R->h_src_stream.data();
        if (paired) *paired = R->chunk.paired ? 1 : 0;
    });
}

int32_t lcty_sample_reads_recruit(lcty_targets* targets, lcty_sample_reads* R, uint32_t max_out, uint32_t* out_cnt, uint32_t* out_loci) {
    return guarded([&] {
        if (!targets || !R || !out_cnt || !out_loci || max_out == 0) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        R->chunk.recruit(targets, max_out, out_cnt, out_loci);
    });
}

int32_t lcty_sample_reads_write_recruited(lcty_sample_reads* R, lcty_fastx_writers* w, uint32_t max_out, const uint32_t* out_cnt,
                                          const uint32_t* out_loci, uint64_t* n_written) {
    return guarded([&] {
        if (!R || !w || !out_cnt || !out_loci || max_out == 0) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const uint64_t written = write_recruited_units(w, R->chunk.n, max_out, out_cnt, out_loci, [&](uint64_t i, std::string& text) {
            for (uint32_t e = 0; e < 2; e++) {                                   // the mates one after the other
                const uint32_t r = R->h_src[2 * i + e];
                if (r != NONE32) bam_record_text(R->F.slice, R->F.rec_off[r], text);
            }
        });
        if (n_written) *n_written = written;
    });
}

void lcty_sample_reads_free(lcty_sample_reads* reads) { delete reads; }

}  // extern "C"

namespace lcty {

// the name lcty_sample_reads_write_recruited writes for pair i: its first read end's
std::string sample_reads_name(lcty_sample_reads* R, uint64_t i) {
    const uint32_t r = R->h_src[2 * i] != NONE32 ? R->h_src[2 * i] : R->h_src[2 * i + 1];
    return r == NONE32 ? std::string() : record_name(R->F.slice, R->F.rec_off[r]);
}

}  // namespace lcty
