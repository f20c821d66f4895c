// lcty_bgzf_index.hpp — the indices of BGZF files and the host passes of the indexed VCF reader (lcty_vcf_fetch.hip):
// the pieces the two index readers and the two VCF readers share. Standard library and lcty_host.hpp only, no HIP call, no zlib and
// no file: the bytes come read and inflated. scripts/vcf_index_probe_host.cpp runs all of it on the CPU alone.
//   the index    a bin / linear index (SAM specification 5.2, 5.3; the tabix format): IndexRef, the chunks of a region
//                (region_chunks) and their merge (merge_chunks) — one definition for the BAI of lcty_sample_bam.hip and the TBI of
//                lcty_vcf_fetch.hip — and the two parsers (parse_bai, parse_tbi)
//   the text     what lcty_vcf_open and lcty_vcf_region (lcty_io.hip) do with one line: the #CHROM line (parse_chrom_line), the head
//                of a record (parse_line_head), the ploidies of the first record (first_record_ploidy), a record of a region
//                (parse_record_line), with their statuses and message texts. The indexed reader calls the same functions, so what it
//                raises is the text of lcty_vcf_open / lcty_vcf_region by construction.
#pragma once

#include <string>
#include <unordered_map>
#include <vector>

#include "lcty_host.hpp"

namespace lcty {

struct Chunk { uint64_t beg, end; };           // virtual offsets of the index

// one reference of a bin / linear index
struct IndexRef { std::unordered_map<uint32_t, std::vector<Chunk>> bins; std::vector<uint64_t> linear; };

// The chunks of [start, end) on one reference, appended to cs: reg2bins (SAM specification 5.3) without the chunks that end at or
// before the linear index's offset of the region's first 16 kb window.
inline void region_chunks(const IndexRef& R, uint32_t start, uint32_t end, std::vector<Chunk>& cs) {
    const uint32_t beg = std::min(start, (1u << 29) - 1), e = std::min(end, 1u << 29) - 1;      // e: last base, inclusive
    uint64_t min_off = 0;
    if (!R.linear.empty()) min_off = R.linear[std::min<size_t>(beg >> 14, R.linear.size() - 1)];
    auto take = [&](uint32_t bin) {
        auto it = R.bins.find(bin);
        if (it == R.bins.end()) return;
        for (const Chunk& c : it->second) if (c.end > min_off && c.beg < c.end) cs.push_back(c);
    };
    take(0);
    static const uint32_t first[5] = {1, 9, 73, 585, 4681}, shift[5] = {26, 23, 20, 17, 14};
    for (int l = 0; l < 5; l++) for (uint32_t k = first[l] + (beg >> shift[l]); k <= first[l] + (e >> shift[l]); k++) take(k);
}

// sorted, and merged where they touch, overlap, or where one starts in the block the last one ends in: one chunk (what lies between
// is walked and filtered)
inline std::vector<Chunk> merge_chunks(std::vector<Chunk>& cs) {
    std::sort(cs.begin(), cs.end(), [](const Chunk& a, const Chunk& c) { return a.beg != c.beg ? a.beg < c.beg : a.end < c.end; });
    std::vector<Chunk> merged;
    for (const Chunk& c : cs) {
        if (!merged.empty() && (c.beg >> 16) <= (merged.back().end >> 16)) merged.back().end = std::max(merged.back().end, c.end);
        else merged.push_back(c);
    }
    return merged;
}

// x[0 .. n): the bytes of a .bai file of a BAM file whose header names n_refs_of_header references. tail_start: the largest chunk end
// of the index (0 without chunks). The trailing n_no_coor is optional, bytes behind it are ignored.
struct Bai {
    std::vector<IndexRef> refs;
    uint64_t tail_start = 0;
    uint64_t n_no_coor = 0; bool has_no_coor = false;
};
inline Bai parse_bai(const uint8_t* x, size_t n, size_t n_refs_of_header, const char* ip) {
    if (n >= 4 && memcmp(x, "CSI\1", 4) == 0) fail(LCTY_ERR_UNSUPPORTED, "%s is a CSI index (only BAI indices are read)", ip);
    if (n >= 2 && x[0] == 0x1f && x[1] == 0x8b) fail(LCTY_ERR_UNSUPPORTED, "%s is compressed: a CSI index? (only BAI indices are read)", ip);
    if (n < 8 || memcmp(x, "BAI\1", 4) != 0) fail(LCTY_ERR_INVALID_DATA, "%s is not a BAI index", ip);
    size_t at = 4;
    auto need = [&](size_t k) { if (k > n - at) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAI index", ip); };
    auto u32 = [&]() { need(4); uint32_t v; memcpy(&v, x + at, 4); at += 4; return v; };
    auto u64 = [&]() { need(8); uint64_t v; memcpy(&v, x + at, 8); at += 8; return v; };
    const uint32_t n_ref = u32();
    if (n_ref != n_refs_of_header) fail(LCTY_ERR_INVALID_DATA, "%s: the index has %u references, the BAM header %zu", ip, n_ref, n_refs_of_header);
    Bai B;
    B.refs.resize(n_ref);
    for (uint32_t r = 0; r < n_ref; r++) {
        const uint32_t n_bin = u32();
        for (uint32_t k = 0; k < n_bin; k++) {
            const uint32_t bin = u32(), n_chunk = u32();
            need(16ull * n_chunk);
            std::vector<Chunk> cs(n_chunk);
            for (uint32_t c = 0; c < n_chunk; c++) { cs[c].beg = u64(); cs[c].end = u64(); }
            if (bin == 37450) { if (n_chunk) B.tail_start = std::max(B.tail_start, cs[0].end); continue; }      // pseudo-bin: file range, counts
            for (const Chunk& c : cs) B.tail_start = std::max(B.tail_start, c.end);
            B.refs[r].bins[bin] = std::move(cs);
        }
        const uint32_t n_intv = u32();
        need(8ull * n_intv);
        B.refs[r].linear.resize(n_intv);
        for (uint32_t k = 0; k < n_intv; k++) B.refs[r].linear[k] = u64();
    }
    if (n - at >= 8) { B.n_no_coor = u64(); B.has_no_coor = true; }
    return B;
}

namespace vcfidx {

struct Tbi {
    std::vector<std::string> names;
    std::vector<IndexRef> refs;
    uint64_t n_no_coor = 0; bool has_no_coor = false;
};

// x[0 .. n): the inflated bytes of a .tbi file. Every count and length is compared with the bytes that are left before it is used.
inline Tbi parse_tbi(const uint8_t* x, uint64_t n, const char* ip) {
    if (n >= 4 && memcmp(x, "CSI\1", 4) == 0) fail(LCTY_ERR_UNSUPPORTED, "%s is a CSI index (only tabix indices are read)", ip);
    if (n < 4 || memcmp(x, "TBI\1", 4) != 0) fail(LCTY_ERR_INVALID_DATA, "%s is not a tabix index", ip);
    uint64_t at = 4;
    auto need = [&](uint64_t k) { if (k > n - at) fail(LCTY_ERR_INVALID_DATA, "%s: truncated tabix index", ip); };
    auto i32 = [&]() { need(4); int32_t v; memcpy(&v, x + at, 4); at += 4; return v; };
    auto u32 = [&]() { need(4); uint32_t v; memcpy(&v, x + at, 4); at += 4; return v; };
    auto u64 = [&]() { need(8); uint64_t v; memcpy(&v, x + at, 8); at += 8; return v; };
    auto count = [&](const char* what, uint64_t each) {          // a count of items of at least `each` bytes
        const int32_t v = i32();
        if (v < 0) fail(LCTY_ERR_INVALID_DATA, "%s: negative %s (%d)", ip, what, v);
        if (static_cast<uint64_t>(v) > (n - at) / each) fail(LCTY_ERR_INVALID_DATA, "%s: truncated tabix index (%s = %d)", ip, what, v);
        return static_cast<uint32_t>(v);
    };
    const uint32_t n_ref = count("n_ref", 8);                    // a reference has at least n_bin and n_intv
    const int32_t format = i32();
    for (int k = 0; k < 5; k++) (void)i32();                     // col_seq, col_beg, col_end, meta, skip
    if (format != 2) fail(LCTY_ERR_INVALID_DATA, "%s: the index is of format %d, not of a VCF file (2)", ip, format);
    const uint32_t l_nm = count("l_nm", 1);
    Tbi T;
    uint64_t p = at;
    const uint64_t names_end = at + l_nm;
    for (uint32_t r = 0; r < n_ref; r++) {
        uint64_t q = p;
        while (q < names_end && x[q]) q++;
        if (q >= names_end) fail(LCTY_ERR_INVALID_DATA, "%s: the %u names of the index are not terminated inside their %u bytes", ip, n_ref, l_nm);
        T.names.emplace_back(reinterpret_cast<const char*>(x + p), q - p);
        p = q + 1;
    }
    at = names_end;
    T.refs.resize(n_ref);
    for (uint32_t r = 0; r < n_ref; r++) {
        const uint32_t n_bin = count("n_bin", 8);
        for (uint32_t k = 0; k < n_bin; k++) {
            const uint32_t bin = u32();
            const uint32_t n_chunk = count("n_chunk", 16);
            std::vector<Chunk> cs(n_chunk);
            for (uint32_t c = 0; c < n_chunk; c++) {
                cs[c].beg = u64(); cs[c].end = u64();
                if (bin != 37450 && cs[c].beg > cs[c].end) fail(LCTY_ERR_INVALID_DATA, "%s: a chunk of bin %u begins behind its end", ip, bin);
            }
            if (bin == 37450) continue;                          // pseudo-bin: file range, counts
            std::vector<Chunk>& into = T.refs[r].bins[bin];
            into.insert(into.end(), cs.begin(), cs.end());
        }
        const uint32_t n_intv = count("n_intv", 8);
        T.refs[r].linear.resize(n_intv);
        for (uint32_t k = 0; k < n_intv; k++) T.refs[r].linear[k] = u64();
    }
    if (n - at >= 8) { T.n_no_coor = u64(); T.has_no_coor = true; }
    else if (n != at) fail(LCTY_ERR_INVALID_DATA, "%s: truncated tabix index", ip);
    return T;
}

// the merged chunks of [start, end) on the reference `contig`; a contig the index does not know has none
inline std::vector<Chunk> plan(const Tbi& T, const char* contig, uint32_t start, uint32_t end) {
    std::vector<Chunk> cs;
    if (end == 0) return cs;                                     // pos < end holds for no record
    // a record is fetched iff pos < end and pos + len(REF) > start: with end <= start these are the records over [end - 1, start]
    const uint32_t s2 = std::min(start, end - 1), e2 = std::max(end, start == 0xFFFFFFFFu ? start : start + 1);
    for (size_t r = 0; r < T.names.size(); r++)
        if (T.names[r] == contig) region_chunks(T.refs[r], s2, e2, cs);
    return merge_chunks(cs);
}

// ---- the text -------------------------------------------------------------------------------------------------------------------

struct Field { const char* p; size_t n; };

// the tab-separated fields of [begin, end)
inline std::vector<Field> split_tabs(const uint8_t* text, uint64_t begin, uint64_t end) {
    std::vector<Field> out;
    uint64_t s = begin;
    for (uint64_t i = begin; i <= end; i++)
        if (i == end || text[i] == '\t') { out.push_back({reinterpret_cast<const char*>(text) + s, size_t(i - s)}); s = i + 1; }
    return out;
}

// The GT subfield of one sample: allele indices (-1 for '.') and whether the separator before the last allele is '|' (a haploid call has
// none and counts as phased). `which` = position of GT among the FORMAT keys.
inline void parse_gt(Field sample, size_t which, std::vector<int32_t>& alleles, bool& phased, const std::string& where) {
    const char* p = sample.p; const char* e = sample.p + sample.n;
    for (size_t skip = 0; skip < which && p < e; skip++) { while (p < e && *p != ':') p++; if (p < e) p++; else { p = e; } }
    const char* q = p;
    while (q < e && *q != ':') q++;
    alleles.clear(); phased = true;
    if (p == q) { alleles.push_back(-1); return; }                     // a dropped trailing field: one missing allele
    while (p < q) {
        if (*p == '.') { alleles.push_back(-1); p++; }
        else {
            if (*p < '0' || *p > '9') fail(LCTY_ERR_INVALID_DATA, "Variant %s: cannot parse the genotype '%.*s'", where.c_str(), int(sample.n), sample.p);
            int64_t v = 0;
            while (p < q && *p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); if (v > 32767) fail(LCTY_ERR_UNSUPPORTED, "Variant %s: allele index above 32767", where.c_str()); p++; }
            alleles.push_back(static_cast<int32_t>(v));
        }
        if (p < q) {
            if (*p != '/' && *p != '|') fail(LCTY_ERR_INVALID_DATA, "Variant %s: cannot parse the genotype '%.*s'", where.c_str(), int(sample.n), sample.p);
            phased = *p == '|';
            p++;
            if (p == q) fail(LCTY_ERR_INVALID_DATA, "Variant %s: cannot parse the genotype '%.*s'", where.c_str(), int(sample.n), sample.p);
        }
    }
}

inline size_t gt_index(Field format, const std::string& where) {
    size_t ix = 0, s = 0;
    for (size_t i = 0; i <= format.n; i++)
        if (i == format.n || format.p[i] == ':') {
            if (i - s == 2 && format.p[s] == 'G' && format.p[s + 1] == 'T') return ix;
            ix++; s = i + 1;
        }
    fail(LCTY_ERR_INVALID_DATA, "Variant %s has no GT field", where.c_str());
}

// a line [b, le) that starts with #CHROM: the sample names behind the ninth column
inline void parse_chrom_line(const uint8_t* t, uint64_t b, uint64_t le, const char* path, std::vector<std::string>& samples) {
    const std::vector<Field> f = split_tabs(t, b, le);
    if (f.size() < 8) fail(LCTY_ERR_INVALID_DATA, "%s: the #CHROM line has %zu columns", path, f.size());
    for (size_t i = 9; i < f.size(); i++) samples.emplace_back(f[i].p, f[i].n);
}
[[noreturn]] inline void fail_record_before_header(const char* path) { fail(LCTY_ERR_INVALID_DATA, "%s: a record comes before the #CHROM line", path); }
[[noreturn]] inline void fail_no_header(const char* path) { fail(LCTY_ERR_INVALID_DATA, "%s has no #CHROM line", path); }
[[noreturn]] inline void fail_no_records() { fail(LCTY_ERR_INVALID_DATA, "Input VCF file does not contain any records"); }          // panvcf.rs:85-86

// CHROM, POS (digits only, 1 <= POS <= 2^32 - 1; pos is 0-based), len(REF) of the record line [b, le)
struct LineHead { std::string chrom; uint32_t pos, ref_len; };
inline LineHead parse_line_head(const uint8_t* t, uint64_t b, uint64_t le, const char* path) {
    uint64_t c[4]; uint32_t nc = 0;
    for (uint64_t i = b; i < le && nc < 4; i++) if (t[i] == '\t') c[nc++] = i;
    if (nc < 4) fail(LCTY_ERR_INVALID_DATA, "%s: a record has fewer than five columns", path);
    LineHead h{std::string(reinterpret_cast<const char*>(&t[b]), c[0] - b), 0, 0};
    uint64_t pos = 0;
    if (c[1] == c[0] + 1) fail(LCTY_ERR_INVALID_DATA, "%s: a record of %s has no position", path, h.chrom.c_str());
    for (uint64_t i = c[0] + 1; i < c[1]; i++) {
        if (t[i] < '0' || t[i] > '9' || pos > 0xFFFFFFFFull) fail(LCTY_ERR_INVALID_DATA, "%s: bad position in a record of %s", path, h.chrom.c_str());
        pos = pos * 10 + (t[i] - '0');
    }
    if (pos < 1 || pos > 0xFFFFFFFFull) fail(LCTY_ERR_INVALID_DATA, "%s: bad position in a record of %s", path, h.chrom.c_str());
    h.pos = static_cast<uint32_t>(pos - 1); h.ref_len = static_cast<uint32_t>(c[3] - c[2] - 1);
    return h;
}

// the ploidies of the record line [b, le), the first of the file: the allele count of every sample's GT
inline void first_record_ploidy(const uint8_t* t, uint64_t b, uint64_t le, const std::string& where, uint32_t S, std::vector<uint32_t>& ploidy) {
    const std::vector<Field> f = split_tabs(t, b, le);
    if (f.size() != 9 + size_t(S)) fail(LCTY_ERR_INVALID_DATA, "Variant %s has %zu columns (expected %u)", where.c_str(), f.size(), 9 + S);
    const size_t which = gt_index(f[8], where);
    std::vector<int32_t> al; bool ph;
    for (uint32_t i = 0; i < S; i++) { parse_gt(f[9 + i], which, al, ph, where); ploidy[i] = static_cast<uint32_t>(al.size()); }
}

// the arrays of lcty_vcf_records while they grow
struct RecordArrays {
    std::vector<uint32_t> pos, rlen, rec_allele{0}; std::vector<uint64_t> allele_off{0}; std::vector<uint8_t> pool, phased; std::vector<int16_t> gt;
};

// One record line [b, le) of a region, of `contig` at 0-based `pos` with len(REF) = ref_len: appended to A, or the reader's error.
// S samples with the first record's ploidies; sample_used (null: all) as lcty_vcf_region takes it. al: scratch.
inline void parse_record_line(const uint8_t* t, uint64_t b, uint64_t le, const char* contig, uint32_t pos, uint32_t ref_len, uint32_t S,
                              const uint32_t* ploidy, const std::vector<std::string>& samples, const uint8_t* sample_used, RecordArrays& A,
                              std::vector<int32_t>& al) {
    const std::string where = std::string(contig) + ":" + std::to_string(uint64_t(pos) + 1);       // format_var, panvcf.rs:187-193
    const std::vector<Field> f = split_tabs(t, b, le);
    if (f.size() != (S ? 9 + size_t(S) : f.size()) || f.size() < 8) fail(LCTY_ERR_INVALID_DATA, "Variant %s has %zu columns (expected %u)", where.c_str(), f.size(), 9 + S);
    A.pos.push_back(pos); A.rlen.push_back(ref_len);
    A.pool.insert(A.pool.end(), f[3].p, f[3].p + f[3].n); A.allele_off.push_back(A.pool.size());
    if (!(f[4].n == 1 && f[4].p[0] == '.')) {
        size_t s = 0;
        for (size_t i = 0; i <= f[4].n; i++)
            if (i == f[4].n || f[4].p[i] == ',') { A.pool.insert(A.pool.end(), f[4].p + s, f[4].p + i); A.allele_off.push_back(A.pool.size()); s = i + 1; }
    }
    A.rec_allele.push_back(static_cast<uint32_t>(A.allele_off.size() - 1));
    if (!S) return;
    const size_t which = gt_index(f[8], where);
    for (uint32_t i = 0; i < S; i++) {
        bool ph = true;
        parse_gt(f[9 + i], which, al, ph, where);
        const uint32_t pl = ploidy[i];
        const bool used = !sample_used || sample_used[i];
        if (used && al.size() != pl)                                                                 // panvcf.rs:161-164
            fail(LCTY_ERR_INVALID_DATA, "Variant %s in sample %s has ploidy %zu (expected %u)", where.c_str(), samples[i].c_str(), al.size(), pl);
        if (used && pl > 1 && !ph)                                                                   // panvcf.rs:167-171
            fail(LCTY_ERR_INVALID_DATA, "Variant %s is unphased in sample %s", where.c_str(), samples[i].c_str());
        for (uint32_t h = 0; h < pl; h++) A.gt.push_back(h < al.size() ? static_cast<int16_t>(al[h]) : int16_t(-1));
        A.phased.push_back(ph ? 1 : 0);
    }
}

}  // namespace vcfidx
}  // namespace lcty
