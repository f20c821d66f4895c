// lcty_gtvcf_host.hpp — the host half of a cohort's genotypes as a VCF (extra/into_vcf.py, extra/into_csv.py): the column of a predicted
// allele (copy_genotype, into_vcf.py:99-114), fixed-point numbers as text and back, the FORMAT key and the header (create_vcf_header,
// 76-96). No HIP include: scripts/gtvcf_probe_host.cpp compiles it with g++ alone. The two functions that print a fixed-point number are
// the ones the kernels of lcty_gtvcf.hip call (LCTY_HD).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "lcty_host.hpp"

#ifdef __HIPCC__
#define LCTY_HD __host__ __device__
#else
#define LCTY_HD
#endif

namespace lcty {
namespace gtvcf {

constexpr uint32_t N_FEATURES = 5;                                       // qual, reads, unexpl, wdist, warn: the bits of field_mask in this order
constexpr uint32_t QUAL_DECIMALS = 1, WDIST_DECIMALS = 5, MAX_DECIMALS = 18;

LCTY_HD inline uint64_t pow10_u64(uint32_t d) { uint64_t p = 1; while (d--) p *= 10; return p; }
LCTY_HD inline uint32_t dec_digits(uint64_t x) { uint32_t d = 1; while (x >= 10) { x /= 10; d++; } return d; }

// A fixed-point value of `decimals` decimals as text, integer arithmetic only: the sign, the integer part, then the fraction without its
// trailing zeros and no point when nothing follows (273 tenths: 27.3, 270: 27, 123 units of 1e-5: 0.00123). pad: all `decimals` digits,
// as Python's `:.1f` / `:.5f` (into_csv.py:96). Absent: "." (pad: "nan"). fixed_width: the bytes fixed_put writes.
struct FixedParts { uint64_t ip, fp; uint32_t ip_digits, fp_digits; bool neg; };
LCTY_HD inline FixedParts fixed_parts(int64_t v, uint32_t decimals, bool pad) {
    FixedParts f;
    f.neg = v < 0;
    const uint64_t a = f.neg ? uint64_t(0) - uint64_t(v) : uint64_t(v), scale = pow10_u64(decimals);
    f.ip = a / scale; f.fp = a % scale; f.fp_digits = decimals;
    if (!pad) while (f.fp_digits && f.fp % 10 == 0) { f.fp /= 10; f.fp_digits--; }
    f.ip_digits = dec_digits(f.ip);
    return f;
}
LCTY_HD inline uint32_t fixed_width(int64_t v, uint32_t decimals, bool pad) {
    if (v == LCTY_GTVCF_ABSENT) return pad ? 3 : 1;
    const FixedParts f = fixed_parts(v, decimals, pad);
    return (f.neg ? 1u : 0u) + f.ip_digits + (f.fp_digits ? 1 + f.fp_digits : 0);
}
LCTY_HD inline void fixed_put(char* at, int64_t v, uint32_t decimals, bool pad) {
    if (v == LCTY_GTVCF_ABSENT) { if (pad) { at[0] = 'n'; at[1] = 'a'; at[2] = 'n'; } else at[0] = '.'; return; }
    const FixedParts f = fixed_parts(v, decimals, pad);
    if (f.neg) *at++ = '-';
    uint64_t x = f.ip;
    for (uint32_t i = f.ip_digits; i-- > 0;) { at[i] = char('0' + x % 10); x /= 10; }
    at += f.ip_digits;
    if (!f.fp_digits) return;
    *at++ = '.';
    x = f.fp;
    for (uint32_t i = f.fp_digits; i-- > 0;) { at[i] = char('0' + x % 10); x /= 10; }
}

inline std::string fixed_text(int64_t v, uint32_t decimals, bool pad) {
    std::string s(fixed_width(v, decimals, pad), ' ');
    fixed_put(&s[0], v, decimals, pad);
    return s;
}

// Decimal text into the fixed-point integer, digit by digit and never through a double: [+-] digits [. digits]. Digits behind the
// `decimals`-th are dropped towards minus infinity (floor, as into_csv.py:91 floors the quality). "nan" in any case and "NA"
// (parse_float, into_vcf.py:14-15) are absent. Anything else — an exponent, "inf", no digit at all — is LCTY_ERR_INVALID_DATA, as is a
// value of more than 18 digits.
inline int64_t fixed_parse(const std::string& text, uint32_t decimals) {
    auto lower = [](char c) { return c >= 'A' && c <= 'Z' ? char(c + 32) : c; };
    if (text == "NA" || (text.size() == 3 && lower(text[0]) == 'n' && lower(text[1]) == 'a' && lower(text[2]) == 'n')) return LCTY_GTVCF_ABSENT;
    size_t i = 0;
    bool neg = false;
    if (i < text.size() && (text[i] == '+' || text[i] == '-')) neg = text[i++] == '-';
    uint64_t v = 0;
    uint32_t n_int = 0, n_frac = 0, n_sig = 0;
    bool dropped = false;
    auto push = [&](char c) {                                            // |v| stays below 10^18
        if (v || c != '0') n_sig++;
        if (n_sig > MAX_DECIMALS) fail(LCTY_ERR_INVALID_DATA, "number `%s` with %u decimals has more than %u digits", text.c_str(), decimals, MAX_DECIMALS);
        v = v * 10 + uint64_t(c - '0');
    };
    for (; i < text.size() && text[i] >= '0' && text[i] <= '9'; i++, n_int++) push(text[i]);
    if (i < text.size() && text[i] == '.') {
        for (i++; i < text.size() && text[i] >= '0' && text[i] <= '9'; i++, n_frac++) {
            if (n_frac < decimals) push(text[i]); else dropped |= text[i] != '0';
        }
    }
    if (i != text.size() || n_int + n_frac == 0) fail(LCTY_ERR_INVALID_DATA, "cannot parse `%s` as a decimal number", text.c_str());
    for (uint32_t d = n_frac; d < decimals; d++) push('0');
    if (neg && dropped) v++;                                             // floor of a negative value
    return neg ? -int64_t(v) : int64_t(v);
}

// ---- the table between into_csv.py and into_vcf.py ------------------------------------------------------------------------------------

// The text of the table: the column line of into_csv.py:125 and the rows of process_sample (72-96). A `?` or `*` row ends behind its
// genotype column. Quality and weight_dist are padded as `:.1f` / `:.5f`; an absent number is `nan`, what Python prints there.
inline std::string predictions_csv_text(uint64_t n_rows, const char* const* sample, const char* const* locus, const lcty_res_summary* rows) {
    std::string s = "sample\tlocus\tgenotype\tquality\ttotal_reads\tunexpl_reads\tweight_dist\twarnings\n";
    auto cell = [&](const char* text, const char* what, uint64_t i, bool may_be_empty) {
        if (!text) fail(LCTY_ERR_INVALID_INPUT, "row %llu: no %s", static_cast<unsigned long long>(i), what);
        const std::string t(text);
        if ((t.empty() && !may_be_empty) || t.find_first_of("\t\n\r") != std::string::npos)
            fail(LCTY_ERR_INVALID_INPUT, "row %llu: `%s` is not a %s of a tab-separated table", static_cast<unsigned long long>(i), text, what);
        s += t;
    };
    for (uint64_t i = 0; i < n_rows; i++) {
        const lcty_res_summary& r = rows[i];
        cell(sample[i], "sample", i, false); s += '\t';
        cell(locus[i], "locus", i, false); s += '\t';
        if (r.state == LCTY_RES_MISSING) { s += "?\n"; continue; }
        if (r.state == LCTY_RES_NO_GENOTYPE) { s += "*\n"; continue; }
        if (r.state != LCTY_RES_CALLED) fail(LCTY_ERR_INVALID_INPUT, "row %llu: state %d", static_cast<unsigned long long>(i), r.state);
        cell(r.genotype, "genotype", i, false); s += '\t';
        s += fixed_text(r.qual10, QUAL_DECIMALS, true); s += '\t';
        s += fixed_text(r.reads, 0, true); s += '\t';
        s += fixed_text(r.unexpl, 0, true); s += '\t';
        s += fixed_text(r.wdist5, WDIST_DECIMALS, true); s += '\t';
        cell(r.warnings, "warning text", i, true); s += '\n';
    }
    return s;
}

// load_predictions (into_vcf.py:18-44) over common.read_csv: `#` lines before the column line are skipped, columns are found by name,
// a row may end early (absent cells), empty lines are skipped as csv.DictReader skips them. No quoting: the table has none.
struct PredictionRow { std::string sample, locus, genotype, warnings; int64_t qual10, reads, unexpl, wdist5; };
struct PredictionTable { std::vector<PredictionRow> rows; std::vector<std::string> samples; };
inline PredictionTable predictions_csv_parse(const std::string& text, const char* what) {
    PredictionTable T;
    enum { SAMPLE, LOCUS, GENOTYPE, QUALITY, READS, UNEXPL, WDIST, WARNINGS, N_COLS };
    static const char* const col_name[N_COLS] = {"sample", "locus", "genotype", "quality", "total_reads", "unexpl_reads", "weight_dist", "warnings"};
    int col_at[N_COLS];
    for (int& c : col_at) c = -1;
    bool have_cols = false;
    uint64_t line_no = 0;
    std::vector<std::string> cells;
    for (size_t at = 0; at < text.size();) {
        size_t e = text.find('\n', at);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(at, e - at);
        at = e + 1; line_no++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!have_cols && !line.empty() && line[0] == '#') continue;
        if (line.empty()) { if (!have_cols) fail(LCTY_ERR_INVALID_DATA, "%s: an empty column line", what); continue; }
        cells.clear();
        for (size_t c0 = 0;;) {
            const size_t c1 = line.find('\t', c0);
            cells.push_back(line.substr(c0, c1 == std::string::npos ? std::string::npos : c1 - c0));
            if (c1 == std::string::npos) break;
            c0 = c1 + 1;
        }
        if (!have_cols) {
            for (size_t c = 0; c < cells.size(); c++)
                for (int k = 0; k < N_COLS; k++) if (cells[c] == col_name[k]) col_at[k] = int(c);
            for (int k : {SAMPLE, LOCUS, GENOTYPE}) if (col_at[k] < 0) fail(LCTY_ERR_INVALID_DATA, "%s: the table has no column `%s`", what, col_name[k]);
            have_cols = true;
            continue;
        }
        auto cell = [&](int k) -> const std::string* { return col_at[k] >= 0 && size_t(col_at[k]) < cells.size() ? &cells[size_t(col_at[k])] : nullptr; };
        PredictionRow r;
        for (int k : {SAMPLE, LOCUS, GENOTYPE}) if (!cell(k) || cell(k)->empty())
            fail(LCTY_ERR_INVALID_DATA, "%s: line %llu has no %s", what, static_cast<unsigned long long>(line_no), col_name[k]);
        r.sample = *cell(SAMPLE); r.locus = *cell(LOCUS); r.genotype = *cell(GENOTYPE);
        auto number = [&](int k, uint32_t decimals) { return cell(k) ? fixed_parse(*cell(k), decimals) : int64_t(LCTY_GTVCF_ABSENT); };
        r.qual10 = number(QUALITY, QUAL_DECIMALS); r.reads = number(READS, 0); r.unexpl = number(UNEXPL, 0); r.wdist5 = number(WDIST, WDIST_DECIMALS);
        if (cell(WARNINGS)) r.warnings = *cell(WARNINGS);
        T.rows.push_back(std::move(r));
    }
    if (!have_cols) fail(LCTY_ERR_INVALID_DATA, "%s: no column line", what);
    for (const PredictionRow& r : T.rows) T.samples.push_back(r.sample);
    std::sort(T.samples.begin(), T.samples.end());                       // bytewise (44)
    T.samples.erase(std::unique(T.samples.begin(), T.samples.end()), T.samples.end());
    return T;
}

// FORMAT of the record lines: GT, then the features field_mask selects (into_vcf.py:138-141)
inline std::string format_key(uint32_t field_mask) {
    static const char* const key[N_FEATURES] = {"qual", "reads", "unexpl", "wdist", "warn"};
    std::string s = "GT";
    for (uint32_t f = 0; f < N_FEATURES; f++) if (field_mask >> f & 1) { s += ':'; s += key[f]; }
    return s;
}

// create_vcf_header (into_vcf.py:76-96) as pysam writes it: the file format and the PASS filter htslib gives every new header, the
// contigs (length 0 = unknown: no `length=`), the seven FORMAT lines, the column line.
inline std::string header_text(const std::vector<std::string>& contigs, const uint64_t* contig_len, const std::vector<std::string>& samples) {
    std::string s = "##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n";
    for (size_t c = 0; c < contigs.size(); c++) {
        s += "##contig=<ID=" + contigs[c];
        if (contig_len && contig_len[c]) s += ",length=" + std::to_string(contig_len[c]);
        s += ">\n";
    }
    s += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
         "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Converted genotype quality\">\n"
         "##FORMAT=<ID=qual,Number=1,Type=Float,Description=\"Raw genotype quality\">\n"
         "##FORMAT=<ID=reads,Number=1,Type=Integer,Description=\"Total number of reads used to predict locus genotype\">\n"
         "##FORMAT=<ID=unexpl,Number=1,Type=Integer,Description=\"Number of unexplained reads within the locus\">\n"
         "##FORMAT=<ID=wdist,Number=1,Type=Float,Description=\"Weighted distance between primary and non-primary genotype predictions\">\n"
         "##FORMAT=<ID=warn,Number=1,Type=String,Description=\"Genotype warnings\">\n"
         "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    for (const std::string& name : samples) { s += '\t'; s += name; }
    s += '\n';
    return s;
}

// copy_genotype's rule (into_vcf.py:99-114) for one predicted allele: its column of the GT matrix of `view`, or LCTY_GTVCF_REF.
// `index`: the samples of the view by name (sample_index), built once for all alleles.
struct SampleIndex { std::vector<std::pair<std::string, uint32_t>> by_name; };
inline SampleIndex sample_index(const lcty_vcf_view& view) {
    if (view.n_samples && (!view.samples || !view.ploidy || !view.hap_off)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    SampleIndex ix;
    const std::vector<std::string> names = split_names(view.samples ? view.samples : "", view.n_samples);
    for (uint32_t i = 0; i < view.n_samples; i++) ix.by_name.emplace_back(names[i], i);
    std::sort(ix.by_name.begin(), ix.by_name.end());
    return ix;
}
inline uint32_t resolve_column(const lcty_vcf_view& view, const SampleIndex& ix, const std::string& genome_name, const std::string& allele) {
    const size_t n = allele.size();
    const bool suffixed = n > 2 && (allele[n - 2] == '.' || allele[n - 2] == '_');     // 102
    if (!suffixed && allele == genome_name) return LCTY_GTVCF_REF;                     // 107-108
    const std::string sample = suffixed ? allele.substr(0, n - 2) : allele;
    const auto it = std::lower_bound(ix.by_name.begin(), ix.by_name.end(), std::make_pair(sample, uint32_t(0)));
    if (it == ix.by_name.end() || it->first != sample)                                 // var.samples[sample]: KeyError
        fail(LCTY_ERR_INVALID_DATA, "allele `%s`: the variants file has no sample `%s`", allele.c_str(), sample.c_str());
    const uint32_t s = it->second, ploidy = view.ploidy[s];
    if (!suffixed) {                                                                   // 110-113
        if (ploidy != 1) fail(LCTY_ERR_INVALID_DATA, "allele `%s` has no haplotype suffix, and sample `%s` has ploidy %u", allele.c_str(), sample.c_str(), ploidy);
        return view.hap_off[s];
    }
    const char d = allele[n - 1];                                                      // 104: int(allele[-1])
    if (d < '0' || d > '9') fail(LCTY_ERR_INVALID_DATA, "allele `%s`: the haplotype `%c` is not a digit", allele.c_str(), d);
    const uint32_t hap = uint32_t(d - '0');
    if (hap == 0 || hap > ploidy)                                                      // 106; 0 would index from the end in Python: refused here
        fail(LCTY_ERR_INVALID_DATA, "allele `%s`: haplotype %u of sample `%s`, whose ploidy is %u", allele.c_str(), hap, sample.c_str(), ploidy);
    return view.hap_off[s] + hap - 1;
}

// ---- the tabix index of a BGZF VCF (the tabix format; bins and linear index as SAM specification 5.3, what pysam.tabix_index(preset='vcf')
// leaves, into_vcf.py:143, 196) -------------------------------------------------------------------------------------------------------

inline uint32_t reg2bin(uint32_t beg, uint32_t end) {                     // [beg, end), end > beg
    --end;
    if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
    return 0;
}

constexpr uint64_t BGZF_CUT = 0xff00;                                    // input bytes of a block of lcty_bgzf_deflate

// The inflated bytes of the .tbi. line_off[n_records + 1]: the offset of every record line in the inflated text and of what follows the
// last; block_off[n_blocks + 1]: the file offset of every block of BGZF_CUT text bytes and the end of the last (lcty_bgzf_deflate).
inline std::string tbi_plain(const std::vector<std::string>& contigs, uint64_t n_records, const uint32_t* contig_ix, const uint32_t* pos, const uint32_t* ref_len,
                             const uint64_t* line_off, const uint64_t* block_off, uint64_t n_blocks) {
    struct Ref {
        std::vector<std::pair<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>>> bins;     // in order of first use; sorted when written
        std::vector<uint64_t> linear; uint64_t first = 0, last = 0, count = 0;
    };
    auto voff = [&](uint64_t u) {
        if (u / BGZF_CUT > n_blocks) fail(LCTY_ERR_INVALID_INPUT, "offset %llu lies behind the %llu blocks of the file", static_cast<unsigned long long>(u),
                                          static_cast<unsigned long long>(n_blocks));
        return block_off[u / BGZF_CUT] << 16 | u % BGZF_CUT;
    };
    std::vector<Ref> refs(contigs.size());
    std::vector<std::vector<uint32_t>> bin_slot(contigs.size());          // per reference: bin -> index in bins + 1 (37 450 bins)
    constexpr uint64_t UNSET = ~uint64_t(0);
    for (uint64_t i = 0; i < n_records; i++) {
        const uint32_t t = contig_ix[i];
        if (t >= contigs.size()) fail(LCTY_ERR_INVALID_INPUT, "record %llu: contig %u of %zu", static_cast<unsigned long long>(i), t, contigs.size());
        if (i && (contig_ix[i - 1] > t || (contig_ix[i - 1] == t && pos[i - 1] > pos[i])))
            fail(LCTY_ERR_INVALID_INPUT, "record %llu comes before its predecessor: a tabix index needs sorted records", static_cast<unsigned long long>(i));
        if (line_off[i + 1] <= line_off[i]) fail(LCTY_ERR_INVALID_INPUT, "line_off does not grow at record %llu", static_cast<unsigned long long>(i));
        const uint64_t beg = pos[i], end = beg + std::max(ref_len[i], 1u);
        if (end > (uint64_t(1) << 29)) fail(LCTY_ERR_UNSUPPORTED, "record %llu ends at %llu: beyond 2^29 a CSI index is needed", static_cast<unsigned long long>(i),
                                            static_cast<unsigned long long>(end));
        const uint64_t v0 = voff(line_off[i]), v1 = voff(line_off[i + 1]);
        Ref& R = refs[t];
        if (bin_slot[t].empty()) bin_slot[t].assign(37450, 0);
        const uint32_t bin = reg2bin(uint32_t(beg), uint32_t(end));
        if (!bin_slot[t][bin]) { R.bins.emplace_back(bin, std::vector<std::pair<uint64_t, uint64_t>>()); bin_slot[t][bin] = uint32_t(R.bins.size()); }
        auto& cs = R.bins[bin_slot[t][bin] - 1].second;
        if (!cs.empty() && cs.back().second == v0) cs.back().second = v1;  // chunks that touch are one
        else cs.emplace_back(v0, v1);
        const uint64_t w1 = (end - 1) >> 14;
        if (R.linear.size() <= w1) R.linear.resize(w1 + 1, UNSET);
        for (uint64_t w = beg >> 14; w <= w1; w++) if (R.linear[w] == UNSET) R.linear[w] = v0;
        if (!R.count) R.first = v0;
        R.last = v1; R.count++;
    }
    std::string out("TBI\1", 4);
    auto i32 = [&](int32_t v) { out.append(reinterpret_cast<const char*>(&v), 4); };
    auto u32 = [&](uint32_t v) { out.append(reinterpret_cast<const char*>(&v), 4); };
    auto u64 = [&](uint64_t v) { out.append(reinterpret_cast<const char*>(&v), 8); };
    std::string names;
    for (const std::string& c : contigs) { names += c; names.push_back('\0'); }
    i32(int32_t(contigs.size())); i32(2); i32(1); i32(2); i32(0); i32('#'); i32(0); i32(int32_t(names.size()));
    out += names;
    for (Ref& R : refs) {
        std::sort(R.bins.begin(), R.bins.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        i32(int32_t(R.bins.size() + (R.count ? 1 : 0)));
        for (const auto& b : R.bins) {
            u32(b.first); i32(int32_t(b.second.size()));
            for (const auto& c : b.second) { u64(c.first); u64(c.second); }
        }
        if (R.count) { u32(37450); i32(2); u64(R.first); u64(R.last); u64(R.count); u64(0); }      // the pseudo-bin: the file range, mapped / unmapped
        i32(int32_t(R.linear.size()));
        uint64_t prev = 0;
        for (uint64_t v : R.linear) { if (v != UNSET) prev = v; u64(prev); }
    }
    u64(0);                                                              // n_no_coor
    return out;
}

}  // namespace gtvcf
}  // namespace lcty
