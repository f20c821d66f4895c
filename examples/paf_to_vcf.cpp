// examples/paf_to_vcf.cpp — `locityper paf-vcf` (src/command/paf_vcf.rs: run 659-693, replace_input 53-61, load_region 157-200) through the
// C ABI, files in, files out:
//
//   paf_to_vcf -i DIR -r REF_HAP [args]
//   paf_to_vcf -p PAF -f FASTA -r REF_HAP [-d FILE|auto|none] -o MERGED [SEPARATE] [-R auto|none|chrom:start-end|BED] [--deflate host|device]
//
//   -i DIR        DB/loci/<locus>/: unless given otherwise, -p = the first of haplotypes.paf.br, .gz, plain that exists, -f =
//                 DIR/haplotypes.fa.gz, -o = DIR/haplotypes.vcf.gz
//   -d            discarded_haplotypes.txt; auto (default) = the one beside the FASTA when it exists
//   -R            the region the positions are shifted to; auto (default) = ref.bed beside the FASTA when it exists, none = the
//                 reference haplotype's own coordinates. `chrom:start` alone, which panics in the reference, is an input error here.
//   outputs that end in .gz are BGZF (lcty_io_write_bgzf; with --deflate device lcty_io_write_bgzf_device: the same inflated bytes,
//                 deflated on the device), others plain; both are written under a temporary name and renamed
//
//   (lcty_fasta_read, lcty_paf_read, lcty_io_read_file, lcty_paf_to_vcf)
// Prints one JSON line with the counts and the per-stage milliseconds. Build: see tests/test_gpu_pafvcf_example.py.
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "locityper_hip.h"

static void ok(int32_t rc, const char* what) {
    if (rc != LCTY_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, lcty_last_error()); std::exit(1); }
}
[[noreturn]] static void die(const std::string& msg) { std::fprintf(stderr, "%s\n", msg.c_str()); std::exit(1); }
static bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }
static bool ends_with(const std::string& s, const char* e) { const size_t n = std::strlen(e); return s.size() >= n && s.compare(s.size() - n, n, e) == 0; }
static std::string parent(const std::string& p) { const size_t k = p.rfind('/'); return k == std::string::npos ? "." : k == 0 ? "/" : p.substr(0, k); }

// digits with the thousands separators PrettyU32 takes
static bool parse_u32(std::string s, uint32_t* out) {
    std::string d;
    for (char c : s) if (c != ',' && c != '_') d.push_back(c);
    if (d.empty() || d.size() > 10 || d.find_first_not_of("0123456789") != std::string::npos) return false;
    const unsigned long long v = std::strtoull(d.c_str(), nullptr, 10);
    if (v > 0xFFFFFFFFull) return false;
    *out = static_cast<uint32_t>(v);
    return true;
}

struct Region { bool given = false; std::string chrom; uint32_t start = 0, end = 0; };

// load_region (157-200)
static Region load_region(const std::string& s, const std::string& fasta) {
    Region r;
    if (s == "none") return r;
    std::string bed;
    if (s == "auto") bed = parent(fasta) + "/ref.bed";
    else {
        const size_t colon = s.rfind(':');
        if (colon != std::string::npos && colon > 0 && !exists(s)) {
            const std::string pos = s.substr(colon + 1);
            const size_t dash = pos.find('-');
            if (dash == std::string::npos) die("Cannot parse interval '" + s + "': chrom:start-end is needed (chrom:start has no end)");
            uint32_t a = 0, b = 0;
            if (!parse_u32(pos.substr(0, dash), &a) || !parse_u32(pos.substr(dash + 1), &b) || a == 0) die("Cannot parse interval '" + s + "'");
            r.given = true; r.chrom = s.substr(0, colon); r.start = a - 1; r.end = b;
            return r;
        }
        bed = s;
    }
    if (!exists(bed)) { std::fprintf(stderr, "Cannot find BED file %s, using relative locus coordinates\n", bed.c_str()); return r; }
    std::ifstream in(bed);
    std::string line;
    if (!std::getline(in, line)) die("BED file " + bed + " is empty");
    while (!line.empty() && std::strchr(" \t\r\n", line.back())) line.pop_back();
    std::vector<std::string> cols;
    for (size_t p = 0; p <= line.size();) { const size_t q = std::min(line.find('\t', p), line.size()); cols.push_back(line.substr(p, q - p)); p = q + 1; }
    if (cols.size() < 3) die("Not enough columns in BED file " + bed + " (" + line + ")");
    if (cols[1].find_first_not_of("0123456789") != std::string::npos || cols[2].find_first_not_of("0123456789") != std::string::npos ||
        !parse_u32(cols[1], &r.start) || !parse_u32(cols[2], &r.end))
        die("Cannot parse line `" + line + "` in BED file " + bed);
    r.given = true; r.chrom = cols[0];
    return r;
}

static lcty_ctx* deflate_on = nullptr;                                  // --deflate device: the context whose device deflates the .gz outputs

static void write_out(const std::string& path, const char* data, uint64_t len) {
    const std::string tmp = parent(path) + "/." + path.substr(path.rfind('/') == std::string::npos ? 0 : path.rfind('/') + 1) + "." + std::to_string(getpid()) + ".tmp";
    if (ends_with(path, ".gz") && deflate_on) ok(lcty_io_write_bgzf_device(deflate_on, tmp.c_str(), reinterpret_cast<const uint8_t*>(data), len, nullptr), tmp.c_str());
    else if (ends_with(path, ".gz")) ok(lcty_io_write_bgzf(tmp.c_str(), reinterpret_cast<const uint8_t*>(data), len), tmp.c_str());
    else {
        std::ofstream out(tmp, std::ios::binary);
        out.write(data, static_cast<std::streamsize>(len));
        out.close();
        if (!out) die("cannot write " + tmp);
    }
    if (std::rename(tmp.c_str(), path.c_str()) != 0) die("cannot rename " + tmp + " to " + path);
}

int main(int argc, char** argv) {
    std::string input, paf, fasta, disc = "auto", merged, separate, ref_hap, region = "auto", deflate = "host";
    bool bad = argc < 2;
    for (int i = 1; i < argc && !bad; i++) {
        const std::string a = argv[i];
        auto value = [&](std::string* to) { if (i + 1 < argc) *to = argv[++i]; else bad = true; };
        if (a == "-i" || a == "--input") value(&input);
        else if (a == "-p" || a == "--paf") value(&paf);
        else if (a == "-f" || a == "--fasta") value(&fasta);
        else if (a == "-d" || a == "--discarded") value(&disc);
        else if (a == "-r" || a == "--ref-hap") value(&ref_hap);
        else if (a == "-R" || a == "--region") value(&region);
        else if (a == "--deflate") value(&deflate);
        else if (a == "-o" || a == "--output") {
            value(&merged);
            if (i + 1 < argc && argv[i + 1][0] != '-') separate = argv[++i];
        } else bad = true;
    }
    if (!input.empty()) {                                               // replace_input
        for (const char* ext : {".br", ".gz", ""}) if (paf.empty() && exists(input + "/haplotypes.paf" + ext)) paf = input + "/haplotypes.paf" + ext;
        if (fasta.empty()) fasta = input + "/haplotypes.fa.gz";
        if (merged.empty()) merged = input + "/haplotypes.vcf.gz";
    }
    if (bad || paf.empty() || fasta.empty() || merged.empty() || ref_hap.empty() || (deflate != "host" && deflate != "device")) {
        std::fprintf(stderr, "usage: paf_to_vcf -i DIR -r REF_HAP [args]\n"
                             "       paf_to_vcf -p PAF -f FASTA -r REF_HAP [-d FILE|auto|none] -o MERGED [SEPARATE] [-R auto|none|chrom:start-end|BED] [--deflate host|device]\n");
        return 2;
    }
    // the haplotypes and their alignments
    uint32_t n = 0; uint64_t nl = 0, sl = 0;
    ok(lcty_fasta_read(fasta.c_str(), &n, nullptr, &nl, nullptr, &sl, nullptr), fasta.c_str());
    std::vector<char> names(nl + 1); std::vector<uint8_t> seqs(sl + 1); std::vector<uint64_t> off(n + 1);
    ok(lcty_fasta_read(fasta.c_str(), &n, names.data(), &nl, seqs.data(), &sl, off.data()), fasta.c_str());
    std::vector<const char*> name_ptr;
    for (const char* p = names.data(); name_ptr.size() < n; p += std::strlen(p) + 1) name_ptr.push_back(p);
    uint64_t n_entries = 0, n_cigar = 0;
    ok(lcty_paf_read(paf.c_str(), name_ptr.data(), n, &n_entries, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_cigar, nullptr), paf.c_str());
    std::vector<uint32_t> id1(n_entries + 1), id2(n_entries + 1), nm(n_entries + 1), al(n_entries + 1), cigar(n_cigar + 1);
    std::vector<uint64_t> cigar_off(n_entries + 1);
    ok(lcty_paf_read(paf.c_str(), name_ptr.data(), n, &n_entries, id1.data(), id2.data(), nm.data(), al.data(), cigar_off.data(), cigar.data(), &n_cigar, nullptr),
       paf.c_str());
    // the discarded haplotypes (run 667-682): a file named explicitly may be absent as well
    uint8_t* disc_text = nullptr; uint64_t disc_len = 0;
    if (disc != "none") {
        const std::string path = disc == "auto" ? parent(fasta) + "/discarded_haplotypes.txt" : disc;
        if (exists(path)) ok(lcty_io_read_file(path.c_str(), &disc_text, &disc_len), path.c_str());
    }
    const Region reg = load_region(region, fasta);

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_pafvcf_out out;
    ok(lcty_paf_to_vcf(ctx, n, names.data(), seqs.data(), off.data(), reinterpret_cast<const char*>(disc_text), disc_len, ref_hap.c_str(), n_entries, id1.data(),
                       id2.data(), cigar_off.data(), cigar.data(), reg.given ? reg.chrom.c_str() : nullptr, reg.start, reg.end, separate.empty() ? 0 : 1, &out),
       "paf-vcf");
    lcty_io_free(disc_text);
    if (deflate == "device") deflate_on = ctx;
    const lcty_pafvcf_stats& st = out.stats;
    if (st.warn_bits & LCTY_PAFVCF_WARN_PRUNED) std::fprintf(stderr, "Haplotypes were previously pruned (~ for some lines), VCF will be inaccurate\n");
    if (st.warn_bits & LCTY_PAFVCF_WARN_REF_SUFFIX) std::fprintf(stderr, "Reference name %s has haplotype suffix; will keep it in the VCF file\n", ref_hap.c_str());
    if (st.n_missing) std::fprintf(stderr, "    %u / %u haplotype-reference alignments are missing\n", st.n_missing, n);
    write_out(merged, out.merged, out.merged_len);
    if (!separate.empty()) write_out(separate, out.separate, out.separate_len);
    lcty_ctx_destroy(ctx);
    std::printf("{\"haplotypes\": %u, \"samples\": %u, \"entries\": %llu, \"missing\": %u, \"bad_len\": %u, \"variants\": %llu, \"shifted\": %llu, \"unique\": %llu, "
                "\"merged\": %llu, \"lines_merged\": %llu, \"lines_separate\": %llu, \"merged_bytes\": %llu, \"separate_bytes\": %llu, \"warn_bits\": %u, "
                "\"ms\": {\"upload\": %.3f, \"variants\": %.3f, \"ranges\": %.3f, \"table\": %.3f, \"text\": %.3f, \"total\": %.3f}}\n",
                n, st.n_samples, static_cast<unsigned long long>(n_entries), st.n_missing, st.n_bad_len, static_cast<unsigned long long>(st.n_variants),
                static_cast<unsigned long long>(st.n_shifted), static_cast<unsigned long long>(st.n_unique), static_cast<unsigned long long>(st.n_merged),
                static_cast<unsigned long long>(st.n_lines_merged), static_cast<unsigned long long>(st.n_lines_separate),
                static_cast<unsigned long long>(st.merged_bytes), static_cast<unsigned long long>(st.separate_bytes), st.warn_bits, st.upload_ms, st.variants_ms,
                st.ranges_ms, st.table_ms, st.text_ms, st.total_ms);
    lcty_pafvcf_out_free(&out);
    return 0;
}
