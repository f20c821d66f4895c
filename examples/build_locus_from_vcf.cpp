// examples/build_locus_from_vcf.cpp — one locus of `locityper target -v pangenome.vcf.gz` through the C ABI, files in, files out
// (add_locus with a VCF, src/command/add.rs:733-782: locus expansion, reconstruction of the phased haplotypes, process_alleles):
//
//   <window.fa[.gz]>       the reference bases of ONE window of the contig that holds the flanks of every allowed expansion,
//                          [start - E_max, min(end + E_max, contig length)); one record. --win-start gives its position (default 0),
//                          --contig-len the length of the contig (default: the window's end)
//   <pangenome.vcf[.gz]>   text VCF, phased GT, read whole                     (lcty_vcf_open, lcty_vcf_region; with --index see below)
//   <window.counts[.br|.lz4]>  what `jellyfish query` returned for the k-mers of the window, one KmerCounts block of one contig
//                          ("-" with -e 0: no expansion, no counts)                                  (lcty_kmer_counts_parse)
//   <contig> <start> <end> <locus> <db_dir>     0-based, half-open  -> <db_dir>/loci/<locus>/
//        ref.bed  haplotypes.fa.gz  kmers.bin.br  [distances.bin]  [discarded_haplotypes.txt]
//   --hap-counts <counts.bin>   the k-mer counts of the SURVIVING haplotypes and of the new reference interval (last), one block — they
//                          are known only once the sequences are: run with --only-seqs first, count, run again
//   --only-seqs            haplotypes.fa.gz and ref.bed alone
//   -e A,B,C               allowed expansions (20000,50000,200000); -w moving window (500); -g reference name (GRCh38)
//   --leave-out N1,N2      samples / haplotypes / the reference name to leave out; --ignore-overlaps; --unknown F (0.0001); --calc-div
//   --index [PATH]         the VCF is BGZF with a tabix index (PATH, default <pangenome.vcf.gz>.tbi): only the chunks of the window are
//                          read, inflated and parsed, on the device (lcty_vcf_indexed_open, lcty_vcf_indexed_fetch); --device-inflate
//                          inflates them there too (knob "sample_bam_inflate"). The JSON line gains the fetch statistics.
// The statistics of the step go to stdout as one JSON line.
//
// Build: see tests/test_gpu_panvcf_example.py.
#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "locityper_hip.h"

static void ok(int32_t rc, const char* what) {
    if (rc != LCTY_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, lcty_last_error()); std::exit(1); }
}

static void write_plain(const std::string& path, const void* data, uint64_t len) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, 1, len, f) != len || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
}

static std::vector<std::string> split_commas(const std::string& s) {
    std::vector<std::string> out;
    size_t b = 0;
    for (size_t i = 0; i <= s.size(); i++)
        if (i == s.size() || s[i] == ',') { if (i > b) out.push_back(s.substr(b, i - b)); b = i + 1; }
    return out;
}

static std::string blob_of(const std::vector<std::string>& v) {
    std::string b;
    for (const std::string& s : v) { b += s; b.push_back('\0'); }
    return b;
}

struct Counts { uint32_t k = 0, n_contigs = 0, counter_bytes = 2; std::vector<uint64_t> off; std::vector<uint16_t> counts; };
static Counts read_counts(const std::string& path) {
    Counts c; uint8_t* raw = nullptr; uint64_t raw_len = 0, used = 0;
    ok(lcty_io_read_file(path.c_str(), &raw, &raw_len), path.c_str());
    ok(lcty_kmer_counts_parse(raw, raw_len, &c.k, &c.n_contigs, nullptr, 0, nullptr, 0, &used), "KmerCounts::load (size)");
    c.counter_bytes = raw[1];
    c.off.resize(c.n_contigs + 1); c.counts.resize(used + 1);
    ok(lcty_kmer_counts_parse(raw, raw_len, &c.k, &c.n_contigs, c.off.data(), c.n_contigs, c.counts.data(), c.counts.size(), &used), "KmerCounts::load");
    lcty_io_free(raw);
    return c;
}

int main(int argc, char** argv) {
    std::vector<std::string> pos, leave_out;
    std::vector<uint32_t> expansions{20000, 50000, 200000};
    std::string ref_name = "GRCh38", hap_counts_path, index_path;
    bool indexed = false, device_inflate = false;
    uint32_t moving_window = 500, win_start = 0, contig_len = 0, k_arg = 25;
    double unknown = 0.0001;
    int32_t overlaps_allowed = 0;
    lcty_db_params prm;
    lcty_db_params_default(&prm);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "-e" || a == "--expand") { expansions.clear(); for (const std::string& v : split_commas(next())) expansions.push_back(static_cast<uint32_t>(std::strtoul(v.c_str(), nullptr, 10))); }
        else if (a == "-w" || a == "--window") moving_window = static_cast<uint32_t>(std::strtoul(next().c_str(), nullptr, 10));
        else if (a == "-g" || a == "--genome") ref_name = next();
        else if (a == "-k") k_arg = static_cast<uint32_t>(std::strtoul(next().c_str(), nullptr, 10));
        else if (a == "--leave-out") { for (const std::string& v : split_commas(next())) leave_out.push_back(v); }
        else if (a == "--ignore-overlaps") overlaps_allowed = 1;
        else if (a == "--unknown" || a == "-u") unknown = std::atof(next().c_str());
        else if (a == "--hap-counts") hap_counts_path = next();
        else if (a == "--only-seqs") prm.only_seqs = 1;
        else if (a == "--calc-div") prm.calc_div = 1;
        else if (a == "--win-start") win_start = static_cast<uint32_t>(std::strtoul(next().c_str(), nullptr, 10));
        else if (a == "--index") { indexed = true; if (i + 1 < argc && std::strlen(argv[i + 1]) > 4 && !std::strcmp(argv[i + 1] + std::strlen(argv[i + 1]) - 4, ".tbi")) index_path = argv[++i]; }
        else if (a == "--device-inflate") device_inflate = true;
        else if (a == "--contig-len") contig_len = static_cast<uint32_t>(std::strtoul(next().c_str(), nullptr, 10));
        else pos.push_back(a);
    }
    if (pos.size() != 8 || expansions.empty() || (hap_counts_path.empty() && !prm.only_seqs)) {
        std::fprintf(stderr, "usage: build_locus_from_vcf <window.fa> <pangenome.vcf> <window.counts|-> <contig> <start> <end> <locus> <db_dir> "
                             "(--hap-counts <counts.bin> | --only-seqs) [-e A,B,C] [-w W] [-g NAME] [-k K] [--leave-out N1,N2] [--ignore-overlaps] "
                             "[--unknown F] [--calc-div] [--win-start N] [--contig-len N] [--index [PATH.tbi]] [--device-inflate]\n");
        return 2;
    }
    const std::string contig = pos[3], locus = pos[6];
    const uint32_t start = static_cast<uint32_t>(std::strtoul(pos[4].c_str(), nullptr, 10)), end = static_cast<uint32_t>(std::strtoul(pos[5].c_str(), nullptr, 10));

    // the window: bases and counts
    uint32_t n_ref = 0; uint64_t nl = 0, sl = 0;
    ok(lcty_fasta_read(pos[0].c_str(), &n_ref, nullptr, &nl, nullptr, &sl, nullptr), pos[0].c_str());
    if (n_ref != 1) { std::fprintf(stderr, "%s: one sequence expected, %u found\n", pos[0].c_str(), n_ref); return 1; }
    std::vector<char> ref_names(nl + 1); std::vector<uint8_t> win(sl + 1); uint64_t win_off[2];
    ok(lcty_fasta_read(pos[0].c_str(), &n_ref, ref_names.data(), &nl, win.data(), &sl, win_off), pos[0].c_str());
    const uint64_t win_len = win_off[1];
    if (!contig_len) contig_len = static_cast<uint32_t>(win_start + win_len);
    Counts wc;
    const bool expand = !(expansions.size() == 1 && expansions[0] == 0);
    if (pos[2] != "-") {
        wc = read_counts(pos[2]);
        if (wc.n_contigs != 1) { std::fprintf(stderr, "%s: one contig expected, %u found\n", pos[2].c_str(), wc.n_contigs); return 1; }
    } else if (expand) { std::fprintf(stderr, "the counts of the window are needed to expand the locus (or -e 0)\n"); return 2; }
    Counts hc;
    if (!prm.only_seqs) hc = read_counts(hap_counts_path);
    const uint32_t k = !prm.only_seqs ? hc.k : pos[2] != "-" ? wc.k : k_arg;
    if (pos[2] != "-" && wc.k != k) { std::fprintf(stderr, "the two count tables differ in k (%u, %u)\n", wc.k, k); return 1; }

    // the VCF: samples, retained columns, the records of the window, the matrix of the retained columns
    lcty_vcf* vcf = nullptr; lcty_vcf_indexed* ivcf = nullptr; lcty_vcf_view view;
    if (indexed) {
        ok(lcty_vcf_indexed_open(pos[1].c_str(), index_path.empty() ? nullptr : index_path.c_str(), &ivcf), pos[1].c_str());
        ok(lcty_vcf_indexed_view_get(ivcf, &view), "vcf view");
    } else {
        ok(lcty_vcf_open(pos[1].c_str(), &vcf), pos[1].c_str());
        ok(lcty_vcf_view_get(vcf, &view), "vcf view");
    }
    const std::string leave_blob = blob_of(leave_out);
    uint32_t n_cols = 0, n_left = 0; uint64_t names_len = 0;
    ok(lcty_panvcf_names(view.n_samples, view.samples, view.ploidy, ref_name.c_str(), static_cast<uint32_t>(leave_out.size()), leave_blob.c_str(), 0, &n_cols, nullptr,
                         nullptr, nullptr, 0, &names_len, &n_left), "HaplotypeNames::new (size)");
    std::vector<uint32_t> col_sample(n_cols), col_hap(n_cols); std::vector<char> names(names_len + 1);
    ok(lcty_panvcf_names(view.n_samples, view.samples, view.ploidy, ref_name.c_str(), static_cast<uint32_t>(leave_out.size()), leave_blob.c_str(), n_cols, &n_cols,
                         col_sample.data(), col_hap.data(), names.data(), names.size(), &names_len, &n_left), "HaplotypeNames::new");
    std::vector<uint8_t> used(view.n_samples, 0);
    for (uint32_t c = 0; c < n_cols; c++) if (col_sample[c] != LCTY_NONE_U32) used[col_sample[c]] = 1;
    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_vcf_records recs;
    lcty_vcf_fetch_stats fs;
    std::memset(&fs, 0, sizeof(fs));
    if (indexed) {
        if (device_inflate) ok(lcty_ctx_set_knob(ctx, "sample_bam_inflate", 1), "knob");
        ok(lcty_vcf_indexed_fetch(ctx, ivcf, contig.c_str(), win_start, static_cast<uint32_t>(win_start + win_len), used.data(), &recs, &fs), "fetch");
    } else ok(lcty_vcf_region(vcf, contig.c_str(), win_start, static_cast<uint32_t>(win_start + win_len), used.data(), &recs), "fetch");
    std::vector<int16_t> gt(static_cast<size_t>(recs.n_recs) * n_cols + 1, 0);
    for (uint32_t v = 0; v < recs.n_recs; v++)
        for (uint32_t c = 0; c < n_cols; c++)
            if (col_sample[c] != LCTY_NONE_U32) gt[static_cast<size_t>(v) * n_cols + c] = recs.gt[static_cast<size_t>(v) * recs.n_haps + view.hap_off[col_sample[c]] + col_hap[c]];

    lcty_locus_vcf_in in;
    std::memset(&in, 0, sizeof(in));
    in.locus = locus.c_str(); in.contig = contig.c_str();
    in.inner_start = start; in.inner_end = end; in.contig_len = contig_len; in.win_start = win_start;
    in.win_seq = win.data(); in.win_len = win_len;
    if (pos[2] != "-") { in.win_counts = wc.counts.data(); in.n_win_counts = wc.off[1]; }
    in.k = k; in.counter_bytes = prm.only_seqs ? 2 : hc.counter_bytes;
    in.n_recs = recs.n_recs; in.n_cols = n_cols;
    in.pos = recs.pos; in.ref_len = recs.ref_len; in.rec_allele = recs.rec_allele; in.allele_off = recs.allele_off; in.allele_bytes = recs.allele_bytes;
    in.gt = gt.data(); in.names = names.data();
    in.expansions = expansions.data(); in.n_expansions = static_cast<uint32_t>(expansions.size()); in.moving_window = moving_window;
    in.unknown_frac = unknown; in.overlaps_allowed = overlaps_allowed;
    if (!prm.only_seqs) { in.hap_counts = hc.counts.data(); in.hap_cnt_off = hc.off.data(); }

    lcty_locus_vcf_out out;
    ok(lcty_db_locus_from_vcf(ctx, &in, &prm, &out), "add_locus");
    lcty_ctx_destroy(ctx);
    if (!prm.only_seqs && hc.n_contigs != out.stats.n_haplotypes + 1) {
        std::fprintf(stderr, "%s: %u contigs, %u surviving haplotypes + the reference expected\n", hap_counts_path.c_str(), hc.n_contigs, out.stats.n_haplotypes);
        return 1;
    }

    const std::string loci = pos[7] + "/loci", dir = loci + "/" + locus;
    mkdir(pos[7].c_str(), 0755); mkdir(loci.c_str(), 0755); mkdir(dir.c_str(), 0755);
    write_plain(dir + "/ref.bed", out.ref_bed, out.ref_bed_len);
    ok(lcty_io_write_gz((dir + "/haplotypes.fa.gz").c_str(), out.files.fasta, out.files.fasta_len), "haplotypes.fa.gz");
    if (out.files.kmers_len) ok(lcty_io_write_br((dir + "/kmers.bin.br").c_str(), out.files.kmers, out.files.kmers_len, 5, nullptr), "kmers.bin.br");
    if (out.files.distances_len) write_plain(dir + "/distances.bin", out.files.distances, out.files.distances_len);
    if (out.files.discarded_len) write_plain(dir + "/discarded_haplotypes.txt", out.files.discarded, out.files.discarded_len);
    const lcty_locus_vcf_stats& s = out.stats;
    std::printf("{\"locus\":\"%s\",\"contig\":\"%s\",\"start\":%u,\"end\":%u,\"attempt\":%d,\"allowed_expansion\":%u,\"crop_bits\":%u,\"warn_bits\":%u,"
                "\"columns\":%u,\"left_out\":%u,\"records\":%u,\"kept_records\":%llu,\"overlaps\":%llu,\"haplotypes\":%u,\"unknown\":%u,\"with_n\":%u,"
                "\"identical\":%u,\"written\":%u,\"shortest\":%llu,\"filter_ms\":%.3f,\"expand_ms\":%.3f,\"reconstruct_ms\":%.3f,\"chain_ms\":%.3f,"
                "\"scan_ms\":%.3f,\"gather_ms\":%.3f,\"build_ms\":%.3f,\"total_ms\":%.3f",
                locus.c_str(), contig.c_str(), s.start, s.end, s.attempt, s.allowed_expansion, s.crop_bits, s.warn_bits, s.n_cols, n_left, s.n_records,
                static_cast<unsigned long long>(s.n_kept_records), static_cast<unsigned long long>(s.total_overlaps), s.n_haplotypes, s.n_unknown, s.n_with_n,
                s.n_identical, out.files.n_kept, static_cast<unsigned long long>(s.shortest), s.filter_ms, s.expand_ms, s.reconstruct_ms, s.recon.chain_ms,
                s.recon.scan_ms, s.recon.gather_ms, s.build_ms, s.total_ms);
    if (indexed)
        std::printf(",\"fetch\":{\"chunks\":%llu,\"file_bytes\":%llu,\"bytes_read\":%llu,\"blocks_inflated\":%llu,\"bytes_inflated\":%llu,\"lines_walked\":%llu,"
                    "\"records_kept\":%llu,\"read_ms\":%.3f,\"inflate_ms\":%.3f,\"upload_ms\":%.3f,\"lines_ms\":%.3f,\"heads_ms\":%.3f,\"alleles_ms\":%.3f,"
                    "\"gt_ms\":%.3f,\"download_ms\":%.3f,\"total_ms\":%.3f}",
                    static_cast<unsigned long long>(fs.n_chunks), static_cast<unsigned long long>(fs.file_bytes), static_cast<unsigned long long>(fs.bytes_read),
                    static_cast<unsigned long long>(fs.blocks_inflated), static_cast<unsigned long long>(fs.bytes_inflated), static_cast<unsigned long long>(fs.lines_walked),
                    static_cast<unsigned long long>(fs.records_kept), fs.ms_read, fs.ms_inflate, fs.ms_upload, fs.ms_lines, fs.ms_heads, fs.ms_alleles, fs.ms_gt,
                    fs.ms_download, fs.ms_total);
    std::printf("}\n");
    lcty_locus_vcf_out_free(&out);
    lcty_vcf_records_free(&recs);
    lcty_vcf_free(vcf);
    lcty_vcf_indexed_close(ivcf);
    return 0;
}
