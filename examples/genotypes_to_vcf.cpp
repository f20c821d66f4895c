// examples/genotypes_to_vcf.cpp — extra/into_csv.py and extra/into_vcf.py (main 199-250, load_database 47-73, process_locus 117-144,
// merge_vcfs 167-196) through the C ABI, files in, files out:
//
//   genotypes_to_vcf (-i predictions.csv | -I list) -d DB -v variants.vcf.gz [-x index] -g GENOME_NAME -o OUTDIR
//                    [--subset-loci NAME ...] [--csv OUT] [--fields all|upstream] [--deflate host|device]
//
//   -i            the table of into_csv.py (lcty_predictions_csv_read)
//   -I            into_csv.py's list: lines `path sample`; the predictions are read from <path>/loci/<locus>/res.json.gz
//                 (lcty_res_summary_read), one row per directory under <path>/loci
//   --csv         write the table (lcty_predictions_csv_write)
//   -d            the database: DB/loci/<locus>/ref.bed gives every locus's interval
//   -v, -x        the phased variants file (BGZF) and its tabix index (default: variants + .tbi); its ##contig lines give the contigs'
//                 indices and lengths (lcty_vcf_indexed_contigs)
//   --fields      the FORMAT fields behind GT: all five (default), or reads:unexpl:wdist as upstream writes them
//   --deflate     device (default): lcty_bgzf_deflate; host: lcty_io_write_bgzf, the block offsets read back from the file. The inflated
//                 bytes are the same.
//
// Writes OUTDIR/<locus>.vcf.gz + .tbi for every locus of the database that has predictions, then OUTDIR/merged.vcf.gz + .tbi, and prints
// one JSON line of counts and stage times. Loci are taken in the order of their names. The ID column is `.`: the fetch does not keep it.
// Build: see tests/test_gpu_gtvcf_example.py.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "locityper_hip.h"

static void ok(int32_t rc, const char* what) {
    if (rc != LCTY_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, lcty_last_error()); std::exit(1); }
}
[[noreturn]] static void die(const std::string& msg) { std::fprintf(stderr, "%s\n", msg.c_str()); std::exit(1); }
static bool is_dir(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

static std::vector<std::string> subdirs(const std::string& dir) {
    std::vector<std::string> out;
    DIR* d = opendir(dir.c_str());
    if (!d) die("Directory `" + dir + "` cannot be read");
    while (const dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name != "." && name != ".." && is_dir(dir + "/" + name)) out.push_back(name);
    }
    closedir(d);
    std::sort(out.begin(), out.end());
    return out;
}

struct Row { std::string sample, locus, genotype, warnings; int64_t qual10, reads, unexpl, wdist5; };
struct Locus { std::string chrom; uint32_t start, end; };

static std::string blob_of(const std::vector<std::string>& names) {
    std::string b;
    for (const std::string& n : names) { b += n; b.push_back('\0'); }
    return b;
}

// the file's BGZF data blocks, one per 0xff00 bytes of text: the offset of each and the end of the last (what lcty_bgzf_deflate returns)
static std::vector<uint64_t> block_offsets(const std::string& path, uint64_t text_len) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const uint64_t n_blocks = (text_len + 0xff00 - 1) / 0xff00;
    std::vector<uint64_t> off(1, 0);
    uint64_t at = 0;
    for (uint64_t b = 0; b < n_blocks; b++) {
        if (at + 18 > raw.size()) die(path + ": fewer BGZF blocks than its text needs");
        at += (uint64_t(raw[at + 16]) | uint64_t(raw[at + 17]) << 8) + 1;
        off.push_back(at);
    }
    return off;
}

struct Times { double deflate_ms = 0, index_ms = 0; uint64_t file_bytes = 0; };

// text as path (BGZF) and path + ".tbi"
static void write_indexed(lcty_ctx* ctx, const std::string& path, bool on_device, const lcty_gtvcf_out& o, uint32_t n_contigs, const char* contigs,
                          const uint32_t* contig_ix, const uint32_t* pos, const uint32_t* ref_len, Times* t) {
    std::vector<uint64_t> block_off;
    const uint8_t* text = reinterpret_cast<const uint8_t*>(o.text);
    if (on_device) {
        std::vector<uint8_t> file(lcty_bgzf_deflate_bound(o.text_len, 1));
        block_off.resize((o.text_len + 0xff00 - 1) / 0xff00 + 1);
        uint64_t n = 0;
        lcty_bgzf_deflate_stats st{};
        ok(lcty_bgzf_deflate(ctx, text, o.text_len, 1, file.data(), file.size(), &n, block_off.data(), &st), "lcty_bgzf_deflate");
        t->deflate_ms += st.ms_total;
        std::ofstream f(path, std::ios::binary);
        f.write(reinterpret_cast<const char*>(file.data()), std::streamsize(n));
        if (!f) die("cannot write " + path);
        t->file_bytes += n;
    } else {
        ok(lcty_io_write_bgzf(path.c_str(), text, o.text_len), "lcty_io_write_bgzf");
        block_off = block_offsets(path, o.text_len);
        t->file_bytes += block_off.back() + 28;
    }
    ok(lcty_tbi_write((path + ".tbi").c_str(), n_contigs, contigs, o.n_lines, contig_ix, pos, ref_len, o.line_off, block_off.data(), block_off.size() - 1), "lcty_tbi_write");
}

int main(int argc, char** argv) {
    std::string csv_in, list_in, db, variants, index, genome, outdir, csv_out, fields = "all", deflate = "device";
    std::set<std::string> subset;
    bool have_subset = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&]() -> std::string { if (i + 1 >= argc) die("option " + a + " needs a value"); return argv[++i]; };
        if (a == "-i") csv_in = value();
        else if (a == "-I") list_in = value();
        else if (a == "-d") db = value();
        else if (a == "-v") variants = value();
        else if (a == "-x") index = value();
        else if (a == "-g") genome = value();
        else if (a == "-o") outdir = value();
        else if (a == "--csv") csv_out = value();
        else if (a == "--fields") fields = value();
        else if (a == "--deflate") deflate = value();
        else if (a == "--subset-loci") { have_subset = true; while (i + 1 < argc && argv[i + 1][0] != '-') subset.insert(argv[++i]); }
        else die("unknown argument " + a);
    }
    if (csv_in.empty() == list_in.empty()) die("one of -i predictions.csv and -I list is needed");
    if (db.empty() || variants.empty() || genome.empty() || outdir.empty()) die("-d, -v, -g and -o are needed");
    if (fields != "all" && fields != "upstream") die("--fields all|upstream");
    if (deflate != "host" && deflate != "device") die("--deflate host|device");
    mkdir(outdir.c_str(), 0777);

    // ---- the predictions
    std::vector<Row> rows;
    if (!csv_in.empty()) {
        lcty_predictions p{};
        ok(lcty_predictions_csv_read(csv_in.c_str(), &p), "lcty_predictions_csv_read");
        for (uint64_t r = 0; r < p.n_rows; r++)
            rows.push_back(Row{p.text + p.sample_off[r], p.text + p.locus_off[r], p.text + p.genotype_off[r], p.text + p.warn_off[r], p.qual10[r], p.reads[r],
                               p.unexpl[r], p.wdist5[r]});
        lcty_predictions_free(&p);
    } else {
        std::ifstream f(list_in);
        if (!f) die("cannot open " + list_in);
        std::vector<lcty_res_summary> sums;
        std::vector<std::string> samples, loci;
        std::set<std::string> seen;
        for (std::string line; std::getline(f, line);) {
            if (line.empty() || line[0] == '#') continue;                // into_csv.py:44-46
            std::istringstream ss(line);
            std::string path, sample, more;
            if (!(ss >> path >> sample) || (ss >> more)) die("the list needs two columns: `" + line + "`");
            if (!seen.insert(sample).second) die("Sample " + sample + " appears twice");
            for (const std::string& locus : subdirs(path + "/loci")) {    // process_sample 67-96
                lcty_res_summary s{};
                ok(lcty_res_summary_read((path + "/loci/" + locus + "/res.json.gz").c_str(), &s), "lcty_res_summary_read");
                sums.push_back(s); samples.push_back(sample); loci.push_back(locus);
            }
        }
        if (seen.empty()) die("Loaded zero samples");
        std::vector<const char*> sp, lp;
        for (size_t r = 0; r < sums.size(); r++) { sp.push_back(samples[r].c_str()); lp.push_back(loci[r].c_str()); }
        if (!csv_out.empty()) ok(lcty_predictions_csv_write(csv_out.c_str(), sums.size(), sp.data(), lp.data(), sums.data()), "lcty_predictions_csv_write");
        for (size_t r = 0; r < sums.size(); r++) {
            const lcty_res_summary& s = sums[r];
            rows.push_back(Row{samples[r], loci[r], s.state == LCTY_RES_CALLED ? s.genotype : s.state == LCTY_RES_MISSING ? "?" : "*",
                               s.state == LCTY_RES_CALLED ? s.warnings : "", s.qual10, s.reads, s.unexpl, s.wdist5});
            lcty_res_summary_free(&sums[r]);
        }
        csv_out.clear();
    }
    if (!csv_out.empty()) {                                              // -i with --csv: the table again, from what was read
        std::vector<lcty_res_summary> sums(rows.size());
        std::vector<const char*> sp, lp;
        for (size_t r = 0; r < rows.size(); r++) {
            Row& w = rows[r];
            sums[r] = lcty_res_summary{&w.genotype[0], &w.warnings[0], w.qual10, w.reads, w.unexpl, w.wdist5,
                                       w.genotype == "*" ? LCTY_RES_NO_GENOTYPE : w.genotype == "?" ? LCTY_RES_MISSING : LCTY_RES_CALLED, 0};
            sp.push_back(w.sample.c_str()); lp.push_back(w.locus.c_str());
        }
        ok(lcty_predictions_csv_write(csv_out.c_str(), sums.size(), sp.data(), lp.data(), sums.data()), "lcty_predictions_csv_write");
    }
    std::set<std::string> sample_set;
    std::map<std::string, std::map<std::string, size_t>> by_locus;       // locus -> sample -> its last row (into_vcf.py:42)
    for (size_t r = 0; r < rows.size(); r++) { sample_set.insert(rows[r].sample); by_locus[rows[r].locus][rows[r].sample] = r; }
    const std::vector<std::string> samples(sample_set.begin(), sample_set.end());          // sorted bytewise (44)

    // ---- the database (load_database 47-73)
    if (!is_dir(db + "/loci")) die("Directory `" + db + "` does not contain \"loci\" subdirectory");
    std::map<std::string, Locus> loci;
    for (const std::string& name : subdirs(db + "/loci")) {
        if (have_subset && !subset.count(name)) continue;
        std::ifstream bed(db + "/loci/" + name + "/ref.bed");
        std::string chrom, locus; long long start = -1, end = -1;
        if (!(bed >> chrom >> start >> end >> locus)) die("cannot read " + db + "/loci/" + name + "/ref.bed");
        if (locus != name) die("Locus directory `" + db + "/loci/" + name + "` contains locus `" + locus + "` (expected `" + name + "`)");
        if (start < 0 || end < start || end > 0xFFFFFFFFll) die("locus " + name + ": a bad interval");
        loci[name] = Locus{chrom, uint32_t(start), uint32_t(end)};
    }

    // ---- the variants file
    lcty_vcf_indexed* vcf = nullptr;
    ok(lcty_vcf_indexed_open(variants.c_str(), index.empty() ? nullptr : index.c_str(), &vcf), "lcty_vcf_indexed_open");
    lcty_vcf_view view{};
    ok(lcty_vcf_indexed_view_get(vcf, &view), "lcty_vcf_indexed_view_get");
    lcty_vcf_contigs contigs{};
    ok(lcty_vcf_indexed_contigs(vcf, &contigs), "lcty_vcf_indexed_contigs");
    std::map<std::string, uint32_t> tid;
    { const char* p = contigs.names; for (uint32_t c = 0; c < contigs.n_contigs; c++) { tid[p] = c; p += std::strlen(p) + 1; } }

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_gtvcf* set = nullptr;
    const std::string sample_blob = blob_of(samples);
    ok(lcty_gtvcf_create(ctx, sample_blob.data(), uint32_t(samples.size()), fields == "all" ? LCTY_GTVCF_ALL : LCTY_GTVCF_UPSTREAM, &set), "lcty_gtvcf_create");

    lcty_gtvcf_stats sum{};
    Times times;
    double fetch_ms = 0;
    uint64_t n_loci = 0, n_records = 0, n_missing = 0;
    auto book = [&](const lcty_gtvcf_stats& s) {
        sum.upload_ms += s.upload_ms; sum.cells_ms += s.cells_ms; sum.merge_ms += s.merge_ms; sum.widths_ms += s.widths_ms; sum.write_ms += s.write_ms;
        sum.download_ms += s.download_ms; sum.text_bytes += s.text_bytes;
    };
    for (const auto& kv : loci) {
        const std::string& name = kv.first; const Locus& L = kv.second;
        const auto preds = by_locus.find(name);
        if (preds == by_locus.end()) { n_missing++; continue; }          // 229-232: genotype predictions missing for this locus
        const auto t = tid.find(L.chrom);
        if (t == tid.end()) die("locus " + name + ": the variants file has no contig " + L.chrom);
        lcty_vcf_records recs{};
        lcty_vcf_fetch_stats fs{};
        ok(lcty_vcf_indexed_fetch(ctx, vcf, L.chrom.c_str(), L.start, L.end, nullptr, &recs, &fs), "lcty_vcf_indexed_fetch");
        fetch_ms += fs.ms_total;
        // the columns of every predicted allele, then the features of every sample
        std::vector<std::string> alleles;
        std::vector<uint32_t> pred_off(samples.size() + 1, 0);
        std::vector<int64_t> qual(samples.size(), LCTY_GTVCF_ABSENT), reads(qual), unexpl(qual), wdist(qual);
        std::vector<uint64_t> warn_off(samples.size() + 1, 0);
        std::string warn;
        for (size_t s = 0; s < samples.size(); s++) {
            const auto it = preds->second.find(samples[s]);
            if (it != preds->second.end() && rows[it->second].genotype != "*" && rows[it->second].genotype != "?") {
                const Row& r = rows[it->second];
                std::istringstream g(r.genotype);
                for (std::string a; std::getline(g, a, ',');) alleles.push_back(a);
                qual[s] = r.qual10; reads[s] = r.reads; unexpl[s] = r.unexpl; wdist[s] = r.wdist5; warn += r.warnings;
            }
            pred_off[s + 1] = uint32_t(alleles.size()); warn_off[s + 1] = warn.size();
        }
        std::vector<uint32_t> cols(alleles.size() + 1);
        const std::string allele_blob = blob_of(alleles);
        ok(lcty_gtvcf_columns(&view, genome.c_str(), uint32_t(alleles.size()), allele_blob.data(), cols.data()), "lcty_gtvcf_columns");
        lcty_gtvcf_locus_in in{};
        in.locus = name.c_str(); in.chrom = L.chrom.c_str(); in.contig_len = contigs.length[t->second]; in.contig_ix = t->second; in.start = L.start; in.end = L.end;
        in.n_recs = recs.n_recs; in.n_haps = recs.n_haps;
        in.pos = recs.pos; in.ref_len = recs.ref_len; in.rec_allele = recs.rec_allele; in.allele_off = recs.allele_off; in.allele_bytes = recs.allele_bytes; in.gt = recs.gt;
        in.pred_off = pred_off.data(); in.pred_col = cols.data();
        in.qual10 = qual.data(); in.reads = reads.data(); in.unexpl = unexpl.data(); in.wdist5 = wdist.data();
        in.warn_off = warn_off.data(); in.warn = warn.data();
        lcty_gtvcf_out o{};
        ok(lcty_gtvcf_add_locus(set, &in, &o), "lcty_gtvcf_add_locus");
        book(o.stats);
        const std::vector<uint32_t> zeros(size_t(recs.n_recs) + 1, 0);
        const std::string chrom_blob = blob_of({L.chrom});
        write_indexed(ctx, outdir + "/" + name + ".vcf.gz", deflate == "device", o, 1, chrom_blob.data(), zeros.data(), recs.pos, recs.ref_len, &times);
        n_loci++; n_records += recs.n_recs;
        lcty_gtvcf_out_free(&o);
        lcty_vcf_records_free(&recs);
    }
    lcty_gtvcf_out m{};
    ok(lcty_gtvcf_merge(set, &m), "lcty_gtvcf_merge");
    book(m.stats);
    write_indexed(ctx, outdir + "/merged.vcf.gz", deflate == "device", m, m.n_contigs, m.contigs, m.line_contig, m.line_pos, m.line_ref_len, &times);
    std::printf("{\"samples\": %zu, \"loci\": %llu, \"loci_without_predictions\": %llu, \"records\": %llu, \"merged_records\": %llu, \"joined\": %llu, "
                "\"text_bytes\": %llu, \"file_bytes\": %llu, \"fields\": \"%s\", \"deflate\": \"%s\", \"fetch_ms\": %.3f, \"upload_ms\": %.3f, \"cells_ms\": %.3f, "
                "\"merge_ms\": %.3f, \"widths_ms\": %.3f, \"write_ms\": %.3f, \"download_ms\": %.3f, \"deflate_ms\": %.3f}\n",
                samples.size(), static_cast<unsigned long long>(n_loci), static_cast<unsigned long long>(n_missing), static_cast<unsigned long long>(n_records),
                static_cast<unsigned long long>(m.n_lines), static_cast<unsigned long long>(m.n_joined), static_cast<unsigned long long>(sum.text_bytes),
                static_cast<unsigned long long>(times.file_bytes), fields.c_str(), deflate.c_str(), fetch_ms, sum.upload_ms, sum.cells_ms, sum.merge_ms, sum.widths_ms,
                sum.write_ms, sum.download_ms, times.deflate_ms);
    lcty_gtvcf_out_free(&m);
    lcty_gtvcf_destroy(set);
    lcty_vcf_indexed_close(vcf);
    lcty_ctx_destroy(ctx);
    return 0;
}
