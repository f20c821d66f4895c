// examples/recruit_bam.cpp — the reads of a sample's indexed BAM file recruited to loci, through the C ABI, files in, files out:
//
//   sample.bam + sample.bam.bai                  coordinate-sorted, indexed        (lcty_sample_bam_open)
//   <locus dir>/haplotypes.fa.gz                 alleles                           (lcty_fasta_read)
//   <locus dir>/kmers.bin.lz4 | .br              off-target k-mer counts           (lcty_io_read_file + lcty_kmer_counts_parse)
//   <locus dir>/ref.bed, or --bed FILE           where the locus lies              (-> lcty_recruit_fetch_regions)
//        -> lcty_targets_*, lcty_sample_bam_fetch (regions + unmapped reads), lcty_sample_reads_recruit
//   OUTDIR/<locus>/reads.fq                      both mates of every recruited pair, one after the other (records without qualities
//                                                are written as FASTA records, as BamRecord::write_to does)
//
// This is recruit_to_targets (src/command/genotype.rs:872-907) for an input given with `-a`. The padding of the regions is 1000, the
// reference's value without an insert size distribution (genotype.rs:848-852), unless --padding says otherwise. Prints the stats of
// the fetch as one JSON line. --inflate device inflates the BGZF blocks of the fetch on the device (knob "sample_bam_inflate";
// default host: zlib). Build: see tests/test_gpu_sample_bam_example.py.
//   ./recruit_bam -a sample.bam [-i index] -d DB/loci/<locus> [-d ...] [--bed FILE] [--padding N] [--alt-contig N] [--single|--paired] [--inflate host|device] -o OUTDIR
//
// With --no-index the files given with -a (one or several) are read front to back, without an index and without regions, as
// `locityper recruit -a a.bam [-a b.bam] --no-index [-^]` reads them (DirectBamReader, src/seq/fastx.rs:692-729; -^ / --interleaved:
// PairedEndInterleaved, 423-453): lcty_bam_stream_open, then per window lcty_bam_stream_next -> lcty_sample_reads_recruit ->
// lcty_sample_reads_write_recruited into the same reads.fq files. Prints the stats of the stream as one JSON line.
//   ./recruit_bam --no-index -a a.bam [-a b.bam ...] [-^|--interleaved] -d DB/loci/<locus> [-d ...] [--inflate host|device] -o OUTDIR
#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "locityper_hip.h"

static void ok(int32_t rc, const char* what) {
    if (rc != LCTY_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, lcty_last_error()); std::exit(1); }
}
static bool exists(const std::string& p) { FILE* f = std::fopen(p.c_str(), "rb"); if (f) std::fclose(f); return f != nullptr; }

// one locus of the targets: alleles and off-target counts as genotype_dir.cpp loads them; makes OUTDIR/<locus> and returns its reads.fq
static std::string add_locus(lcty_targets* targets, const std::string& db, const std::string& outdir) {
    uint32_t A = 0; uint64_t names_len = 0, seqs_len = 0;
    const std::string fa = db + "/haplotypes.fa.gz";
    ok(lcty_fasta_read(fa.c_str(), &A, nullptr, &names_len, nullptr, &seqs_len, nullptr), "haplotypes.fa.gz");
    std::vector<char> name_blob(names_len); std::vector<uint8_t> seqs(seqs_len); std::vector<uint64_t> seq_off(A + 1);
    ok(lcty_fasta_read(fa.c_str(), &A, name_blob.data(), &names_len, seqs.data(), &seqs_len, seq_off.data()), "haplotypes.fa.gz");
    const std::string kp = exists(db + "/kmers.bin.lz4") ? db + "/kmers.bin.lz4" : db + "/kmers.bin.br";
    uint8_t* buf = nullptr; uint64_t len = 0;
    ok(lcty_io_read_file(kp.c_str(), &buf, &len), "kmers.bin");
    uint32_t k = 0, n_c = 0; uint64_t consumed = 0;
    ok(lcty_kmer_counts_parse(buf, len, &k, &n_c, nullptr, 0, nullptr, 0, &consumed), "KmerCounts::load (sizes)");
    if (n_c != A) { std::fprintf(stderr, "kmers.bin has %u contigs, the FASTA %u\n", n_c, A); std::exit(1); }
    std::vector<uint64_t> cnt_off(A + 1);
    uint64_t n_counts = 0;
    for (uint32_t a = 0; a < A; a++) n_counts += seq_off[a + 1] - seq_off[a] + 1 - k;
    std::vector<uint16_t> counts(n_counts);
    ok(lcty_kmer_counts_parse(buf, len, &k, &n_c, cnt_off.data(), A, counts.data(), n_counts, &consumed), "KmerCounts::load");
    lcty_io_free(buf);
    ok(lcty_targets_add_locus(targets, A, seqs.data(), seq_off.data(), counts.data(), cnt_off.data(), k, nullptr), "lcty_targets_add_locus");
    std::string locus = db;
    while (!locus.empty() && locus.back() == '/') locus.pop_back();
    locus = locus.substr(locus.find_last_of('/') + 1);
    mkdir((outdir + "/" + locus).c_str(), 0777);
    return outdir + "/" + locus + "/reads.fq";
}

int main(int argc, char** argv) {
    std::string bam_path, index_path, bed, outdir;
    std::vector<std::string> dirs, bam_paths;
    uint32_t padding = 1000, alt_contig = 10000000;
    int paired = -1, inflate_on_device = 0, no_index = 0, interleaved = 0;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "-a") { bam_path = next(); bam_paths.push_back(bam_path); }
        else if (a == "--no-index") no_index = 1;
        else if (a == "-^" || a == "--interleaved") interleaved = 1;
        else if (a == "-i") index_path = next();
        else if (a == "-d") dirs.push_back(next());
        else if (a == "--bed") bed = next();
        else if (a == "--padding") padding = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--alt-contig") alt_contig = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--single") paired = 0;
        else if (a == "--paired") paired = 1;
        else if (a == "--inflate") {
            const std::string v = next();
            if (v != "host" && v != "device") { std::fprintf(stderr, "--inflate takes host or device\n"); return 2; }
            inflate_on_device = v == "device";
        }
        else if (a == "-o") outdir = next();
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (bam_path.empty() || dirs.empty() || outdir.empty()) {
        std::fprintf(stderr, "usage: recruit_bam -a sample.bam [-i index] -d DB/loci/<locus> [-d ...] [--bed FILE] [--padding N] [--alt-contig N] [--single|--paired] [--inflate host|device] -o OUTDIR\n");
        return 2;
    }
    if (!no_index && (bam_paths.size() > 1 || interleaved)) { std::fprintf(stderr, "several -a files and -^ go with --no-index\n"); return 2; }

    if (no_index) {
        lcty_ctx* ctx = nullptr;
        ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
        ok(lcty_ctx_set_knob(ctx, "sample_bam_inflate", inflate_on_device), "lcty_ctx_set_knob");
        lcty_recruit_params rp;
        ok(lcty_recruit_params_default(&rp, LCTY_TECH_ILLUMINA, interleaved), "lcty_recruit_params_default");
        lcty_targets* targets = nullptr;
        ok(lcty_targets_create(ctx, &rp, &targets), "lcty_targets_create");
        std::vector<std::string> out_paths;
        mkdir(outdir.c_str(), 0777);
        for (const std::string& db : dirs) out_paths.push_back(add_locus(targets, db, outdir));
        ok(lcty_targets_finalize(targets, nullptr), "lcty_targets_finalize");
        std::vector<const char*> paths, inputs;
        for (const std::string& p : out_paths) paths.push_back(p.c_str());
        for (const std::string& p : bam_paths) inputs.push_back(p.c_str());
        lcty_fastx_writers* writers = nullptr;
        ok(lcty_fastx_writers_open(paths.data(), static_cast<uint32_t>(paths.size()), &writers), "lcty_fastx_writers_open");
        lcty_bam_stream* stream = nullptr;
        ok(lcty_bam_stream_open(ctx, inputs.data(), static_cast<uint32_t>(inputs.size()), interleaved, &stream), "lcty_bam_stream_open");
        lcty_bam_stream_stats st;
        std::memset(&st, 0, sizeof(st));
        const uint32_t max_out = 8;
        std::vector<uint32_t> cnt, loci;
        uint64_t recruited = 0;
        for (;;) {
            lcty_sample_reads* reads = nullptr;                                   // belongs to the stream: never freed here
            uint64_t n = 0;
            ok(lcty_bam_stream_next(stream, &reads, &n, &st), "lcty_bam_stream_next");
            if (!n) break;
            cnt.assign(n, 0); loci.assign(n * max_out, 0);
            ok(lcty_sample_reads_recruit(targets, reads, max_out, cnt.data(), loci.data()), "lcty_sample_reads_recruit");
            uint64_t n_written = 0;
            ok(lcty_sample_reads_write_recruited(reads, writers, max_out, cnt.data(), loci.data(), &n_written), "lcty_sample_reads_write_recruited");
            recruited += n_written;
        }
        ok(lcty_fastx_writers_close(writers), "lcty_fastx_writers_close");
        std::printf("{\"interleaved\": %d, \"files\": %llu, \"file_bytes\": %llu, \"bytes_read\": %llu, \"blocks_inflated\": %llu, \"bytes_inflated\": %llu, "
                    "\"windows\": %llu, \"windows_enlarged\": %llu, \"bytes_carried\": %llu, \"records_walked\": %llu, \"records_kept\": %llu, "
                    "\"bases_kept\": %llu, \"reads\": %llu, \"recruited\": %llu, \"ms_read\": %.3f, \"ms_inflate\": %.3f, \"ms_walk\": %.3f, "
                    "\"ms_upload\": %.3f, \"ms_record\": %.3f, \"ms_pair\": %.3f, \"ms_unpack\": %.3f, \"ms_total\": %.3f}\n",
                    interleaved, (unsigned long long)st.files, (unsigned long long)st.file_bytes, (unsigned long long)st.bytes_read,
                    (unsigned long long)st.blocks_inflated, (unsigned long long)st.bytes_inflated, (unsigned long long)st.windows,
                    (unsigned long long)st.windows_enlarged, (unsigned long long)st.bytes_carried, (unsigned long long)st.records_walked,
                    (unsigned long long)st.records_kept, (unsigned long long)st.bases_kept, (unsigned long long)st.reads, (unsigned long long)recruited,
                    st.ms_read, st.ms_inflate, st.ms_walk, st.ms_upload, st.ms_record, st.ms_pair, st.ms_unpack, st.ms_total);
        lcty_bam_stream_close(stream);
        lcty_targets_destroy(targets);
        lcty_ctx_destroy(ctx);
        return 0;
    }

    lcty_sample_bam* bam = nullptr;
    ok(lcty_sample_bam_open(bam_path.c_str(), index_path.empty() ? nullptr : index_path.c_str(), &bam), "lcty_sample_bam_open");
    uint32_t n_contigs = 0; const char* cnames = nullptr; const uint64_t* cname_off = nullptr; const uint32_t* clen = nullptr;
    ok(lcty_sample_bam_contigs(bam, &n_contigs, &cnames, &cname_off, &clen), "lcty_sample_bam_contigs");
    if (paired < 0) ok(lcty_sample_bam_is_paired(bam, &paired), "lcty_sample_bam_is_paired");

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    ok(lcty_ctx_set_knob(ctx, "sample_bam_inflate", inflate_on_device), "lcty_ctx_set_knob");
    lcty_recruit_params rp;
    ok(lcty_recruit_params_default(&rp, LCTY_TECH_ILLUMINA, paired), "lcty_recruit_params_default");
    lcty_targets* targets = nullptr;
    ok(lcty_targets_create(ctx, &rp, &targets), "lcty_targets_create");

    // ---- the loci (add_locus) and their intervals
    std::vector<uint32_t> tid, start, end;
    auto read_bed = [&](const std::string& path) {                             // load_recr_targets / Interval::parse_bed (genotype.rs:799-820)
        std::ifstream in(path);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(1); }
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string chrom; uint64_t s = 0, e = 0;
            if (!(ls >> chrom >> s >> e)) continue;
            uint32_t t = 0;
            while (t < n_contigs && chrom != cnames + cname_off[t]) t++;
            if (t == n_contigs) { std::fprintf(stderr, "Cannot parse locus coordinates (unknown contig %s), the region may be absent from the BAM/CRAM file\n", chrom.c_str()); continue; }
            tid.push_back(t); start.push_back(static_cast<uint32_t>(s)); end.push_back(static_cast<uint32_t>(e));
        }
    };
    std::vector<std::string> out_paths;
    mkdir(outdir.c_str(), 0777);
    for (const std::string& db : dirs) {
        out_paths.push_back(add_locus(targets, db, outdir));
        if (bed.empty()) read_bed(db + "/ref.bed");
    }
    if (!bed.empty()) read_bed(bed);
    ok(lcty_targets_finalize(targets, nullptr), "lcty_targets_finalize");

    // ---- postprocess_targets, the fetch, recruitment, the per-locus files
    std::vector<uint32_t> rt(tid.size() + n_contigs), rs(rt.size()), re(rt.size());
    uint32_t n_regions = 0;
    ok(lcty_recruit_fetch_regions(static_cast<uint32_t>(tid.size()), tid.data(), start.data(), end.data(), n_contigs, clen, padding, alt_contig, 1000,
                                  rt.data(), rs.data(), re.data(), &n_regions), "lcty_recruit_fetch_regions");
    lcty_sample_reads* reads = nullptr;
    lcty_sample_bam_stats st;
    ok(lcty_sample_bam_fetch(ctx, bam, n_regions, rt.data(), rs.data(), re.data(), 1, 0, paired, &reads, &st), "lcty_sample_bam_fetch");
    const uint32_t max_out = 8;
    std::vector<uint32_t> cnt(st.n_pairs + 1), loci((st.n_pairs + 1) * max_out);
    ok(lcty_sample_reads_recruit(targets, reads, max_out, cnt.data(), loci.data()), "lcty_sample_reads_recruit");
    std::vector<const char*> paths;
    for (const std::string& p : out_paths) paths.push_back(p.c_str());
    lcty_fastx_writers* writers = nullptr;
    ok(lcty_fastx_writers_open(paths.data(), static_cast<uint32_t>(paths.size()), &writers), "lcty_fastx_writers_open");
    uint64_t n_written = 0;
    ok(lcty_sample_reads_write_recruited(reads, writers, max_out, cnt.data(), loci.data(), &n_written), "lcty_sample_reads_write_recruited");
    ok(lcty_fastx_writers_close(writers), "lcty_fastx_writers_close");
    std::printf("{\"paired\": %d, \"regions\": %llu, \"chunks\": %llu, \"file_bytes\": %llu, \"bytes_read\": %llu, \"blocks_inflated\": %llu, "
                "\"bytes_inflated\": %llu, \"records_walked\": %llu, \"records_primary\": %llu, \"records_kept\": %llu, \"pairs\": %llu, "
                "\"discarded\": %llu, \"recruited\": %llu, \"ms_read\": %.3f, \"ms_inflate\": %.3f, \"ms_walk\": %.3f, \"ms_upload\": %.3f, "
                "\"ms_record\": %.3f, \"ms_pair\": %.3f, \"ms_unpack\": %.3f, \"ms_total\": %.3f}\n",
                paired, (unsigned long long)st.n_regions, (unsigned long long)st.n_chunks, (unsigned long long)st.file_bytes,
                (unsigned long long)st.bytes_read, (unsigned long long)st.blocks_inflated, (unsigned long long)st.bytes_inflated,
                (unsigned long long)st.records_walked, (unsigned long long)st.records_primary, (unsigned long long)st.records_kept,
                (unsigned long long)st.n_pairs, (unsigned long long)st.n_discarded, (unsigned long long)n_written, st.ms_read, st.ms_inflate,
                st.ms_walk, st.ms_upload, st.ms_record, st.ms_pair, st.ms_unpack, st.ms_total);
    lcty_sample_reads_free(reads);
    lcty_targets_destroy(targets);
    lcty_sample_bam_close(bam);
    lcty_ctx_destroy(ctx);
    return 0;
}
