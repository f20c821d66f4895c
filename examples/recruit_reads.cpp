// examples/recruit_reads.cpp — the reads of FASTA / FASTQ files recruited to loci, through the C ABI, files in, files out:
//
//   R1 [R2]                                      FASTA / FASTQ, plain, gzip or BGZF (lcty_fastx_open | lcty_fastx_device_open)
//   <locus dir>/haplotypes.fa.gz                 alleles                           (lcty_fasta_read)
//   <locus dir>/kmers.bin.lz4 | .br              off-target k-mer counts           (lcty_io_read_file + lcty_kmer_counts_parse)
//        -> lcty_targets_*, then chunk by chunk: the host route (lcty_fastx_next + lcty_recruit + lcty_fastx_write_recruited) or the
//           device route (lcty_fastx_device_next + lcty_fastx_device_recruit + lcty_fastx_device_write_recruited)
//   OUTDIR/<locus>/reads.fq                      both mates of every recruited pair, one after the other
//
// This is recruit_single_thread (src/seq/recruit.rs:1000-1030) for `locityper genotype -i R1 [R2] [--interleaved]`. Both routes write
// the same bytes. Prints one JSON line: the counts, and for the device route its stage times. --window N and --inflate host|device set
// the knobs "fastx_window_bytes" and "sample_bam_inflate" of the device route. Build: see tests/test_gpu_fastx_example.py.
//   ./recruit_reads -i R1 [R2] [--interleaved] -d DB/loci/<locus> [-d ...] [--parse host|device] [--chunk N] [--window N] [--inflate host|device] -o OUTDIR
#include <sys/stat.h>

#include <chrono>
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
static bool exists(const std::string& p) { FILE* f = std::fopen(p.c_str(), "rb"); if (f) std::fclose(f); return f != nullptr; }
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
    std::string outdir, parse = "device";
    std::vector<std::string> inputs, dirs;
    int interleaved = 0, inflate_on_device = 0;
    uint64_t chunk = 1u << 20;
    long long window = -1;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "-i") { inputs.push_back(next()); if (i + 1 < argc && argv[i + 1][0] != '-') inputs.push_back(argv[++i]); }
        else if (a == "--interleaved") interleaved = 1;
        else if (a == "-d") dirs.push_back(next());
        else if (a == "--parse") parse = next();
        else if (a == "--chunk") chunk = std::strtoull(next(), nullptr, 10);
        else if (a == "--window") window = std::strtoll(next(), nullptr, 10);
        else if (a == "--inflate") {
            const std::string v = next();
            if (v != "host" && v != "device") { std::fprintf(stderr, "--inflate takes host or device\n"); return 2; }
            inflate_on_device = v == "device";
        }
        else if (a == "-o") outdir = next();
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (inputs.empty() || inputs.size() > 2 || dirs.empty() || outdir.empty() || (parse != "host" && parse != "device") || chunk == 0) {
        std::fprintf(stderr, "usage: recruit_reads -i R1 [R2] [--interleaved] -d DB/loci/<locus> [-d ...] [--parse host|device] [--chunk N] [--window N] [--inflate host|device] -o OUTDIR\n");
        return 2;
    }
    const char* p1 = inputs[0].c_str();
    const char* p2 = inputs.size() > 1 ? inputs[1].c_str() : nullptr;
    const int paired = p2 || interleaved;

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    ok(lcty_ctx_set_knob(ctx, "sample_bam_inflate", inflate_on_device), "lcty_ctx_set_knob");
    ok(lcty_ctx_set_knob(ctx, "fastx_window_bytes", window), "lcty_ctx_set_knob");
    lcty_recruit_params rp;
    ok(lcty_recruit_params_default(&rp, LCTY_TECH_ILLUMINA, paired), "lcty_recruit_params_default");
    lcty_targets* targets = nullptr;
    ok(lcty_targets_create(ctx, &rp, &targets), "lcty_targets_create");

    // ---- the loci: alleles and off-target counts as recruit_bam.cpp loads them
    std::vector<std::string> out_paths;
    mkdir(outdir.c_str(), 0777);
    for (const std::string& db : dirs) {
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
        if (n_c != A) { std::fprintf(stderr, "kmers.bin has %u contigs, the FASTA %u\n", n_c, A); return 1; }
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
        out_paths.push_back(outdir + "/" + locus + "/reads.fq");
    }
    ok(lcty_targets_finalize(targets, nullptr), "lcty_targets_finalize");
    std::vector<const char*> paths;
    for (const std::string& p : out_paths) paths.push_back(p.c_str());
    lcty_fastx_writers* writers = nullptr;
    ok(lcty_fastx_writers_open(paths.data(), static_cast<uint32_t>(paths.size()), &writers), "lcty_fastx_writers_open");

    // ---- read -> recruit -> write, chunk by chunk
    const uint32_t max_out = 8;
    std::vector<uint32_t> cnt, loci;
    uint64_t n_units = 0, n_recruited = 0, n_chunks = 0;
    double ms_recruit = 0, ms_write = 0, ms_parse = 0;
    const double t_start = now_ms();
    lcty_fastx_device_stats st;
    std::memset(&st, 0, sizeof(st));
    if (parse == "device") {
        lcty_fastx_device* f = nullptr;
        ok(lcty_fastx_device_open(ctx, p1, p2, interleaved, &f), "lcty_fastx_device_open");
        for (;;) {
            uint64_t n = 0, w = 0;
            ok(lcty_fastx_device_next(f, chunk, &n, &st), "lcty_fastx_device_next");
            if (!n) break;
            cnt.assign(n, 0); loci.assign(n * max_out, 0);
            double t0 = now_ms();
            ok(lcty_fastx_device_recruit(targets, f, max_out, cnt.data(), loci.data()), "lcty_fastx_device_recruit");
            ms_recruit += now_ms() - t0; t0 = now_ms();
            ok(lcty_fastx_device_write_recruited(f, writers, max_out, cnt.data(), loci.data(), &w), "lcty_fastx_device_write_recruited");
            ms_write += now_ms() - t0;
            n_units += n; n_recruited += w; n_chunks++;
        }
        ms_parse = st.ms_total;
        lcty_fastx_device_close(f);
    } else {
        lcty_fastx* f = nullptr;
        ok(lcty_fastx_open(p1, p2, interleaved, &f), "lcty_fastx_open");
        for (;;) {
            uint64_t n = 0, w = 0;
            lcty_reads_host view;
            double t0 = now_ms();
            ok(lcty_fastx_next(f, chunk, &view, &n), "lcty_fastx_next");
            ms_parse += now_ms() - t0;
            if (!n) break;
            cnt.assign(n, 0); loci.assign(n * max_out, 0);
            t0 = now_ms();
            ok(lcty_recruit(targets, &view, paired, max_out, cnt.data(), loci.data()), "lcty_recruit");
            ms_recruit += now_ms() - t0; t0 = now_ms();
            ok(lcty_fastx_write_recruited(f, writers, max_out, cnt.data(), loci.data(), &w), "lcty_fastx_write_recruited");
            ms_write += now_ms() - t0;
            n_units += n; n_recruited += w; n_chunks++;
        }
        lcty_fastx_close(f);
    }
    ok(lcty_fastx_writers_close(writers), "lcty_fastx_writers_close");
    std::printf("{\"parse\": \"%s\", \"paired\": %d, \"reads\": %llu, \"chunks\": %llu, \"recruited\": %llu, \"bytes_read\": %llu, \"bytes_inflated\": %llu, "
                "\"windows\": %llu, \"windows_enlarged\": %llu, \"records\": %llu, \"ms_read\": %.3f, \"ms_inflate\": %.3f, \"ms_upload\": %.3f, "
                "\"ms_lines\": %.3f, \"ms_records\": %.3f, \"ms_pack\": %.3f, \"ms_parse\": %.3f, \"ms_recruit\": %.3f, \"ms_write\": %.3f, \"ms_total\": %.3f}\n",
                parse.c_str(), paired, (unsigned long long)n_units, (unsigned long long)n_chunks, (unsigned long long)n_recruited,
                (unsigned long long)st.bytes_read, (unsigned long long)st.bytes_inflated, (unsigned long long)st.windows,
                (unsigned long long)st.windows_enlarged, (unsigned long long)st.records, st.ms_read, st.ms_inflate, st.ms_upload, st.ms_lines,
                st.ms_records, st.ms_pack, ms_parse, ms_recruit, ms_write, now_ms() - t_start);
    lcty_targets_destroy(targets);
    lcty_ctx_destroy(ctx);
    return 0;
}
