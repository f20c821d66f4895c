// examples/count_kmers.cpp — the genome-wide k-mer counts of a locus's sequences without a Jellyfish database (JfKmerGetter::new /
// fetch, src/seq/counts.rs:258-369) and the reference window of the locus (seq::fetch_seq, src/seq/mod.rs:149) through the C ABI,
// files in, files out:
//
//   count_kmers -g genome.fa[.gz] -k K [-c COUNTER_BYTES] -s seqs.fa[.gz] [-r ref.fa[.gz]] [-R contig:start-end WINDOW.fa] -o counts.bin
//
//   -g   the genome, loaded once and kept packed on the device                                     (lcty_genome_load_fasta)
//   -s   the sequences to count, upper-case A C G T (the haplotypes of a locus)                    (lcty_fasta_read)
//   -r   one record, the reference sequence of the locus: its N runs are filled with A and it is counted LAST, the order of
//        process_alleles (command/add.rs:626-636) — counts.bin is then what examples/build_locus_db.cpp takes
//   -R   also writes the window [start, end) of a contig (0-based, half open) as FASTA: capitals A C G T, N for everything else —
//        the reference window examples/build_locus_from_vcf.cpp and examples/estimate_bg.cpp take            (lcty_genome_fetch)
//   -o   ONE KmerCounts block (counts.rs:108-124)                                (lcty_genome_kmer_counts, lcty_kmer_counts_write)
//   -c   counter bytes of the block, 2 by default: values are clamped to 65 535 (255 with -c 1)
// The statistics of the call go to stdout as one JSON line.
//
// Build: see tests/test_gpu_kmer_count_example.py.
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

struct Fasta { uint32_t n = 0; std::vector<char> names; std::vector<uint8_t> seqs; std::vector<uint64_t> off; };
static Fasta read_fasta(const std::string& path) {
    Fasta f; uint64_t nl = 0, sl = 0;
    ok(lcty_fasta_read(path.c_str(), &f.n, nullptr, &nl, nullptr, &sl, nullptr), path.c_str());
    f.names.resize(nl + 1); f.seqs.resize(sl + 1); f.off.resize(f.n + 1);
    ok(lcty_fasta_read(path.c_str(), &f.n, f.names.data(), &nl, f.seqs.data(), &sl, f.off.data()), path.c_str());
    f.seqs.resize(sl);
    return f;
}

static void write_file(const std::string& path, const void* data, uint64_t len) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, 1, len, f) != len || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
}

int main(int argc, char** argv) {
    std::string genome_path, seqs_path, ref_path, region, window_path, out_path;
    uint32_t k = 0, counter_bytes = 2;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "-g") genome_path = next();
        else if (a == "-k") k = static_cast<uint32_t>(std::atoi(next().c_str()));
        else if (a == "-c") counter_bytes = static_cast<uint32_t>(std::atoi(next().c_str()));
        else if (a == "-s") seqs_path = next();
        else if (a == "-r") ref_path = next();
        else if (a == "-R") { region = next(); window_path = next(); }
        else if (a == "-o") out_path = next();
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (genome_path.empty() || seqs_path.empty() || out_path.empty() || k == 0) {
        std::fprintf(stderr, "usage: count_kmers -g genome.fa[.gz] -k K [-c COUNTER_BYTES] -s seqs.fa[.gz] [-r ref.fa[.gz]] "
                             "[-R contig:start-end WINDOW.fa] -o counts.bin\n");
        return 2;
    }
    Fasta q = read_fasta(seqs_path);
    if (!ref_path.empty()) {
        const Fasta ref = read_fasta(ref_path);
        if (ref.n != 1) { std::fprintf(stderr, "%s: one sequence expected, %u found\n", ref_path.c_str(), ref.n); return 1; }
        for (uint8_t c : ref.seqs) q.seqs.push_back(c == 'N' ? 'A' : c);                  // add.rs:626-632
        q.off.push_back(q.seqs.size());
        q.n++;
    }

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_genome* genome = nullptr;
    ok(lcty_genome_load_fasta(ctx, genome_path.c_str(), &genome), genome_path.c_str());
    uint32_t n_contigs = 0; uint64_t n_bases = 0;
    ok(lcty_genome_info(genome, &n_contigs, &n_bases), "lcty_genome_info");

    uint64_t n_values = 0;
    for (uint32_t i = 0; i < q.n; i++) { const uint64_t len = q.off[i + 1] - q.off[i]; n_values += len + 1 > k ? len + 1 - k : 0; }
    std::vector<uint16_t> counts(n_values + 1);
    std::vector<uint64_t> cnt_off(q.n + 1);
    lcty_genome_count_stats st;
    ok(lcty_genome_kmer_counts(genome, k, counter_bytes, q.n, q.seqs.data(), q.off.data(), counts.data(), cnt_off.data(), &st), "lcty_genome_kmer_counts");
    uint64_t need = 0;
    ok(lcty_kmer_counts_write(k, counter_bytes, q.n, cnt_off.data(), counts.data(), nullptr, 0, &need), "KmerCounts::save (size)");
    std::vector<uint8_t> block(need + 1);
    ok(lcty_kmer_counts_write(k, counter_bytes, q.n, cnt_off.data(), counts.data(), block.data(), need, &need), "KmerCounts::save");
    write_file(out_path, block.data(), need);

    if (!region.empty()) {
        const size_t colon = region.rfind(':'), dash = region.rfind('-');
        if (colon == std::string::npos || dash == std::string::npos || dash < colon) { std::fprintf(stderr, "-R takes contig:start-end\n"); return 2; }
        const std::string contig = region.substr(0, colon);
        const uint64_t start = std::strtoull(region.c_str() + colon + 1, nullptr, 10), end = std::strtoull(region.c_str() + dash + 1, nullptr, 10);
        std::vector<uint8_t> window(end > start ? end - start : 1);
        ok(lcty_genome_fetch(genome, contig.c_str(), start, end, window.data()), region.c_str());
        const uint64_t woff[2] = {0, end - start};
        ok(lcty_fasta_write_text(1, region.c_str(), window.data(), woff, nullptr, 0, &need), "write_fasta (size)");
        std::vector<char> text(need + 1);
        ok(lcty_fasta_write_text(1, region.c_str(), window.data(), woff, text.data(), need, &need), "write_fasta");
        write_file(window_path, text.data(), need);
    }
    std::printf("{\"k\":%u,\"counter_bytes\":%u,\"genome_contigs\":%u,\"genome_bases\":%llu,\"n_seqs\":%u,\"n_query_kmers\":%llu,\"n_distinct\":%llu,"
                "\"table_slots\":%llu,\"n_scanned\":%llu,\"n_hits\":%llu,\"scan_run\":%u,\"table_ms\":%.3f,\"scan_ms\":%.3f,\"gather_ms\":%.3f,\"total_ms\":%.3f}\n",
                k, counter_bytes, n_contigs, static_cast<unsigned long long>(n_bases), q.n, static_cast<unsigned long long>(st.n_query_kmers),
                static_cast<unsigned long long>(st.n_distinct), static_cast<unsigned long long>(st.table_slots),
                static_cast<unsigned long long>(st.n_scanned), static_cast<unsigned long long>(st.n_hits), st.scan_run, st.table_ms, st.scan_ms,
                st.gather_ms, st.total_ms);
    lcty_genome_destroy(genome);
    lcty_ctx_destroy(ctx);
    return 0;
}
