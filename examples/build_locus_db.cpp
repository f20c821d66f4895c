// examples/build_locus_db.cpp — the database files of one locus (`locityper target`, process_alleles: src/command/add.rs:585-652)
// through the C ABI, files in, files out:
//
//   <haplotypes.fa[.gz]>   the haplotype sequences of the locus                                   (lcty_fasta_read)
//   <ref.fa[.gz]>          the reference sequence of the locus, one record (N runs allowed)
//   <counts.bin[.br|.lz4]> what `jellyfish query` returned for them, as ONE KmerCounts block (src/seq/counts.rs:108-124) of
//                          n_haplotypes + 1 contigs, the reference sequence last (the order of add.rs:633-636)
//                                                                                                  (lcty_io_read_file, lcty_kmer_counts_parse)
//   <db_dir> <locus>       -> <db_dir>/loci/<locus>/
//        haplotypes.fa.gz            identical haplotypes folded (discard_identical)              (lcty_io_write_gz)
//        kmers.bin.br                off-target counts, then the counts as given                  (lcty_io_write_br)
//        distances.bin               with --calc-div: non-shared minimizers of every pair
//        discarded_haplotypes.txt    only when something was discarded
//   [--calc-div] [--div-k K] [--div-w W] [--only-seqs]
//
// Build: see tests/test_gpu_db_example.py.
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

struct Fasta { uint32_t n = 0; std::vector<char> names; std::vector<uint8_t> seqs; std::vector<uint64_t> off; };
static Fasta read_fasta(const std::string& path) {
    Fasta f; uint64_t nl = 0, sl = 0;
    ok(lcty_fasta_read(path.c_str(), &f.n, nullptr, &nl, nullptr, &sl, nullptr), path.c_str());
    f.names.resize(nl + 1); f.seqs.resize(sl + 1); f.off.resize(f.n + 1);
    ok(lcty_fasta_read(path.c_str(), &f.n, f.names.data(), &nl, f.seqs.data(), &sl, f.off.data()), path.c_str());
    return f;
}

static void write_plain(const std::string& path, const uint8_t* data, uint64_t len) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, 1, len, f) != len || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
}

int main(int argc, char** argv) {
    std::vector<std::string> pos;
    lcty_db_params prm;
    lcty_db_params_default(&prm);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--calc-div") prm.calc_div = 1;
        else if (a == "--only-seqs") prm.only_seqs = 1;
        else if (a == "--div-k" && i + 1 < argc) prm.div_k = static_cast<uint32_t>(std::atoi(argv[++i]));
        else if (a == "--div-w" && i + 1 < argc) prm.div_w = static_cast<uint32_t>(std::atoi(argv[++i]));
        else pos.push_back(a);
    }
    if (pos.size() != 5) {
        std::fprintf(stderr, "usage: build_locus_db <haplotypes.fa> <ref.fa> <counts.bin> <db_dir> <locus> [--calc-div] [--div-k K] [--div-w W] [--only-seqs]\n");
        return 2;
    }
    const Fasta haps = read_fasta(pos[0]), ref = read_fasta(pos[1]);
    if (ref.n != 1) { std::fprintf(stderr, "%s: one sequence expected, %u found\n", pos[1].c_str(), ref.n); return 1; }

    uint8_t* raw = nullptr; uint64_t raw_len = 0;
    uint32_t k = 0, n_contigs = 0, counter_bytes = 2; uint64_t used = 0;
    std::vector<uint64_t> cnt_off; std::vector<uint16_t> counts;
    if (!prm.only_seqs) {
        ok(lcty_io_read_file(pos[2].c_str(), &raw, &raw_len), pos[2].c_str());
        ok(lcty_kmer_counts_parse(raw, raw_len, &k, &n_contigs, nullptr, 0, nullptr, 0, &used), "KmerCounts::load (size)");
        if (n_contigs != haps.n + 1) { std::fprintf(stderr, "%s: %u contigs, %u haplotypes + the reference expected\n", pos[2].c_str(), n_contigs, haps.n); return 1; }
        counter_bytes = raw[1];
        cnt_off.resize(n_contigs + 1); counts.resize(used + 1);
        ok(lcty_kmer_counts_parse(raw, raw_len, &k, &n_contigs, cnt_off.data(), n_contigs, counts.data(), counts.size(), &used), "KmerCounts::load");
        lcty_io_free(raw);
    }

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_db_files files;
    ok(lcty_db_build_locus(ctx, haps.n, haps.names.data(), haps.seqs.data(), haps.off.data(), ref.seqs.data(), ref.off[1],
                           prm.only_seqs ? nullptr : counts.data(), prm.only_seqs ? nullptr : cnt_off.data(), k, counter_bytes, &prm, &files),
       "process_alleles");
    lcty_ctx_destroy(ctx);

    const std::string loci = pos[3] + "/loci", dir = loci + "/" + pos[4];
    mkdir(pos[3].c_str(), 0755); mkdir(loci.c_str(), 0755); mkdir(dir.c_str(), 0755);
    ok(lcty_io_write_gz((dir + "/haplotypes.fa.gz").c_str(), files.fasta, files.fasta_len), "haplotypes.fa.gz");
    if (files.kmers_len) ok(lcty_io_write_br((dir + "/kmers.bin.br").c_str(), files.kmers, files.kmers_len, 5, nullptr), "kmers.bin.br");
    if (files.distances_len) write_plain(dir + "/distances.bin", files.distances, files.distances_len);
    if (files.discarded_len) write_plain(dir + "/discarded_haplotypes.txt", files.discarded, files.discarded_len);
    std::printf("%u of %u haplotypes kept", files.n_kept, haps.n);
    if (prm.calc_div) std::printf(", %llu pairs with divergence >= 0.2 (highest %.5f)", static_cast<unsigned long long>(files.check.n_high), files.check.highest);
    if (files.warn_bits & LCTY_DB_WARN_REF_MISMATCH) std::printf(", WARNING: the reference sequence does not match the k-mer counts");
    std::printf("\n");
    lcty_db_files_free(&files);
    return 0;
}
