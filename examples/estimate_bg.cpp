// examples/estimate_bg.cpp — the background distributions of a sample (PREPROC/distr.gz) through the C ABI, files in, files out:
//
//   <bg.bam>                   the sample's alignments over the background region (a slice of its BAM: `samtools view -b in.bam
//                              chr:start-end`), read sequentially                           (lcty_bg_reads_load)
//   <padded.fa>                the reference sequence of the region +- 50 kb (BgRegion::new, src/command/preproc.rs:1357-1385),
//                              one record                                                   (lcty_fasta_read)
//   <padded_kmer_counts.u16>   little-endian u16 counts of every k-mer of that sequence (`jellyfish query` on it; k follows from
//                              the number of counts)
//   <chr:start-end>            the background interval, 1-based inclusive as samtools writes it
//   <tech>                     illumina | hifi | pacbio | ont
//   --fetch [index_path]       optional, last: <bg.bam> is the sample's whole, coordinate-sorted BAM file with its BAI index
//                              (<bg.bam>.bai unless given) and the region's records are read through the index
//                                                                                           (lcty_sample_bam_open, lcty_bg_reads_fetch)
//        -> lcty_bg_estimate (estimate_bg_distrs with `-a`, preproc.rs:1157-1192) -> lcty_bg_to_json
//   <out_dir>/distr.gz         BgDistr as JSON                                              (lcty_io_write_gz)
//
// Build: see tests/test_gpu_bg_example.py.
//   ./estimate_bg <bg.bam> <padded.fa> <padded_kmer_counts.u16> <chr:start-end> <tech> <out_dir> [--fetch [index_path]]
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

int main(int argc, char** argv) {
    const bool fetch = argc >= 8 && std::strcmp(argv[7], "--fetch") == 0;
    if (!(argc == 7 || (fetch && argc <= 9))) {
        std::fprintf(stderr, "usage: estimate_bg <bg.bam> <padded.fa> <padded_kmer_counts.u16> <chr:start-end> <tech> <out_dir> [--fetch [index_path]]\n");
        return 2;
    }
    const char* index_path = argc == 9 ? argv[8] : nullptr;
    const std::string bam = argv[1], fa = argv[2], counts_path = argv[3], region = argv[4], tech = argv[5], out_dir = argv[6];

    // chr:start-end (1-based, inclusive) -> [start, end); the padded interval as Interval::add_padding clips it at 0
    const size_t colon = region.rfind(':'), dash = region.rfind('-');
    if (colon == std::string::npos || dash == std::string::npos || dash < colon) { std::fprintf(stderr, "bad region %s\n", region.c_str()); return 2; }
    const std::string contig = region.substr(0, colon);
    const uint32_t start = static_cast<uint32_t>(std::strtoul(region.c_str() + colon + 1, nullptr, 10)) - 1;
    const uint32_t end = static_cast<uint32_t>(std::strtoul(region.c_str() + dash + 1, nullptr, 10));
    const uint32_t padded_start = start > 50000 ? start - 50000 : 0;

    lcty_bg_params params;
    lcty_bg_params_default(&params);
    if (tech == "illumina" || tech == "sr") params.technology = LCTY_TECH_ILLUMINA;
    else if (tech == "hifi") params.technology = LCTY_TECH_HIFI;
    else if (tech == "pacbio" || tech == "pb") params.technology = LCTY_TECH_PACBIO;
    else if (tech == "ont" || tech == "nanopore") params.technology = LCTY_TECH_NANOPORE;
    else { std::fprintf(stderr, "unknown technology %s\n", tech.c_str()); return 2; }

    // the padded reference sequence
    uint32_t n_seqs = 0; uint64_t names_len = 0, seqs_len = 0;
    ok(lcty_fasta_read(fa.c_str(), &n_seqs, nullptr, &names_len, nullptr, &seqs_len, nullptr), "padded FASTA");
    if (n_seqs != 1) { std::fprintf(stderr, "%s: one sequence expected, %u found\n", fa.c_str(), n_seqs); return 1; }
    std::vector<char> names(names_len); std::vector<uint8_t> seq(seqs_len); std::vector<uint64_t> seq_off(2);
    ok(lcty_fasta_read(fa.c_str(), &n_seqs, names.data(), &names_len, seq.data(), &seqs_len, seq_off.data()), "padded FASTA");
    const uint32_t padded_len = static_cast<uint32_t>(seq_off[1]);

    // k-mer counts of the padded sequence
    FILE* f = std::fopen(counts_path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", counts_path.c_str()); return 1; }
    std::vector<uint16_t> counts;
    uint16_t chunk[4096]; size_t got;
    while ((got = std::fread(chunk, 2, 4096, f)) > 0) counts.insert(counts.end(), chunk, chunk + got);
    std::fclose(f);
    if (counts.empty() || counts.size() > padded_len) { std::fprintf(stderr, "%s: %zu counts for %u bases\n", counts_path.c_str(), counts.size(), padded_len); return 1; }
    const uint32_t k = padded_len + 1 - static_cast<uint32_t>(counts.size());

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_bg_reads* reads = nullptr;
    if (fetch) {
        lcty_sample_bam* sample = nullptr;
        lcty_sample_bam_stats st;
        ok(lcty_sample_bam_open(bam.c_str(), index_path, &sample), "lcty_sample_bam_open");
        ok(lcty_bg_reads_fetch(ctx, sample, contig.c_str(), start, end, padded_start, padded_len, &params, &reads, &st), "fetch + load_alns");
        lcty_sample_bam_close(sample);
        std::printf("fetched %llu of %llu bytes, %llu records walked, %llu kept\n", static_cast<unsigned long long>(st.bytes_read),
                    static_cast<unsigned long long>(st.file_bytes), static_cast<unsigned long long>(st.records_walked),
                    static_cast<unsigned long long>(st.records_kept));
    } else
        ok(lcty_bg_reads_load(bam.c_str(), contig.c_str(), start, end, padded_start, padded_len, &params, &reads), "load_alns");
    lcty_bg bg; double read_len = 0;
    ok(lcty_bg_estimate(ctx, reads, seq.data(), padded_start, padded_len, counts.data(), k, start, end, &params, &bg, &read_len, nullptr),
       "estimate_bg_distrs");
    lcty_bg_reads_free(reads);
    lcty_ctx_destroy(ctx);

    uint64_t need = 0;
    ok(lcty_bg_to_json(&bg, read_len, params.ploidy, nullptr, 0, &need), "BgDistr::save (size)");
    std::vector<char> text(need);
    ok(lcty_bg_to_json(&bg, read_len, params.ploidy, text.data(), need, &need), "BgDistr::save");
    mkdir(out_dir.c_str(), 0755);
    ok(lcty_io_write_gz((out_dir + "/distr.gz").c_str(), reinterpret_cast<const uint8_t*>(text.data()), need - 1), "distr.gz");
    std::printf("read length %.2f, window %u, insert %s, distr.gz written\n", read_len, bg.window, bg.is_paired ? "paired" : "none");
    return 0;
}
