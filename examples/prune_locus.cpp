// examples/prune_locus.cpp — `locityper prune` for one locus (process_locus + prune_files, src/command/prune.rs:471-582) through the C ABI,
// a locus directory in, a pruned locus directory out:
//
//   <locus_dir>   DB/loci/<locus>/ with
//        haplotypes.fa.gz                     the haplotypes of the locus                       (lcty_fasta_read)
//        haplotypes.paf[.br|.gz]              their pairwise alignments with dv tags            (lcty_io_read_file)
//        kmers.bin.br | kmers.bin.lz4         both KmerCounts blocks            [optional]
//        distances.bin                                                           [optional]
//        discarded_haplotypes.txt                                                [optional]
//   -> <out_dir>/{haplotypes.fa.gz, kmers.bin.br, distances.bin, haplotypes.paf.br, discarded_haplotypes.txt, all_haplotypes.nwk.gz}
//                                                                                               (lcty_db_prune_locus, lcty_io_write_gz / _br)
//      when no haplotype is discarded the input files are copied as they are (copy_output_files, prune.rs:430-451)
//   [-t THRESHOLD] [-n N_CLUSTERS] [--power min|max|INT] [-f|--field STR] [--skip-tree]
//   [--only-tree: writes <locus_dir>/all_haplotypes.nwk.gz and stops; no <out_dir>]
//
// Prints one JSON line with the counts and the per-stage milliseconds. Build: see tests/test_gpu_prune_example.py.
#include <sys/stat.h>

#include <cmath>
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

static bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

struct Blob {
    uint8_t* p = nullptr; uint64_t n = 0;
    ~Blob() { lcty_io_free(p); }
    void read(const std::string& path) { ok(lcty_io_read_file(path.c_str(), &p, &n), path.c_str()); }
};

static void copy_file(const std::string& from, const std::string& to) {
    std::ifstream in(from, std::ios::binary);
    std::ofstream out(to, std::ios::binary);
    out << in.rdbuf();
    if (!in || !out) { std::fprintf(stderr, "cannot copy %s to %s\n", from.c_str(), to.c_str()); std::exit(1); }
}

static void write_plain(const std::string& path, const uint8_t* p, uint64_t n) {
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n));
    if (!out) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
}

int main(int argc, char** argv) {
    lcty_prune_params prm;
    lcty_prune_params_default(&prm);
    std::string dir, out_dir, field = "dv";
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if ((a == "-t" || a == "--threshold") && i + 1 < argc) prm.threshold = std::atof(argv[++i]);
        else if ((a == "-n" || a == "--n-clusters") && i + 1 < argc) prm.n_clusters = static_cast<uint32_t>(std::strtoul(argv[++i], nullptr, 10));
        else if (a == "--power" && i + 1 < argc) {
            const std::string v = argv[++i];
            if (v == "min" || v == "-inf") prm.power = LCTY_PRUNE_POWER_MIN;
            else if (v == "max" || v == "inf") prm.power = LCTY_PRUNE_POWER_MAX;
            else prm.power = v == "geom" ? 0 : std::atoi(v.c_str());
        }
        else if ((a == "-f" || a == "--field") && i + 1 < argc) field = argv[++i];
        else if (a == "--only-tree") prm.only_tree = 1;
        else if (a == "--skip-tree") prm.skip_tree = 1;
        else if (dir.empty()) dir = a;
        else if (out_dir.empty()) out_dir = a;
        else { dir.clear(); break; }
    }
    if (dir.empty() || (out_dir.empty() && !prm.only_tree)) {
        std::fprintf(stderr, "usage: prune_locus <locus_dir> <out_dir> [-t THRESHOLD] [-n N_CLUSTERS] [--power min|max|INT] [-f FIELD] [--skip-tree]\n"
                             "       prune_locus <locus_dir> --only-tree [...]\n");
        return 2;
    }
    // the haplotypes
    const std::string fa = dir + "/haplotypes.fa.gz";
    uint32_t n = 0; uint64_t nl = 0, sl = 0;
    ok(lcty_fasta_read(fa.c_str(), &n, nullptr, &nl, nullptr, &sl, nullptr), fa.c_str());
    std::vector<char> names(nl + 1); std::vector<uint8_t> seqs(sl + 1); std::vector<uint64_t> off(n + 1);
    ok(lcty_fasta_read(fa.c_str(), &n, names.data(), &nl, seqs.data(), &sl, off.data()), fa.c_str());
    // the alignments (LOCUS_PAFS: the first that exists), the k-mer counts, the distances, the old discarded haplotypes
    std::string paf_path, kmers_path;
    for (const char* ext : {".br", ".gz", ""}) if (paf_path.empty() && exists(dir + "/haplotypes.paf" + ext)) paf_path = dir + "/haplotypes.paf" + ext;
    if (paf_path.empty()) { std::fprintf(stderr, "Could not find haplotype alignments at %s/haplotypes.paf*\n", dir.c_str()); return 1; }
    for (const char* ext : {".br", ".lz4"}) if (kmers_path.empty() && exists(dir + "/kmers.bin" + ext)) kmers_path = dir + "/kmers.bin" + ext;
    const std::string dist_path = dir + "/distances.bin", disc_path = dir + "/discarded_haplotypes.txt";
    Blob paf, kmers, dists, disc;
    paf.read(paf_path);
    if (!prm.only_tree && !kmers_path.empty()) kmers.read(kmers_path);
    if (!prm.only_tree && exists(dist_path)) dists.read(dist_path);
    const bool have_disc = exists(disc_path);
    if (have_disc) disc.read(disc_path);

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_prune_files f;
    ok(lcty_db_prune_locus(ctx, n, names.data(), seqs.data(), off.data(), paf.p, paf.n, kmers.p, kmers.n, dists.p, dists.n,
                           have_disc ? reinterpret_cast<const char*>(disc.p) : nullptr, disc.n, field.c_str(), &prm, &f), "process_locus");
    lcty_ctx_destroy(ctx);

    if (!prm.skip_tree) {
        const std::string nwk = (prm.only_tree ? dir : out_dir) + "/all_haplotypes.nwk.gz";
        if (!prm.only_tree) mkdir(out_dir.c_str(), 0777);
        ok(lcty_io_write_gz(nwk.c_str(), f.newick, f.newick_len), nwk.c_str());
    }
    int32_t stored = 0;
    if (!prm.only_tree) {
        mkdir(out_dir.c_str(), 0777);
        if (f.discarded_len) write_plain(out_dir + "/discarded_haplotypes.txt", f.discarded, f.discarded_len);
        if (f.unchanged) {
            copy_file(fa, out_dir + "/haplotypes.fa.gz");
            for (const char* base : {"kmers.bin.br", "kmers.bin.lz4", "distances.bin", "haplotypes.paf.br", "haplotypes.paf.gz", "haplotypes.paf"})
                if (exists(dir + "/" + base)) copy_file(dir + "/" + base, out_dir + "/" + base);
        } else {
            ok(lcty_io_write_gz((out_dir + "/haplotypes.fa.gz").c_str(), f.fasta, f.fasta_len), "haplotypes.fa.gz");
            if (f.kmers_len) ok(lcty_io_write_br((out_dir + "/kmers.bin.br").c_str(), f.kmers, f.kmers_len, 5, &stored), "kmers.bin.br");
            if (f.distances_len) write_plain(out_dir + "/distances.bin", f.distances, f.distances_len);
            ok(lcty_io_write_br((out_dir + "/haplotypes.paf.br").c_str(), f.paf, f.paf_len, 5, &stored), "haplotypes.paf.br");
        }
    }
    std::printf("{\"haplotypes\": %u, \"kept\": %u, \"keep\": [", n, f.n_keep);
    for (uint32_t t = 0; t < f.n_keep; t++) std::printf("%s%u", t ? ", " : "", f.keep[t]);
    if (std::isfinite(f.threshold)) std::printf("], \"threshold\": %.17g", f.threshold); else std::printf("], \"threshold\": null");
    std::printf(", \"unchanged\": %s, \"warn_bits\": %u, \"missing\": %llu, \"negative\": %llu, \"conflicting\": %llu, "
                "\"rescans\": %llu, \"rep_pairs\": %llu, \"build_ms\": %.3f, \"merge_ms\": %.3f, \"repr_ms\": %.3f, \"host_ms\": %.3f, \"total_ms\": %.3f}\n",
                f.unchanged ? "true" : "false", f.warn_bits, static_cast<unsigned long long>(f.div.n_missing),
                static_cast<unsigned long long>(f.div.n_negative), static_cast<unsigned long long>(f.div.n_conflicting),
                static_cast<unsigned long long>(f.stats.n_rescans), static_cast<unsigned long long>(f.stats.n_rep_pairs), f.stats.build_ms,
                f.stats.merge_ms, f.stats.repr_ms, f.stats.host_ms, f.stats.total_ms);
    lcty_prune_files_free(&f);
    return 0;
}
