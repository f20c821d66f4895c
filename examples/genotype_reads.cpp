// examples/genotype_reads.cpp — a sample's reads in, the genotype of every locus out, through the C ABI, with no reads.fq and no aln.bam
// in between:
//
//   R1 [R2] | sample.bam + index                 the sample's reads (lcty_fastx_device_open | lcty_sample_bam_open + lcty_sample_bam_fetch)
//   a.bam [b.bam ...] --no-index [-^]            the same from whole BAM files without an index, read front to back in windows
//                                                (lcty_bam_stream_open, lcty_bam_stream_next; -^: name-grouped pairs)
//   PREPROC/distr.gz                             background distributions         (lcty_io_read_file + lcty_bg_from_json)
//   <locus dir>/haplotypes.fa.gz                 alleles                          (lcty_fasta_read)
//   <locus dir>/kmers.bin.lz4 | .br              off-target k-mer counts          (lcty_io_read_file + lcty_kmer_counts_parse)
//   <locus dir>/ref.bed                          -a: where the locus lies         (-> lcty_recruit_fetch_regions)
//   <locus dir>/haplotypes-basis.fa.gz           --basis: the alleles the mapper sees
//   <locus dir>/haplotypes.paf[.gz]              optional: pairwise haplotype alignments (lcty_locus_set_hap_alns + lcty_recover_alignments)
//        -> lcty_targets_*, chunk by chunk recruitment and lcty_recruited_add_fastx | _add_sample; per locus lcty_locus_create,
//           lcty_locus_build_map_index, lcty_reads_map_append_recruited in parts of --map-chunk pairs, lcty_score_reads; then the loci
//           back to back through lcty_solve
//   OUTDIR/loci/<locus>/res.json.gz              the genotype call, as genotype_dir.cpp writes it
//   OUTDIR/loci/<locus>/alns/00.bam (+ .bai)     --out-bam: read placements on the call, named from the set's kept names
//
// This is `locityper genotype` from recruit_to_targets to the output files (command/genotype.rs:872-1260) with the seam of reads.fq ->
// external mapper -> aln.bam closed. The loci are solved with lcty_solve, one after the other: lcty_solve_queue gives the same calls
// entry by entry but does not hand out the per-genotype likelihoods res.json.gz holds. No lock or success files, no subsampling, no
// CRAM. Prints one JSON line of stats. Build: see tests/test_gpu_genotype_reads_example.py.
//   ./genotype_reads -i R1 [R2] [--interleaved] | -a sample.bam [-x index] | -a a.bam [-a b.bam ...] --no-index [-^] -p PREPROC/distr.gz -d DB/loci/<locus> [-d ...] [--basis]
//                    [--chunk N] [--map-chunk N] [--seed S] [--out-bam] [--padding N] [--alt-contig N] -o OUTDIR
#include <sys/stat.h>

#include <chrono>
#include <cmath>
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
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Locus {
    std::string dir, name;
    uint32_t A = 0, k = 0;
    std::vector<char> name_blob; std::vector<const char*> names;
    std::vector<uint8_t> seqs; std::vector<uint64_t> seq_off, cnt_off; std::vector<uint16_t> counts;
    std::vector<uint16_t> basis;
    lcty_locus* loc = nullptr; lcty_reads* reads = nullptr;
    std::vector<uint32_t> dist; bool edit_distances = false;
    uint64_t n_pairs = 0;
};

static void load_locus(Locus& L, bool use_basis) {
    const std::string fa = L.dir + "/haplotypes.fa.gz";
    uint64_t names_len = 0, seqs_len = 0;
    ok(lcty_fasta_read(fa.c_str(), &L.A, nullptr, &names_len, nullptr, &seqs_len, nullptr), "haplotypes.fa.gz");
    L.name_blob.resize(names_len); L.seqs.resize(seqs_len); L.seq_off.resize(L.A + 1);
    ok(lcty_fasta_read(fa.c_str(), &L.A, L.name_blob.data(), &names_len, L.seqs.data(), &seqs_len, L.seq_off.data()), "haplotypes.fa.gz");
    for (uint64_t i = 0, n = 0; n < L.A; n++) { L.names.push_back(&L.name_blob[i]); while (L.name_blob[i]) i++; i++; }
    const std::string kp = exists(L.dir + "/kmers.bin.lz4") ? L.dir + "/kmers.bin.lz4" : L.dir + "/kmers.bin.br";
    uint8_t* buf = nullptr; uint64_t len = 0;
    ok(lcty_io_read_file(kp.c_str(), &buf, &len), "kmers.bin");
    uint32_t n_c = 0; uint64_t consumed = 0;
    ok(lcty_kmer_counts_parse(buf, len, &L.k, &n_c, nullptr, 0, nullptr, 0, &consumed), "KmerCounts::load (sizes)");
    if (n_c != L.A) { std::fprintf(stderr, "kmers.bin has %u contigs, the FASTA %u\n", n_c, L.A); std::exit(1); }
    L.cnt_off.resize(L.A + 1);
    uint64_t n_counts = 0;
    for (uint32_t a = 0; a < L.A; a++) n_counts += L.seq_off[a + 1] - L.seq_off[a] + 1 - L.k;
    L.counts.resize(n_counts);
    ok(lcty_kmer_counts_parse(buf, len, &L.k, &n_c, L.cnt_off.data(), L.A, L.counts.data(), n_counts, &consumed), "KmerCounts::load");
    lcty_io_free(buf);
    // the alleles the mapper sees: all of them, or those named in haplotypes-basis.fa.gz (genotype.rs:1007-1052)
    const std::string bfa = L.dir + "/haplotypes-basis.fa.gz";
    if (use_basis && exists(bfa)) {
        uint32_t B = 0; uint64_t bn = 0, bs = 0;
        ok(lcty_fasta_read(bfa.c_str(), &B, nullptr, &bn, nullptr, &bs, nullptr), "haplotypes-basis.fa.gz");
        std::vector<char> blob(bn); std::vector<uint8_t> s(bs); std::vector<uint64_t> so(B + 1);
        ok(lcty_fasta_read(bfa.c_str(), &B, blob.data(), &bn, s.data(), &bs, so.data()), "haplotypes-basis.fa.gz");
        for (uint64_t i = 0, n = 0; n < B; n++) {
            const char* nm = &blob[i];
            uint32_t a = 0;
            while (a < L.A && std::strcmp(L.names[a], nm)) a++;
            if (a == L.A) { std::fprintf(stderr, "basis haplotype %s is not an allele of %s\n", nm, L.name.c_str()); std::exit(1); }
            L.basis.push_back(static_cast<uint16_t>(a));
            while (blob[i]) i++;
            i++;
        }
    } else for (uint32_t a = 0; a < L.A; a++) L.basis.push_back(static_cast<uint16_t>(a));
}

int main(int argc, char** argv) {
    std::string bam_path, index_path, distr, outdir;
    std::vector<std::string> inputs, dirs, bam_paths;
    int interleaved = 0; bool use_basis = false, out_bam = false, no_index = false;
    uint64_t chunk = 1u << 20, map_chunk = 1u << 16, seed = 1;
    uint32_t padding = 1000, alt_contig = 10000000;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "-i") { inputs.push_back(next()); if (i + 1 < argc && argv[i + 1][0] != '-') inputs.push_back(argv[++i]); }
        else if (a == "--interleaved" || a == "-^") interleaved = 1;
        else if (a == "-a") { bam_path = next(); bam_paths.push_back(bam_path); }
        else if (a == "--no-index") no_index = true;
        else if (a == "-x") index_path = next();
        else if (a == "-p") distr = next();
        else if (a == "-d") dirs.push_back(next());
        else if (a == "--basis") use_basis = true;
        else if (a == "--chunk") chunk = std::strtoull(next(), nullptr, 10);
        else if (a == "--map-chunk") map_chunk = std::strtoull(next(), nullptr, 10);
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--out-bam") out_bam = true;
        else if (a == "--padding") padding = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--alt-contig") alt_contig = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "-o") outdir = next();
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if ((inputs.empty() == bam_path.empty()) || inputs.size() > 2 || (!no_index && bam_paths.size() > 1) || (no_index && bam_path.empty()) || distr.empty() || dirs.empty() || outdir.empty() || !chunk || !map_chunk) {
        std::fprintf(stderr, "usage: genotype_reads -i R1 [R2] [--interleaved] | -a sample.bam [-x index] | -a a.bam [-a b.bam ...] --no-index [-^] -p PREPROC/distr.gz -d DB/loci/<locus> [-d ...] [--basis] "
                             "[--chunk N] [--map-chunk N] [--seed S] [--out-bam] [--padding N] [--alt-contig N] -o OUTDIR\n");
        return 2;
    }
    const double t_start = now_ms();
    double ms_parse = 0, ms_recruit = 0, ms_scatter = 0, ms_map = 0, ms_score = 0, ms_solve = 0;

    uint8_t* buf = nullptr; uint64_t len = 0;
    ok(lcty_io_read_file(distr.c_str(), &buf, &len), "distr.gz");
    lcty_bg bg; double read_len = 0;
    ok(lcty_bg_from_json(reinterpret_cast<const char*>(buf), len, &bg, &read_len), "BgDistr::load");
    lcty_io_free(buf);
    if (no_index && (interleaved != 0) != (bg.is_paired != 0)) {
        std::fprintf(stderr, "%s: distr.gz was made from %s reads\n", interleaved ? "-^ reads pairs" : "without -^ every record is a read", bg.is_paired ? "paired" : "single-end");
        return 2;
    }

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_recruit_params rp;
    ok(lcty_recruit_params_default(&rp, bg.technology, bg.is_paired), "lcty_recruit_params_default");
    lcty_targets* targets = nullptr;
    ok(lcty_targets_create(ctx, &rp, &targets), "lcty_targets_create");

    // ---- the loci
    std::vector<Locus> loci(dirs.size());
    mkdir(outdir.c_str(), 0777); mkdir((outdir + "/loci").c_str(), 0777);
    for (size_t l = 0; l < dirs.size(); l++) {
        Locus& L = loci[l];
        L.dir = dirs[l];
        while (!L.dir.empty() && L.dir.back() == '/') L.dir.pop_back();
        L.name = L.dir.substr(L.dir.find_last_of('/') + 1);
        load_locus(L, use_basis);
        ok(lcty_targets_add_locus(targets, L.A, L.seqs.data(), L.seq_off.data(), L.counts.data(), L.cnt_off.data(), L.k, nullptr), "lcty_targets_add_locus");
        mkdir((outdir + "/loci/" + L.name).c_str(), 0777);
    }
    ok(lcty_targets_finalize(targets, nullptr), "lcty_targets_finalize");
    lcty_recruited* set = nullptr;
    ok(lcty_recruited_create(targets, out_bam, &set), "lcty_recruited_create");

    // ---- the sample's reads: recruited chunk by chunk, kept on the device
    const uint32_t max_out = 8;
    std::vector<uint32_t> cnt, out_loci;
    uint64_t n_reads = 0;
    if (!inputs.empty()) {
        lcty_fastx_device* f = nullptr;
        ok(lcty_fastx_device_open(ctx, inputs[0].c_str(), inputs.size() > 1 ? inputs[1].c_str() : nullptr, interleaved, &f), "lcty_fastx_device_open");
        lcty_fastx_device_stats st;
        std::memset(&st, 0, sizeof(st));
        for (;;) {
            uint64_t n = 0;
            ok(lcty_fastx_device_next(f, chunk, &n, &st), "lcty_fastx_device_next");
            if (!n) break;
            cnt.assign(n, 0); out_loci.assign(n * max_out, 0);
            double t0 = now_ms();
            ok(lcty_fastx_device_recruit(targets, f, max_out, cnt.data(), out_loci.data()), "lcty_fastx_device_recruit");
            ms_recruit += now_ms() - t0; t0 = now_ms();
            ok(lcty_recruited_add_fastx(set, f, max_out, cnt.data(), out_loci.data()), "lcty_recruited_add_fastx");
            ms_scatter += now_ms() - t0;
            n_reads += n;
        }
        ms_parse = st.ms_total;
        lcty_fastx_device_close(f);
    } else if (no_index) {
        std::vector<const char*> paths;
        for (const std::string& p : bam_paths) paths.push_back(p.c_str());
        lcty_bam_stream* stream = nullptr;
        ok(lcty_bam_stream_open(ctx, paths.data(), static_cast<uint32_t>(paths.size()), interleaved, &stream), "lcty_bam_stream_open");
        lcty_bam_stream_stats st;
        std::memset(&st, 0, sizeof(st));
        for (;;) {
            lcty_sample_reads* sr = nullptr;                                    // belongs to the stream: never freed here
            uint64_t n = 0;
            ok(lcty_bam_stream_next(stream, &sr, &n, &st), "lcty_bam_stream_next");
            if (!n) break;
            cnt.assign(n, 0); out_loci.assign(n * max_out, 0);
            double t0 = now_ms();
            ok(lcty_sample_reads_recruit(targets, sr, max_out, cnt.data(), out_loci.data()), "lcty_sample_reads_recruit");
            ms_recruit += now_ms() - t0; t0 = now_ms();
            ok(lcty_recruited_add_sample(set, sr, max_out, cnt.data(), out_loci.data()), "lcty_recruited_add_sample");
            ms_scatter += now_ms() - t0;
            n_reads += n;
        }
        ms_parse = st.ms_total;
        lcty_bam_stream_close(stream);
    } else {
        lcty_sample_bam* bam = nullptr;
        ok(lcty_sample_bam_open(bam_path.c_str(), index_path.empty() ? nullptr : index_path.c_str(), &bam), "lcty_sample_bam_open");
        uint32_t n_contigs = 0; const char* cnames = nullptr; const uint64_t* cname_off = nullptr; const uint32_t* clen = nullptr;
        ok(lcty_sample_bam_contigs(bam, &n_contigs, &cnames, &cname_off, &clen), "lcty_sample_bam_contigs");
        std::vector<uint32_t> tid, start, end;
        for (const Locus& L : loci) {                                           // load_recr_targets / Interval::parse_bed (genotype.rs:799-820)
            std::ifstream in(L.dir + "/ref.bed");
            if (!in) { std::fprintf(stderr, "cannot open %s/ref.bed\n", L.dir.c_str()); return 1; }
            std::string line;
            while (std::getline(in, line)) {
                std::istringstream ls(line);
                std::string chrom; uint64_t s = 0, e = 0;
                if (!(ls >> chrom >> s >> e)) continue;
                uint32_t t = 0;
                while (t < n_contigs && chrom != cnames + cname_off[t]) t++;
                if (t == n_contigs) { std::fprintf(stderr, "unknown contig %s in %s/ref.bed\n", chrom.c_str(), L.dir.c_str()); continue; }
                tid.push_back(t); start.push_back(static_cast<uint32_t>(s)); end.push_back(static_cast<uint32_t>(e));
            }
        }
        std::vector<uint32_t> rt(tid.size() + n_contigs), rs(rt.size()), re(rt.size());
        uint32_t n_regions = 0;
        ok(lcty_recruit_fetch_regions(static_cast<uint32_t>(tid.size()), tid.data(), start.data(), end.data(), n_contigs, clen, padding, alt_contig, 1000,
                                      rt.data(), rs.data(), re.data(), &n_regions), "lcty_recruit_fetch_regions");
        lcty_sample_reads* sr = nullptr;
        lcty_sample_bam_stats st;
        ok(lcty_sample_bam_fetch(ctx, bam, n_regions, rt.data(), rs.data(), re.data(), 1, 0, bg.is_paired, &sr, &st), "lcty_sample_bam_fetch");
        ms_parse = st.ms_total;
        n_reads = st.n_pairs;
        cnt.assign(n_reads + 1, 0); out_loci.assign((n_reads + 1) * max_out, 0);
        double t0 = now_ms();
        ok(lcty_sample_reads_recruit(targets, sr, max_out, cnt.data(), out_loci.data()), "lcty_sample_reads_recruit");
        ms_recruit += now_ms() - t0; t0 = now_ms();
        ok(lcty_recruited_add_sample(set, sr, max_out, cnt.data(), out_loci.data()), "lcty_recruited_add_sample");
        ms_scatter += now_ms() - t0;
        lcty_sample_reads_free(sr);
        lcty_sample_bam_close(bam);
    }

    // ---- per locus: the locus, its map index, the batch mapped from the set, recovery, scores
    lcty_map_params mp;
    ok(bg.technology == LCTY_TECH_ILLUMINA ? lcty_map_params_default(&mp) : lcty_map_params_default_long(&mp), "lcty_map_params_default");
    uint64_t bytes_resident = 0;
    std::string recruited_json;
    for (size_t l = 0; l < loci.size(); l++) {
        Locus& L = loci[l];
        uint64_t n_bases = 0;
        ok(lcty_recruited_sizes(set, static_cast<uint32_t>(l), &L.n_pairs, &n_bases), "lcty_recruited_sizes");
        bytes_resident += n_bases / 32 * 12 + L.n_pairs * 32;
        recruited_json += (l ? ", " : "") + std::to_string(L.n_pairs);
        lcty_params prm;
        lcty_params_default(&prm);
        prm.strict_subset = L.basis.size() < L.A;                               // locs.rs:486
        ok(lcty_params_resolve(&prm, &bg), "params");
        ok(lcty_locus_create(ctx, L.A, L.seqs.data(), L.seq_off.data(), L.counts.data(), L.cnt_off.data(), L.k, &bg, &prm, &L.loc), "lcty_locus_create");
        ok(lcty_locus_build_map_index(L.loc, L.basis.data(), static_cast<uint32_t>(L.basis.size()), mp.k), "lcty_locus_build_map_index");
        // The records and CIGAR words of a locus are known once it is mapped: the batch is made with room for a few records per read
        // end and made again with four times as much when the mapper's records outgrow it.
        double t0 = now_ms();
        uint64_t cap_recs = 8 * L.n_pairs + 64, cap_cigar = 64 * L.n_pairs + 1024;
        for (int attempt = 0;; attempt++) {
            ok(lcty_reads_create(L.loc, L.n_pairs ? L.n_pairs : 1, n_bases ? n_bases : 32, cap_recs, cap_cigar, &L.reads), "lcty_reads_create");
            int32_t rc = LCTY_OK;
            for (uint64_t at = 0; at < L.n_pairs && rc == LCTY_OK; at += map_chunk)
                rc = lcty_reads_map_append_recruited(L.reads, set, static_cast<uint32_t>(l), at, std::min<uint64_t>(map_chunk, L.n_pairs - at), &mp);
            if (rc == LCTY_OK) break;
            if (rc != LCTY_ERR_INVALID_INPUT || !std::strstr(lcty_last_error(), "capacity") || attempt == 8) ok(rc, "lcty_reads_map_append_recruited");
            lcty_reads_destroy(L.reads); L.reads = nullptr;
            cap_recs *= 4; cap_cigar *= 4;
        }
        ms_map += now_ms() - t0; t0 = now_ms();
        ok(lcty_score_reads(L.reads), "lcty_score_reads");
        for (const char* paf_name : {"/haplotypes.paf.gz", "/haplotypes.paf"}) {  // genotype.rs:1131-1160, 149-150: --transfer 0.1 100
            const std::string paf = L.dir + paf_name;
            if (!exists(paf)) continue;
            uint64_t n_ent = 0, n_words = 0, n_recovered = 0;
            ok(lcty_paf_read(paf.c_str(), L.names.data(), L.A, &n_ent, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_words, nullptr), "haplotypes.paf (size)");
            std::vector<uint32_t> id1(n_ent + 1), id2(n_ent + 1), nm(n_ent + 1), al(n_ent + 1), words(n_words + 1);
            std::vector<uint64_t> woff(n_ent + 1);
            L.dist.assign(static_cast<size_t>(L.A) * L.A, 0u);
            L.edit_distances = true;
            ok(lcty_paf_read(paf.c_str(), L.names.data(), L.A, &n_ent, id1.data(), id2.data(), nm.data(), al.data(), woff.data(), words.data(), &n_words, L.dist.data()), "haplotypes.paf");
            ok(lcty_locus_set_hap_alns(L.loc, static_cast<uint32_t>(n_ent), id1.data(), id2.data(), woff.data(), words.data(), nm.data(), al.data(), 100, 0.1), "HapAlns");
            ok(lcty_recover_alignments(L.reads, &n_recovered), "transfer_alignments");
            ok(lcty_score_reads(L.reads), "lcty_score_reads after recovery");
            break;
        }
        ms_score += now_ms() - t0;
    }

    // ---- the loci back to back: solve, res.json.gz, alns/00.bam
    lcty_stage stages[2]; uint32_t n_stages = 0;
    ok(lcty_stages_default(stages, &n_stages), "Scheme::default");
    std::string calls_json;
    for (size_t l = 0; l < loci.size(); l++) {
        Locus& L = loci[l];
        const std::string outd = outdir + "/loci/" + L.name;
        const uint64_t G = lcty_count_genotypes(L.A, 2);
        std::vector<uint16_t> gts(G * 2);
        ok(lcty_generate_genotypes(L.A, 2, gts.data(), G), "genotypes");
        std::vector<double> mean(G), var(G); std::vector<uint32_t> att(G);
        lcty_call call;
        double t0 = now_ms();
        ok(lcty_solve(L.reads, 2, stages, n_stages, seed, nullptr, &call, mean.data(), var.data(), att.data()), "lcty_solve");
        ms_solve += now_ms() - t0;
        std::vector<uint16_t> out_gts(call.n_out * 2); std::vector<double> om(call.n_out), ov(call.n_out);
        for (uint64_t t = 0; t < call.n_out; t++) {
            out_gts[2 * t] = gts[2 * call.ixs[t]]; out_gts[2 * t + 1] = gts[2 * call.ixs[t] + 1];
            om[t] = mean[call.ixs[t]]; ov[t] = var[call.ixs[t]];
        }
        std::vector<uint32_t> gdist(call.n_out + 1);
        double wdist = NAN; uint32_t warn2 = 0;
        if (!L.dist.empty())
            ok(lcty_call_checks(out_gts.data(), call.n_out, 2, call.ln_probs, static_cast<uint32_t>(call.n_good), L.dist.data(), L.A, gdist.data(), &wdist, &warn2), "find_weighted_dist");
        const uint32_t* gd = L.dist.empty() ? nullptr : gdist.data();
        uint64_t need = 0;
        ok(lcty_res_to_json(&call, out_gts.data(), 2, L.names.data(), L.A, om.data(), ov.data(), gd, L.edit_distances, wdist, nullptr, 0, &need), "to_json (size)");
        std::vector<char> json(need);
        ok(lcty_res_to_json(&call, out_gts.data(), 2, L.names.data(), L.A, om.data(), ov.data(), gd, L.edit_distances, wdist, json.data(), need, &need), "to_json");
        ok(lcty_io_write_gz((outd + "/res.json.gz").c_str(), reinterpret_cast<const uint8_t*>(json.data()), need - 1), "res.json.gz");
        calls_json += std::string(l ? ", " : "") + "\"" + L.names[out_gts[0]] + "," + L.names[out_gts[1]] + "\"";

        if (out_bam) {
            // the table lcty_write_bam takes: the batch's records from the device, the set's view for the sequences — turned to the
            // orientation a BAM stores, that of the read end's primary record — and the set's names
            const uint64_t R = L.n_pairs;
            lcty_reads_host view; const uint64_t* name_off = nullptr; const char* read_names = nullptr;
            ok(lcty_recruited_view(set, static_cast<uint32_t>(l), &view, nullptr), "lcty_recruited_view");
            ok(lcty_recruited_names(set, static_cast<uint32_t>(l), &name_off, &read_names), "lcty_recruited_names");
            std::vector<uint64_t> aln_off(R + 1), cig_off(R + 1);
            ok(lcty_reads_get_records(L.reads, aln_off.data(), nullptr, 0, cig_off.data(), nullptr, 0), "records (size)");
            std::vector<lcty_aln_rec> recs(aln_off[R] + 1); std::vector<uint32_t> cigar(cig_off[R] + 1);
            ok(lcty_reads_get_records(L.reads, aln_off.data(), recs.data(), recs.size(), cig_off.data(), cigar.data(), cigar.size()), "records");
            const uint64_t nb = view.mate_off[2 * R];
            std::vector<uint32_t> b2(nb / 16 + 2, 0), nmv(nb / 32 + 1, 0);
            for (uint64_t r = 0; r < R; r++)
                for (uint32_t e = 0; e < 2; e++) {
                    const uint32_t ln = view.mate_len[2 * r + e];
                    const uint64_t off = view.mate_off[2 * r + e];
                    bool reverse = false;
                    for (uint64_t q = aln_off[r]; q < aln_off[r + 1]; q++) {
                        const uint16_t fl = recs[q].flags;
                        if (((fl & LCTY_FLAG_MATE2) != 0) == (e == 1) && !(fl & (LCTY_FLAG_SECONDARY | LCTY_FLAG_SUPPL))) { reverse = (fl & LCTY_FLAG_REVERSE) != 0; break; }
                    }
                    for (uint32_t i = 0; i < ln; i++) {
                        const uint64_t from = off + (reverse ? ln - 1 - i : i), to = off + i;
                        const uint32_t code = (view.bases2[from >> 4] >> (2 * (from & 15))) & 3u, other = (view.nmask[from >> 5] >> (from & 31)) & 1u;
                        if (other) nmv[to >> 5] |= 1u << (to & 31);
                        else b2[to >> 4] |= (reverse ? 3u - code : code) << (2 * (to & 15));
                    }
                }
            lcty_reads_host table = view;
            table.bases2 = b2.data(); table.nmask = nmv.data();
            table.aln_off = aln_off.data(); table.recs = recs.data(); table.cigar_off = cig_off.data(); table.cigar = cigar.data();
            const uint16_t* best = &out_gts[0];
            const uint32_t attempts = stages[n_stages - 1].attempts;
            std::vector<uint64_t> seeds(attempts);
            ok(lcty_chain_seeds(seed + 77, attempts, seeds.data()), "seeds");
            std::vector<uint64_t> read_off(call.n_good + 1);
            uint64_t n_cnt = 0, n_rec = 0;
            ok(lcty_assignment_counts(L.reads, best, 2, &stages[n_stages - 1].solver, attempts, seeds.data(), read_off.data(), nullptr, 0, &n_cnt), "counts (size)");
            std::vector<uint16_t> cnts(n_cnt ? n_cnt : 1);
            ok(lcty_assignment_counts(L.reads, best, 2, &stages[n_stages - 1].solver, attempts, seeds.data(), read_off.data(), cnts.data(), n_cnt, &n_cnt), "counts");
            mkdir((outd + "/alns").c_str(), 0777);
            ok(lcty_write_bam((outd + "/alns/00.bam").c_str(), L.reads, &table, name_off, read_names, nullptr, nullptr, L.names.data(), best, 2,
                              static_cast<uint16_t>(attempts), read_off.data(), cnts.data(), &n_rec), "lcty_write_bam");
        }
    }
    std::printf("{\"reads\": %llu, \"recruited\": [%s], \"calls\": [%s], \"ms_parse\": %.3f, \"ms_recruit\": %.3f, \"ms_scatter\": %.3f, \"ms_map\": %.3f, "
                "\"ms_score\": %.3f, \"ms_solve\": %.3f, \"ms_total\": %.3f, \"bytes_resident\": %llu}\n",
                static_cast<unsigned long long>(n_reads), recruited_json.c_str(), calls_json.c_str(), ms_parse, ms_recruit, ms_scatter, ms_map, ms_score, ms_solve,
                now_ms() - t_start, static_cast<unsigned long long>(bytes_resident));
    for (Locus& L : loci) { lcty_reads_destroy(L.reads); lcty_locus_destroy(L.loc); }
    lcty_recruited_destroy(set);
    lcty_targets_destroy(targets);
    lcty_ctx_destroy(ctx);
    return 0;
}
