// examples/align_locus.cpp — the pairwise alignments of one locus's haplotypes (`locityper align`: the backbone strategy of
// src/seq/align.rs, or with --tr-div the transitive one) through the C ABI, files in, files out:
//
//   <haplotypes.fa.gz>  the haplotypes of the locus                                            (lcty_fasta_read)
//   -> <out.paf.gz>     DB/loci/<locus>/haplotypes.paf.gz                                      (lcty_align_haplotypes, lcty_paf_write_text,
//                                                                                               lcty_io_write_gz)
//   pairs as load_pairs has them (command/align.rs:256-299; duplicates are dropped, the first one counts):
//   [--all]  [--pairs-file FILE: lines `query ref`, '#' comments]  [--against NAME ...: NAME as the reference of every other haplotype]
//   [-D THRESH_DIV] [--against-div DIV] [--skip-div] [-k K1,K2,..] [-g MAX_GAP]
//   [--tr-div DIV: lcty_align_haplotypes_transitive with that divergence; without it the backbone route]  [--tr-anchor SIZE]
//
// Prints one JSON line with the counts and the per-stage milliseconds. Build: see tests/test_gpu_align_example.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "locityper_hip.h"

static void ok(int32_t rc, const char* what) {
    if (rc != LCTY_OK) { std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, lcty_last_error()); std::exit(1); }
}

int main(int argc, char** argv) {
    lcty_align_params prm;
    lcty_align_params_default(&prm);
    std::string fa, out_path, pairs_file;
    std::vector<std::string> against;
    bool all = false, transitive = false;
    lcty_align_tr_params trp;
    lcty_align_tr_params_default(&trp);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--all") all = true;
        else if (a == "--pairs-file" && i + 1 < argc) pairs_file = argv[++i];
        else if (a == "--against") { while (i + 1 < argc && argv[i + 1][0] != '-') against.push_back(argv[++i]); }
        else if (a == "-D" && i + 1 < argc) prm.thresh_div = std::atof(argv[++i]);
        else if (a == "--against-div" && i + 1 < argc) prm.against_div = std::atof(argv[++i]);
        else if (a == "--skip-div") prm.skip_div = 1;
        else if (a == "--tr-div" && i + 1 < argc) { trp.transitive_div = std::atof(argv[++i]); transitive = true; }
        else if (a == "--tr-anchor" && i + 1 < argc) trp.transitive_anchor = static_cast<uint32_t>(std::strtoul(argv[++i], nullptr, 10));
        else if (a == "-g" && i + 1 < argc) prm.max_gap = static_cast<uint32_t>(std::strtoul(argv[++i], nullptr, 10));
        else if (a == "-k" && i + 1 < argc) {
            std::stringstream ss(argv[++i]);
            std::string tok;
            prm.n_backbone_ks = 0;
            while (std::getline(ss, tok, ',') && prm.n_backbone_ks < 8) prm.backbone_ks[prm.n_backbone_ks++] = static_cast<uint32_t>(std::strtoul(tok.c_str(), nullptr, 10));
        }
        else if (fa.empty()) fa = a;
        else if (out_path.empty()) out_path = a;
        else { fa.clear(); break; }
    }
    if (fa.empty() || out_path.empty()) {
        std::fprintf(stderr, "usage: align_locus <haplotypes.fa.gz> <out.paf.gz> [--all] [--pairs-file FILE] [--against NAME ...] [-D DIV] [--against-div DIV] "
                             "[--skip-div] [-k K1,K2,..] [-g MAX_GAP] [--tr-div DIV] [--tr-anchor SIZE]\n");
        return 2;
    }
    uint32_t n = 0; uint64_t nl = 0, sl = 0;
    ok(lcty_fasta_read(fa.c_str(), &n, nullptr, &nl, nullptr, &sl, nullptr), fa.c_str());
    std::vector<char> names(nl + 1); std::vector<uint8_t> seqs(sl + 1); std::vector<uint64_t> off(n + 1);
    ok(lcty_fasta_read(fa.c_str(), &n, names.data(), &nl, seqs.data(), &sl, off.data()), fa.c_str());
    std::vector<std::string> name_of(n);
    { const char* p = names.data(); for (uint32_t a = 0; a < n; a++) { name_of[a] = p; p += std::strlen(p) + 1; } }
    auto id_of = [&](const std::string& s) -> int64_t { for (uint32_t a = 0; a < n; a++) if (name_of[a] == s) return a; return -1; };

    // load_pairs: (reference, query); a pair is kept once, whatever its order
    std::vector<uint32_t> ref, query;
    std::set<std::pair<uint32_t, uint32_t>> seen;
    auto push = [&](uint32_t i, uint32_t j) {
        if (seen.insert({i < j ? i : j, i < j ? j : i}).second) { ref.push_back(i); query.push_back(j); }
    };
    if (all) for (uint32_t i = 0; i < n; i++) for (uint32_t j = i + 1; j < n; j++) push(i, j);
    if (!pairs_file.empty()) {
        std::ifstream f(pairs_file);
        if (!f) { std::fprintf(stderr, "%s: cannot open\n", pairs_file.c_str()); return 1; }
        std::string line;
        while (std::getline(f, line)) {
            if (!line.empty() && line[0] == '#') continue;
            std::stringstream ss(line);
            std::string a, b, c;
            if (!(ss >> a)) continue;
            if (!(ss >> b) || (ss >> c)) { std::fprintf(stderr, "Cannot parse pair `%s`: exactly two names required\n", line.c_str()); return 1; }
            const int64_t i1 = id_of(a), i2 = id_of(b);                      // parse_pair returns (id2, id1): the second name is the reference
            if (i1 < 0 || i2 < 0) { std::fprintf(stderr, "Cannot find sequence `%s`\n", (i1 < 0 ? a : b).c_str()); continue; }
            if (i1 == i2) { std::fprintf(stderr, "Cannot align sequence to itself (%s)\n", a.c_str()); continue; }
            push(static_cast<uint32_t>(i2), static_cast<uint32_t>(i1));
        }
    }
    std::vector<uint8_t> against_flag(n, 0);
    for (const std::string& nm : against) {
        const int64_t i = id_of(nm);
        if (i < 0) { std::fprintf(stderr, "Cannot find sequence `%s` (--against)\n", nm.c_str()); continue; }
        for (uint32_t j = 0; j < n; j++) if (j != i) push(static_cast<uint32_t>(i), j);
        against_flag[i] = 1;
    }
    if (ref.empty()) { std::fprintf(stderr, "no pairs: give --all, --pairs-file or --against\n"); return 1; }

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    lcty_align_out res;
    lcty_align_stats st;
    lcty_align_tr_out tro{};
    lcty_align_tr_stats trs{};
    if (transitive)
        ok(lcty_align_haplotypes_transitive(ctx, n, seqs.data(), off.data(), ref.size(), ref.data(), query.data(), against.empty() ? nullptr : against_flag.data(),
                                            &prm, &trp, &res, &tro, &st, &trs), "align_sequences");
    else
        ok(lcty_align_haplotypes(ctx, n, seqs.data(), off.data(), ref.size(), ref.data(), query.data(), against.empty() ? nullptr : against_flag.data(), &prm, &res,
                                 &st), "align_sequences");
    lcty_align_tr_out_free(&tro);
    lcty_ctx_destroy(ctx);
    std::string blob;
    for (uint32_t a = 0; a < n; a++) { blob += name_of[a]; blob.push_back('\0'); }
    uint64_t need = 0;
    ok(lcty_paf_write_text(&prm, n, blob.data(), off.data(), ref.size(), ref.data(), query.data(), &res, nullptr, 0, &need), "paf (size)");
    std::vector<char> text(need + 1);
    ok(lcty_paf_write_text(&prm, n, blob.data(), off.data(), ref.size(), ref.data(), query.data(), &res, text.data(), need, &need), "paf");
    ok(lcty_io_write_gz(out_path.c_str(), reinterpret_cast<const uint8_t*>(text.data()), need), out_path.c_str());
    lcty_align_out_free(&res);
    std::printf("{\"haplotypes\": %u, \"pairs\": %llu, \"aligned\": %llu, \"skipped\": %llu, \"dropped\": %llu, \"kmer_matches\": %llu, \"chain_points\": %llu, "
                "\"stretches\": {\"trivial\": %llu, \"simple\": %llu, \"small_dp\": %llu, \"general_dp\": %llu}, \"dp_cells\": %llu, \"batches\": %llu, "
                "\"accelerated\": %llu, \"rounds\": %llu, \"bytes_h2d\": %llu, \"bytes_d2h\": %llu, \"ms\": {\"div\": %.3f, \"index\": %.3f, \"match\": %.3f, \"chain\": %.3f, \"fill\": %.3f, "
                "\"select\": %.3f, \"total\": %.3f}}\n",
                n, static_cast<unsigned long long>(ref.size()), static_cast<unsigned long long>(st.n_aligned), static_cast<unsigned long long>(st.n_skipped),
                static_cast<unsigned long long>(st.n_dropped), static_cast<unsigned long long>(st.n_kmer_matches), static_cast<unsigned long long>(st.n_chain_points),
                static_cast<unsigned long long>(st.n_trivial), static_cast<unsigned long long>(st.n_simple), static_cast<unsigned long long>(st.n_small_dp),
                static_cast<unsigned long long>(st.n_general_dp), static_cast<unsigned long long>(st.dp_cells), static_cast<unsigned long long>(st.n_batches),
                static_cast<unsigned long long>(trs.n_accelerated), static_cast<unsigned long long>(trs.n_rounds), static_cast<unsigned long long>(st.bytes_h2d), static_cast<unsigned long long>(st.bytes_d2h), st.div_ms, st.index_ms, st.match_ms, st.chain_ms,
                st.fill_ms, st.select_ms, st.total_ms);
    return 0;
}
