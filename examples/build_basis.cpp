// examples/build_basis.cpp — the basis haplotypes of one locus (`locityper augment`, the basis step: construct_dominant_set,
// src/command/augment.rs:350-396) through the C ABI, files in, files out:
//
//   <locus_dir>   DB/loci/<locus>/ with
//        haplotypes.fa.gz                the haplotypes of the locus                               (lcty_fasta_read)
//        haplotypes.paf[.gz|.br]         their pairwise alignments                                 (lcty_paf_read)
//   -> <locus_dir>/haplotypes-basis.<tag>.fa.gz   the chosen haplotypes in id order               (lcty_basis_build, lcty_fasta_write_text,
//                                                                                                   lcty_io_write_gz)
//      with --default also the relative symlink haplotypes-basis.fa.gz -> haplotypes-basis.<tag>.fa.gz (create_symlink, augment.rs:281-289)
//   [-x DIVERGENCE] [-w WINDOW] [-s STEP] [-t TAG] [--basis-lo NAME ...] [--default]
//
// Prints one JSON line: {"tag": .., "basis": [ids], "names": [..], "bound": .., "optimal": ..}.
// Build: see tests/test_gpu_basis_example.py.
#include <sys/stat.h>
#include <unistd.h>

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

static bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

int main(int argc, char** argv) {
    lcty_basis_params prm;
    lcty_basis_params_default(&prm);
    std::string dir, tag;
    std::vector<std::string> lo;
    bool make_default = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if ((a == "-x" || a == "--divergence") && i + 1 < argc) prm.divergence = std::atof(argv[++i]);
        else if ((a == "-w" || a == "--window") && i + 1 < argc) prm.window = static_cast<uint32_t>(std::strtoul(argv[++i], nullptr, 10));
        else if ((a == "-s" || a == "--step") && i + 1 < argc) prm.step = static_cast<uint32_t>(std::strtoul(argv[++i], nullptr, 10));
        else if ((a == "-t" || a == "--tag") && i + 1 < argc) tag = argv[++i];
        else if (a == "--default") make_default = true;
        else if (a == "--basis-lo") { while (i + 1 < argc && argv[i + 1][0] != '-') lo.push_back(argv[++i]); }
        else if (dir.empty()) dir = a;
        else { dir.clear(); break; }
    }
    if (dir.empty()) {
        std::fprintf(stderr, "usage: build_basis <locus_dir> [-x DIVERGENCE] [-w WINDOW] [-s STEP] [-t TAG] [--basis-lo NAME ...] [--default]\n");
        return 2;
    }
    // the haplotypes
    const std::string fa = dir + "/haplotypes.fa.gz";
    uint32_t n = 0; uint64_t nl = 0, sl = 0;
    ok(lcty_fasta_read(fa.c_str(), &n, nullptr, &nl, nullptr, &sl, nullptr), fa.c_str());
    std::vector<char> names(nl + 1); std::vector<uint8_t> seqs(sl + 1); std::vector<uint64_t> off(n + 1);
    ok(lcty_fasta_read(fa.c_str(), &n, names.data(), &nl, seqs.data(), &sl, off.data()), fa.c_str());
    std::vector<const char*> name_of(n);
    { const char* p = names.data(); for (uint32_t a = 0; a < n; a++) { name_of[a] = p; p += std::strlen(p) + 1; } }
    std::vector<uint32_t> lens(n);
    for (uint32_t a = 0; a < n; a++) lens[a] = static_cast<uint32_t>(off[a + 1] - off[a]);
    // --basis-lo: the haplotypes that must not be in the basis
    std::vector<uint8_t> mask(n, 0);
    std::string lo_blob;
    for (const std::string& nm : lo) {
        uint32_t a = 0;
        while (a < n && nm != name_of[a]) a++;
        if (a == n) { std::fprintf(stderr, "--basis-lo %s: no such haplotype\n", nm.c_str()); return 1; }
        mask[a] = 1;
        lo_blob += nm; lo_blob.push_back('\0');
    }
    if (tag.empty()) {
        char buf[160];
        ok(lcty_basis_tag(&prm, lo.empty() ? nullptr : lo_blob.data(), static_cast<uint32_t>(lo.size()), buf, sizeof(buf)), "construct_basis_tag");
        tag = buf;
    }
    // the alignments (LOCUS_PAFS: the first that exists)
    std::string paf;
    for (const char* ext : {".gz", ".br", ""}) if (paf.empty() && exists(dir + "/haplotypes.paf" + ext)) paf = dir + "/haplotypes.paf" + ext;
    if (paf.empty()) { std::fprintf(stderr, "%s: no haplotypes.paf[.gz|.br]\n", dir.c_str()); return 1; }
    uint64_t ne = 0, nc = 0;
    ok(lcty_paf_read(paf.c_str(), name_of.data(), n, &ne, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nc, nullptr), paf.c_str());
    std::vector<uint32_t> id1(ne + 1), id2(ne + 1), nm(ne + 1), al(ne + 1), cigar(nc + 1);
    std::vector<uint64_t> coff(ne + 1);
    ok(lcty_paf_read(paf.c_str(), name_of.data(), n, &ne, id1.data(), id2.data(), nm.data(), al.data(), coff.data(), cigar.data(), &nc, nullptr), paf.c_str());

    lcty_ctx* ctx = nullptr;
    ok(lcty_ctx_create(0, &ctx), "lcty_ctx_create");
    std::vector<uint32_t> ids(n);
    uint32_t n_ids = 0, bound = 0; int32_t optimal = 0;
    lcty_basis_stats st;
    ok(lcty_basis_build(ctx, n, lens.data(), ne, id1.data(), id2.data(), nm.data(), al.data(), coff.data(), cigar.data(), lo.empty() ? nullptr : mask.data(),
                        &prm, ids.data(), &n_ids, &bound, &optimal, &st), "construct_dominant_set");
    lcty_ctx_destroy(ctx);

    // haplotypes-basis.<tag>.fa.gz: the chosen haplotypes in id order (augment.rs:385-389)
    std::string bnames; std::vector<uint8_t> bseqs; std::vector<uint64_t> boff{0};
    for (uint32_t t = 0; t < n_ids; t++) {
        const uint32_t a = ids[t];
        bnames += name_of[a]; bnames.push_back('\0');
        bseqs.insert(bseqs.end(), seqs.begin() + off[a], seqs.begin() + off[a + 1]);
        boff.push_back(bseqs.size());
    }
    uint64_t need = 0;
    ok(lcty_fasta_write_text(n_ids, bnames.data(), bseqs.data(), boff.data(), nullptr, 0, &need), "write_fasta (size)");
    std::vector<char> text(need + 1);
    ok(lcty_fasta_write_text(n_ids, bnames.data(), bseqs.data(), boff.data(), text.data(), need, &need), "write_fasta");
    const std::string base = "haplotypes-basis." + tag + ".fa.gz", path = dir + "/" + base;
    ok(lcty_io_write_gz(path.c_str(), reinterpret_cast<const uint8_t*>(text.data()), need), path.c_str());
    if (make_default) {
        const std::string link = dir + "/haplotypes-basis.fa.gz";
        unlink(link.c_str());                                    // also a link that points to a missing file (augment.rs:283-286)
        if (symlink(base.c_str(), link.c_str()) != 0) { std::perror(link.c_str()); return 1; }
    }
    std::printf("{\"tag\": \"%s\", \"basis\": [", tag.c_str());
    for (uint32_t t = 0; t < n_ids; t++) std::printf("%s%u", t ? ", " : "", ids[t]);
    std::printf("], \"names\": [");
    for (uint32_t t = 0; t < n_ids; t++) std::printf("%s\"%s\"", t ? ", " : "", name_of[ids[t]]);
    std::printf("], \"haplotypes\": %u, \"bound\": %u, \"optimal\": %s, \"rows\": [%llu, %llu, %llu]}\n", n, bound, optimal ? "true" : "false",
                static_cast<unsigned long long>(st.n_rows_raw), static_cast<unsigned long long>(st.n_rows_unique),
                static_cast<unsigned long long>(st.n_rows_minimal));
    return 0;
}
