// vcf_index_probe_host.cpp — the parsers of untrusted bytes in front of every BGZF reader (locityper_amd/csrc/lcty_bgzf_index.hpp: the
// tabix and the BAI parser, the chunk plan, the line functions of the VCF readers; lcty_bgzf.hpp: the head of a BGZF block; no HIP,
// nothing inflated) over a corpus of byte strings, stand-alone on the CPU, for tests/test_vcf_indexed_host.py and
// tests/test_bgzf_read_host.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/vcf_index_probe_host.cpp
//       -o vcf_index_probe_host && ./vcf_index_probe_host corpus.bin
// The corpus is written by tests/vcf_index_cases.py (write_corpus):
//   u32 n_index_cases, per case  u32 n, u32 status, n bytes of an inflated .tbi
//   u32 n_line_cases,  per case  u32 n, u32 status, u32 n_samples, n_samples x u32 ploidy, n bytes of one record line
// and may end there, or go on (tests/test_bgzf_read_host.py) with
//   u32 n_bai_cases,   per case  u32 n, u32 status, u32 n_refs_of_header, n bytes of a .bai
//   u32 n_head_cases,  per case  u32 n, u32 verdict, u32 csize, u32 isize, u32 head, n bytes in front of bgzf_head (the three fields
//                                count where the verdict is not "not a block")
// Every case runs on a buffer of exactly n bytes, so that a read outside it is the sanitizer's to see. An index that parses is also
// planned over a few regions of each of its references. It exits 1 when a status differs from what the corpus says.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lcty_bgzf.hpp"
#include "lcty_bgzf_index.hpp"

namespace lcty { void set_last_error(const std::string&) {} }

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t cases = 0, refused = 0, wrong = 0, chunks = 0;
    uint32_t n_cases = 0;
    if (!rd(f, &n_cases, 4)) { fprintf(stderr, "short file\n"); return 2; }
    for (uint32_t c = 0; c < n_cases; c++, cases++) {
        uint32_t head[2];
        if (!rd(f, head, 8) || head[0] > (1u << 26)) { fprintf(stderr, "case %llu: bad header\n", (unsigned long long)cases); return 2; }
        const uint32_t n = head[0];
        uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (!rd(f, data, n)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
        uint32_t status = 0;
        try {
            const lcty::vcfidx::Tbi T = lcty::vcfidx::parse_tbi(data, n, "corpus.tbi");
            static const uint32_t regions[][2] = {{0, 1}, {100, 200}, {16384, 16385}, {16000, 17000}, {0, 0xFFFFFFFFu}, {500, 500}, {70000, 10}, {0xFFFFFFFFu, 0}};
            for (const std::string& name : T.names)
                for (const auto& r : regions) chunks += lcty::vcfidx::plan(T, name.c_str(), r[0], r[1]).size();
            chunks += lcty::vcfidx::plan(T, "nobody", 0, 100).size();
        } catch (const lcty::Error& e) { status = static_cast<uint32_t>(e.code); refused++; }
        if (status != head[1]) { wrong++; fprintf(stderr, "index case %u (%u bytes): status %u, corpus says %u\n", c, n, status, head[1]); }
        free(data);
    }
    if (!rd(f, &n_cases, 4)) { fprintf(stderr, "short file\n"); return 2; }
    for (uint32_t c = 0; c < n_cases; c++, cases++) {
        uint32_t head[3];
        if (!rd(f, head, 12) || head[0] > (1u << 26) || head[2] > (1u << 16)) { fprintf(stderr, "case %llu: bad header\n", (unsigned long long)cases); return 2; }
        const uint32_t n = head[0], S = head[2];
        std::vector<uint32_t> ploidy(S);
        uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (!rd(f, ploidy.data(), 4ull * S) || !rd(f, data, n)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
        std::vector<std::string> samples;
        for (uint32_t i = 0; i < S; i++) samples.push_back("S" + std::to_string(i));
        uint32_t status = 0;
        try {
            const lcty::vcfidx::LineHead h = lcty::vcfidx::parse_line_head(data, 0, n, "corpus.vcf");
            lcty::vcfidx::RecordArrays A; std::vector<int32_t> al;
            lcty::vcfidx::parse_record_line(data, 0, n, h.chrom.c_str(), h.pos, h.ref_len, S, ploidy.data(), samples, nullptr, A, al);
            if (A.pos.size() != 1 || A.rec_allele.size() != 2 || A.allele_off.back() != A.pool.size() || A.phased.size() != S) { wrong++; fprintf(stderr, "line case %u: broken arrays\n", c); }
        } catch (const lcty::Error& e) { status = static_cast<uint32_t>(e.code); refused++; }
        if (status != head[1]) { wrong++; fprintf(stderr, "line case %u: status %u, corpus says %u\n", c, status, head[1]); }
        free(data);
    }
    if (rd(f, &n_cases, 4)) {                                                  // the two sections a corpus may go on with
        for (uint32_t c = 0; c < n_cases; c++, cases++) {
            uint32_t head[3];
            if (!rd(f, head, 12) || head[0] > (1u << 26)) { fprintf(stderr, "case %llu: bad header\n", (unsigned long long)cases); return 2; }
            const uint32_t n = head[0];
            uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
            if (!rd(f, data, n)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
            uint32_t status = 0;
            try {
                const lcty::Bai B = lcty::parse_bai(data, n, head[2], "corpus.bai");
                std::vector<lcty::Chunk> cs;
                for (const lcty::IndexRef& R : B.refs) { lcty::region_chunks(R, 0, 1u << 29, cs); lcty::region_chunks(R, 16000, 17000, cs); }
                chunks += lcty::merge_chunks(cs).size();
            } catch (const lcty::Error& e) { status = static_cast<uint32_t>(e.code); refused++; }
            if (status != head[1]) { wrong++; fprintf(stderr, "BAI case %u (%u bytes): status %u, corpus says %u\n", c, n, status, head[1]); }
            free(data);
        }
        if (!rd(f, &n_cases, 4)) { fprintf(stderr, "short file\n"); return 2; }
        for (uint32_t c = 0; c < n_cases; c++, cases++) {
            uint32_t head[5];
            if (!rd(f, head, 20) || head[0] > (1u << 26)) { fprintf(stderr, "case %llu: bad header\n", (unsigned long long)cases); return 2; }
            const uint32_t n = head[0];
            uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
            if (!rd(f, data, n)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
            lcty::BgzfHead h{0, 0, 0};
            const uint32_t v = lcty::bgzf_head(data, n, h);
            if (v != lcty::BGZF_OK) refused++;
            if (v != head[1] || (v != lcty::BGZF_NOT_A_BLOCK && (h.csize != head[2] || h.isize != head[3] || h.head != head[4]))) {
                wrong++;
                fprintf(stderr, "head case %u (%u bytes): verdict %u csize %u isize %u head %u, corpus says %u %u %u %u\n", c, n, v, h.csize, h.isize, h.head,
                        head[1], head[2], head[3], head[4]);
            }
            free(data);
        }
    }
    fclose(f);
    printf("%llu cases, %llu refused, %llu chunks planned, %llu wrong\n", (unsigned long long)cases, (unsigned long long)refused, (unsigned long long)chunks,
           (unsigned long long)wrong);
    return wrong ? 1 : 0;
}
