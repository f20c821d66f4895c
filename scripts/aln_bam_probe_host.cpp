// aln_bam_probe_host.cpp — the two host passes of lcty_bam_read_device (locityper_amd/csrc/lcty_aln_bam_parse.hpp: the header parse and
// the walk of record lengths; no HIP) over a corpus of byte strings, stand-alone on the CPU, for tests/test_aln_bam_parse_host.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/aln_bam_probe_host.cpp
//       -o aln_bam_probe_host && ./aln_bam_probe_host corpus.bin
// The corpus is written by tests/aln_bam_cases.py (write_corpus): per case
//   u32 n, u32 n_alleles, u32 names_len, u32 status, u32 n_ref, u32 n_rec, u32 stop, u32 last_off,
//   names_len bytes of 0-terminated allele names, n bytes of an inflated file
// Every case runs on a buffer of exactly n bytes, so that a read outside it is the sanitizer's to see. It exits 1 when a status, the
// number of references or of records walked, the way the walk stopped or the last record's offset differ from what the corpus says.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lcty_aln_bam_parse.hpp"

namespace lcty { void set_last_error(const std::string&) {} }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t cases = 0, refused = 0, wrong = 0, records = 0;
    uint32_t head[8];
    while (fread(head, 4, 8, f) == 8) {
        const uint32_t n = head[0], n_alleles = head[1], names_len = head[2];
        if (n > (1u << 26) || names_len > (1u << 20)) { fprintf(stderr, "case %llu: bad header\n", (unsigned long long)cases); return 2; }
        std::vector<char> blob(names_len + 1, '\0');
        uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (fread(blob.data(), 1, names_len, f) != names_len || fread(data, 1, n, f) != n) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
        const std::vector<std::string> names = lcty::split_names(blob.data(), n_alleles);
        std::vector<const char*> ptrs;
        for (const std::string& s : names) ptrs.push_back(s.c_str());
        uint32_t status = 0, n_ref = 0, stop = 0, last = 0;
        std::vector<uint64_t> rec_off;
        try {
            const lcty::alnbam::Header H = lcty::alnbam::parse_header(data, n, ptrs.data(), n_alleles, "corpus");
            n_ref = H.n_ref;
            stop = lcty::alnbam::walk_records(data, n, H.first_record, rec_off);
            for (const uint64_t o : rec_off) {                                   // what the device stage may take for granted
                if (o + 36 > n || o + 4 + lcty::alnbam::rd32(data + o) > n) { fprintf(stderr, "case %llu: a record leaves the bytes\n", (unsigned long long)cases); wrong++; break; }
                (void)lcty::alnbam::is_primary_at(data, o);
            }
            last = rec_off.empty() ? 0u : static_cast<uint32_t>(rec_off.back());
        } catch (const lcty::Error& e) { status = static_cast<uint32_t>(e.code); refused++; }
        if (status != head[3] || n_ref != head[4] || rec_off.size() != head[5] || stop != head[6] || last != head[7]) {
            wrong++;
            fprintf(stderr, "case %llu: status %u refs %u records %zu stop %u last %u, corpus says %u %u %u %u %u\n", (unsigned long long)cases, status, n_ref,
                    rec_off.size(), stop, last, head[3], head[4], head[5], head[6], head[7]);
        }
        records += rec_off.size();
        free(data);
        cases++;
    }
    fclose(f);
    printf("%llu cases, %llu refused, %llu records walked, %llu wrong\n", (unsigned long long)cases, (unsigned long long)refused, (unsigned long long)records,
           (unsigned long long)wrong);
    return wrong ? 1 : 0;
}
