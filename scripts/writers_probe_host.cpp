// writers_probe_host.cpp — the host code every source of recruited reads writes its per-locus files with
// (locityper_amd/csrc/lcty_writers.hpp: write_recruited_units, record_name, bam_record_text) on the CPU, no HIP, for
// tests/test_writers_host.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/writers_probe_host.cpp
//       -lz -o writers_probe_host && ./writers_probe_host DIR/answers.txt DIR/slice.bin
// slice.bin holds BAM records one behind the other, as a slice of inflated blocks does. answers.txt, one token after the other:
//   n_writers max_out n_units, a path per writer (".gz": gzip), then per unit:  cnt locus{max_out} off1 off2
// where off1 / off2 are the bytes at which the unit's records start in the slice (-1: no such mate). The slice and the answers are
// copied into heap blocks of exactly their size, so that a read past either is the sanitizer's to see. Output: "status S written W"
// and, when S is not 0, the message on the next line.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "lcty_writers.hpp"

using namespace lcty;

static std::string last_error;
namespace lcty { void set_last_error(const std::string& msg) { last_error = msg; } }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: writers_probe_host DIR/answers.txt DIR/slice.bin\n"); return 2; }
    std::ifstream in(argv[1]), bin(argv[2], std::ios::binary);
    if (!in || !bin) { fprintf(stderr, "cannot open the corpus\n"); return 2; }
    const std::string bytes((std::istreambuf_iterator<char>(bin)), std::istreambuf_iterator<char>());
    std::unique_ptr<uint8_t[]> slice(new uint8_t[bytes.size()]);
    memcpy(slice.get(), bytes.data(), bytes.size());
    uint32_t n_writers, max_out; uint64_t n;
    in >> n_writers >> max_out >> n;
    lcty_fastx_writers w;
    w.gz.assign(n_writers, nullptr); w.plain.assign(n_writers, nullptr); w.paths.resize(n_writers);
    for (uint32_t i = 0; i < n_writers; i++) {
        in >> w.paths[i];
        const std::string& p = w.paths[i];
        if (p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0) w.gz[i] = gzopen(p.c_str(), "wb1");
        else w.plain[i] = fopen(p.c_str(), "wb");
        if (!w.gz[i] && !w.plain[i]) { fprintf(stderr, "cannot create %s\n", p.c_str()); return 2; }
    }
    std::unique_ptr<uint32_t[]> cnt(new uint32_t[n]), loci(new uint32_t[n * max_out]);
    std::vector<int64_t> off(2 * n);
    for (uint64_t i = 0; i < n; i++) {
        in >> cnt[i];
        for (uint32_t j = 0; j < max_out; j++) in >> loci[i * max_out + j];
        in >> off[2 * i] >> off[2 * i + 1];
    }
    if (!in) { fprintf(stderr, "bad corpus\n"); return 2; }
    uint64_t written = 0;
    const int32_t status = guarded([&] {
        written = write_recruited_units(&w, n, max_out, cnt.get(), loci.get(), [&](uint64_t i, std::string& text) {
            for (int e = 0; e < 2; e++)
                if (off[2 * i + e] >= 0) bam_record_text(slice.get(), static_cast<uint64_t>(off[2 * i + e]), text);
        });
    });
    printf("status %d written %llu\n", status, static_cast<unsigned long long>(written));
    if (status) printf("%s\n", last_error.c_str());
    return 0;
}
