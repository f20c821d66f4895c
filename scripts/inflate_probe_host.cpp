// inflate_probe_host.cpp — the host instantiation of locityper_amd/csrc/lcty_inflate.hpp (no HIP), for tests/test_bgzf_inflate_host.py:
//   g++ -O2 -std=c++17 -shared -fPIC -I locityper_amd/csrc scripts/inflate_probe_host.cpp -o libinflate_probe_host.so   (ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/inflate_probe_host.cpp
//       -o inflate_probe_host && ./inflate_probe_host corpus.bin                                                      (stand-alone)
// The stand-alone program reads a corpus written by tests/inflate_cases.py (write_corpus): per case
//   u32 n, u32 isize, u32 accept | raw << 1, u32 end, n bytes of stream and trailer, isize bytes of expected output when accept
// and runs the decoder on buffers of exactly n and isize bytes, so that a read or write outside them is the sanitizer's to see. It
// exits 1 when a verdict, the output bytes or the end of a stream differ from what the corpus says.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lcty_inflate.hpp"

using namespace lcty::inflate;

namespace {
State g_state;

// CRC-32 of n bytes through the ring, in pieces of at most RING bytes, as flush takes them
uint32_t crc_bytes(const uint8_t* p, uint64_t n) {
    crc_init(&g_state);
    uint32_t reg = 0xFFFFFFFFu, pos = 0;
    while (n) {
        const uint32_t k = static_cast<uint32_t>(n < RING ? n : RING);
        for (uint32_t i = 0; i < k; i++) g_state.ring[(pos + i) & (RING - 1)] = p[i];
        reg = crc_extend(&g_state, reg, pos, pos + k);
        pos += k; p += k; n -= k;
    }
    return ~reg;
}
}  // namespace

extern "C" {

uint32_t inflate_probe_block(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t isize, int with_trailer, uint32_t* end) {
    return inflate_block(&g_state, src, n, dst, isize, with_trailer != 0, end);
}
uint32_t inflate_probe_crc(const uint8_t* p, uint64_t n) { return crc_bytes(p, n); }
const char* inflate_probe_class(uint32_t c) { return class_name(c); }
uint32_t inflate_probe_state_bytes() { return sizeof(State); }

}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t cases = 0, accepted = 0, wrong = 0;
    uint64_t by_class[N_CLASSES] = {0};
    uint32_t head[4];
    while (fread(head, 4, 4, f) == 4) {
        const uint32_t n = head[0], isize = head[1], accept = head[2] & 1u, raw = head[2] & 2u, want_end = head[3];
        if (n > (1u << 17) || isize > (1u << 17)) { fprintf(stderr, "case %llu: bad header\n", (unsigned long long)cases); return 2; }
        uint8_t* src = static_cast<uint8_t*>(malloc(n ? n : 1));
        uint8_t* dst = static_cast<uint8_t*>(malloc(isize ? isize : 1));
        std::vector<uint8_t> want((accept ? isize : 0) + 1);
        if (fread(src, 1, n, f) != n || fread(want.data(), 1, want.size() - 1, f) != want.size() - 1) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
        memset(dst, 0xA5, isize ? isize : 1);
        uint32_t end = 0xFFFFFFFFu;
        const uint32_t rc = inflate_block(&g_state, src, n, dst, isize, !raw, &end);
        by_class[rc < N_CLASSES ? rc : N_CLASSES - 1]++;
        bool ok = (rc == OK) == (accept != 0);
        if (ok && accept) ok = memcmp(dst, want.data(), isize) == 0 && end == want_end && crc_bytes(dst, isize) == crc_bytes(want.data(), isize);
        if (!ok) {
            wrong++;
            fprintf(stderr, "case %llu: status %u (%s), corpus says %s, end %u / %u\n", (unsigned long long)cases, rc, class_name(rc), accept ? "accept" : "refuse", end, want_end);
        }
        accepted += rc == OK;
        free(src); free(dst);
        cases++;
    }
    fclose(f);
    printf("%llu cases, %llu accepted, %llu wrong\n", (unsigned long long)cases, (unsigned long long)accepted, (unsigned long long)wrong);
    for (uint32_t c = 1; c < N_CLASSES; c++) if (by_class[c]) printf("  refused, %s: %llu\n", class_name(c), (unsigned long long)by_class[c]);
    return wrong ? 1 : 0;
}
