// deflate_probe_host.cpp — the host instantiation of locityper_amd/csrc/lcty_deflate.hpp (no HIP), for tests/test_bgzf_deflate_host.py:
//   g++ -O2 -std=c++17 -shared -fPIC -I locityper_amd/csrc scripts/deflate_probe_host.cpp -o libdeflate_probe_host.so   (ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/deflate_probe_host.cpp
//       -o deflate_probe_host && ./deflate_probe_host corpus.bin                                                      (stand-alone)
// The stand-alone program reads a corpus written by tests/deflate_cases.py (write_corpus): per case u32 n and n bytes. It encodes every
// case from a buffer of exactly n bytes into one of exactly n + 5 bytes rounded up to whole 32-bit words (the encoder ORs words), so
// that a read or write outside them is the sanitizer's to see, puts the trailer (the encoder's CRC-32, n) behind the stream and inflates
// it with lcty_inflate.hpp in the same process, again into exactly n bytes. It exits 1 when a stream is longer than n + 5 bytes, is
// refused by the decoder (which checks the CRC), does not end where the encoder says or does not give the input back.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lcty_deflate.hpp"
#include "lcty_inflate.hpp"

namespace D = lcty::deflate;
namespace I = lcty::inflate;

namespace {
D::State g_state;
I::State g_inflate;
uint32_t g_tok[D::MAX_IN];
uint32_t g_crc = 0;
}  // namespace

extern "C" {

// the stream of src[0, n) into dst[0, cap): its length; 0xFFFFFFFF when n > 0xff00 or cap < n + 5. *form: 0 stored, 1 fixed, 2 dynamic
uint32_t deflate_probe_block(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t cap, uint32_t* form) {
    if (n > D::MAX_IN || cap < n + 5) return D::REFUSED;
    const uint32_t words = (n + 5 + 3) / 4;
    uint32_t* out = static_cast<uint32_t*>(malloc(words * 4));
    uint32_t f = 0;
    const uint32_t len = D::deflate_block(&g_state, g_tok, src, n, out, words, &g_crc, &f);
    if (len != D::REFUSED) memcpy(dst, out, len);
    free(out);
    if (form) *form = f;
    return len;
}
uint32_t deflate_probe_last_crc() { return g_crc; }
void deflate_probe_code_lengths(const uint32_t* freq, uint32_t n_sym, uint32_t max_bits, uint8_t* out_lens) {
    if (n_sym > D::LIT_SLOTS || max_bits < 1 || max_bits > 15) return;
    D::code_lengths(&g_state, freq, n_sym, max_bits, out_lens, false);
}
uint32_t deflate_probe_state_bytes() { return sizeof(D::State); }

}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t cases = 0, wrong = 0, by_form[3] = {0, 0, 0}, bytes_in = 0, bytes_out = 0;
    uint32_t n = 0;
    while (fread(&n, 4, 1, f) == 1) {
        if (n > D::MAX_IN) { fprintf(stderr, "case %llu: bad header\n", (unsigned long long)cases); return 2; }
        uint8_t* src = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (fread(src, 1, n, f) != n) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)cases); return 2; }
        const uint32_t words = (n + 5 + 3) / 4;
        uint32_t* out = static_cast<uint32_t*>(malloc(words * 4));
        memset(out, 0xA5, words * 4);
        uint32_t crc = 0, form = 9;
        const uint32_t len = D::deflate_block(&g_state, g_tok, src, n, out, words, &crc, &form);
        bool ok = len != D::REFUSED && len <= n + 5 && form < 3;
        if (ok) {
            uint8_t* member = static_cast<uint8_t*>(malloc(len + 8));
            uint8_t* back = static_cast<uint8_t*>(malloc(n ? n : 1));
            memcpy(member, out, len);
            for (int k = 0; k < 4; k++) { member[len + k] = static_cast<uint8_t>(crc >> (8 * k)); member[len + 4 + k] = static_cast<uint8_t>(n >> (8 * k)); }
            uint32_t end = 0xFFFFFFFFu;
            const uint32_t rc = I::inflate_block(&g_inflate, member, len + 8, back, n, true, &end);
            ok = rc == I::OK && end == len && memcmp(back, src, n) == 0;
            if (!ok) fprintf(stderr, "case %llu (%u bytes, form %u, stream %u): the decoder says %u (%s), end %u\n", (unsigned long long)cases, n, form, len, rc, I::class_name(rc), end);
            free(member); free(back);
            by_form[form]++; bytes_in += n; bytes_out += len;
        } else fprintf(stderr, "case %llu (%u bytes): stream %u, form %u\n", (unsigned long long)cases, n, len, form);
        wrong += !ok;
        free(src); free(out);
        cases++;
    }
    fclose(f);
    printf("%llu cases, %llu wrong; %llu stored, %llu fixed, %llu dynamic; %llu bytes in, %llu out\n", (unsigned long long)cases, (unsigned long long)wrong,
           (unsigned long long)by_form[0], (unsigned long long)by_form[1], (unsigned long long)by_form[2], (unsigned long long)bytes_in, (unsigned long long)bytes_out);
    return wrong ? 1 : 0;
}
