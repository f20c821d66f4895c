// lcty_crc.hpp — CRC-32 (RFC 1952 8) for the decoder (lcty_inflate.hpp) and the encoder (lcty_deflate.hpp) of one BGZF block, host and
// device: the byte table's entries, and the product / power of x modulo P that joins the CRCs of neighbouring shares. A run of bytes is
// cut into CRC_SHARES contiguous shares; each share's register is taken from 0 over its own bytes and moved over the bytes behind it
// (times x^(8 * their number)); the register of the whole run is the register before it moved over all of it, xor the shares.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define LCTY_CRC_FN __device__ __forceinline__
#else
#define LCTY_CRC_FN inline
#endif

namespace lcty {
namespace crc {

constexpr uint32_t CRC_POLY = 0xEDB88320u, CRC_SHARES = 64;

LCTY_CRC_FN uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}
// a * b modulo P, bit-reflected (bit 31 is x^0)
LCTY_CRC_FN uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; k++) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) modulo P
LCTY_CRC_FN uint32_t crc_xpow8(uint32_t n) {
    uint32_t p = 0x80000000u, base = 0x00800000u;            // 1, x^8
    for (int k = 0; k < 32; k++) {
        if ((n >> k) & 1u) p = crc_mul(p, base);
        base = crc_mul(base, base);
    }
    return p;
}

}  // namespace crc
}  // namespace lcty
