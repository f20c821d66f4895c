// lcty_inflate.hpp — raw DEFLATE (RFC 1951) for one BGZF block (SAM specification 4.1; the gzip trailer of RFC 1952), stated once for
// the host and the device. A group of LANES lanes decodes one block: the symbol decode is the same in every lane (one
// chain of table lookups), the byte copies of matches, stored blocks, the input window, the flush and the CRC are shared out by lane.
// On the device the group is a wavefront alone in its workgroup and State lies in LDS; compiled without HIP (scripts/
// inflate_probe_host.cpp) the group is one thread, which is how the text is tested and sanitized on the CPU.
//   Acceptance: exactly what zlib's inflate accepts for a gzip member of window 15 without dictionary, given ISIZE bytes of room.
//   BTYPE 3; a stored LEN != ~NLEN; HLIT > 286 or HDIST > 30; a code-length code that is incomplete or over-subscribed (no code at all
//   passes inflate_table and ends as a missing end-of-block code); a repeat (16) without a previous length; a repeat past
//   HLIT + HDIST; no code for symbol 256; a literal/length or distance set that is over-subscribed, or incomplete unless it is a
//   single code of length 1 (no distance code at all is legal until a distance is decoded); the unused code of such a set; symbols
//   286, 287, distance symbols 30, 31; a distance before the start of the block's output; output past ISIZE or short of it; input
//   that ends early; CRC32 and ISIZE of the trailer, read at the first byte boundary behind the stream, that do not match.
//   Bounds: the output goes through a ring of RING bytes indexed modulo RING, the input through a window indexed modulo WIN, tables by
//   masked bit fields; the block's input is read at min(i, n - 1) and its output written below min(pos, isize). No index depends on a
//   check that could be skipped.
//   Termination: every turn of every loop consumes at least one input bit or produces at least one output byte, or counts a fixed
//   table; bits behind the input read as zero and the first turn that has used one ends in E_INPUT.
#pragma once

#include <cstdint>

#include "lcty_crc.hpp"

#ifdef __HIPCC__
#define LCTY_INF_FN __device__ __forceinline__
#else
#define LCTY_INF_FN inline
#endif
#ifdef __HIP_DEVICE_COMPILE__
#define LCTY_INF_LANE (threadIdx.x & 63u)
#define LCTY_INF_LANES 64u
#define LCTY_INF_SYNC() __syncthreads()                      // one wavefront per workgroup: orders its LDS traffic, costs no wait
#define LCTY_INF_UNI(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#else
#define LCTY_INF_LANE 0u
#define LCTY_INF_LANES 1u
#define LCTY_INF_SYNC() ((void)0)
#define LCTY_INF_UNI(x) static_cast<uint32_t>(x)
#endif

namespace lcty {
namespace inflate {

// the classes of error, one small integer each (class_name says them)
enum : uint32_t {
    OK = 0, E_INPUT = 1, E_BTYPE = 2, E_STORED = 3, E_COUNTS = 4, E_CLCODE = 5, E_REPEAT = 6, E_NO_EOB = 7, E_LITSET = 8, E_DISTSET = 9,
    E_LITSYM = 10, E_DISTSYM = 11, E_FAR = 12, E_OVER = 13, E_SHORT = 14, E_CRC = 15, E_ISIZE = 16, E_TASK = 17, N_CLASSES = 18
};
inline const char* class_name(uint32_t c) {
    static const char* const names[N_CLASSES] = {
        "ok", "input ends inside the stream", "block type 3", "stored length and its complement differ", "too many length or distance codes",
        "invalid code-length code", "invalid length repeat", "no end-of-block code", "invalid literal/length code set", "invalid distance code set",
        "invalid literal/length code", "invalid distance code", "distance before the start of the block", "more output than ISIZE",
        "less output than ISIZE", "CRC32 mismatch", "ISIZE mismatch", "block outside its buffers"};
    return c < N_CLASSES ? names[c] : "unknown";
}

constexpr uint32_t RING = 32768, WIN = 1024, WIN_CHUNK = 256, MAX_ISIZE = 65536;
constexpr uint32_t LIT_BITS = 10, DIST_BITS = 8, MAX_CODE = 15, MAX_LENS = 352;

// one canonical Huffman code: a primary table over the next PB bits (symbol | length << 9, 0 = not there) and, for longer codes and
// for the codes nobody has, the counts per length with the symbols in code order
struct Code { uint16_t count[MAX_CODE + 1]; uint16_t sorted[288]; };
struct State {
    uint8_t ring[RING];                  // the last RING bytes of output, by position modulo RING
    uint8_t win[WIN];                    // the input around the read position, by position modulo WIN
    uint16_t lit_tab[1u << LIT_BITS]; uint16_t dist_tab[1u << DIST_BITS];
    Code lit, dist;
    uint8_t lens[MAX_LENS];
    uint32_t crc_tab[256];
};

// ---- CRC-32 (lcty_crc.hpp: the byte table, crc_mul and crc_xpow8 that join the CRCs of neighbouring shares), over the ring ----------------
using crc::CRC_SHARES; using crc::crc_mul; using crc::crc_table_entry; using crc::crc_xpow8;
// what share `share` of CRC_SHARES adds to the register of the bytes [from, to) of the ring: the register of its own contiguous
// bytes from 0, moved over the bytes behind it
LCTY_INF_FN uint32_t crc_share(const State* st, uint32_t from, uint32_t to, uint32_t share) {
    const uint32_t n = to - from, per = (n + CRC_SHARES - 1) / CRC_SHARES;
    uint32_t b = from + share * per, e = b + per;
    if (b > to) b = to;
    if (e > to) e = to;
    uint32_t r = 0;
    for (uint32_t i = b; i < e; i++) r = st->crc_tab[(r ^ st->ring[i & (RING - 1)]) & 255u] ^ (r >> 8);
    return e > b ? crc_mul(r, crc_xpow8(to - e)) : 0u;
}
// the register after the bytes [from, to) of the ring, from the register before them
LCTY_INF_FN uint32_t crc_extend(const State* st, uint32_t reg, uint32_t from, uint32_t to) {
    if (to <= from) return reg;
    uint32_t sum = 0;
#ifdef __HIP_DEVICE_COMPILE__
    sum = crc_share(st, from, to, LCTY_INF_LANE);
    for (int o = 32; o; o >>= 1) sum ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum), o));
    sum = LCTY_INF_UNI(sum);
#else
    for (uint32_t s = 0; s < CRC_SHARES; s++) sum ^= crc_share(st, from, to, s);
#endif
    return crc_mul(reg, crc_xpow8(to - from)) ^ sum;
}
LCTY_INF_FN void crc_init(State* st) {
    for (uint32_t i = LCTY_INF_LANE; i < 256u; i += LCTY_INF_LANES) st->crc_tab[i] = crc_table_entry(i);
    LCTY_INF_SYNC();
}

// ---- the tables of one code -----------------------------------------------------------------------------------------------------
// inflate_table's verdict on n lengths: 0 fine, 1 over-subscribed, 2 incomplete (and not the single code of length 1 that a
// literal/length or distance set may be). Fills code->count / sorted and the primary table of 1 << pb entries.
LCTY_INF_FN uint32_t build_code(const uint8_t* lens, uint32_t n, Code* code, uint16_t* tab, uint32_t pb, bool may_be_single) {
    const uint32_t lane = LCTY_INF_LANE;
    LCTY_INF_SYNC();                                         // the lengths are written, the tables of the block before are read
    if (lane == 0) {
        for (uint32_t l = 0; l <= MAX_CODE; l++) code->count[l] = 0;
        for (uint32_t i = 0; i < n; i++) code->count[lens[i] & MAX_CODE]++;
    }
    for (uint32_t i = lane; i < (1u << pb); i += LCTY_INF_LANES) tab[i] = 0;
    LCTY_INF_SYNC();
    uint32_t offs[MAX_CODE + 2], next[MAX_CODE + 2];
    int32_t left = 1;
    uint32_t max = 0, code0 = 0;
    offs[1] = 0; next[0] = 0;
    bool over = false;
    for (uint32_t l = 1; l <= MAX_CODE; l++) {
        const uint32_t c = LCTY_INF_UNI(code->count[l]);
        left = left * 2 - static_cast<int32_t>(c);
        if (left < 0) over = true;
        if (over) left = 0;                                  // the verdict is out; keeps the sum small
        if (c) max = l;
        code0 = (code0 + (l > 1 ? LCTY_INF_UNI(code->count[l - 1]) : 0u)) << 1;
        next[l] = code0;
        offs[l + 1] = offs[l] + c;
    }
    if (over) return 1;
    if (max == 0) return 0;                                  // no code at all: every lookup ends as an invalid code
    if (left > 0 && !(may_be_single && max == 1)) return 2;
    // the symbols in code order, and the primary entries of the codes of at most pb bits: one lane, in symbol order
    if (lane == 0) {
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t l = lens[i] & MAX_CODE;
            if (!l) continue;
            code->sorted[offs[l]++ % 288u] = static_cast<uint16_t>(i);
            const uint32_t c = next[l]++;
            if (l > pb) continue;
            uint32_t rev = 0;
            for (uint32_t k = 0; k < l; k++) rev |= ((c >> k) & 1u) << (l - 1 - k);
            for (uint32_t at = rev; at < (1u << pb); at += 1u << l) tab[at] = static_cast<uint16_t>(i | (l << 9));
        }
    }
    LCTY_INF_SYNC();
    return 0;
}

// ---- the input: bits from the window ------------------------------------------------------------------------------------------------
struct Bits {
    const uint8_t* src; uint32_t n;      // the block's deflate stream and trailer
    uint32_t ip, loaded;                 // bytes taken into `hold`; bytes of src copied to the window (a multiple of WIN_CHUNK)
    uint64_t hold; uint32_t nbits;
};
LCTY_INF_FN uint8_t src_byte(const Bits& b, uint32_t i) { return i < b.n ? b.src[i < b.n ? i : b.n - 1] : static_cast<uint8_t>(0); }
// at least 32 bits in hold (zeros behind the input)
LCTY_INF_FN void refill(State* st, Bits& b) {
    if (b.nbits >= 32) return;
    while (b.ip + 4 > b.loaded) {                            // ip grows by 4 a refill and a refill needs a consumed bit: bounded by used()
        LCTY_INF_SYNC();
        for (uint32_t j = b.loaded + LCTY_INF_LANE; j < b.loaded + WIN_CHUNK; j += LCTY_INF_LANES) st->win[j & (WIN - 1)] = src_byte(b, j);
        b.loaded += WIN_CHUNK;
        LCTY_INF_SYNC();
    }
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4; k++) w |= static_cast<uint32_t>(st->win[(b.ip + k) & (WIN - 1)]) << (8 * k);
    b.hold |= static_cast<uint64_t>(LCTY_INF_UNI(w)) << b.nbits;
    b.nbits += 32; b.ip += 4;
}
LCTY_INF_FN uint32_t peek(const Bits& b, uint32_t k) { return static_cast<uint32_t>(b.hold) & ((1u << k) - 1u); }       // k <= 16
LCTY_INF_FN void drop(Bits& b, uint32_t k) { b.hold >>= k; b.nbits -= k; }                                               // k <= nbits
LCTY_INF_FN uint32_t take(Bits& b, uint32_t k) { const uint32_t v = peek(b, k); drop(b, k); return v; }
// bits of the stream used so far; overrun: some of them lie behind the input
LCTY_INF_FN uint64_t used(const Bits& b) { return 8ull * b.ip - b.nbits; }
LCTY_INF_FN bool overrun(const Bits& b) { return used(b) > 8ull * b.n; }

// the next symbol of a code: 0 .. 287, or 0xFFFF for a code nobody has. Needs 15 bits in hold.
LCTY_INF_FN uint32_t decode(Bits& b, const Code* code, const uint16_t* tab, uint32_t pb) {
    const uint32_t e = LCTY_INF_UNI(tab[peek(b, pb)]);
    if (e) { drop(b, e >> 9); return e & 511u; }
    uint32_t c = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= MAX_CODE; l++) {
        c |= static_cast<uint32_t>(b.hold >> (l - 1)) & 1u;
        const uint32_t cnt = LCTY_INF_UNI(code->count[l]);
        if (c < first + cnt) { drop(b, l); return LCTY_INF_UNI(code->sorted[(index + (c - first)) % 288u]); }
        index += cnt; first = (first + cnt) << 1; c <<= 1;
    }
    drop(b, 1);                                              // progress; the caller ends the block
    return 0xFFFFu;
}

// ---- the output: the ring, flushed to the block's place as it advances ------------------------------------------------------------------
struct Out { uint8_t* dst; uint32_t isize, pos, flushed, crc; };
LCTY_INF_FN void flush(State* st, Out& o) {
    LCTY_INF_SYNC();
    const uint32_t to = o.pos < o.isize ? o.pos : o.isize;
    for (uint32_t i = o.flushed + LCTY_INF_LANE; i < to; i += LCTY_INF_LANES) o.dst[i] = st->ring[i & (RING - 1)];
    o.crc = crc_extend(st, o.crc, o.flushed, to);
    if (to > o.flushed) o.flushed = to;
    LCTY_INF_SYNC();
}
// room for k more bytes (k <= RING / 2) in the ring; false: they would pass ISIZE
LCTY_INF_FN bool room(State* st, Out& o, uint32_t k) {
    if (o.pos + k > o.isize) return false;
    if (o.pos + k - o.flushed > RING) flush(st, o);
    return true;
}

LCTY_INF_FN void fixed_lengths(State* st) {
    for (uint32_t i = LCTY_INF_LANE; i < 320u; i += LCTY_INF_LANES)
        st->lens[i] = static_cast<uint8_t>(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
}

// the lengths of a dynamic block (RFC 1951 3.2.7) into st->lens; *nlen, *ndist
LCTY_INF_FN uint32_t dynamic_lengths(State* st, Bits& b, uint32_t* nlen, uint32_t* ndist) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    refill(st, b);
    const uint32_t hlit = take(b, 5) + 257, hdist = take(b, 5) + 1, hclen = take(b, 4) + 4;
    if (overrun(b)) return E_INPUT;
    if (hlit > 286 || hdist > 30) return E_COUNTS;
    LCTY_INF_SYNC();
    for (uint32_t i = LCTY_INF_LANE; i < 19u; i += LCTY_INF_LANES) st->lens[i] = 0;
    LCTY_INF_SYNC();
    for (uint32_t i = 0; i < hclen; i++) {
        refill(st, b);
        const uint32_t l = take(b, 3);
        if (LCTY_INF_LANE == 0) st->lens[order[i]] = static_cast<uint8_t>(l);
    }
    if (overrun(b)) return E_INPUT;
    // the code-length code shares the distance code's tables: both are rebuilt before they are used again
    const uint32_t bad = build_code(st->lens, 19, &st->dist, st->dist_tab, 7, false);
    if (bad) return E_CLCODE;
    const uint32_t total = hlit + hdist;
    uint32_t have = 0, prev = 0;
    LCTY_INF_SYNC();
    while (have < total) {
        refill(st, b);
        uint32_t sym = decode(b, &st->dist, st->dist_tab, 7);
        if (sym == 0xFFFFu) sym = 0;                         // no code-length code at all: inflate reads a length 0 of one bit
        uint32_t rep = 1, len = sym;
        if (sym == 16) { if (have == 0) return E_REPEAT; len = prev; rep = 3 + take(b, 2); }
        else if (sym == 17) { len = 0; rep = 3 + take(b, 3); }
        else if (sym == 18) { len = 0; rep = 11 + take(b, 7); }
        else if (sym > 18) return E_CLCODE;
        if (overrun(b)) return E_INPUT;
        if (have + rep > total) return E_REPEAT;
        // behind the 19 lengths of the code-length code, which is still being read
        for (uint32_t i = LCTY_INF_LANE; i < rep; i += LCTY_INF_LANES) st->lens[(32 + have + i) % MAX_LENS] = static_cast<uint8_t>(len);
        have += rep; prev = len;
    }
    *nlen = hlit; *ndist = hdist;
    return OK;
}

// ---- one block ----------------------------------------------------------------------------------------------------------------------
// The deflate stream at src[0, n) into dst[0, isize), then the trailer behind it. *end (may be null) gets the offset of the first byte
// behind the stream whenever the stream itself was accepted. with_trailer false: the stream alone (the CRC is still computed).
LCTY_INF_FN uint32_t inflate_block(State* st, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t isize, bool with_trailer, uint32_t* end) {
    static const uint16_t len_base[32] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258, 0, 0, 0};
    static const uint8_t len_extra[32] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0, 0, 0, 0};
    static const uint16_t dist_base[32] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577, 0, 0};
    static const uint8_t dist_extra[32] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 0, 0};
    if (n == 0 || n > (1u << 17) || isize > MAX_ISIZE) return n == 0 ? E_INPUT : E_TASK;
    const uint32_t lane = LCTY_INF_LANE;
    crc_init(st);
    Bits b{src, n, 0, 0, 0, 0};
    Out o{dst, isize, 0, 0, 0xFFFFFFFFu};
    uint32_t last = 0;
    while (!last) {
        refill(st, b);
        last = take(b, 1);
        const uint32_t type = take(b, 2);
        if (overrun(b)) return E_INPUT;
        if (type == 3) return E_BTYPE;
        if (type == 0) {
            drop(b, b.nbits & 7u);
            refill(st, b);
            const uint32_t len = take(b, 16);
            refill(st, b);
            const uint32_t nlen = take(b, 16);
            if (overrun(b)) return E_INPUT;
            if (len != (~nlen & 0xFFFFu)) return E_STORED;
            const uint32_t at = b.ip - b.nbits / 8;          // hold has whole bytes only
            if (at + len > n) return E_INPUT;
            for (uint32_t done = 0; done < len;) {
                const uint32_t k = len - done < RING / 2 ? len - done : RING / 2;
                if (!room(st, o, k)) return E_OVER;
                for (uint32_t i = lane; i < k; i += LCTY_INF_LANES) st->ring[(o.pos + i) & (RING - 1)] = src_byte(b, at + done + i);
                o.pos += k; done += k;
            }
            b.ip = at + len; b.loaded = b.ip & ~(WIN_CHUNK - 1); b.hold = 0; b.nbits = 0;
            continue;
        }
        uint32_t nlen = 288, ndist = 32;
        if (type == 1) { LCTY_INF_SYNC(); fixed_lengths(st); }
        else { const uint32_t e = dynamic_lengths(st, b, &nlen, &ndist); if (e) return e; }
        LCTY_INF_SYNC();
        const uint8_t* ll = st->lens + (type == 1 ? 0 : 32);
        if (type == 2 && LCTY_INF_UNI(ll[256]) == 0) return E_NO_EOB;
        if (build_code(ll, nlen, &st->lit, st->lit_tab, LIT_BITS, true)) return E_LITSET;
        if (build_code(ll + nlen, ndist, &st->dist, st->dist_tab, DIST_BITS, true)) return E_DISTSET;
        for (;;) {
            refill(st, b);
            const uint32_t sym = decode(b, &st->lit, st->lit_tab, LIT_BITS);
            if (overrun(b)) return E_INPUT;
            if (sym < 256) {
                if (!room(st, o, 1)) return E_OVER;
                if (lane == 0) st->ring[o.pos & (RING - 1)] = static_cast<uint8_t>(sym);
                o.pos++;
                continue;
            }
            if (sym == 256) break;
            if (sym >= 286) return E_LITSYM;                 // 286, 287, and the codes nobody has
            const uint32_t len = len_base[(sym - 257) & 31u] + take(b, len_extra[(sym - 257) & 31u]);
            refill(st, b);
            const uint32_t dsym = decode(b, &st->dist, st->dist_tab, DIST_BITS);
            if (overrun(b)) return E_INPUT;
            if (dsym >= 30) return E_DISTSYM;
            const uint32_t dist = dist_base[dsym & 31u] + take(b, dist_extra[dsym & 31u]);
            if (overrun(b)) return E_INPUT;
            if (dist > o.pos) return E_FAR;
            if (!room(st, o, len)) return E_OVER;
            // every source byte lies before pos: byte i of the match is byte i modulo dist of the dist bytes before it. A ring slot that
            // a byte of this match takes held a byte at or behind the one the same turn reads (dist <= RING), so no source is lost.
            LCTY_INF_SYNC();
            for (uint32_t i = lane; i < len; i += LCTY_INF_LANES) {
                const uint32_t from = o.pos - dist + (dist >= len ? i : i % dist);
                st->ring[(o.pos + i) & (RING - 1)] = st->ring[from & (RING - 1)];
            }
            o.pos += len;
        }
    }
    flush(st, o);
    const uint32_t at = static_cast<uint32_t>((used(b) + 7) / 8);
    if (end) *end = at;
    if (o.pos < isize) return E_SHORT;
    if (!with_trailer) return OK;
    if (at + 8 > n) return E_INPUT;
    uint32_t crc = 0, size = 0;
    for (uint32_t k = 0; k < 4; k++) { crc |= static_cast<uint32_t>(src_byte(b, at + k)) << (8 * k); size |= static_cast<uint32_t>(src_byte(b, at + 4 + k)) << (8 * k); }
    if (LCTY_INF_UNI(crc) != ~o.crc) return E_CRC;
    if (LCTY_INF_UNI(size) != o.pos) return E_ISIZE;
    return OK;
}

}  // namespace inflate
}  // namespace lcty
