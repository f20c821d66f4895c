// lcty_deflate.hpp — a raw DEFLATE encoder (RFC 1951) for one BGZF block of at most 0xff00 bytes, stated once for the host and the
// device. A group of LANES lanes encodes one block. On the device the group is a wavefront alone in its workgroup and
// State lies in LDS; compiled without HIP (scripts/deflate_probe_host.cpp) the group is one thread that runs the same bodies with a
// stride of one, which is how the text is tested and sanitized on the CPU. The bytes are a function of the block's bytes alone: the
// host build and the device build emit the same stream.
//   Matches: positions are taken in groups of GROUP, in order. Every position of a group first reads head[hash(4 bytes at p)], which
//   holds the latest position of earlier groups with that hash; then all insert themselves with an atomic maximum, which does not
//   depend on the order of the lanes. A position compares itself with distance 1 (runs) and with its candidate, byte by byte: length
//   3 .. 258 (a candidate counts from 4 bytes), distance 1 .. 32 768, never a byte at or behind the block's end. Positions a match
//   taken in an earlier group already covers are not compared.
//   Parse: greedy, inside the same loop: the starts of a group's tokens are walked from the bit mask of its matches, one step per
//   match taken (literals between two matches are one step together). tok[p] holds the token that starts at p, 0 where none does.
//   Forms: the histograms give the bit cost of the dynamic and the fixed form; stored is n + 5 bytes. The smallest in bytes is taken
//   (stored before fixed before dynamic on ties), so a block never takes more than n + 5 bytes.
//   Codes: symbols ranked by (count, symbol), lengths by the in-place minimum-redundancy construction of Moffat and Katajainen, then
//   limited by moving codes down from the deepest level until the Kraft sum is exactly 1 (15 bits, 7 for the code-length code);
//   codes are canonical. An alphabet with one used symbol gets a single code of 1 bit (the code-length code a second, unused one, so
//   that it is complete); no match in the block: no distance code at all (HDIST = 1, length 0).
//   Emission: the bit lengths of a group's tokens are scanned (wave_scan_incl of lcty_scan.hpp), every lane ORs its token's bits into
//   the 32-bit words of an output zeroed before; the header of a dynamic block is written by one lane.
//   Bounds: every index into the tables is masked or taken modulo the table, into the output clamped below cap_words, into tok and
//   the input below n; a task with n > MAX_IN or an output of less than n + 5 bytes is refused before anything is touched.
#pragma once

#include <cstdint>
#include <cstring>

#include "lcty_crc.hpp"

#ifdef __HIPCC__
#include "lcty_scan.hpp"
#define LCTY_DEF_FN __device__ __forceinline__
#else
#define LCTY_DEF_FN inline
#endif
#ifdef __HIP_DEVICE_COMPILE__
#define LCTY_DEF_LANE (threadIdx.x & 63u)
#define LCTY_DEF_LANES 64u
#define LCTY_DEF_SYNC() __syncthreads()                      // one wavefront per workgroup: orders its LDS and global traffic
#define LCTY_DEF_UNI(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#define LCTY_DEF_MAX(p, v) atomicMax((p), (v))
#define LCTY_DEF_ADD(p, v) atomicAdd((p), (v))
#define LCTY_DEF_OR(p, v) atomicOr((p), (v))
#else
#define LCTY_DEF_LANE 0u
#define LCTY_DEF_LANES 1u
#define LCTY_DEF_SYNC() ((void)0)
#define LCTY_DEF_UNI(x) static_cast<uint32_t>(x)
#define LCTY_DEF_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define LCTY_DEF_ADD(p, v) (*(p) += (v))
#define LCTY_DEF_OR(p, v) (*(p) |= (v))
#endif

namespace lcty {
namespace deflate {

enum : uint32_t { STORED = 0, FIXED = 1, DYNAMIC = 2, REFUSED = 0xFFFFFFFFu };

constexpr uint32_t MAX_IN = 0xff00, GROUP = 64, HASH_BITS = 12, MIN_MATCH = 3, MIN_CAND = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr uint32_t N_LIT = 286, N_DIST = 30, N_CL = 19, LIT_SLOTS = 288, MAX_BITS = 15, MAX_CL_BITS = 7, EOB = 256, NO_HASH = 0xFFFFFFFFu;
constexpr uint32_t TOK_LITERAL = 0x80000000u;                // tok: 0 none, TOK_LITERAL | byte, or length << 16 | distance - 1

struct State {
    uint32_t head[1u << HASH_BITS];      // position + 1 of the latest 4 bytes with this hash in the groups before, 0 = none
    uint32_t freq_lit[LIT_SLOTS], freq_dist[32], freq_cl[32];
    uint32_t key[LIT_SLOTS];             // code_lengths: the counts in rising order, then the tree in place
    uint16_t sym[LIT_SLOTS];             // whose they are
    uint16_t code_lit[LIT_SLOTS], code_dist[32], code_cl[32];      // bit-reversed: the first bit of the code is bit 0
    uint8_t len_lit[LIT_SLOTS], len_dist[32], len_cl[32];
    uint8_t lens[320];                   // literal/length lengths [0, hlit) and distance lengths behind them
    uint16_t rle[320];                   // the same run-length coded: code-length symbol | extra bits << 5
    uint32_t count[16], next[16];
    uint32_t crc_tab[256];
    uint32_t g_hash[GROUP], g_cand[GROUP], g_tok[GROUP];           // one group's values by lane
    uint32_t n_rle, hlit, hdist, hclen, form, bits;                // what lane 0 decided, for all lanes
};

LCTY_DEF_FN uint32_t load32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
LCTY_DEF_FN uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HASH_BITS); }
LCTY_DEF_FN uint32_t log2_floor(uint32_t v) { return 31u - static_cast<uint32_t>(__builtin_clz(v | 1u)); }

// length 3 .. 258 -> the index of its symbol behind 257, the number of extra bits and their value; the same for a distance - 1
LCTY_DEF_FN void length_symbol(uint32_t len, uint32_t* idx, uint32_t* xbits, uint32_t* xval) {
    const uint32_t l = len - 3;
    if (len >= MAX_MATCH) { *idx = 28; *xbits = 0; *xval = 0; return; }
    if (l < 8) { *idx = l; *xbits = 0; *xval = 0; return; }
    const uint32_t k = log2_floor(l) - 2;
    *idx = 4 * k + 4 + ((l >> k) & 3u); *xbits = k; *xval = l & ((1u << k) - 1u);
}
LCTY_DEF_FN void distance_symbol(uint32_t d, uint32_t* idx, uint32_t* xbits, uint32_t* xval) {
    if (d < 4) { *idx = d; *xbits = 0; *xval = 0; return; }
    const uint32_t k = log2_floor(d) - 1;
    *idx = 2 * k + 2 + ((d >> k) & 1u); *xbits = k; *xval = d & ((1u << k) - 1u);
}
LCTY_DEF_FN uint32_t length_extra(uint32_t idx) { return idx < 8 || idx >= 28 ? 0u : idx / 4 - 1; }
LCTY_DEF_FN uint32_t distance_extra(uint32_t idx) { return idx < 4 ? 0u : idx / 2 - 1; }
LCTY_DEF_FN uint32_t fixed_length(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

// bytes that src[p ..] and src[c ..] share, c < p < n: at most MAX_MATCH, and p + the result <= n
LCTY_DEF_FN uint32_t match_length(const uint8_t* src, uint32_t n, uint32_t p, uint32_t c) {
    const uint32_t max = n - p < MAX_MATCH ? n - p : MAX_MATCH;
    uint32_t l = 0;
    while (l + 4 <= max && load32(src + c + l) == load32(src + p + l)) l += 4;
    while (l < max && src[c + l] == src[p + l]) l++;
    return l;
}

// ---- code lengths -----------------------------------------------------------------------------------------------------------------------
// lens[0, n_sym) from freq[0, n_sym), n_sym <= LIT_SLOTS: 0 for a count of 0, else 1 .. max_bits with Kraft sum 1 (one used symbol: a
// single code of 1 bit; `complete` gives a second symbol the other one)
LCTY_DEF_FN void code_lengths(State* st, const uint32_t* freq, uint32_t n_sym, uint32_t max_bits, uint8_t* lens, bool complete) {
    LCTY_DEF_SYNC();
    for (uint32_t i = LCTY_DEF_LANE; i < n_sym; i += LCTY_DEF_LANES) {
        lens[i] = 0;
        const uint32_t f = freq[i];
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t j = 0; j < n_sym; j++) { const uint32_t g = freq[j]; r += (g && (g < f || (g == f && j < i))) ? 1u : 0u; }
        st->key[r % LIT_SLOTS] = f; st->sym[r % LIT_SLOTS] = static_cast<uint16_t>(i);
    }
    LCTY_DEF_SYNC();
    if (LCTY_DEF_LANE == 0) {
        uint32_t* A = st->key;
        int32_t n = 0;
        for (uint32_t i = 0; i < n_sym; i++) n += freq[i] ? 1 : 0;
        if (n == 1) {
            const uint32_t s = st->sym[0] % n_sym;
            lens[s] = 1;
            if (complete) lens[s == 0 ? 1 : 0] = 1;
        } else if (n >= 2) {
            // Moffat and Katajainen, "In-place calculation of minimum-redundancy codes" (1995): A rising -> the depth of every leaf
            A[0] += A[1];
            int32_t root = 0, leaf = 2;
            for (int32_t next = 1; next < n - 1; next++) {
                if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = static_cast<uint32_t>(next); } else A[next] = A[leaf++];
                if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = static_cast<uint32_t>(next); } else A[next] += A[leaf++];
            }
            A[n - 2] = 0;
            for (int32_t next = n - 3; next >= 0; next--) A[next] = A[A[next] % LIT_SLOTS] + 1;
            int32_t avbl = 1, used = 0, dpth = 0, next = n - 1;
            root = n - 2;
            while (avbl > 0 && next >= 0) {
                while (root >= 0 && static_cast<int32_t>(A[root]) == dpth) { used++; root--; }
                while (avbl > used && next >= 0) { A[next--] = static_cast<uint32_t>(dpth); avbl--; }
                avbl = 2 * used; dpth++; used = 0;
            }
            // the limit: every deeper leaf to max_bits, then codes moved one level down until the sum is 1
            for (uint32_t l = 0; l < 16; l++) st->count[l] = 0;
            for (int32_t i = 0; i < n; i++) st->count[A[i] < max_bits ? (A[i] ? A[i] : 1u) : max_bits]++;
            uint32_t total = 0;
            for (uint32_t l = max_bits; l > 0; l--) total += st->count[l] << (max_bits - l);
            while (total > (1u << max_bits)) {
                st->count[max_bits]--;
                for (uint32_t l = max_bits - 1; l > 0; l--) if (st->count[l]) { st->count[l]--; st->count[l + 1] += 2; break; }
                total--;
            }
            // the rarest symbols get the longest codes
            int32_t j = n;
            for (uint32_t l = 1; l <= max_bits; l++)
                for (uint32_t c = st->count[l]; c > 0 && j > 0; c--) lens[st->sym[--j] % n_sym] = static_cast<uint8_t>(l);
        }
    }
    LCTY_DEF_SYNC();
}

// canonical codes of lens[0, n), bit-reversed (one lane)
LCTY_DEF_FN void canonical_codes(State* st, const uint8_t* lens, uint32_t n, uint16_t* codes) {
    for (uint32_t l = 0; l < 16; l++) st->count[l] = 0;
    for (uint32_t i = 0; i < n; i++) st->count[lens[i] & 15u]++;
    st->count[0] = 0;
    uint32_t code = 0;
    st->next[0] = 0;
    for (uint32_t l = 1; l < 16; l++) { code = (code + st->count[l - 1]) << 1; st->next[l] = code; }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t l = lens[i] & 15u;
        uint32_t c = l ? st->next[l]++ : 0u, rev = 0;
        for (uint32_t k = 0; k < l; k++) rev |= ((c >> k) & 1u) << (l - 1 - k);
        codes[i] = static_cast<uint16_t>(rev);
    }
}

// ---- bits into the zeroed output ------------------------------------------------------------------------------------------------------
// v (at most 48 bits) at bit `pos`; a zero word is not stored, so nothing behind the stream's last word is touched
LCTY_DEF_FN void put_bits(uint32_t* out, uint32_t cap_words, uint32_t pos, uint64_t v) {
    const uint32_t w = pos >> 5, sh = pos & 31u, last = cap_words - 1;
    const uint64_t lo = v << sh;
    const uint32_t a = static_cast<uint32_t>(lo), b = static_cast<uint32_t>(lo >> 32), c = sh ? static_cast<uint32_t>(v >> (64 - sh)) : 0u;
    if (a) LCTY_DEF_OR(&out[w < last ? w : last], a);
    if (b) LCTY_DEF_OR(&out[w + 1 < last ? w + 1 : last], b);
    if (c) LCTY_DEF_OR(&out[w + 2 < last ? w + 2 : last], c);
}

// the bits of token t under the codes in st: *v (first bit = bit 0); returns their number, 0 for no token
LCTY_DEF_FN uint32_t token_bits(const State* st, uint32_t t, uint64_t* v) {
    if (!t) { *v = 0; return 0; }
    if (t & TOK_LITERAL) { *v = st->code_lit[t & 255u]; return st->len_lit[t & 255u]; }
    uint32_t li, lb, lv, di, db, dv;
    length_symbol((t >> 16) & 511u, &li, &lb, &lv);
    distance_symbol(t & 32767u, &di, &db, &dv);
    const uint32_t ls = (257 + li) % LIT_SLOTS;
    uint32_t nb = st->len_lit[ls];
    uint64_t x = st->code_lit[ls];
    x |= static_cast<uint64_t>(lv) << nb; nb += lb;
    x |= static_cast<uint64_t>(st->code_dist[di & 31u]) << nb; nb += st->len_dist[di & 31u];
    x |= static_cast<uint64_t>(dv) << nb; nb += db;
    *v = x;
    return nb;
}

// g[0, GROUP) -> the sums of the entries before each, from *carry on; *carry moves over the group
LCTY_DEF_FN void group_offsets(uint32_t* g, uint32_t* carry) {
    LCTY_DEF_SYNC();
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t x = g[LCTY_DEF_LANE], incl = wave_scan_incl(x, AddOp{});
    g[LCTY_DEF_LANE] = *carry + incl - x;
    *carry += LCTY_DEF_UNI(__shfl(incl, 63));
#else
    for (uint32_t j = 0; j < GROUP; j++) { const uint32_t x = g[j]; g[j] = *carry; *carry += x; }
#endif
    LCTY_DEF_SYNC();
}
// bit j: g[j] is not 0
LCTY_DEF_FN uint64_t group_mask(const uint32_t* g) {
#ifdef __HIP_DEVICE_COMPILE__
    return __ballot(g[LCTY_DEF_LANE] != 0);
#else
    uint64_t m = 0;
    for (uint32_t j = 0; j < GROUP; j++) m |= static_cast<uint64_t>(g[j] != 0) << j;
    return m;
#endif
}

// ---- CRC-32 of src[0, n) in CRC_SHARES shares (lcty_crc.hpp) -----------------------------------------------------------------------------
LCTY_DEF_FN uint32_t crc_of(State* st, const uint8_t* src, uint32_t n) {
    for (uint32_t i = LCTY_DEF_LANE; i < 256u; i += LCTY_DEF_LANES) st->crc_tab[i] = crc::crc_table_entry(i);
    LCTY_DEF_SYNC();
    const uint32_t per = (n + crc::CRC_SHARES - 1) / crc::CRC_SHARES;
    uint32_t sum = 0;
    for (uint32_t s = LCTY_DEF_LANE; s < crc::CRC_SHARES; s += LCTY_DEF_LANES) {
        uint32_t b = s * per, e = b + per;
        if (b > n) b = n;
        if (e > n) e = n;
        uint32_t r = 0;
        for (uint32_t i = b; i < e; i++) r = st->crc_tab[(r ^ src[i]) & 255u] ^ (r >> 8);
        if (e > b) sum ^= crc::crc_mul(r, crc::crc_xpow8(n - e));
    }
#ifdef __HIP_DEVICE_COMPILE__
    for (int o = 32; o; o >>= 1) sum ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(sum), o));
    sum = LCTY_DEF_UNI(sum);
#endif
    return ~(crc::crc_mul(0xFFFFFFFFu, crc::crc_xpow8(n)) ^ sum);
}

// ---- one block ----------------------------------------------------------------------------------------------------------------------
// src[0, n), n <= MAX_IN, as a raw DEFLATE stream that ends on a byte boundary in the bytes of out[0, cap_words); tok: MAX_IN words of
// scratch. Returns the stream's bytes (at most n + 5), REFUSED for a task outside its buffers; *crc the CRC-32 of src, *form the form.
LCTY_DEF_FN uint32_t deflate_block(State* st, uint32_t* tok, const uint8_t* src, uint32_t n, uint32_t* out, uint32_t cap_words, uint32_t* crc,
                                   uint32_t* form) {
    static const uint8_t order[N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    if (n > MAX_IN || static_cast<uint64_t>(cap_words) * 4 < n + 5ull) return REFUSED;
    const uint32_t lane = LCTY_DEF_LANE;
    LCTY_DEF_SYNC();                                         // the block before is done with st
    *crc = crc_of(st, src, n);
    for (uint32_t i = lane; i < (1u << HASH_BITS); i += LCTY_DEF_LANES) st->head[i] = 0;
    for (uint32_t i = lane; i < LIT_SLOTS; i += LCTY_DEF_LANES) { st->freq_lit[i] = i == EOB ? 1u : 0u; st->len_lit[i] = 0; st->code_lit[i] = 0; }
    for (uint32_t i = lane; i < 32u; i += LCTY_DEF_LANES) { st->freq_dist[i] = 0; st->freq_cl[i] = 0; st->len_dist[i] = 0; st->len_cl[i] = 0; st->code_dist[i] = 0; }
    LCTY_DEF_SYNC();

    // ---- matches, the greedy parse and the histograms, group by group
    uint32_t cur = 0;                                        // where the next token starts: the same in every lane
    for (uint32_t base = 0; base < n; base += GROUP) {
        for (uint32_t j = lane; j < GROUP; j += LCTY_DEF_LANES) {
            const uint32_t p = base + j;
            uint32_t h = NO_HASH, cand = 0;
            if (p + 4 <= n) { h = hash4(load32(src + p)); cand = st->head[h]; }
            st->g_hash[j] = h; st->g_cand[j] = cand;
        }
        LCTY_DEF_SYNC();
        for (uint32_t j = lane; j < GROUP; j += LCTY_DEF_LANES) {
            const uint32_t p = base + j, h = st->g_hash[j];
            if (h != NO_HASH) LCTY_DEF_MAX(&st->head[h & ((1u << HASH_BITS) - 1u)], p + 1);
            uint32_t len = 0, dist = 0;
            if (p < n && p >= cur) {
                if (p >= 1) { const uint32_t l = match_length(src, n, p, p - 1); if (l >= MIN_MATCH) { len = l; dist = 1; } }
                const uint32_t cand = st->g_cand[j];
                if (cand && cand <= p && p - (cand - 1) <= MAX_DIST && len < MAX_MATCH) {
                    const uint32_t l = match_length(src, n, p, cand - 1);
                    if (l >= MIN_CAND && l > len) { len = l; dist = p - (cand - 1); }
                }
            }
            st->g_tok[j] = len ? (len << 16) | (dist - 1) : 0u;
        }
        LCTY_DEF_SYNC();
        const uint64_t matches = group_mask(st->g_tok);
        const uint32_t end = n - base < GROUP ? n - base : GROUP;
#ifdef __HIP_DEVICE_COMPILE__
        const int own = static_cast<int>(st->g_tok[lane]);
#endif
        uint64_t starts = 0;
        while (cur < base + end) {
            uint32_t j = cur - base;                         // < end <= 64
            const uint64_t rest = matches >> j;
            uint32_t lits = rest ? static_cast<uint32_t>(__builtin_ctzll(rest)) : GROUP;
            if (lits > end - j) lits = end - j;
            if (lits) starts |= (lits >= 64 ? ~0ull : (1ull << lits) - 1ull) << j;
            cur += lits; j += lits;
            if (j < end) {                                   // a match starts at j
#ifdef __HIP_DEVICE_COMPILE__
                const uint32_t t = static_cast<uint32_t>(__builtin_amdgcn_readlane(own, static_cast<int>(j)));
#else
                const uint32_t t = st->g_tok[j];
#endif
                starts |= 1ull << j;
                cur += (t >> 16) & 511u;
            }
        }
        for (uint32_t j = lane; j < GROUP; j += LCTY_DEF_LANES) {
            const uint32_t p = base + j;
            if (p >= n) continue;
            uint32_t t = 0;
            if ((starts >> j) & 1ull) {
                t = st->g_tok[j];
                if (t) {
                    uint32_t li, lb, lv, di, db, dv;
                    length_symbol((t >> 16) & 511u, &li, &lb, &lv);
                    distance_symbol(t & 32767u, &di, &db, &dv);
                    LCTY_DEF_ADD(&st->freq_lit[(257 + li) % LIT_SLOTS], 1u);
                    LCTY_DEF_ADD(&st->freq_dist[di & 31u], 1u);
                } else {
                    t = TOK_LITERAL | src[p];
                    LCTY_DEF_ADD(&st->freq_lit[t & 255u], 1u);
                }
            }
            tok[p] = t;
        }
        LCTY_DEF_SYNC();
    }

    // ---- the codes of the dynamic form, its header run-length coded, and the cost of the three forms
    code_lengths(st, st->freq_lit, N_LIT, MAX_BITS, st->len_lit, false);
    code_lengths(st, st->freq_dist, N_DIST, MAX_BITS, st->len_dist, false);
    if (lane == 0) {
        uint32_t hlit = N_LIT, hdist = N_DIST;
        while (hlit > 257 && !st->len_lit[hlit - 1]) hlit--;
        while (hdist > 1 && !st->len_dist[hdist - 1]) hdist--;
        for (uint32_t i = 0; i < hlit; i++) st->lens[i] = st->len_lit[i];
        for (uint32_t i = 0; i < hdist; i++) st->lens[hlit + i] = st->len_dist[i];
        const uint32_t total = hlit + hdist;
        uint32_t m = 0;
        auto emit = [&](uint32_t s, uint32_t x) { st->rle[m % 320u] = static_cast<uint16_t>(s | (x << 5)); m++; st->freq_cl[s & 31u]++; };
        for (uint32_t i = 0; i < total;) {
            const uint32_t v = st->lens[i];
            uint32_t run = 1;
            while (i + run < total && st->lens[i + run] == v) run++;
            uint32_t r = run;
            if (v == 0) {
                while (r >= 11) { const uint32_t k = r < 138 ? r : 138; emit(18, k - 11); r -= k; }
                if (r >= 3) { emit(17, r - 3); r = 0; }
                while (r) { emit(0, 0); r--; }
            } else {
                emit(v, 0); r--;
                while (r >= 3) { const uint32_t k = r < 6 ? r : 6; emit(16, k - 3); r -= k; }
                while (r) { emit(v, 0); r--; }
            }
            i += run;
        }
        st->n_rle = m; st->hlit = hlit; st->hdist = hdist;
    }
    code_lengths(st, st->freq_cl, N_CL, MAX_CL_BITS, st->len_cl, true);
    if (lane == 0) {
        uint32_t hclen = N_CL;
        while (hclen > 4 && !st->len_cl[order[hclen - 1]]) hclen--;
        uint64_t dyn = 3 + 14 + 3 * hclen, fix = 3;
        for (uint32_t s = 0; s < N_CL; s++) dyn += static_cast<uint64_t>(st->freq_cl[s]) * (st->len_cl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
        for (uint32_t s = 0; s < N_LIT; s++) {
            const uint32_t x = s > 256 ? length_extra(s - 257) : 0u;
            dyn += static_cast<uint64_t>(st->freq_lit[s]) * (st->len_lit[s] + x);
            fix += static_cast<uint64_t>(st->freq_lit[s]) * (fixed_length(s) + x);
        }
        for (uint32_t s = 0; s < N_DIST; s++) {
            dyn += static_cast<uint64_t>(st->freq_dist[s]) * (st->len_dist[s] + distance_extra(s));
            fix += static_cast<uint64_t>(st->freq_dist[s]) * (5u + distance_extra(s));
        }
        const uint64_t dyn_bytes = (dyn + 7) / 8, fix_bytes = (fix + 7) / 8, stored_bytes = n + 5ull;
        uint32_t f = DYNAMIC;
        if (stored_bytes <= fix_bytes && stored_bytes <= dyn_bytes) f = STORED;
        else if (fix_bytes <= dyn_bytes) f = FIXED;
        st->form = f; st->hclen = hclen;
        st->bits = static_cast<uint32_t>(f == STORED ? 8 * stored_bytes : f == FIXED ? fix : dyn);
        if (f == FIXED) {
            for (uint32_t s = 0; s < LIT_SLOTS; s++) st->len_lit[s] = static_cast<uint8_t>(fixed_length(s));
            for (uint32_t s = 0; s < 32u; s++) st->len_dist[s] = 5;
        }
        if (f != STORED) {
            canonical_codes(st, st->len_lit, LIT_SLOTS, st->code_lit);
            canonical_codes(st, st->len_dist, 32, st->code_dist);
            canonical_codes(st, st->len_cl, N_CL, st->code_cl);
        }
    }
    LCTY_DEF_SYNC();
    const uint32_t f = LCTY_DEF_UNI(st->form), bits = LCTY_DEF_UNI(st->bits), bytes = (bits + 7) / 8;
    *form = f;
    if (f == STORED) {
        uint8_t* o = reinterpret_cast<uint8_t*>(out);
        if (lane == 0) { o[0] = 1; o[1] = static_cast<uint8_t>(n); o[2] = static_cast<uint8_t>(n >> 8); o[3] = static_cast<uint8_t>(~n); o[4] = static_cast<uint8_t>(~n >> 8); }
        for (uint32_t i = lane; i < n; i += LCTY_DEF_LANES) o[5 + i] = src[i];
        LCTY_DEF_SYNC();
        return n + 5;
    }

    // ---- emission: bytes <= n + 5 <= 4 cap_words
    for (uint32_t i = lane; i < (bytes + 3) / 4 && i < cap_words; i += LCTY_DEF_LANES) out[i] = 0;
    LCTY_DEF_SYNC();
    uint32_t pos = 0;
    if (f == FIXED) {
        if (lane == 0) put_bits(out, cap_words, 0, 1u | (1u << 1));
        pos = 3;
    } else {
        const uint32_t hlit = LCTY_DEF_UNI(st->hlit), hdist = LCTY_DEF_UNI(st->hdist), hclen = LCTY_DEF_UNI(st->hclen), m = LCTY_DEF_UNI(st->n_rle);
        if (lane == 0) put_bits(out, cap_words, 0, 1u | (2u << 1) | ((hlit - 257) << 3) | ((hdist - 1) << 8) | ((hclen - 4) << 13));
        for (uint32_t i = lane; i < hclen; i += LCTY_DEF_LANES) put_bits(out, cap_words, 17 + 3 * i, st->len_cl[order[i % N_CL]]);
        pos = 17 + 3 * hclen;
        for (uint32_t b0 = 0; b0 < m; b0 += GROUP) {
            for (uint32_t j = lane; j < GROUP; j += LCTY_DEF_LANES) {
                const uint32_t r = b0 + j < m ? st->rle[(b0 + j) % 320u] : 0u, s = r & 31u;
                st->g_hash[j] = b0 + j < m ? st->len_cl[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u) : 0u;
            }
            group_offsets(st->g_hash, &pos);
            for (uint32_t j = lane; j < GROUP; j += LCTY_DEF_LANES) {
                if (b0 + j >= m) continue;
                const uint32_t r = st->rle[(b0 + j) % 320u], s = r & 31u;
                put_bits(out, cap_words, st->g_hash[j], st->code_cl[s] | (static_cast<uint64_t>(r >> 5) << st->len_cl[s]));
            }
        }
    }
    for (uint32_t base = 0; base < n; base += GROUP) {
        for (uint32_t j = lane; j < GROUP; j += LCTY_DEF_LANES) {
            const uint32_t p = base + j, t = p < n ? tok[p] : 0u;
            uint64_t v;
            st->g_tok[j] = t;
            st->g_hash[j] = token_bits(st, t, &v);
        }
        group_offsets(st->g_hash, &pos);
        for (uint32_t j = lane; j < GROUP; j += LCTY_DEF_LANES) {
            uint64_t v;
            if (token_bits(st, st->g_tok[j], &v)) put_bits(out, cap_words, st->g_hash[j], v);
        }
    }
    if (lane == 0) put_bits(out, cap_words, pos, st->code_lit[EOB]);
    LCTY_DEF_SYNC();
    return bytes;
}

}  // namespace deflate
}  // namespace lcty
