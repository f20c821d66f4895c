// lcty_seq.hpp — the sequence primitives every stage shares, one definition each: base codes, the k-mer hash, canonical k-mers
// from ASCII and from the packed streams, the packing of a base, and the minimizer walk of the reference as it is written there.
// No state; host and device. This is where bit-exactness with the reference is decided (a tie rule, an UNDEF hash, a base that
// is not ACGT), so a stage that needs one of these calls it here and does not restate it.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace lcty {

constexpr uint64_t UNDEF64 = ~0ull;            // Kmer::UNDEF for u64 (src/seq/kmers.rs:45): the hash of a k-mer over a base that is not ACGT
// never a valid canonical k-mer for k <= 31 and never a minimizer (kmers.rs:27-30), hence the free marker of the key tables (lcty_table.hpp)

// A 0, C 1, G 2, T 3; anything else (N, IUPAC codes, lower case: the reference matches the four capitals only) is 4
__host__ __device__ inline uint32_t base_enc(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
// the base as an aligner sees it: every byte outside ACGT is N
__host__ __device__ inline uint8_t base_norm(uint8_t c) { return base_enc(c) < 4u ? c : static_cast<uint8_t>('N'); }

// Minimizer::fast_hash for u64 (kmers.rs:93-103)
__host__ __device__ inline uint64_t fast_hash64(uint64_t x) {
    x = ~x;
    x ^= x >> 23;
    x *= 0x2127599bf4325c37ull;
    x ^= x >> 47;
    return x;
}

// the slot hash of most of the project's own key tables (lcty_table.hpp: MixHash; not the reference's)
__host__ __device__ inline uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// Canonical k-mer (kmers::<_, CANONICAL>, kmers.rs:163-202) of the k ASCII bases from s[p] on, K = uint64_t (k <= 32) or unsigned
// __int128 (k <= 64). False: a base is not ACGT (the reference's UNDEF), *kmer is then not meaningful. *kmer is the smaller of the
// forward and the reverse-complement value; *forward says that it is the forward one, a palindrome (fw == rv) counting as forward.
// Callers: the `places` bit of the map index is *forward (fw <= rv), the key of the db tables is *kmer (min).
template <typename K>
__host__ __device__ inline bool canonical_kmer_ascii(const uint8_t* s, uint64_t p, uint32_t k, K* kmer, bool* forward = nullptr) {
    K fw = 0, rv = 0;
    bool ok = true;
    for (uint32_t t = 0; t < k; t++) {
        const uint32_t e = base_enc(s[p + t]);
        ok &= e < 4u;
        fw = (fw << 2) | (e & 3u);
        rv = (rv >> 2) | (static_cast<K>(3u - (e & 3u)) << (2 * k - 2));
    }
    const bool fwd = fw <= rv;
    *kmer = fwd ? fw : rv;
    if (forward) *forward = fwd;
    return ok;
}

// base `c` (ASCII) at position `at` of a packed read: two bits in bases2 (LSB first, 16 bases a word; 0 where the base is not ACGT),
// one bit in nmask (32 bases a word) where it is not. Both arrays are zero before the first base is packed.
// base_bits: the two values of one base, for a packer that builds whole words in registers (pack_kernel of lcty_fastx_device.hip).
__host__ __device__ inline void base_bits(uint8_t c, uint32_t& two, uint32_t& not_acgt) {
    const uint32_t e = base_enc(c);
    two = e < 4u ? e : 0u; not_acgt = e < 4u ? 0u : 1u;
}
inline void pack_base(uint32_t* bases2, uint32_t* nmask, uint64_t at, uint8_t c) {
    uint32_t two, not_acgt;
    base_bits(c, two, not_acgt);
    if (!not_acgt) bases2[at >> 4] |= two << (2 * (at & 15));
    else nmask[at >> 5] |= 1u << (at & 31);
}

// minimizers::<u64, _, CANONICAL or not> (kmers.rs:265-331) as written there, for the sequences the closed forms of the callers do not
// take (a base outside ACGT, a hash equal to UNDEF) and as the definition of what those forms compute:
//   - a ring of the last hashes; the running `h < best_hash` keeps the older of two equal hashes;
//   - a base outside ACGT encodes as 0 in both directions and sets first_kmer = i + k: hashes before first_kmer are UNDEF (298-306);
//   - when the best position leaves the window, find_min (243-258) rescans start..=i for the leftmost minimum; a window whose
//     minimum is UNDEF moves first_window on by w - 1 from its OLD value, not from i (318-324);
//   - a minimizer is reported when the best position passes the last reported one (326-329).
// base(i) -> 0..4, called once per i in ascending order; ring(j) -> reference to the hash slot of position j, a ring that holds at
// least w positions (the caller fills it with UNDEF64 first, as the reference does); emit(pos, hash, forward) with pos the first
// base of the k-mer. Forced inline, so that a kernel's code is what it was with the loop in its body. The forward flags of the
// last 64 positions are bits of one word (w < 64, kmers.rs:270). CANONICAL needs k <= 31; the other form takes k = 32 as well,
// hence its mask. len < 2^31 (both callers check): positions, first_kmer = i + k and first_window stay inside 32 bits.
// Instantiations: host_minimizers (lcty_recruit.hip: ASCII, canonical, with positions) and db_minim_walk_kernel (lcty_db.hip: ASCII,
// not canonical, one lane per sequence). walk_minimizers of lcty_recruit.hip (packed words, ring in LDS) is the same walk written
// out for the device; see DESIGN.md 4.16.
template <bool CANONICAL, class Base, class Ring, class Emit>
__host__ __device__ __forceinline__ void minimizers_as_written(uint32_t len, uint32_t k, uint32_t w, Base&& base, Ring&& ring, Emit&& emit) {
    const uint32_t k_1 = k - 1, w_1 = w - 1, rv_shift = 2 * k - 2;
    const uint64_t mask = (!CANONICAL && k == 32) ? ~0ull : (1ull << (2 * k)) - 1;
    uint64_t fw_kmer = 0, rv_kmer = 0, fwd_bits = ~0ull;              // forward flag of position j at bit j & 63
    int64_t last_pos = -1;
    uint32_t best_pos = 0;
    uint64_t best_hash = UNDEF64;
    uint32_t first_kmer = k_1, first_window = k_1 + w_1;
    for (uint32_t i = 0; i < len; i++) {
        const uint32_t e = base(i);
        uint64_t fw_enc = e, rv_enc = 3ull - e;
        if (e > 3u) { first_kmer = i + k; fw_enc = 0; rv_enc = 0; }
        fw_kmer = ((fw_kmer << 2) | fw_enc) & mask;
        if (CANONICAL) rv_kmer = (rv_kmer >> 2) | (rv_enc << rv_shift);
        const bool fwd = !CANONICAL || !(rv_kmer < fw_kmer);
        const uint64_t h = i < first_kmer ? UNDEF64 : fast_hash64(fwd ? fw_kmer : rv_kmer);
        ring(i) = h;
        if (CANONICAL) fwd_bits = (fwd_bits & ~(1ull << (i & 63u))) | (static_cast<uint64_t>(fwd) << (i & 63u));
        if (h < best_hash) { best_hash = h; best_pos = i; }
        if (i < first_window) continue;
        const uint32_t start = i - w_1;
        if (best_pos < start) {
            best_pos = start; best_hash = ring(start);
            for (uint32_t j = start + 1; j <= i; j++) { const uint64_t v = ring(j); if (v < best_hash) { best_pos = j; best_hash = v; } }
            if (best_hash == UNDEF64) { first_window = first_window + w_1; continue; }
        }
        if (static_cast<int64_t>(best_pos) > last_pos) {
            last_pos = best_pos;
            emit(best_pos - k_1, best_hash, ((fwd_bits >> (best_pos & 63u)) & 1ull) != 0);
        }
    }
}

#ifdef __HIPCC__
// Canonical k-mer (src/seq/kmers.rs:192-196) of the window starting at base q of a mate whose
// 2-bit stream starts at 64-bit word `w64` (mate offsets are multiples of 32 bases).
// The stream is LSB-first: x = sum enc[q+t] << 2t, hence rv = ~x (masked) and fw = digit-reverse(x). *forward as in
// canonical_kmer_ascii: fw <= rv, a palindrome counting as forward. w64[word + 1] is read only when the window reaches into it.
__device__ inline uint64_t canonical_kmer_2bit(const uint64_t* w64, uint32_t q, uint32_t k, bool* forward = nullptr) {
    const uint32_t word = q >> 5, sh = (q & 31u) * 2u;
    uint64_t x = w64[word] >> sh;
    if (sh + 2u * k > 64u) x |= w64[word + 1] << (64u - sh);
    const uint64_t mask = (1ull << (2u * k)) - 1ull;
    x &= mask;
    const uint64_t rv = (~x) & mask;
    uint64_t y = __brevll(x);
    y = ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
    const uint64_t fw = y >> (64u - 2u * k);
    if (forward) *forward = !(rv < fw);
    return rv < fw ? rv : fw;
}

// any "not ACGT" base inside [q, q+k) of the mate's 1-bit stream starting at 32-bit word `nm`
__device__ inline bool window_has_n(const uint32_t* nm, uint32_t q, uint32_t k) {
    const uint32_t w = q >> 5, s = q & 31u;
    uint32_t bits = nm[w] >> s;
    if (s + k > 32u) bits |= nm[w + 1] << (32u - s);
    return (bits & ((1u << k) - 1u)) != 0u;
}

// ---- k-mers of 32..63 bases (the reference keeps every k-mer of UniqueKmers in a u128, locs.rs:919-963): 128-bit keys as {lo, hi}
// pairs ----
struct Kmer128 { uint64_t lo, hi; };
__device__ __forceinline__ uint64_t pair_reverse64(uint64_t x) {
    const uint64_t y = __brevll(x);
    return ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
}
// canonical k-mer of the window at base q, 32 <= k <= 63 (the 64-bit form above, on two words)
__device__ inline Kmer128 canonical_kmer_2bit128(const uint64_t* w64, uint32_t q, uint32_t k) {
    const uint32_t word = q >> 5, sh = (q & 31u) * 2u, last = (q + k - 1) >> 5;
    const uint64_t a = w64[word], b = last > word ? w64[word + 1] : 0ull, c = last > word + 1 ? w64[word + 2] : 0ull;
    uint64_t xlo = a, xhi = b;
    if (sh) { xlo = (a >> sh) | (b << (64u - sh)); xhi = (b >> sh) | (c << (64u - sh)); }
    const uint32_t hb = 2u * k - 64u;                                    // bits of the k-mer in the high word: 0..62
    const uint64_t hmask = (1ull << hb) - 1ull;
    xhi &= hmask;
    const uint64_t rlo = ~xlo, rhi = (~xhi) & hmask;                      // the reverse complement's value
    const uint64_t ylo = pair_reverse64(xhi), yhi = pair_reverse64(xlo); // the digits of x in reverse order, at the top of 128 bits
    const uint32_t s = 128u - 2u * k;                                     // 2..64
    const uint64_t flo = s == 64u ? yhi : (ylo >> s) | (yhi << (64u - s)), fhi = s == 64u ? 0ull : yhi >> s;
    const bool rv_less = rhi < fhi || (rhi == fhi && rlo < flo);
    return rv_less ? Kmer128{rlo, rhi} : Kmer128{flo, fhi};
}
// any "not ACGT" base inside [q, q+k), k <= 63
__device__ inline bool window_has_n_wide(const uint32_t* nm, uint32_t q, uint32_t k) {
    const uint32_t w = q >> 5, s = q & 31u, last = (q + k - 1) >> 5;
    uint64_t bits = (static_cast<uint64_t>(nm[w]) | (last > w ? static_cast<uint64_t>(nm[w + 1]) << 32 : 0ull)) >> s;
    if (last > w + 1) bits |= static_cast<uint64_t>(nm[w + 2]) << (64u - s);       // s > 0 here: three words only with an offset
    return (bits & ((1ull << k) - 1ull)) != 0ull;
}
#endif

}  // namespace lcty
