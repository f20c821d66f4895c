// lcty_db.hip — locus database build: what `locityper target` does to the alleles of one locus (process_alleles, command/add.rs:585-652)
// once their sequences, the reference sequence of the locus and the k-mer counts of both are known.
//   minimizer lists      kmers::minimizers::<u64, _, NON_CANONICAL> + sort_unstable (seq/kmers.rs:265-331, seq/minim_div.rs:53-61)
//   all-pairs divergence jaccard_distance over TriangleMatrix::indices (minim_div.rs:16-40, ext/trimat.rs:15-17)
//   off-target counts    KmerCounts::off_target_counts (seq/counts.rs:180-230) with the preparation of add.rs:626-644
//   discard_identical    add.rs:546-582
// Out of scope (include/locityper_hip.h says so too): running Jellyfish, pangenome-VCF reconstruction and locus expansion, ref.bed, lock
// and success files, haplotype-to-haplotype alignment, prune / augment.
//
// Everything here is integer work; the one f64 (the divergence) is a single IEEE division made on the host.
//
// The divergence is NOT computed by merging lists. With c_a[h] the multiplicity of hash h in the list of haplotype a, the merge of
// minim_div.rs:23-33 (equal heads advance both sides) counts overlap(i, j) = sum_h min(c_i[h], c_j[h]), and
//   min(c_i, c_j) = sum_{t >= 1} [c_i >= t] [c_j >= t],
// so with one column per distinct (hash, t) — t-th copy of the hash — every haplotype is a row of bits and overlap = B B^T, a 0/1 Gram
// matrix: popcount(x & y) over 64-bit words. The column of (hash, t) is base[hash] + t - 1, base handed out by an atomic counter over a
// device hash table of the distinct hashes (any bijection serves: the sums are integer, their order does not matter). Columns are
// processed in chunks so that the bit matrix keeps to a fixed budget; the u32 overlap triangle accumulates over the chunks.
#include "lcty_bitonic.hpp"
#include "lcty_common.hpp"
#include "lcty_seq.hpp"
#include "lcty_table.hpp"

#include <algorithm>
#include <thread>
#include <unordered_map>

namespace {
using namespace lcty;

constexpr uint32_t kSortCap = 8192;                        // entries a workgroup sorts in LDS (64 KB); longer lists are sorted on the host
constexpr uint32_t kTile = 1024;                           // k-mer end positions per workgroup of the clean-sequence minimizer kernel
constexpr uint32_t kMaxW = 63;

// ---- minimizers -------------------------------------------------------------------------------------------------------------------------
// flags[a] = 1: the sequence holds a base outside ACGT, or one of its k-mers hashes to UNDEF (one 64-bit value in 2^64 does): the
// stateful rules of kmers.rs:298-324 apply and the sequence takes the serial walk.
__global__ __launch_bounds__(256) void db_classify_kernel(const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ seq_off, uint32_t k,
                                                          uint32_t* __restrict__ flags) {
    const uint32_t a = blockIdx.x;
    const uint8_t* s = seqs + seq_off[a];
    const uint64_t len = seq_off[a + 1] - seq_off[a];
    bool bad = false;
    for (uint64_t p = uint64_t(blockIdx.y) * 256 + threadIdx.x; p < len; p += uint64_t(gridDim.y) * 256) {
        if (base_enc(s[p]) > 3) { bad = true; break; }
        if (p + 1 >= k) {
            uint64_t km = 0;
            for (uint32_t t = 0; t < k; t++) km = (km << 2) | (base_enc(s[p + 1 - k + t]) & 3);
            if (fast_hash64(km) == UNDEF64) { bad = true; break; }
        }
    }
    if (bad) flags[a] = 1;
}

// Clean sequences. Position p (the last base of a k-mer, k - 1 <= p < len) is pushed by the reference iff it is the leftmost minimum of
// some window of w consecutive k-mers: the running update `h < best_hash` keeps the older of two equal hashes and find_min the leftmost,
// so `best` is the leftmost minimum of the current window at every step, its position never moves back, and `best_pos > last_pos`
// pushes each such position once. With l = the hashes directly left of p that are GREATER (at most w - 1, not past k - 1) and r = the
// hashes directly right of p that are GREATER OR EQUAL (at most w - 1, not past len - 1), such a window exists iff l + r + 1 >= w.
template <bool WRITE>
__global__ __launch_bounds__(256) void db_minim_fast_kernel(const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ seq_off,
                                                            const uint32_t* __restrict__ flags, uint32_t k, uint32_t w,
                                                            unsigned long long* __restrict__ cnt, const uint64_t* __restrict__ min_off,
                                                            uint64_t* __restrict__ out) {
    __shared__ uint64_t hs[kTile + 2 * kMaxW];
    __shared__ uint64_t found[kTile];
    __shared__ uint32_t n_found;
    __shared__ unsigned long long base;
    const uint32_t a = blockIdx.x;
    if (flags[a]) return;
    const uint8_t* s = seqs + seq_off[a];
    const int64_t len = int64_t(seq_off[a + 1] - seq_off[a]);
    if (len < int64_t(k) + w - 1) return;                                    // no full window
    const int64_t first = int64_t(k) - 1, last = len - 1;
    const int64_t p0 = first + int64_t(blockIdx.y) * kTile;                  // this workgroup's positions: [p0, p0 + kTile)
    if (p0 > last) return;
    const int64_t lo = p0 - (int64_t(w) - 1) > first ? p0 - (int64_t(w) - 1) : first;
    const int64_t hi = p0 + kTile - 1 + (int64_t(w) - 1) < last ? p0 + kTile - 1 + (int64_t(w) - 1) : last;
    if (threadIdx.x == 0) n_found = 0;
    for (int64_t q = lo + threadIdx.x; q <= hi; q += 256) {
        uint64_t km = 0;
        for (uint32_t t = 0; t < k; t++) km = (km << 2) | base_enc(s[q + 1 - k + t]);
        hs[q - lo] = fast_hash64(km);
    }
    __syncthreads();
    for (int64_t p = p0 + threadIdx.x; p < p0 + kTile && p <= last; p += 256) {
        const uint64_t h = hs[p - lo];
        uint32_t l = 0, r = 0;
        while (l < w - 1 && p - 1 - l >= first && hs[p - 1 - l - lo] > h) l++;
        while (r < w - 1 && p + 1 + r <= last && hs[p + 1 + r - lo] >= h) r++;
        if (l + r + 1 >= w) found[atomicAdd(&n_found, 1u)] = h;
    }
    __syncthreads();
    if (threadIdx.x == 0) base = atomicAdd(&cnt[a], static_cast<unsigned long long>(n_found));
    if (WRITE) {
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < n_found; t += 256) out[min_off[a] + base + t] = found[t];
    }
}

// The loop of the reference as written (minimizers_as_written, lcty_seq.hpp: not canonical, k up to 32), one lane per sequence, the
// ring of hashes in the lane's private memory.
template <bool WRITE>
__global__ __launch_bounds__(64) void db_minim_walk_kernel(const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ seq_off,
                                                           const uint32_t* __restrict__ list, uint32_t n_list, uint32_t k, uint32_t w,
                                                           unsigned long long* __restrict__ cnt, const uint64_t* __restrict__ min_off,
                                                           uint64_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_list) return;
    const uint32_t a = list[t];
    const uint8_t* s = seqs + seq_off[a];
    const uint64_t len = seq_off[a + 1] - seq_off[a];
    uint64_t hashes[64], m = 0;
    for (uint32_t q = 0; q < 64; q++) hashes[q] = UNDEF64;
    uint64_t* dst = WRITE ? out + min_off[a] : nullptr;
    minimizers_as_written<false>(static_cast<uint32_t>(len), k, w,                // check_db_haps: fewer than 2^31 bases
        [&](uint32_t i) { return base_enc(s[i]); },
        [&](uint32_t j) -> uint64_t& { return hashes[j & 63]; },
        [&](uint32_t, uint64_t h, bool) { if (WRITE) dst[m] = h; m++; });
    cnt[a] = m;
}

// One workgroup sorts one list in LDS (the bitonic network of lcty_bitonic.hpp over the next power of two, padded with all-ones, which sort last).
__global__ __launch_bounds__(1024) void db_sort_kernel(uint64_t* __restrict__ hashes, const uint64_t* __restrict__ min_off) {
    __shared__ uint64_t s[kSortCap];
    const uint32_t a = blockIdx.x;
    const uint64_t n = min_off[a + 1] - min_off[a];
    if (n < 2 || n > kSortCap) return;
    uint64_t* v = hashes + min_off[a];
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t t = threadIdx.x; t < P; t += 1024) s[t] = t < n ? v[t] : UNDEF64;
    __syncthreads();
    bitonic_sort_lds<1024>(P, BitonicKeys{s});
    for (uint32_t t = threadIdx.x; t < n; t += 1024) v[t] = s[t];
}

// ---- column index -----------------------------------------------------------------------------------------------------------------------
// A key table over the distinct hashes (lcty_table.hpp). A list can hold UNDEF (k = w = 1 and a non-ACGT first base push it,
// kmers.rs:326-329), which equals the free marker and is never stored: its columns live in slot `cap`, one behind the table.
__device__ inline uint64_t lower_bound_dev(const uint64_t* v, uint64_t n, uint64_t h) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (v[mid] < h) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the last entry of every run of equal hashes enters the hash with the length of its run: mult[slot] = max_a c_a[h]
__global__ __launch_bounds__(256) void db_runs_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ min_off,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ mult, uint64_t cap) {
    const uint32_t a = blockIdx.x;
    const uint64_t* v = hashes + min_off[a];
    const uint64_t n = min_off[a + 1] - min_off[a];
    for (uint64_t i = uint64_t(blockIdx.y) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.y) * 256) {
        const uint64_t h = v[i];
        if (i + 1 < n && v[i + 1] == h) continue;
        const uint64_t run = i - lower_bound_dev(v, n, h) + 1;
        const uint64_t slot = h == UNDEF64 ? cap : keytable::claim<keytable::MulHash, UNDEF64>(keys, cap - 1, h).slot;
        atomicMax(&mult[slot], static_cast<uint32_t>(run));
    }
}
__global__ __launch_bounds__(256) void db_bases_kernel(const uint32_t* __restrict__ mult, uint32_t* __restrict__ base, uint64_t n_slots,
                                                       uint32_t* __restrict__ n_cols) {
    const uint64_t s = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (s < n_slots && mult[s]) base[s] = atomicAdd(n_cols, mult[s]);
}
// column of entry i of list a: base[hash] + its rank within its run
__global__ __launch_bounds__(256) void db_cols_kernel(const uint64_t* __restrict__ hashes, const uint64_t* __restrict__ min_off,
                                                      const uint64_t* __restrict__ keys, const uint32_t* __restrict__ base, uint64_t cap,
                                                      uint32_t* __restrict__ col) {
    const uint32_t a = blockIdx.x;
    const uint64_t* v = hashes + min_off[a];
    const uint64_t n = min_off[a + 1] - min_off[a];
    for (uint64_t i = uint64_t(blockIdx.y) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.y) * 256) {
        const uint64_t h = v[i];
        const uint64_t slot = h == UNDEF64 ? cap : keytable::find<keytable::MulHash, UNDEF64>(keys, cap - 1, h).slot;      // db_runs_kernel claimed it
        col[min_off[a] + i] = base[slot] + static_cast<uint32_t>(i - lower_bound_dev(v, n, h));
    }
}
// bits of the columns [c0, c1) of every row; B[n_pad][W] 64-bit words, W * 64 >= c1 - c0
__global__ __launch_bounds__(256) void db_bits_kernel(const uint32_t* __restrict__ col, const uint64_t* __restrict__ min_off, uint32_t c0, uint32_t c1,
                                                      unsigned long long* __restrict__ B, uint64_t W) {
    const uint32_t a = blockIdx.x;
    const uint64_t n = min_off[a + 1] - min_off[a];
    const uint32_t* c = col + min_off[a];
    for (uint64_t i = uint64_t(blockIdx.y) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.y) * 256) {
        const uint32_t x = c[i];
        if (x >= c0 && x < c1) atomicOr(&B[uint64_t(a) * W + ((x - c0) >> 6)], 1ull << ((x - c0) & 63));
    }
}

// ---- the Gram tile kernel -----------------------------------------------------------------------------------------------------------------
// ov[tri(i, j)] += popcount(B[i] & B[j]) for a 64 x 64 block of pairs per workgroup, 32 words of both row blocks staged in LDS per step.
// A thread owns the 4 x 4 pairs (ty + 16 a, tx + 16 b): the 16 lanes that differ in tx read 16 consecutive rows of the padded image
// (33 words a row: banks 2 tx + 2 kk, no conflict), the lanes that share ty read one address (broadcast). Per word and pair: two
// v_and_b32 and two v_bcnt_u32_b32 (the count adds into the accumulator), 8 ds_read_b64 per 16 pairs.
constexpr uint32_t kGB = 64, kGK = 32, kGP = kGK + 1;
__global__ __launch_bounds__(256) void db_gram_kernel(const uint64_t* __restrict__ B, uint64_t W, uint32_t n, uint32_t* __restrict__ ov) {
    if (blockIdx.x < blockIdx.y) return;                                      // blocks on and above the diagonal: column block >= row block
    __shared__ uint64_t xs[kGB * kGP], ys[kGB * kGP];
    const uint32_t bi = blockIdx.y, bj = blockIdx.x;
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint32_t lr = threadIdx.x >> 2, lw = (threadIdx.x & 3) * 8;         // staging: row and first word of this thread's 8 words
    const uint64_t* gx = B + (uint64_t(bi) * kGB + lr) * W + lw;
    const uint64_t* gy = B + (uint64_t(bj) * kGB + lr) * W + lw;
    uint32_t acc[4][4] = {};
    for (uint64_t k0 = 0; k0 < W; k0 += kGK) {
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) {
            xs[lr * kGP + lw + q] = gx[k0 + q];
            ys[lr * kGP + lw + q] = gy[k0 + q];
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t kk = 0; kk < kGK; kk++) {
            uint64_t x[4], y[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) { x[q] = xs[(ty + 16 * q) * kGP + kk]; y[q] = ys[(tx + 16 * q) * kGP + kk]; }
#pragma unroll
            for (uint32_t p = 0; p < 4; p++)
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) acc[p][q] += __popcll(x[p] & y[q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t p = 0; p < 4; p++)
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint64_t i = uint64_t(bi) * kGB + ty + 16 * p, j = uint64_t(bj) * kGB + tx + 16 * q;
            if (i < j && j < n) ov[i * (2 * uint64_t(n) - i - 1) / 2 + (j - i - 1)] += acc[p][q];     // TriangleMatrix::indices: rows i, then j > i
        }
}

// ---- off-target counts (k <= 31: 64-bit canonical k-mers; all-ones = a k-mer over a non-ACGT base, Kmer::UNDEF) -------------------------
// the key of the tables is the value of canonical_kmer_ascii: min(fw, rv)
__global__ __launch_bounds__(256) void db_ref_insert_kernel(const uint8_t* __restrict__ ref, uint64_t n_kmers, uint32_t k, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ first, uint32_t* __restrict__ occ, uint64_t cap) {
    const uint64_t p = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (p >= n_kmers) return;
    uint64_t km;
    if (!canonical_kmer_ascii(ref, p, k, &km)) return;                                              // the map's UNDEF entry is max_value whatever happens (counts.rs:198, 202)
    const uint64_t s = keytable::claim<keytable::MulHash, UNDEF64>(keys, cap - 1, km).slot;      // a k-mer of k <= 31 bases is never all-ones
    atomicMin(&first[s], static_cast<uint32_t>(p));
    atomicAdd(&occ[s], 1u);
}
__global__ __launch_bounds__(256) void db_ref_value_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ first, const uint32_t* __restrict__ occ,
                                                           uint64_t cap, const uint16_t* __restrict__ ref_counts, uint32_t max_value,
                                                           uint16_t* __restrict__ value, uint32_t* __restrict__ negatives) {
    const uint64_t s = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (s >= cap || keys[s] == UNDEF64) return;
    const uint32_t f = ref_counts[first[s]], m = occ[s];
    value[s] = static_cast<uint16_t>(f == max_value ? f : (f > m ? f - m : 0));
    if (f != max_value && m > f) *negatives = 1;
}
__global__ __launch_bounds__(256) void db_offt_kernel(const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ seq_off, const uint16_t* __restrict__ counts,
                                                      const uint64_t* __restrict__ cnt_off, uint32_t k, const uint64_t* __restrict__ keys,
                                                      const uint16_t* __restrict__ value, uint64_t cap, uint32_t max_value, uint16_t* __restrict__ out) {
    const uint32_t a = blockIdx.x;
    const uint8_t* s = seqs + seq_off[a];
    const uint64_t n = cnt_off[a + 1] - cnt_off[a];
    for (uint64_t p = uint64_t(blockIdx.y) * 256 + threadIdx.x; p < n; p += uint64_t(gridDim.y) * 256) {
        uint64_t km;
        uint16_t v;
        if (!canonical_kmer_ascii(s, p, k, &km)) v = static_cast<uint16_t>(max_value);
        else {
            const keytable::Probe at = keytable::find<keytable::MulHash, UNDEF64>(keys, cap - 1, km);
            v = at.found ? value[at.slot] : counts[cnt_off[a] + p];
        }
        out[cnt_off[a] + p] = v;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// what the kernels here take: positions inside a sequence are 31 bits wide
HapSet check_db_haps(uint32_t n, const uint8_t* seqs, const uint64_t* seq_off, uint32_t min_seqs) {
    return check_haps(n, seqs, seq_off, HapLimits{min_seqs, UINT32_MAX, 1ull << 31});
}
void check_kw(uint32_t k, uint32_t w) {
    if (k < 1 || k > 32) fail(LCTY_ERR_INVALID_INPUT, "minimizer k = %u: must be 1..32 (64-bit k-mers)", k);
    if (w < 1 || w > kMaxW)
        fail(LCTY_ERR_INVALID_INPUT, "minimizer window w = %u: must be 1..63 (the circular array of kmers.rs:205-236 holds 64 hashes and the "
             "loop asserts w < 64)", w);
}
dim3 per_allele_grid(uint32_t n, uint64_t max_items) {
    return dim3(n, static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>((max_items + 255) / 256, 1), 64)));
}

struct Lists {
    DevBuf<uint64_t> hashes, d_off;
    std::vector<uint64_t> off;        // [n + 1]
    uint64_t max_n = 0;
};

// sorted minimizer lists of every sequence on the device
void build_lists(lcty_ctx* ctx, const HapSet& hs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t k, uint32_t w, Lists& L, lcty_db_stats& st) {
    hipStream_t s = ctx->stream;
    double t0 = now_ms();
    const uint32_t n = hs.n;
    const uint64_t max_len = hs.max_len;
    DevHaps d; DevBuf<uint32_t> d_flags, d_list; DevBuf<unsigned long long> d_cnt;
    d_flags.alloc(n); d_cnt.alloc(n);
    st.bytes_h2d += d.upload(ctx, hs, seqs, seq_off, 0);
    d_flags.zero(s); d_cnt.zero(s);
    hipLaunchKernelGGL(db_classify_kernel, per_allele_grid(n, max_len), dim3(256), 0, s, d.seqs.p, d.off.p, k, d_flags.p);
    std::vector<uint32_t> flags(n), walk;
    d_flags.download(flags.data(), n, s);
    LCTY_HIP(hipStreamSynchronize(s));
    for (uint32_t a = 0; a < n; a++) if (flags[a]) walk.push_back(a);
    st.n_walk += walk.size(); st.n_fast += n - walk.size();
    if (!walk.empty()) { d_list.alloc(walk.size()); d_list.upload(walk.data(), walk.size(), s); }
    const uint32_t n_walk = static_cast<uint32_t>(walk.size());
    const dim3 fast_grid(n, static_cast<uint32_t>(std::max<uint64_t>((max_len + kTile - 1) / kTile, 1)));
    if (fast_grid.y > 65535) fail(LCTY_ERR_UNSUPPORTED, "a sequence of %llu bases: more than 65 535 tiles", static_cast<unsigned long long>(max_len));
    // pass 1: lengths of the lists
    hipLaunchKernelGGL(db_minim_fast_kernel<false>, fast_grid, dim3(256), 0, s, d.seqs.p, d.off.p, d_flags.p, k, w, d_cnt.p, nullptr, nullptr);
    if (n_walk) hipLaunchKernelGGL(db_minim_walk_kernel<false>, dim3((n_walk + 63) / 64), dim3(64), 0, s, d.seqs.p, d.off.p, d_list.p, n_walk, k, w, d_cnt.p, nullptr, nullptr);
    std::vector<unsigned long long> cnt(n);
    d_cnt.download(cnt.data(), n, s);
    LCTY_HIP(hipStreamSynchronize(s));
    L.off.assign(n + 1, 0);
    L.max_n = 0;
    for (uint32_t a = 0; a < n; a++) { L.off[a + 1] = L.off[a] + cnt[a]; L.max_n = std::max<uint64_t>(L.max_n, cnt[a]); }
    const uint64_t total = L.off[n];
    if (total >= (1ull << 32)) fail(LCTY_ERR_UNSUPPORTED, "%llu minimizers: the column index is 32 bits wide", static_cast<unsigned long long>(total));
    L.hashes.alloc(std::max<uint64_t>(total, 1)); L.d_off.alloc(n + 1);
    L.d_off.upload(L.off.data(), n + 1, s);
    d_cnt.zero(s);
    // pass 2: the hashes (the clean kernel places them in any order inside a list: the list is sorted next)
    hipLaunchKernelGGL(db_minim_fast_kernel<true>, fast_grid, dim3(256), 0, s, d.seqs.p, d.off.p, d_flags.p, k, w, d_cnt.p, L.d_off.p, L.hashes.p);
    if (n_walk) hipLaunchKernelGGL(db_minim_walk_kernel<true>, dim3((n_walk + 63) / 64), dim3(64), 0, s, d.seqs.p, d.off.p, d_list.p, n_walk, k, w, d_cnt.p, L.d_off.p, L.hashes.p);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));
    double t1 = now_ms();
    st.minim_ms += t1 - t0;
    st.n_minimizers += total;
    // sort: lists of up to kSortCap entries in LDS, longer ones on the host
    hipLaunchKernelGGL(db_sort_kernel, dim3(n), dim3(1024), 0, s, L.hashes.p, L.d_off.p);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));
    double t2 = now_ms();
    st.sort_ms += t2 - t1;
    std::vector<uint32_t> big;
    for (uint32_t a = 0; a < n; a++) if (cnt[a] > kSortCap) big.push_back(a);
    if (!big.empty()) {
        const unsigned n_thr = static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(ctx->knob("host_threads", 16), 1), 64));
        std::vector<std::vector<uint64_t>> bufs(big.size());
        for (size_t b = 0; b < big.size(); b++) {
            bufs[b].resize(cnt[big[b]]);
            L.hashes.download(bufs[b].data(), bufs[b].size(), s, L.off[big[b]]);
            st.bytes_d2h += 8 * bufs[b].size();
        }
        LCTY_HIP(hipStreamSynchronize(s));
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < std::min<size_t>(n_thr, big.size()); t++)
            pool.emplace_back([&, t] { for (size_t b = t; b < big.size(); b += n_thr) std::sort(bufs[b].begin(), bufs[b].end()); });
        for (auto& th : pool) th.join();
        for (size_t b = 0; b < big.size(); b++) {
            L.hashes.upload(bufs[b].data(), bufs[b].size(), s, L.off[big[b]]);
            st.bytes_h2d += 8 * bufs[b].size();
        }
        LCTY_HIP(hipStreamSynchronize(s));
        st.n_sorted_host += big.size();
        st.sort_host_ms += now_ms() - t2;
    }
}

void divergences(lcty_ctx* ctx, const HapSet& hs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t k, uint32_t w, uint32_t* uniq, double* diverg,
                 lcty_db_check* check, lcty_db_stats& st) {
    hipStream_t s = ctx->stream;
    const uint32_t n = hs.n;
    Lists L;
    build_lists(ctx, hs, seqs, seq_off, k, w, L, st);
    const uint64_t total = L.off[n], n_pairs = uint64_t(n) * (n - 1) / 2;
    double t0 = now_ms();
    // column index
    const uint64_t cap = keytable::table_slots(total, 1, 1024);
    DevBuf<uint64_t> keys; DevBuf<uint32_t> mult, base, col, n_cols;
    keys.alloc(cap + 1); mult.alloc(cap + 2); base.alloc(cap + 2); col.alloc(std::max<uint64_t>(total, 1)); n_cols.alloc(1);
    LCTY_HIP(hipMemsetAsync(keys.p, 0xFF, (cap + 1) * 8, s));
    mult.zero(s); base.zero(s); n_cols.zero(s);
    const dim3 eg = per_allele_grid(n, L.max_n);
    hipLaunchKernelGGL(db_runs_kernel, eg, dim3(256), 0, s, L.hashes.p, L.d_off.p, keys.p, mult.p, cap);
    hipLaunchKernelGGL(db_bases_kernel, dim3(static_cast<uint32_t>((cap + 1 + 255) / 256)), dim3(256), 0, s, mult.p, base.p, cap + 1, n_cols.p);
    hipLaunchKernelGGL(db_cols_kernel, eg, dim3(256), 0, s, L.hashes.p, L.d_off.p, keys.p, base.p, cap, col.p);
    LCTY_HIP(hipGetLastError());
    uint32_t U = 0;
    n_cols.download(&U, 1, s);
    LCTY_HIP(hipStreamSynchronize(s));
    keys.release(); mult.release(); base.release();
    double t1 = now_ms();
    st.index_ms += t1 - t0;
    st.n_columns += U;
    // Gram tiles over column chunks
    const uint64_t n_pad = (uint64_t(n) + kGB - 1) / kGB * kGB;
    size_t free_b = 0, total_b = 0;
    LCTY_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = std::min<uint64_t>(free_b / 8, 256ull << 20);                 // the bit matrix keeps to 1/8 of what is free, 256 MB at most
    uint64_t W = std::max<uint64_t>(budget / (8 * n_pad) / kGK * kGK, kGK);               // 64-bit words per row and chunk, a multiple of the slab
    const int64_t knob_cols = ctx->knob("db_chunk_cols", 0);
    if (knob_cols > 0) W = std::max<uint64_t>((uint64_t(knob_cols) + 64 * kGK - 1) / (64 * kGK) * kGK, kGK);
    W = std::min<uint64_t>(W, std::max<uint64_t>((uint64_t(U) + 64 * kGK - 1) / (64 * kGK) * kGK, kGK));
    DevBuf<unsigned long long> B; DevBuf<uint32_t> ov;
    B.alloc(n_pad * W); ov.alloc(std::max<uint64_t>(n_pairs, 1));
    ov.zero(s);
    st.bitmat_bytes = std::max<uint64_t>(st.bitmat_bytes, n_pad * W * 8);
    const uint32_t nb = static_cast<uint32_t>(n_pad / kGB);
    for (uint64_t c0 = 0; c0 < U; c0 += W * 64) {
        const uint32_t c1 = static_cast<uint32_t>(std::min<uint64_t>(U, c0 + W * 64));
        B.zero(s);
        hipLaunchKernelGGL(db_bits_kernel, eg, dim3(256), 0, s, col.p, L.d_off.p, static_cast<uint32_t>(c0), c1, B.p, W);
        hipLaunchKernelGGL(db_gram_kernel, dim3(nb, nb), dim3(256), 0, s, reinterpret_cast<const uint64_t*>(B.p), W, n, ov.p);
        st.n_chunks++;
    }
    LCTY_HIP(hipGetLastError());
    std::vector<uint32_t> h_ov(n_pairs);
    ov.download(h_ov.data(), n_pairs, s);
    LCTY_HIP(hipStreamSynchronize(s));
    st.bytes_d2h += 4 * n_pairs;
    double t2 = now_ms();
    st.tiles_ms += t2 - t1;
    // jaccard_distance's last lines (minim_div.rs:34-39) and check_divergencies (add.rs:521-543)
    lcty_db_check ck{};
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = i + 1; j < n; j++, at++) {
            const uint32_t n1 = static_cast<uint32_t>(L.off[i + 1] - L.off[i]), n2 = static_cast<uint32_t>(L.off[j + 1] - L.off[j]);
            const uint32_t union_ = n1 + n2 - h_ov[at], un = union_ - h_ov[at];
            const double d = double(un) / double(union_);
            uniq[at] = un;
            if (diverg) diverg[at] = d;
            if (d >= 0.2) {
                ck.n_high++;
                if (d > ck.highest) { ck.highest = d; ck.highest_i = i; ck.highest_j = j; }
            }
        }
    if (check) *check = ck;
    st.host_ms += now_ms() - t2;
}

struct U128Hash { size_t operator()(unsigned __int128 x) const { return size_t(fast_hash64(uint64_t(x)) ^ (fast_hash64(uint64_t(x >> 64)) * 31)); } };

// KmerCounts::off_target_counts for 32 <= k <= 63 on the host, in the closed form proved at off_target() below
void off_target_host(uint32_t n, const uint8_t* seqs, const uint64_t* seq_off, const uint16_t* counts, const uint64_t* cnt_off, uint32_t k,
                     uint32_t max_value, const uint8_t* ref, uint64_t n_ref, const uint16_t* ref_counts, uint16_t* out, bool* negatives, unsigned n_thr) {
    typedef unsigned __int128 u128;
    struct Ent { uint32_t first, occ; };
    std::unordered_map<u128, Ent, U128Hash> map;
    map.reserve(n_ref * 2);
    for (uint64_t p = 0; p < n_ref; p++) {
        u128 km;
        if (!canonical_kmer_ascii(ref, p, k, &km)) continue;                   // the key: min(fw, rv)
        auto it = map.find(km);
        if (it == map.end()) map.emplace(km, Ent{static_cast<uint32_t>(p), 1u}); else it->second.occ++;
    }
    *negatives = false;
    std::unordered_map<u128, uint16_t, U128Hash> val;
    val.reserve(map.size() * 2);
    for (const auto& kv : map) {
        const uint32_t f = ref_counts[kv.second.first], m = kv.second.occ;
        val.emplace(kv.first, static_cast<uint16_t>(f == max_value ? f : (f > m ? f - m : 0)));
        if (f != max_value && m > f) *negatives = true;
    }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < n_thr; t++)
        pool.emplace_back([&, t] {
            for (uint32_t a = t; a < n; a += n_thr) {
                const uint8_t* s = seqs + seq_off[a];
                const uint64_t m = cnt_off[a + 1] - cnt_off[a];
                for (uint64_t p = 0; p < m; p++) {
                    u128 km;
                    uint16_t v;
                    if (!canonical_kmer_ascii(s, p, k, &km)) v = static_cast<uint16_t>(max_value);
                    else { auto it = val.find(km); v = it == val.end() ? counts[cnt_off[a] + p] : it->second; }
                    out[cnt_off[a] + p] = v;
                }
            }
        });
    for (auto& th : pool) th.join();
}

uint32_t max_value_of(uint32_t counter_bytes) {                                // KmerCounts::load, counts.rs:131-133 (KmerCount = u16)
    if (counter_bytes < 1 || counter_bytes > 8) fail(LCTY_ERR_INVALID_INPUT, "counter length %u: must be 1..8 bytes", counter_bytes);
    return counter_bytes >= 2 ? 65535u : 255u;
}

// add.rs:626-644 + counts.rs:180-230.
//
// The reference walks the k-mers of the target in order: `val = map.entry(kmer).or_insert(count)`, then, unless val == max_value,
// `have_negatives |= val == 0; val = val.saturating_sub(1)`. For one k-mer with occurrences at positions p_1 < ... < p_m:
//  - or_insert stores the count at p_1 (`first`) and ignores the counts at p_2..p_m, whatever they are;
//  - a value only ever decreases, so it equals max_value at some visit iff first == max_value, and then no visit changes it: value = first;
//  - otherwise every one of the m visits decrements with saturation: after visit t the value is max(first - t, 0), so the final value is
//    first.saturating_sub(m), and a visit finds 0 iff some t <= m has first - (t - 1) <= 0, i.e. iff m > first.
// Hence value = first == max_value ? first : first.saturating_sub(m), have_negatives = any k-mer with first != max_value and m > first,
// which needs only the lowest position (atomicMin) and the number of occurrences (atomicAdd) of every k-mer: no order.
void off_target(lcty_ctx* ctx, uint32_t n, const uint8_t* seqs, const uint64_t* seq_off, const uint16_t* counts, const uint64_t* cnt_off, uint32_t k,
                uint32_t counter_bytes, const uint8_t* ref_seq, uint64_t ref_len, const uint16_t* ref_counts_in, uint64_t n_ref_counts, uint16_t* out,
                uint32_t* warn, lcty_db_stats& st) {
    if (k < 2 || k > 63) fail(LCTY_ERR_INVALID_INPUT, "k = %u: must be 2..63 (128-bit k-mers, counts.rs:189)", k);
    const uint32_t max_value = max_value_of(counter_bytes);
    const HapSet hs = check_db_haps(n, seqs, seq_off, 1);
    if (!counts || !cnt_off || !ref_seq || !ref_counts_in || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (ref_len >= (1ull << 31)) fail(LCTY_ERR_UNSUPPORTED, "reference sequence longer than 2^31 - 1 bases");
    for (uint32_t a = 0; a < n; a++) {
        const uint64_t len = seq_off[a + 1] - seq_off[a], want = len + 1 >= k ? len + 1 - k : 0;
        if (cnt_off[a + 1] < cnt_off[a] || cnt_off[a + 1] - cnt_off[a] != want)
            fail(LCTY_ERR_INVALID_DATA, "k-mer counts contain %llu k-mers for contig %u (expected %llu)",
                 static_cast<unsigned long long>(cnt_off[a + 1] - cnt_off[a]), a, static_cast<unsigned long long>(want));
    }
    const uint64_t n_ref = ref_len + 1 >= k ? ref_len + 1 - k : 0;
    if (n_ref_counts != n_ref)
        fail(LCTY_ERR_INVALID_DATA, "k-mer counts contain %llu k-mers for the reference sequence (expected %llu)",
             static_cast<unsigned long long>(n_ref_counts), static_cast<unsigned long long>(n_ref));
    double t0 = now_ms();
    // n_runs (seq/mod.rs:57-74): runs of N become A, and the counts of the k-mers over them 0
    std::vector<uint8_t> ref(ref_seq, ref_seq + ref_len);
    std::vector<uint16_t> ref_counts(ref_counts_in, ref_counts_in + n_ref);
    bool any_run = false;
    for (uint64_t i = 0; i < ref_len;) {
        if (ref[i] != 'N') { i++; continue; }
        uint64_t e = i;
        while (e < ref_len && ref[e] == 'N') e++;
        std::fill(ref.begin() + i, ref.begin() + e, uint8_t('A'));
        const uint64_t from = i + 1 >= k ? i + 1 - k : 0, to = std::min<uint64_t>(e, n_ref);
        if (from < to) std::fill(ref_counts.begin() + from, ref_counts.begin() + to, uint16_t(0));
        any_run = true;
        i = e;
    }
    const uint64_t n_counts = cnt_off[n];
    bool negatives = false;
    st.host_ms += now_ms() - t0;
    t0 = now_ms();
    if (k >= 32) {
        const unsigned n_thr = static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(ctx->knob("host_threads", 16), 1), 64));
        off_target_host(n, seqs, seq_off, counts, cnt_off, k, max_value, ref.data(), n_ref, ref_counts.data(), out, &negatives, n_thr);
        st.host_ms += now_ms() - t0;
    } else {
        ctx->activate();
        hipStream_t s = ctx->stream;
        uint64_t max_n = 0;
        for (uint32_t a = 0; a < n; a++) max_n = std::max(max_n, cnt_off[a + 1] - cnt_off[a]);
        const uint64_t cap = keytable::table_slots(n_ref, 1, 1024);
        DevHaps d; DevBuf<uint8_t> d_ref; DevBuf<uint64_t> d_cnt_off; DevBuf<uint16_t> d_counts, d_out, d_ref_counts, d_value;
        DevBuf<uint64_t> keys; DevBuf<uint32_t> first, occ, d_neg;
        d_ref.alloc(std::max<uint64_t>(ref_len, 1)); d_cnt_off.alloc(n + 1);
        d_counts.alloc(std::max<uint64_t>(n_counts, 1)); d_out.alloc(std::max<uint64_t>(n_counts, 1)); d_ref_counts.alloc(std::max<uint64_t>(n_ref, 1));
        d_value.alloc(cap + 1); keys.alloc(cap + 1); first.alloc(cap + 1); occ.alloc(cap + 1); d_neg.alloc(1);
        st.bytes_h2d += d.upload(ctx, hs, seqs, seq_off, 0);
        d_ref.upload(ref.data(), ref_len, s); d_cnt_off.upload(cnt_off, n + 1, s);
        d_counts.upload(counts, n_counts, s); d_ref_counts.upload(ref_counts.data(), n_ref, s);
        st.bytes_h2d += ref_len + 8ull * (n + 1) + 2 * (n_counts + n_ref);
        LCTY_HIP(hipMemsetAsync(keys.p, 0xFF, (cap + 1) * 8, s));
        LCTY_HIP(hipMemsetAsync(first.p, 0xFF, (cap + 1) * 4, s));
        occ.zero(s); d_neg.zero(s); d_value.zero(s);
        if (n_ref) {
            hipLaunchKernelGGL(db_ref_insert_kernel, dim3(static_cast<uint32_t>((n_ref + 255) / 256)), dim3(256), 0, s, d_ref.p, n_ref, k, keys.p, first.p, occ.p, cap);
            hipLaunchKernelGGL(db_ref_value_kernel, dim3(static_cast<uint32_t>((cap + 255) / 256)), dim3(256), 0, s, keys.p, first.p, occ.p, cap, d_ref_counts.p,
                               max_value, d_value.p, d_neg.p);
        }
        if (n_counts)
            hipLaunchKernelGGL(db_offt_kernel, per_allele_grid(n, max_n), dim3(256), 0, s, d.seqs.p, d.off.p, d_counts.p, d_cnt_off.p, k, keys.p, d_value.p, cap,
                               max_value, d_out.p);
        LCTY_HIP(hipGetLastError());
        uint32_t neg = 0;
        d_neg.download(&neg, 1, s);
        d_out.download(out, n_counts, s);
        LCTY_HIP(hipStreamSynchronize(s));
        st.bytes_d2h += 2 * n_counts;
        negatives = neg != 0;
        st.offt_ms += now_ms() - t0;
    }
    if (warn) *warn = (negatives ? LCTY_DB_WARN_NEGATIVES_SEEN : 0u) | (negatives && !any_run ? LCTY_DB_WARN_REF_MISMATCH : 0u);
}

uint64_t hash_bytes(const uint8_t* p, uint64_t n) {                            // FNV-1a over 8-byte words with a final mix: a filter before memcmp, nothing more
    uint64_t h = 0xcbf29ce484222325ull ^ n;
    uint64_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t v; memcpy(&v, p + i, 8); h = (h ^ v) * 0x100000001b3ull; h ^= h >> 29; }
    for (; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return fast_hash64(h);
}

// discard_identical (add.rs:546-582): the first of equal sequences is kept, the order stays; owner[i] = input index of the kept
// haplotype that input i equals (i itself when kept). Text as lines 567-578: "<kept> = <name>, <name>\n" per kept haplotype that folded any.
void discard_identical(uint32_t n, const uint8_t* seqs, const uint64_t* seq_off, const std::vector<std::string>& names, std::vector<uint32_t>& kept,
                       std::vector<uint32_t>& owner, std::string& text) {
    std::unordered_map<uint64_t, std::vector<uint32_t>> seen;
    seen.reserve(n * 2);
    kept.clear(); owner.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* s = seqs + seq_off[i];
        const uint64_t len = seq_off[i + 1] - seq_off[i];
        std::vector<uint32_t>& cand = seen[hash_bytes(s, len)];
        uint32_t own = i;
        for (uint32_t c : cand)
            if (seq_off[c + 1] - seq_off[c] == len && memcmp(seqs + seq_off[c], s, len) == 0) { own = c; break; }
        owner[i] = own;
        if (own == i) { cand.push_back(i); kept.push_back(i); }
    }
    text.clear();
    if (kept.size() == n) return;
    std::vector<std::vector<uint32_t>> folded(n);
    for (uint32_t i = 0; i < n; i++) if (owner[i] != i) folded[owner[i]].push_back(i);
    for (uint32_t kidx : kept) {
        if (folded[kidx].empty()) continue;
        text += names[kidx] + " = ";
        for (size_t t = 0; t < folded[kidx].size(); t++) { if (t) text += ", "; text += names[folded[kidx][t]]; }
        text += "\n";
    }
}

}  // namespace

extern "C" {

void lcty_db_params_default(lcty_db_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->div_k = 15; p->div_w = 15;               // add.rs:77-78
    p->calc_div = 0;                            // add.rs:76: no divergences unless asked
    p->only_seqs = 0;
}

int32_t lcty_db_minimizers(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t k, uint32_t w, uint64_t* min_off,
                           uint64_t** hashes, lcty_db_stats* stats) {
    return guarded([&] {
        if (hashes) *hashes = nullptr;
        if (!ctx || !min_off || !hashes) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_seqs < 1) fail(LCTY_ERR_INVALID_INPUT, "no sequences");
        check_kw(k, w);
        const HapSet hs = check_db_haps(n_seqs, seqs, seq_off, 1);
        ctx->activate();
        lcty_db_stats st{};
        const double t0 = now_ms();
        Lists L;
        build_lists(ctx, hs, seqs, seq_off, k, w, L, st);
        const uint64_t total = L.off[n_seqs];
        Handoff h;
        uint64_t* hashes_out = from(h, L.hashes, total, ctx->stream);
        LCTY_HIP(hipStreamSynchronize(ctx->stream));
        st.bytes_d2h += 8 * total;
        memcpy(min_off, L.off.data(), 8 * (n_seqs + 1));
        *hashes = hashes_out; h.commit();
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

int32_t lcty_db_divergences(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t k, uint32_t w, uint32_t* uniq,
                            double* diverg, lcty_db_check* check, lcty_db_stats* stats) {
    return guarded([&] {
        if (!ctx || !uniq) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_kw(k, w);
        if (n_seqs < 2) fail(LCTY_ERR_INVALID_DATA, "Less than two haplotypes available");
        const HapSet hs = check_db_haps(n_seqs, seqs, seq_off, 2);
        ctx->activate();
        lcty_db_stats st{};
        const double t0 = now_ms();
        divergences(ctx, hs, seqs, seq_off, k, w, uniq, diverg, check, st);
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

int32_t lcty_db_off_target(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, const uint16_t* counts, const uint64_t* cnt_off,
                           uint32_t k, uint32_t counter_bytes, const uint8_t* ref_seq, uint64_t ref_len, const uint16_t* ref_counts, uint64_t n_ref_counts,
                           uint16_t* out, uint32_t* warn_bits, lcty_db_stats* stats) {
    return guarded([&] {
        if (!ctx) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_seqs < 1) fail(LCTY_ERR_INVALID_INPUT, "no sequences");
        lcty_db_stats st{};
        const double t0 = now_ms();
        off_target(ctx, n_seqs, seqs, seq_off, counts, cnt_off, k, counter_bytes, ref_seq, ref_len, ref_counts, n_ref_counts, out, warn_bits, st);
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

int32_t lcty_db_discard_identical(uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, const char* names, uint32_t* kept, uint32_t* n_kept,
                                  uint32_t* owner, char* text, uint64_t cap, uint64_t* needed) {
    return guarded([&] {
        if (!n_kept || !needed) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_db_haps(n_seqs, seqs, seq_off, 0);
        std::vector<uint32_t> kv, ov; std::string tx;
        discard_identical(n_seqs, seqs, seq_off, split_names(names, n_seqs), kv, ov, tx);
        *n_kept = static_cast<uint32_t>(kv.size()); *needed = tx.size();
        if (kept) memcpy(kept, kv.data(), 4 * kv.size());
        if (owner) memcpy(owner, ov.data(), 4 * ov.size());
        if (text) {
            if (cap < tx.size()) fail(LCTY_ERR_INVALID_INPUT, "text buffer too small (%llu < %zu)", static_cast<unsigned long long>(cap), tx.size());
            memcpy(text, tx.data(), tx.size());
        }
    });
}

int32_t lcty_db_build_locus(lcty_ctx* ctx, uint32_t n_seqs, const char* names, const uint8_t* seqs, const uint64_t* seq_off, const uint8_t* ref_seq,
                            uint64_t ref_len, const uint16_t* counts, const uint64_t* cnt_off, uint32_t k, uint32_t counter_bytes,
                            const lcty_db_params* params, lcty_db_files* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !params || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_seqs < 2) fail(LCTY_ERR_INVALID_DATA, "Less than two haplotypes available");          // check_sequences, add.rs:656-658
        check_db_haps(n_seqs, seqs, seq_off, 2);
        if (params->calc_div) check_kw(params->div_k, params->div_w);
        const double t0 = now_ms();
        lcty_db_stats st{};
        std::vector<uint32_t> kept, owner; std::string disc;
        const std::vector<std::string> nm = split_names(names, n_seqs);
        discard_identical(n_seqs, seqs, seq_off, nm, kept, owner, disc);
        const uint32_t m = static_cast<uint32_t>(kept.size());
        // the kept haplotypes, their names and (unless only_seqs) their blocks of the count table, in input order
        std::vector<uint8_t> ks; std::vector<uint64_t> koff{0}, kcoff{0}; std::vector<uint16_t> kc; std::string knames;
        if (!params->only_seqs) {
            if (!counts || !cnt_off || !ref_seq) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            for (uint32_t a = 0; a <= n_seqs; a++) if (cnt_off[a + 1] < cnt_off[a]) fail(LCTY_ERR_INVALID_INPUT, "cnt_off is not ascending at %u", a);
        }
        for (uint32_t a : kept) {
            ks.insert(ks.end(), seqs + seq_off[a], seqs + seq_off[a + 1]); koff.push_back(ks.size());
            knames += nm[a]; knames.push_back('\0');
            if (!params->only_seqs) { kc.insert(kc.end(), counts + cnt_off[a], counts + cnt_off[a + 1]); kcoff.push_back(kc.size()); }
        }
        st.host_ms += now_ms() - t0;
        std::vector<uint8_t> fasta, kmers, dists;
        sized([&](uint8_t* o, uint64_t c, uint64_t* nd) { return lcty_fasta_write_text(m, knames.data(), ks.data(), koff.data(), reinterpret_cast<char*>(o), c, nd); }, fasta);
        lcty_db_check ck{};
        uint32_t warn = 0;
        if (!params->only_seqs) {
            if (params->calc_div) {
                ctx->activate();
                if (m < 2) fail(LCTY_ERR_INVALID_DATA, "Less than two different haplotypes available");
                std::vector<uint32_t> uniq(uint64_t(m) * (m - 1) / 2);
                divergences(ctx, check_db_haps(m, ks.data(), koff.data(), 2), ks.data(), koff.data(), params->div_k, params->div_w, uniq.data(), nullptr, &ck, st);
                sized([&](uint8_t* o, uint64_t c, uint64_t* nd) { return lcty_distances_write(params->div_k, params->div_w, m, uniq.data(), o, c, nd); }, dists);
            }
            std::vector<uint16_t> offt(kc.size());
            off_target(ctx, m, ks.data(), koff.data(), kc.data(), kcoff.data(), k, counter_bytes, ref_seq, ref_len, counts + cnt_off[n_seqs],
                       cnt_off[n_seqs + 1] - cnt_off[n_seqs], offt.data(), &warn, st);
            std::vector<uint8_t> b1, b2;
            sized([&](uint8_t* o, uint64_t c, uint64_t* nd) { return lcty_kmer_counts_write(k, counter_bytes, m, kcoff.data(), offt.data(), o, c, nd); }, b1);
            sized([&](uint8_t* o, uint64_t c, uint64_t* nd) { return lcty_kmer_counts_write(k, counter_bytes, m, kcoff.data(), kc.data(), o, c, nd); }, b2);
            kmers = b1; kmers.insert(kmers.end(), b2.begin(), b2.end());                         // off-target first (add.rs:648-650)
        }
        st.total_ms = now_ms() - t0;
        lcty_db_files o{}; Handoff h;
        o.n_kept = m; o.warn_bits = warn; o.check = ck; o.stats = st;
        o.fasta = h.copy(fasta); o.fasta_len = fasta.size();
        o.kmers = h.copy(kmers); o.kmers_len = kmers.size();
        o.distances = h.copy(dists); o.distances_len = dists.size();
        o.discarded = h.bytes(disc); o.discarded_len = disc.size();
        o.kept = h.copy(kept);
        *out = o; h.commit();
    });
}

void lcty_db_files_free(lcty_db_files* f) {
    if (!f) return;
    free(f->fasta); free(f->kmers); free(f->distances); free(f->discarded); free(f->kept);
    memset(f, 0, sizeof(*f));
}

}  // extern "C"
