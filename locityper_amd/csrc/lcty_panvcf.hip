// lcty_panvcf.hip — a locus from a pangenome VCF (`locityper target -v`): the variation filter and the reconstruction of every phased
// haplotype over an interval (src/seq/panvcf.rs), the boundary search and the expansion of the locus (src/command/add.rs:365-518, 733-755)
// and the whole step up to lcty_db_build_locus. The contract of every entry point is stated in the header and in DESIGN.md 5k.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <unordered_set>
#include <vector>

#include "lcty_common.hpp"
#include "lcty_device.hpp"
#include "lcty_scan.hpp"

namespace {

using namespace lcty;

constexpr int TILE = 64;                            // records x columns of one transpose tile
constexpr int TILE_THREADS = 256;
constexpr int COL_THREADS = 256;                    // chain / segment kernels: one wavefront per column, four columns per workgroup
constexpr int GATHER_THREADS = 256;
constexpr uint32_t GATHER_TILE = GATHER_THREADS * 8;   // output bytes of one gather workgroup: an aligned 8-byte word per thread
constexpr int BOUND_THREADS = 256;
constexpr uint32_t EFFECT_MARGIN = 9;               // add.rs:397
constexpr uint32_t NONE = 0xFFFFFFFFu;

// words of the flag block of one reconstruction
enum { F_BREAK = 0, F_STRADDLE = 1, F_BAD = 2, F_KEPT = 3, F_OOB = 4, F_COUNT = 8 };

// one accepted non-reference allele of a column: bytes [dst, dst + alt_len) of the column are pool[src ...], the reference resumes
// behind them at ref_next (relative to the interval)
struct Seg { uint32_t dst, alt_len, ref_next, _pad; uint64_t src; };
static_assert(sizeof(Seg) == 24, "Seg layout");

// ---- device: scans (lcty_scan.hpp) -----------------------------------------------------------------------------------------------------

struct LoadUniqueKmer { const uint16_t* p; __device__ uint32_t operator()(uint64_t i) const { return p[i] <= 1 ? 1u : 0u; } };     // add.rs:389
struct LoadVarEnd { const uint32_t* pos; const uint32_t* rlen; __device__ uint64_t operator()(uint64_t i) const { return uint64_t(pos[i]) + rlen[i]; } };

// ---- device: variation filter and reconstruction -------------------------------------------------------------------------------------

// (a) One 64 x 64 tile of the record-major genotype matrix: kept[v] = some column carries allele >= 1 (filter_variants, panvcf.rs:173-177),
// an allele index the record does not have is reported, and the tile goes to the haplotype-major copy (gt_t == nullptr: the filter alone).
__global__ __launch_bounds__(TILE_THREADS) void panvcf_tile_kernel(const int16_t* __restrict__ gt, uint32_t n_recs, uint32_t n_cols,
                                                                  const uint32_t* __restrict__ rec_allele, uint8_t* __restrict__ kept,
                                                                  int16_t* __restrict__ gt_t, uint32_t* __restrict__ flags) {
    __shared__ int16_t tile[TILE][TILE + 1];
    const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const uint32_t v0 = blockIdx.x * TILE, h0 = blockIdx.y * TILE;
    for (uint32_t r = wave; r < TILE; r += TILE_THREADS / WAVE) {
        const uint32_t v = v0 + r, h = h0 + lane;
        int16_t a = 0;
        if (v < n_recs && h < n_cols) a = gt[uint64_t(v) * n_cols + h];
        tile[r][lane] = a;
        if (v < n_recs) {
            if (__ballot(a >= 1) && lane == 0) kept[v] = 1;
            if (rec_allele && int64_t(a) >= int64_t(rec_allele[v + 1]) - int64_t(rec_allele[v])) atomicMin(&flags[F_BAD], v);
        }
    }
    if (!gt_t) return;
    __syncthreads();
    for (uint32_t c = wave; c < TILE; c += TILE_THREADS / WAVE) {
        const uint32_t h = h0 + c, v = v0 + lane;
        if (h < n_cols && v < n_recs) gt_t[uint64_t(h) * n_recs + v] = tile[lane][c];
    }
}

// (a) per record: the allele table is sound, and the verdict of the walk of panvcf.rs:264-271 for a kept record — skipped, inside, the first
// that ends the walk (F_BREAK), the first that straddles an end of the interval (F_STRADDLE).
__global__ void panvcf_verdict_kernel(uint32_t n_recs, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rlen,
                                      const uint32_t* __restrict__ rec_allele, const uint64_t* __restrict__ allele_off, uint64_t n_alleles,
                                      uint64_t pool_len, const uint8_t* __restrict__ kept, uint32_t ref_start, uint32_t ref_end,
                                      uint32_t* __restrict__ flags) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < n_recs;
    bool k = false;
    if (live) {
        const uint64_t a0 = rec_allele[v], a1 = rec_allele[v + 1];
        bool ok = a0 < a1 && a1 <= n_alleles;
        if (ok) {
            for (uint64_t i = a0; i < a1 && ok; i++) ok = allele_off[i] <= allele_off[i + 1] && allele_off[i + 1] <= pool_len && allele_off[i + 1] - allele_off[i] < 0x7FFFFFFFull;
            ok = ok && allele_off[a0 + 1] - allele_off[a0] == rlen[v];
        }
        if (!ok) atomicMin(&flags[F_BAD], v);
        k = kept[v] != 0;
        if (k) {
            const uint64_t vs = pos[v], ve = vs + rlen[v];
            if (ve <= ref_start) {}
            else if (ref_end <= vs) atomicMin(&flags[F_BREAK], v);
            else if (vs < ref_start || ref_end < ve) atomicMin(&flags[F_STRADDLE], v);
        }
    }
    const uint64_t m = __ballot(k);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(&flags[F_KEPT], uint32_t(__popcll(m)));
}

__device__ inline uint32_t walk_limit(const uint32_t* flags, uint32_t n_recs) {
    const uint32_t a = flags[F_BREAK], b = flags[F_STRADDLE];
    const uint32_t m = a < b ? a : b;
    return m < n_recs ? m : n_recs;
}

// (b) The walk of one column (panvcf.rs:273-307), one wavefront: 64 consecutive records per batch from the haplotype-major matrix; a ballot
// picks the non-reference and the missing entries, the accept rule `var_start >= prev_end` runs over the set bits in record order with prev_end
// carried from batch to batch. Per column: the accepted entries as one 64-bit mask per batch, their number, the length of the sequence,
// unknown_nts, the ignored overlaps and the first of them.
__global__ __launch_bounds__(COL_THREADS) void panvcf_chain_kernel(const int16_t* __restrict__ gt_t, uint32_t n_recs, uint32_t n_cols,
                                                                   const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rlen,
                                                                   const uint32_t* __restrict__ rec_allele, const uint64_t* __restrict__ allele_off,
                                                                   const uint8_t* __restrict__ kept, const uint32_t* __restrict__ flags,
                                                                   uint32_t ref_start, uint32_t ref_end, uint32_t n_batches,
                                                                   uint64_t* __restrict__ accmask, uint32_t* __restrict__ n_acc,
                                                                   uint64_t* __restrict__ out_len, uint32_t* __restrict__ unknown,
                                                                   uint32_t* __restrict__ n_ovl, uint32_t* __restrict__ first_ovl) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t h = blockIdx.x * (COL_THREADS / WAVE) + threadIdx.x / WAVE;
    if (h >= n_cols) return;                                            // whole wavefronts leave; nothing below waits for another wavefront
    const uint32_t limit = walk_limit(flags, n_recs);
    uint64_t prev_end = ref_start;
    uint32_t unk = 0, accepted = 0, overlaps = 0, first = NONE;
    long long delta = 0;
    for (uint32_t b = 0; b < n_batches; b++) {
        const uint32_t v = b * WAVE + lane;
        uint64_t acc = 0;
        if (b * WAVE < limit) {                                         // wave-uniform
            bool in = v < limit && kept[v];
            uint32_t p = 0, rl = 0;
            int16_t a = 0;
            if (in) {
                p = pos[v]; rl = rlen[v];
                in = uint64_t(p) + rl > ref_start;                       // var_end <= ref_start: skipped
                if (in) a = gt_t[uint64_t(h) * n_recs + v];
            }
            if (in && a < 0) unk += rl;                                 // missing: the reference allele, ref_len unknown bases
            uint64_t m = __ballot(in && a >= 1);
            while (m) {
                const int bit = __ffsll(static_cast<unsigned long long>(m)) - 1;
                m &= m - 1;
                const uint64_t vs = __shfl(p, bit), ve = vs + __shfl(rl, bit);
                if (vs >= prev_end) { acc |= 1ull << bit; prev_end = ve; }
                else { overlaps++; if (first == NONE) first = b * WAVE + bit; }
            }
            if ((acc >> lane) & 1) {
                const uint64_t ai = uint64_t(rec_allele[v]) + uint32_t(a);
                delta += static_cast<long long>(allele_off[ai + 1] - allele_off[ai]) - static_cast<long long>(rl);
            }
            accepted += __popcll(acc);
        }
        if (lane == 0) accmask[uint64_t(h) * n_batches + b] = acc;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) { unk += __shfl_xor(unk, off); delta += __shfl_xor(delta, off); }
    if (lane == 0) {
        n_acc[h] = accepted;
        out_len[h] = static_cast<uint64_t>(static_cast<long long>(ref_end - ref_start) + delta);
        unknown[h] = unk; n_ovl[h] = overlaps; first_ovl[h] = first;
    }
}

// (c) The segment list of one column from its masks, one wavefront: the destination of an accepted allele is its reference offset plus
// the length changes of the accepted alleles before it — an exclusive scan inside the batch and a carry across batches.
__global__ __launch_bounds__(COL_THREADS) void panvcf_segment_kernel(const int16_t* __restrict__ gt_t, uint32_t n_recs, uint32_t n_cols,
                                                                     const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rlen,
                                                                     const uint32_t* __restrict__ rec_allele, const uint64_t* __restrict__ allele_off,
                                                                     uint32_t ref_start, uint32_t n_batches, const uint64_t* __restrict__ accmask,
                                                                     const uint64_t* __restrict__ seg_off, Seg* __restrict__ segs) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t h = blockIdx.x * (COL_THREADS / WAVE) + threadIdx.x / WAVE;
    if (h >= n_cols) return;
    const uint64_t s0 = seg_off[h], s1 = seg_off[h + 1];
    uint64_t rank0 = 0;
    long long carry = 0;
    for (uint32_t b = 0; b < n_batches; b++) {
        const uint64_t acc = accmask[uint64_t(h) * n_batches + b];
        if (!acc) continue;                                             // wave-uniform
        const uint32_t v = b * WAVE + lane;
        const bool mine = (acc >> lane) & 1;
        uint32_t p = 0, rl = 0, alt = 0;
        uint64_t src = 0;
        if (mine) {
            p = pos[v]; rl = rlen[v];
            const uint64_t ai = uint64_t(rec_allele[v]) + uint32_t(gt_t[uint64_t(h) * n_recs + v]);
            src = allele_off[ai]; alt = static_cast<uint32_t>(allele_off[ai + 1] - src);
        }
        const long long d = mine ? static_cast<long long>(alt) - static_cast<long long>(rl) : 0;
        const long long incl = wave_scan_incl(d, AddOp{});
        if (mine) {
            const uint64_t slot = s0 + rank0 + __popcll(acc & ((1ull << lane) - 1));
            if (slot < s1) {
                Seg s;
                s.dst = static_cast<uint32_t>(static_cast<long long>(p - ref_start) + carry + incl - d);
                s.alt_len = alt; s.ref_next = p + rl - ref_start; s._pad = 0; s.src = src;
                segs[slot] = s;
            }
        }
        carry += __shfl(incl, WAVE - 1);
        rank0 += __popcll(acc);
    }
}

// the last segment of [lo, hi) that starts at or before byte p of the column, or lo - 1
__device__ inline long long last_seg_at(const Seg* __restrict__ segs, long long lo, long long hi, uint32_t p) {
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (segs[mid].dst <= p) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// (d) One workgroup per (column, tile of the output): a thread owns one aligned 8-byte word of the concatenated output, finds the segment of
// its first byte by bisection from the tile's first segment, assembles the word from the reference / the allele pool and stores it whole when
// all of it belongs to the column. A byte 'N' sets the column's flag (seq::has_n, add.rs:776).
__global__ __launch_bounds__(GATHER_THREADS) void panvcf_gather_kernel(const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ seg_off,
                                                                       const Seg* __restrict__ segs, const uint8_t* __restrict__ ref, uint64_t ref_len,
                                                                       const uint8_t* __restrict__ pool, uint64_t pool_len, uint8_t* __restrict__ out,
                                                                       uint8_t* __restrict__ has_n, uint32_t* __restrict__ flags) {
    __shared__ long long j_first;
    const uint32_t h = blockIdx.y;
    const uint64_t cb = seq_off[h], ce = seq_off[h + 1];
    const uint64_t w0 = cb / 8 + uint64_t(blockIdx.x) * GATHER_THREADS;
    if (w0 * 8 >= ce) return;                                           // the whole workgroup is behind the column
    const long long s0 = static_cast<long long>(seg_off[h]), s1 = static_cast<long long>(seg_off[h + 1]);
    if (threadIdx.x == 0) j_first = last_seg_at(segs, s0, s1, static_cast<uint32_t>((w0 * 8 > cb ? w0 * 8 : cb) - cb));
    __syncthreads();
    const uint64_t w = w0 + threadIdx.x;
    const uint64_t lo = w * 8 > cb ? w * 8 : cb, hi = w * 8 + 8 < ce ? w * 8 + 8 : ce;
    bool seen_n = false;
    if (lo < hi) {
        const long long jf = j_first;
        long long j = last_seg_at(segs, jf < s0 ? s0 : jf, s1, static_cast<uint32_t>(lo - cb));
        uint64_t word = 0;
        for (uint64_t g = lo; g < hi; g++) {
            const uint32_t p = static_cast<uint32_t>(g - cb);
            while (j + 1 < s1 && segs[j + 1].dst <= p) j++;
            uint8_t c = 0;
            if (j < s0) {
                if (p < ref_len) c = ref[p]; else flags[F_OOB] = 1;
            } else {
                const Seg s = segs[j];
                const uint32_t o = p - s.dst;
                if (o < s.alt_len) {
                    if (s.src + o < pool_len) c = pool[s.src + o]; else flags[F_OOB] = 1;
                } else {
                    const uint64_t r = uint64_t(s.ref_next) + (o - s.alt_len);
                    if (r < ref_len) c = ref[r]; else flags[F_OOB] = 1;
                }
            }
            seen_n |= c == 'N';
            word |= uint64_t(c) << (8 * (g - w * 8));
        }
        if (hi - lo == 8) *reinterpret_cast<uint64_t*>(out + w * 8) = word;
        else for (uint64_t g = lo; g < hi; g++) out[g] = static_cast<uint8_t>(word >> (8 * (g - w * 8)));
    }
    if (__ballot(seen_n) && (threadIdx.x & (WAVE - 1)) == 0) has_n[h] = 1;
}

// (e) The surviving columns, one after the other: workgroup (tile, k) copies its part of column cols[k]; a thread stores one aligned word.
__global__ __launch_bounds__(GATHER_THREADS) void panvcf_compact_kernel(const uint32_t* __restrict__ cols, const uint64_t* __restrict__ src_off,
                                                                        const uint64_t* __restrict__ dst_off, const uint8_t* __restrict__ src,
                                                                        uint8_t* __restrict__ dst) {
    const uint64_t sb = src_off[cols[blockIdx.y]], cb = dst_off[blockIdx.y], ce = dst_off[blockIdx.y + 1];
    const uint64_t w = cb / 8 + uint64_t(blockIdx.x) * GATHER_THREADS + threadIdx.x;
    const uint64_t lo = w * 8 > cb ? w * 8 : cb, hi = w * 8 + 8 < ce ? w * 8 + 8 : ce;
    if (lo >= hi) return;
    uint64_t word = 0;
    for (uint64_t g = lo; g < hi; g++) word |= uint64_t(src[sb + (g - cb)]) << (8 * (g - w * 8));
    if (hi - lo == 8) *reinterpret_cast<uint64_t*>(dst + w * 8) = word;
    else for (uint64_t g = lo; g < hi; g++) dst[g] = static_cast<uint8_t>(word >> (8 * (g - w * 8)));
}

// ---- device: boundary search ----------------------------------------------------------------------------------------------------------

struct BestPos { double val; uint32_t idx; };
// LEFT: the last maximum, RIGHT: the first (add.rs:420-428)
__device__ inline bool pos_better(const BestPos& a, const BestPos& b, bool left) {
    if (a.idx == NONE) return false;
    if (b.idx == NONE) return true;
    return a.val > b.val || (a.val == b.val && (left ? a.idx > b.idx : a.idx < b.idx));
}
__device__ inline BestPos block_best(BestPos c, bool left, BestPos* part) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, n_waves = blockDim.x / WAVE;
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        BestPos o; o.val = __shfl_xor(c.val, off); o.idx = __shfl_xor(c.idx, off);
        if (pos_better(o, c, left)) c = o;
    }
    if (lane == 0) part[wave] = c;
    __syncthreads();
    BestPos r = part[0];
    for (uint32_t w = 1; w < n_waves; w++) if (pos_better(part[w], r, left)) r = part[w];
    return r;
}

__global__ void boundary_sorted_kernel(uint32_t n_recs, const uint32_t* __restrict__ pos, uint32_t* __restrict__ flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r + 1 < n_recs && pos[r + 1] < pos[r]) atomicMin(flag, r + 1);
}

// One thread per position of [start, end): the window's share of k-mers seen at most once, then every record that can reach the position —
// those from the first whose running maximum of pos + ref_len comes within the margin up to the last that starts within it — applied in
// record order (add.rs:399-415), the distance penalty (421 / 425), and the workgroup's best position.
__global__ __launch_bounds__(BOUND_THREADS) void boundary_weights_kernel(uint32_t start, uint32_t n, const uint32_t* __restrict__ cum, uint32_t kpw,
                                                                         uint32_t n_recs, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ rlen,
                                                                         const uint64_t* __restrict__ end_max, double per_bp_drop, bool left,
                                                                         double* __restrict__ weights, BestPos* __restrict__ partial) {
    __shared__ BestPos part[BOUND_THREADS / WAVE];
    const uint32_t idx = blockIdx.x * BOUND_THREADS + threadIdx.x;
    BestPos c{0.0, NONE};
    if (idx < n) {
        const uint64_t x = uint64_t(start) + idx;
        double w = static_cast<double>(cum[idx + kpw] - cum[idx]) / static_cast<double>(kpw);
        uint32_t lo = 0, hi = n_recs;                                   // first record with end_max + 8 >= x
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (end_max[mid] + (EFFECT_MARGIN - 1) >= x) hi = mid; else lo = mid + 1; }
        const uint32_t r0 = lo;
        lo = r0; hi = n_recs;                                           // first record with pos > x + 9
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (uint64_t(pos[mid]) > x + EFFECT_MARGIN) hi = mid; else lo = mid + 1; }
        const uint32_t r1 = lo;
        const double effect_divisor = static_cast<double>(EFFECT_MARGIN + 1);
        for (uint32_t r = r0; r < r1; r++) {
            const uint64_t vs = pos[r], ve = vs + rlen[r];
            if (x >= vs && x < ve) w = 0.0;
            else if (x < vs) { const uint64_t i = vs - 1 - x; if (i < EFFECT_MARGIN) w *= static_cast<double>(EFFECT_MARGIN - uint32_t(i)) / effect_divisor; }
            else { const uint64_t i = x - ve; if (i < EFFECT_MARGIN) w *= static_cast<double>(uint32_t(i) + 1) / effect_divisor; }
        }
        const uint32_t dist = left ? n - 1 - idx : idx;
        const double t = w * per_bp_drop;                               // (w * per_bp_drop) * i, never fused
        const double u = t * static_cast<double>(dist);
        w -= u;
        weights[idx] = w;
        c.val = w; c.idx = idx;
    }
    const BestPos b = block_best(c, left, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(SCAN_THREADS) void boundary_best_kernel(uint32_t n_partial, const BestPos* __restrict__ partial, bool left, BestPos* __restrict__ out) {
    __shared__ BestPos part[SCAN_THREADS / WAVE];
    BestPos c{0.0, NONE};
    for (uint32_t i = threadIdx.x; i < n_partial; i += SCAN_THREADS) if (pos_better(partial[i], c, left)) c = partial[i];
    const BestPos b = block_best(c, left, part);
    if (threadIdx.x == 0) *out = b;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------

void sync(lcty_ctx* ctx) { LCTY_HIP(hipStreamSynchronize(ctx->stream)); }

// find_best_boundary (add.rs:371-435). Returns whether a position was found; weights (may be null) receives the end - start final weights.
bool find_boundary(lcty_ctx* ctx, uint32_t start, uint32_t end, uint32_t n_recs, const uint32_t* pos, const uint32_t* rlen, uint32_t k,
                   const uint16_t* counts, uint64_t n_counts, uint32_t allowed_expansion, uint32_t moving_window, bool left, uint32_t* position,
                   double* weights) {
    if (end < start) fail(LCTY_ERR_INVALID_INPUT, "boundary search: end %u < start %u", end, start);
    if (n_recs && (!pos || !rlen)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (start == end) {                                                 // add.rs:381-387
        for (uint32_t r = 0; r < n_recs; r++)
            if (pos[r] <= start && uint64_t(end) <= uint64_t(pos[r]) + rlen[r]) return false;
        *position = start;
        return true;
    }
    if (k < 1 || moving_window < k) fail(LCTY_ERR_INVALID_INPUT, "boundary search: moving window %u is shorter than k = %u", moving_window, k);
    if (!allowed_expansion) fail(LCTY_ERR_INVALID_INPUT, "boundary search: allowed expansion is 0");
    const uint32_t n = end - start, kpw = moving_window + 1 - k;
    if (n_counts != uint64_t(n) + kpw - 1)                              // assert_eq!(weights.len(), end - start), add.rs:394
        fail(LCTY_ERR_INVALID_INPUT, "boundary search: %llu k-mer counts for %u positions (expected %llu)", static_cast<unsigned long long>(n_counts), n,
             static_cast<unsigned long long>(uint64_t(n) + kpw - 1));
    if (!counts) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    ctx->activate();
    hipStream_t s = ctx->stream;
    const uint32_t n_blocks = (n + BOUND_THREADS - 1) / BOUND_THREADS;
    DevBuf<uint16_t> d_counts; DevBuf<uint32_t> d_cum, d_pos, d_rlen, d_flag; DevBuf<uint64_t> d_endmax; DevBuf<double> d_w; DevBuf<BestPos> d_part, d_best;
    d_counts.alloc(n_counts); d_counts.upload(counts, n_counts, s);
    d_cum.alloc(n_counts + 1);
    d_pos.alloc(std::max(n_recs, 1u)); d_rlen.alloc(std::max(n_recs, 1u)); d_endmax.alloc(std::max(n_recs, 1u));
    d_pos.upload(pos, n_recs, s); d_rlen.upload(rlen, n_recs, s);
    d_flag.alloc(1); d_w.alloc(n); d_part.alloc(n_blocks); d_best.alloc(1);
    uint32_t unsorted = NONE;
    d_flag.upload(&unsorted, 1, s);
    launch_scan<uint32_t>(s, n_counts, LoadUniqueKmer{d_counts.p}, AddOp{}, 0u, d_cum.p, true);
    if (n_recs) {
        hipLaunchKernelGGL(boundary_sorted_kernel, dim3((n_recs + 255) / 256), dim3(256), 0, s, n_recs, d_pos.p, d_flag.p);
        LCTY_HIP(hipGetLastError());
        launch_scan<uint64_t>(s, n_recs, LoadVarEnd{d_pos.p, d_rlen.p}, MaxOp{}, uint64_t(0), d_endmax.p, false);
    }
    const double per_bp_drop = 0.2 / static_cast<double>(allowed_expansion);           // add.rs:418-419
    hipLaunchKernelGGL(boundary_weights_kernel, dim3(n_blocks), dim3(BOUND_THREADS), 0, s, start, n, d_cum.p, kpw, n_recs, d_pos.p, d_rlen.p,
                       d_endmax.p, per_bp_drop, left, d_w.p, d_part.p);
    LCTY_HIP(hipGetLastError());
    hipLaunchKernelGGL(boundary_best_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, n_blocks, d_part.p, left, d_best.p);
    LCTY_HIP(hipGetLastError());
    BestPos best{};
    d_best.download(&best, 1, s);
    d_flag.download(&unsorted, 1, s);
    if (weights) d_w.download(weights, n, s);
    sync(ctx);
    if (unsorted != NONE) fail(LCTY_ERR_INVALID_DATA, "boundary search: record %u starts before its predecessor (the records must be sorted by position)", unsorted);
    if (best.idx >= n) fail(LCTY_ERR_RUNTIME, "boundary search returned no position");
    if (best.val == 0.0) return false;                                  // add.rs:430-431
    *position = start + best.idx;
    return true;
}

// the records htslib's fetch(start, end) returns: pos < end and pos + ref_len > start, in file order
void fetch_records(uint32_t n_recs, const uint32_t* pos, const uint32_t* rlen, uint32_t start, uint32_t end, std::vector<uint32_t>& p, std::vector<uint32_t>& l) {
    p.clear(); l.clear();
    for (uint32_t r = 0; r < n_recs; r++)
        if (pos[r] < end && uint64_t(pos[r]) + rlen[r] > start) { p.push_back(pos[r]); l.push_back(rlen[r]); }
}

struct Window {
    uint32_t start; uint64_t len; const uint8_t* seq; uint32_t k; const uint16_t* counts; uint64_t n_counts;
    uint64_t end() const { return start + len; }
};

// expand_locus (add.rs:438-518) for one allowed expansion. false: no boundary on one of the sides.
bool expand_once(lcty_ctx* ctx, const char* locus, uint32_t inner_start, uint32_t inner_end, uint32_t contig_len, const Window& win, uint32_t n_recs,
                 const uint32_t* pos, const uint32_t* rlen, uint32_t allowed_expansion, uint32_t moving_window, uint32_t* new_start, uint32_t* new_end,
                 uint32_t* crop_bits) {
    uint32_t left_start = inner_start > allowed_expansion ? inner_start - allowed_expansion : 0;
    const uint64_t left_end = uint64_t(inner_start) + moving_window;
    const uint32_t right_start = inner_end - moving_window;
    uint64_t right_end = std::min<uint64_t>(uint64_t(inner_end) + allowed_expansion, contig_len);
    if (left_start < win.start || right_end > win.end() || left_end > win.end() || right_start < win.start)
        fail(LCTY_ERR_INVALID_INPUT, "the window %u-%llu does not hold the flanks %u-%llu of locus %s at expansion %u", win.start,
             static_cast<unsigned long long>(win.end()), left_start, static_cast<unsigned long long>(right_end), locus, allowed_expansion);
    const uint8_t* lseq = win.seq + (left_start - win.start);
    for (uint64_t i = left_end - left_start; i-- > 0;)                  // crop at the last N (468-482)
        if (lseq[i] == 'N') {
            left_start += static_cast<uint32_t>(i) + 1;
            if (left_start > inner_start) fail(LCTY_ERR_INVALID_INPUT, "Unknown sequence at the locus %s", locus);
            *crop_bits |= 1u;
            break;
        }
    const uint8_t* rseq = win.seq + (right_start - win.start);
    for (uint64_t i = 0; i < right_end - right_start; i++)              // crop at the first N (483-493)
        if (rseq[i] == 'N') {
            right_end = right_start + i;
            if (right_end < inner_end) fail(LCTY_ERR_INVALID_INPUT, "Unknown sequence at the locus %s", locus);
            *crop_bits |= 2u;
            break;
        }
    std::vector<uint32_t> p, l;
    const uint32_t k = win.k;
    // a k-mer's count belongs to its position: the counts of a flank are a slice of the window's
    fetch_records(n_recs, pos, rlen, left_start, inner_start + 1, p, l);
    uint32_t ns = 0, ne = 0;
    if (!find_boundary(ctx, left_start, inner_start + 1, static_cast<uint32_t>(p.size()), p.data(), l.data(), k, win.counts + (left_start - win.start),
                       left_end - left_start + 1 - k, allowed_expansion, moving_window, true, &ns, nullptr)) return false;
    fetch_records(n_recs, pos, rlen, inner_end - 1, static_cast<uint32_t>(right_end), p, l);
    if (!find_boundary(ctx, inner_end - 1, static_cast<uint32_t>(right_end), static_cast<uint32_t>(p.size()), p.data(), l.data(), k,
                       win.counts + (right_start - win.start), right_end - right_start + 1 - k, allowed_expansion, moving_window, false, &ne, nullptr)) return false;
    *new_start = ns; *new_end = ne + 1;
    return true;
}

void expand_locus(lcty_ctx* ctx, const char* locus, uint32_t inner_start, uint32_t inner_end, uint32_t contig_len, const Window& win, uint32_t n_recs,
                  const uint32_t* pos, const uint32_t* rlen, uint32_t n_expansions, const uint32_t* expansions, uint32_t moving_window, lcty_expand_out* out) {
    if (!locus || !out || !expansions || !n_expansions) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    memset(out, 0, sizeof(*out));
    if (inner_end <= inner_start || inner_end > contig_len) fail(LCTY_ERR_INVALID_INPUT, "locus %s: bad interval %u-%u on a contig of %u", locus, inner_start, inner_end, contig_len);
    for (uint32_t i = 0; i < n_expansions; i++) {                       // Args::validate: strictly increasing, 0 only alone
        if (i && expansions[i] <= expansions[i - 1]) fail(LCTY_ERR_INVALID_INPUT, "allowed expansions must be strictly increasing");
        if (!expansions[i] && n_expansions > 1) fail(LCTY_ERR_INVALID_INPUT, "an allowed expansion of 0 stands alone");
    }
    const double t0 = now_ms();
    out->attempt = -1;
    for (uint32_t i = 0; i < n_expansions; i++) {
        const uint32_t e = expansions[i];
        uint32_t ns = inner_start, ne = inner_end, crop = 0;
        bool ok = true;
        if (e) {
            if (!win.seq || !win.counts) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            const uint32_t mw = std::max(win.k, moving_window);         // add.rs:812
            if (inner_end - inner_start < mw)                            // add.rs:450-453
                fail(LCTY_ERR_INVALID_INPUT, "Locus %s is shorter (%u) than the moving window (%u)", locus, inner_end - inner_start, mw);
            if (win.k < 1 || win.len < win.k || win.n_counts != win.len + 1 - win.k)
                fail(LCTY_ERR_INVALID_DATA, "the window holds %llu bases and %llu counts of %u-mers", static_cast<unsigned long long>(win.len),
                     static_cast<unsigned long long>(win.n_counts), win.k);
            ok = expand_once(ctx, locus, inner_start, inner_end, contig_len, win, n_recs, pos, rlen, e, mw, &ns, &ne, &crop);
        }
        out->n_attempts = i + 1;
        if (ok) { out->start = ns; out->end = ne; out->attempt = static_cast<int32_t>(i); out->allowed_expansion = e; out->crop_bits = crop; break; }
    }
    out->total_ms = now_ms() - t0;
    if (out->attempt < 0)                                               // add.rs:751-753
        fail(LCTY_ERR_RUNTIME, "Cannot expand locus %s to one of the sides due to a long variant overlapping boundary.\n    "
             "Try increasing -e/--expand parameter or manually modifying region boundaries.", locus);
}

struct Records {
    uint32_t n; const uint32_t* pos; const uint32_t* rlen; const uint32_t* rec_allele; const uint64_t* allele_off; const uint8_t* pool;
    uint32_t n_cols; const int16_t* gt;
};

void check_records(const Records& r, bool with_alleles) {
    if (!r.n_cols) fail(LCTY_ERR_INVALID_DATA, "Loaded zero haplotypes");
    if (r.n_cols > 65535u * 4) fail(LCTY_ERR_UNSUPPORTED, "%u haplotype columns (at most %u)", r.n_cols, 65535u * 4);
    if (r.n && (!r.gt || (with_alleles && (!r.pos || !r.rlen || !r.rec_allele || !r.allele_off)))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
}

// filter_variants' has_variation (panvcf.rs:173-181) of every record: the row reduction alone
void filter_records(lcty_ctx* ctx, const Records& r, uint8_t* kept, uint64_t* n_kept) {
    check_records(r, false);
    uint64_t cnt = 0;
    if (r.n) {
        ctx->activate();
        hipStream_t s = ctx->stream;
        DevBuf<int16_t> d_gt; DevBuf<uint8_t> d_kept; DevBuf<uint32_t> d_flags;
        const uint64_t cells = uint64_t(r.n) * r.n_cols;
        d_gt.alloc(cells); d_gt.upload(r.gt, cells, s);
        d_kept.alloc(r.n); d_kept.zero(s);
        d_flags.alloc(F_COUNT); d_flags.zero(s);
        hipLaunchKernelGGL(panvcf_tile_kernel, dim3((r.n + TILE - 1) / TILE, (r.n_cols + TILE - 1) / TILE), dim3(TILE_THREADS), 0, s, d_gt.p, r.n, r.n_cols,
                           static_cast<const uint32_t*>(nullptr), d_kept.p, static_cast<int16_t*>(nullptr), d_flags.p);
        LCTY_HIP(hipGetLastError());
        d_kept.download(kept, r.n, s);
        sync(ctx);
        for (uint32_t v = 0; v < r.n; v++) cnt += kept[v];
    }
    if (n_kept) *n_kept = cnt;
}

std::string var_name(const char* contig, uint32_t pos) { return std::string(contig ? contig : "??") + ":" + std::to_string(uint64_t(pos) + 1); }   // format_var, panvcf.rs:187-193

void free_out(lcty_panvcf_out* o) {
    free(o->seqs); free(o->seq_off); free(o->names); free(o->kept_cols); free(o->col_unknown); free(o->col_len); free(o->col_reason);
    memset(o, 0, sizeof(*o));
}

// filter_variants + reconstruct_sequences + the has_n filter of add_locus; the arrays of *out (zero on entry) belong to h
void reconstruct(lcty_ctx* ctx, const char* contig, uint32_t ref_start, uint32_t ref_end, const uint8_t* ref_seq, const Records& r, const char* names,
                 double unknown_frac, bool overlaps_allowed, Handoff& h, lcty_panvcf_out* out) {
    if (!ref_seq || !names) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (ref_end <= ref_start) fail(LCTY_ERR_INVALID_INPUT, "empty interval %u-%u", ref_start, ref_end);
    check_records(r, true);
    const std::vector<std::string> nm = split_names(names, r.n_cols);
    const uint32_t V = r.n, H = r.n_cols;
    const uint64_t ref_len = ref_end - ref_start;
    const uint64_t n_alleles = V ? r.rec_allele[V] : 0;
    if (V && r.rec_allele[0] != 0) fail(LCTY_ERR_INVALID_DATA, "the allele table does not start at 0");
    const uint64_t pool_len = n_alleles ? r.allele_off[n_alleles] : 0;
    if (pool_len && !r.pool) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    const uint32_t n_batches = (V + WAVE - 1) / WAVE;
    lcty_panvcf_stats st{};
    const double t0 = now_ms();
    ctx->activate();
    hipStream_t s = ctx->stream;

    DevBuf<uint8_t> d_ref, d_pool, d_kept, d_hasn, d_out, d_out2;
    DevBuf<uint32_t> d_pos, d_rlen, d_rec, d_flags, d_nacc, d_unk, d_novl, d_first, d_cols;
    DevBuf<uint64_t> d_aoff, d_mask, d_len, d_segoff, d_seqoff, d_newoff;
    DevBuf<int16_t> d_gt, d_gtt;
    DevBuf<Seg> d_segs;
    d_ref.alloc(ref_len); d_ref.upload(ref_seq, ref_len, s);
    d_pool.alloc(std::max<uint64_t>(pool_len, 1)); d_pool.upload(r.pool, pool_len, s);
    d_pos.alloc(std::max(V, 1u)); d_rlen.alloc(std::max(V, 1u)); d_rec.alloc(uint64_t(V) + 1); d_aoff.alloc(n_alleles + 1);
    d_kept.alloc(std::max(V, 1u)); d_kept.zero(s);
    uint32_t flags[F_COUNT] = {V, V, V, 0, 0, 0, 0, 0};
    d_flags.alloc(F_COUNT); d_flags.upload(flags, F_COUNT, s);
    const uint64_t cells = uint64_t(V) * H;
    d_gt.alloc(std::max<uint64_t>(cells, 1)); d_gtt.alloc(std::max<uint64_t>(cells, 1));
    d_mask.alloc(std::max<uint64_t>(uint64_t(H) * n_batches, 1));
    d_nacc.alloc(H); d_unk.alloc(H); d_novl.alloc(H); d_first.alloc(H); d_len.alloc(H); d_hasn.alloc(H); d_hasn.zero(s);
    d_segoff.alloc(uint64_t(H) + 1); d_seqoff.alloc(uint64_t(H) + 1);
    if (V) {
        d_pos.upload(r.pos, V, s); d_rlen.upload(r.rlen, V, s); d_rec.upload(r.rec_allele, uint64_t(V) + 1, s); d_aoff.upload(r.allele_off, n_alleles + 1, s);
        d_gt.upload(r.gt, cells, s);
    }
    sync(ctx);
    st.upload_ms = now_ms() - t0;
    st.bytes_h2d = ref_len + pool_len + cells * 2 + uint64_t(V) * 12 + n_alleles * 8;

    // (a) rows: kept records, the transposed matrix, the verdicts
    double t = now_ms();
    if (V) {
        hipLaunchKernelGGL(panvcf_tile_kernel, dim3((V + TILE - 1) / TILE, (H + TILE - 1) / TILE), dim3(TILE_THREADS), 0, s, d_gt.p, V, H, d_rec.p, d_kept.p,
                           d_gtt.p, d_flags.p);
        LCTY_HIP(hipGetLastError());
        hipLaunchKernelGGL(panvcf_verdict_kernel, dim3((V + 255) / 256), dim3(256), 0, s, V, d_pos.p, d_rlen.p, d_rec.p, d_aoff.p, n_alleles, pool_len, d_kept.p,
                           ref_start, ref_end, d_flags.p);
        LCTY_HIP(hipGetLastError());
    }
    LCTY_HIP(hipMemcpyAsync(flags, d_flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
    sync(ctx);
    st.rows_ms = now_ms() - t;
    if (flags[F_BAD] < V)
        fail(LCTY_ERR_INVALID_DATA, "Variant %s (record %u): a genotype names an allele the record does not have, or its allele table is broken",
             var_name(contig, r.pos[flags[F_BAD]]).c_str(), flags[F_BAD]);
    out->n_kept_records = flags[F_KEPT];

    // (b) chain, (c) scans
    t = now_ms();
    const uint32_t col_blocks = (H + COL_THREADS / WAVE - 1) / (COL_THREADS / WAVE);
    hipLaunchKernelGGL(panvcf_chain_kernel, dim3(col_blocks), dim3(COL_THREADS), 0, s, d_gtt.p, V, H, d_pos.p, d_rlen.p, d_rec.p, d_aoff.p, d_kept.p, d_flags.p,
                       ref_start, ref_end, n_batches, d_mask.p, d_nacc.p, d_len.p, d_unk.p, d_novl.p, d_first.p);
    LCTY_HIP(hipGetLastError());
    sync(ctx);
    st.chain_ms = now_ms() - t;
    t = now_ms();
    launch_scan<uint64_t>(s, H, LoadU32AsU64{d_nacc.p}, AddOp{}, uint64_t(0), d_segoff.p, true);
    launch_scan<uint64_t>(s, H, LoadU64{d_len.p}, AddOp{}, uint64_t(0), d_seqoff.p, true);
    std::vector<uint64_t> seq_off(uint64_t(H) + 1);
    std::vector<uint32_t> unk(H), novl(H), first(H);
    uint64_t n_segs = 0;
    d_seqoff.download(seq_off.data(), uint64_t(H) + 1, s); d_segoff.download(&n_segs, 1, s, H);
    d_unk.download(unk.data(), H, s); d_novl.download(novl.data(), H, s); d_first.download(first.data(), H, s);
    sync(ctx);
    // the first ignored overlap in record-major order; forbidden: the error of panvcf.rs:293-295
    uint64_t total_overlaps = 0; uint32_t ovl_rec = NONE, ovl_col = 0;
    for (uint32_t h = 0; h < H; h++) {
        total_overlaps += novl[h];
        if (first[h] < ovl_rec) { ovl_rec = first[h]; ovl_col = h; }
    }
    if (total_overlaps && !overlaps_allowed)
        fail(LCTY_ERR_INVALID_DATA, "Overlapping variants forbidden (%s for %s)", var_name(contig, r.pos[ovl_rec]).c_str(), nm[ovl_col].c_str());
    if (flags[F_STRADDLE] < flags[F_BREAK])                             // panvcf.rs:268-271
        fail(LCTY_ERR_INVALID_INPUT, "Variant %s overlaps the boundary of the region %u-%u", var_name(contig, r.pos[flags[F_STRADDLE]]).c_str(), ref_start + 1, ref_end);
    uint64_t max_len = 0;
    for (uint32_t h = 0; h < H; h++) {
        const uint64_t len = seq_off[h + 1] - seq_off[h];
        if (len >= 0x7FFFFFFFull) fail(LCTY_ERR_UNSUPPORTED, "haplotype %s would be %llu bases long", nm[h].c_str(), static_cast<unsigned long long>(len));
        max_len = std::max(max_len, len);
    }
    const uint64_t total = seq_off[H];
    d_segs.alloc(std::max<uint64_t>(n_segs, 1));
    d_out.alloc((total + 7) / 8 * 8 + 8);
    hipLaunchKernelGGL(panvcf_segment_kernel, dim3(col_blocks), dim3(COL_THREADS), 0, s, d_gtt.p, V, H, d_pos.p, d_rlen.p, d_rec.p, d_aoff.p, ref_start, n_batches,
                       d_mask.p, d_segoff.p, d_segs.p);
    LCTY_HIP(hipGetLastError());
    sync(ctx);
    st.scan_ms = now_ms() - t;
    st.n_segments = n_segs; st.out_bytes = total;

    // (d) gather
    t = now_ms();
    const uint32_t tiles = static_cast<uint32_t>((max_len + 7) / GATHER_TILE + 1);      // a column may begin anywhere inside its first word
    std::vector<uint8_t> hasn(H);
    for (uint32_t h0 = 0; h0 < H; h0 += 65535) {
        const uint32_t hn = std::min(H - h0, 65535u);
        hipLaunchKernelGGL(panvcf_gather_kernel, dim3(tiles, hn), dim3(GATHER_THREADS), 0, s, d_seqoff.p + h0, d_segoff.p + h0, d_segs.p, d_ref.p, ref_len, d_pool.p,
                           pool_len, d_out.p, d_hasn.p + h0, d_flags.p);
        LCTY_HIP(hipGetLastError());
    }
    d_hasn.download(hasn.data(), H, s);
    LCTY_HIP(hipMemcpyAsync(flags, d_flags.p, sizeof(flags), hipMemcpyDeviceToHost, s));
    sync(ctx);
    st.gather_ms = now_ms() - t;
    if (flags[F_OOB]) fail(LCTY_ERR_RUNTIME, "reconstruction read outside its sources");

    // discard_unknown (panvcf.rs:205-207), then has_n (add.rs:776)
    t = now_ms();
    std::vector<uint32_t> keep; std::vector<uint64_t> new_off{0};
    std::vector<uint32_t> col_len(H); std::vector<uint8_t> reason(H);
    std::string kept_names;
    for (uint32_t h = 0; h < H; h++) {
        col_len[h] = static_cast<uint32_t>(seq_off[h + 1] - seq_off[h]);
        const double bound = unknown_frac * static_cast<double>(col_len[h]);
        if (static_cast<double>(unk[h]) > bound) { reason[h] = LCTY_PANVCF_UNKNOWN; out->n_unknown++; }
        else if (hasn[h]) { reason[h] = LCTY_PANVCF_HAS_N; out->n_with_n++; }
        else {
            reason[h] = LCTY_PANVCF_KEPT;
            keep.push_back(h); new_off.push_back(new_off.back() + col_len[h]);
            kept_names += nm[h]; kept_names.push_back('\0');
        }
    }
    // (e) compaction
    const uint32_t K = static_cast<uint32_t>(keep.size());
    const uint64_t kept_total = new_off.back();
    out->seqs = static_cast<uint8_t*>(h.raw(kept_total));                               // the copy lands in the caller's buffer
    if (K == H) {
        d_out.download(out->seqs, kept_total, s);
    } else if (K) {
        d_cols.alloc(K); d_cols.upload(keep.data(), K, s);
        d_newoff.alloc(uint64_t(K) + 1); d_newoff.upload(new_off.data(), uint64_t(K) + 1, s);
        d_out2.alloc((kept_total + 7) / 8 * 8 + 8);
        for (uint32_t k0 = 0; k0 < K; k0 += 65535) {
            const uint32_t kn = std::min(K - k0, 65535u);
            hipLaunchKernelGGL(panvcf_compact_kernel, dim3(tiles, kn), dim3(GATHER_THREADS), 0, s, d_cols.p + k0, d_seqoff.p, d_newoff.p + k0, d_out.p, d_out2.p);
            LCTY_HIP(hipGetLastError());
        }
        d_out2.download(out->seqs, kept_total, s);
    }
    sync(ctx);
    st.compact_ms = now_ms() - t;
    st.bytes_d2h = kept_total + uint64_t(H) * 25;
    st.total_ms = now_ms() - t0;

    out->n_seqs = K; out->n_cols = H; out->total_overlaps = total_overlaps; out->stats = st;
    out->seq_off = h.copy(new_off);
    out->names = h.copy(kept_names.data(), kept_names.size()); out->names_len = kept_names.size();
    out->kept_cols = h.copy(keep);
    out->col_unknown = h.copy(unk); out->col_len = h.copy(col_len); out->col_reason = h.copy(reason);
}

}  // namespace

extern "C" {

int32_t lcty_panvcf_names(uint32_t n_samples, const char* samples, const uint32_t* ploidy, const char* ref_name, uint32_t n_leave_out, const char* leave_out,
                          uint32_t cap_cols, uint32_t* n_cols, uint32_t* col_sample, uint32_t* col_hap, char* names, uint64_t cap_names, uint64_t* names_len,
                          uint32_t* n_left_out) {
    return guarded([&] {
        if (!ref_name || !n_cols || !names_len || (n_samples && (!samples || !ploidy)) || (n_leave_out && !leave_out)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const std::vector<std::string> sm = split_names(samples, n_samples), lo = split_names(leave_out, n_leave_out);
        const std::unordered_set<std::string> leave(lo.begin(), lo.end());
        std::unordered_set<std::string> seen;
        std::vector<uint32_t> cs, ch; std::string blob;
        uint32_t left = 0, n_kept_samples = 0;
        auto push = [&](uint32_t sample, uint32_t hap, const std::string& name) { cs.push_back(sample); ch.push_back(hap); blob += name; blob.push_back('\0'); };
        if (leave.count(ref_name)) left++;                              // panvcf.rs:75-82
        else { seen.insert(ref_name); push(LCTY_NONE_U32, 0, ref_name); }
        for (uint32_t i = 0; i < n_samples; i++) {
            const std::string& sample = sm[i];
            if (leave.count(sample)) { left += ploidy[i]; continue; }
            if (ploidy[i] == 0) fail(LCTY_ERR_INVALID_DATA, "Sample %s has zero ploidy", sample.c_str());
            if (ploidy[i] > 255) fail(LCTY_ERR_INVALID_DATA, "Sample %s has extremely high ploidy", sample.c_str());
            for (uint32_t hap = 0; hap < ploidy[i]; hap++) {
                const std::string name = ploidy[i] == 1 ? sample : sample + "." + std::to_string(hap + 1);
                if (leave.count(name)) { left++; continue; }
                if (!seen.insert(name).second) fail(LCTY_ERR_INVALID_DATA, "Duplicate haplotype name (%s)", name.c_str());
                push(i, hap, name);
            }
            n_kept_samples++;
        }
        if (!n_kept_samples) fail(LCTY_ERR_INVALID_DATA, "Loaded zero haplotypes");
        *n_cols = static_cast<uint32_t>(cs.size()); *names_len = blob.size();
        if (n_left_out) *n_left_out = left;
        if (col_sample || col_hap || names) {
            if (!col_sample || !col_hap || !names) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            if (cap_cols < cs.size() || cap_names < blob.size()) fail(LCTY_ERR_INVALID_INPUT, "output buffers too small (%zu columns, %zu name bytes)", cs.size(), blob.size());
            memcpy(col_sample, cs.data(), 4 * cs.size()); memcpy(col_hap, ch.data(), 4 * ch.size()); memcpy(names, blob.data(), blob.size());
        }
    });
}

int32_t lcty_panvcf_filter(lcty_ctx* ctx, uint32_t n_recs, uint32_t n_cols, const int16_t* gt, uint8_t* kept, uint64_t* n_kept) {
    return guarded([&] {
        if (!ctx || (n_recs && !kept)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        filter_records(ctx, Records{n_recs, nullptr, nullptr, nullptr, nullptr, nullptr, n_cols, gt}, kept, n_kept);
    });
}

int32_t lcty_panvcf_reconstruct(lcty_ctx* ctx, const char* contig, uint32_t ref_start, uint32_t ref_end, const uint8_t* ref_seq, uint32_t n_recs,
                                const uint32_t* pos, const uint32_t* ref_len, const uint32_t* rec_allele, const uint64_t* allele_off, const uint8_t* allele_bytes,
                                uint32_t n_cols, const int16_t* gt, const char* names, double unknown_frac, int32_t overlaps_allowed, lcty_panvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_panvcf_out o{}; Handoff h;
        reconstruct(ctx, contig, ref_start, ref_end, ref_seq, Records{n_recs, pos, ref_len, rec_allele, allele_off, allele_bytes, n_cols, gt}, names, unknown_frac,
                    overlaps_allowed != 0, h, &o);
        *out = o; h.commit();
    });
}

void lcty_panvcf_out_free(lcty_panvcf_out* out) {
    if (out) free_out(out);
}

int32_t lcty_db_find_boundary(lcty_ctx* ctx, uint32_t start, uint32_t end, uint32_t n_recs, const uint32_t* pos, const uint32_t* ref_len, uint32_t k,
                              const uint16_t* counts, uint64_t n_counts, uint32_t allowed_expansion, uint32_t moving_window, int32_t left, int32_t* found,
                              uint32_t* position, double* weights) {
    return guarded([&] {
        if (!ctx || !found || !position) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *found = find_boundary(ctx, start, end, n_recs, pos, ref_len, k, counts, n_counts, allowed_expansion, moving_window, left != 0, position, weights) ? 1 : 0;
    });
}

int32_t lcty_db_expand_locus(lcty_ctx* ctx, const char* locus, uint32_t inner_start, uint32_t inner_end, uint32_t contig_len, uint32_t win_start,
                             const uint8_t* win_seq, uint64_t win_len, uint32_t k, const uint16_t* win_counts, uint64_t n_win_counts, uint32_t n_recs,
                             const uint32_t* pos, const uint32_t* ref_len, uint32_t n_expansions, const uint32_t* expansions, uint32_t moving_window,
                             lcty_expand_out* out) {
    return guarded([&] {
        if (!ctx) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_recs && (!pos || !ref_len)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        expand_locus(ctx, locus, inner_start, inner_end, contig_len, Window{win_start, win_len, win_seq, k, win_counts, n_win_counts}, n_recs, pos, ref_len,
                     n_expansions, expansions, moving_window, out);
    });
}

int32_t lcty_db_locus_from_vcf(lcty_ctx* ctx, const lcty_locus_vcf_in* in, const lcty_db_params* params, lcty_locus_vcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !in || !params || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (!in->locus || !in->contig || !in->win_seq || !in->names || !in->expansions || !in->n_expansions) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (!params->only_seqs && (!in->hap_counts || !in->hap_cnt_off))
            fail(LCTY_ERR_INVALID_INPUT, "the k-mer counts of the haplotypes are missing (or set only_seqs: the sequences alone)");
        lcty_locus_vcf_stats st{};
        const double t0 = now_ms();
        const Records all{in->n_recs, in->pos, in->ref_len, in->rec_allele, in->allele_off, in->allele_bytes, in->n_cols, in->gt};
        const Window win{in->win_start, in->win_len, in->win_seq, in->k, in->win_counts, in->n_win_counts};
        st.n_cols = in->n_cols; st.n_records = in->n_recs;
        // the records with variation among the retained columns (filter_variants): what the boundary search looks at
        lcty_expand_out ex{};
        if (in->n_expansions == 1 && in->expansions[0] == 0) {
            ex.start = in->inner_start; ex.end = in->inner_end; ex.n_attempts = 1;
        } else {
            check_records(all, true);
            std::vector<uint8_t> kept(std::max(in->n_recs, 1u));
            filter_records(ctx, all, kept.data(), nullptr);
            std::vector<uint32_t> kp, kl;
            for (uint32_t v = 0; v < in->n_recs; v++) if (kept[v]) { kp.push_back(in->pos[v]); kl.push_back(in->ref_len[v]); }
            st.filter_ms = now_ms() - t0;
            expand_locus(ctx, in->locus, in->inner_start, in->inner_end, in->contig_len, win, static_cast<uint32_t>(kp.size()), kp.data(), kl.data(), in->n_expansions,
                         in->expansions, in->moving_window, &ex);
        }
        st.expand_ms = ex.total_ms;
        st.start = ex.start; st.end = ex.end; st.attempt = ex.attempt; st.allowed_expansion = ex.allowed_expansion; st.crop_bits = ex.crop_bits;
        if (ex.end <= ex.start || ex.start < win.start || ex.end > win.end())
            fail(LCTY_ERR_INVALID_INPUT, "the window %u-%llu does not hold the locus %u-%u", win.start, static_cast<unsigned long long>(win.end()), ex.start, ex.end);
        // the records of the new interval: the contiguous run from the first to the last that fetch would return (those between are skipped by the walk)
        uint32_t first = in->n_recs, last = 0;
        for (uint32_t v = 0; v < in->n_recs; v++)
            if (in->pos[v] < ex.end && uint64_t(in->pos[v]) + in->ref_len[v] > ex.start) { if (first == in->n_recs) first = v; last = v + 1; }
        Records sub = all;
        std::vector<uint32_t> rec_allele;
        if (first < last) {
            sub.n = last - first; sub.pos += first; sub.rlen += first; sub.gt += uint64_t(first) * in->n_cols;
            rec_allele.assign(in->rec_allele + first, in->rec_allele + last + 1);
            const uint32_t a0 = rec_allele[0];
            for (uint32_t& a : rec_allele) a -= a0;
            sub.rec_allele = rec_allele.data(); sub.allele_off = in->allele_off + a0;
        } else {
            sub.n = 0;
        }
        lcty_panvcf_out rec{}; Handoff h_rec;                               // the reconstruction: read here, never handed out
        const uint8_t* ref_seq = in->win_seq + (ex.start - win.start);
        const uint64_t ref_len = ex.end - ex.start;
        // allele_off of the run keeps its absolute offsets into the pool: the pool goes along whole
        reconstruct(ctx, in->contig, ex.start, ex.end, ref_seq, sub, in->names, in->unknown_frac, in->overlaps_allowed != 0, h_rec, &rec);
        st.reconstruct_ms = rec.stats.total_ms; st.recon = rec.stats;
        st.n_kept_records = rec.n_kept_records; st.total_overlaps = rec.total_overlaps; st.n_unknown = rec.n_unknown; st.n_with_n = rec.n_with_n;
        st.n_haplotypes = rec.n_seqs;
        // check_sequences without a reference (add.rs:655-690)
        if (rec.n_seqs < 2) fail(LCTY_ERR_INVALID_DATA, "Less than two haplotypes available for locus %s", in->locus);
        uint64_t shortest = ~0ull;
        for (uint32_t a = 0; a < rec.n_seqs; a++) shortest = std::min(shortest, rec.seq_off[a + 1] - rec.seq_off[a]);
        st.shortest = shortest;
        if (shortest < 1000) st.warn_bits |= LCTY_LOCUS_WARN_VERY_SHORT; else if (shortest < 10000) st.warn_bits |= LCTY_LOCUS_WARN_SHORT;
        constexpr uint64_t AFFIX = 5;
        if (shortest < AFFIX) fail(LCTY_ERR_INVALID_INPUT, "a haplotype of locus %s has %llu bases, fewer than the %llu compared at the boundary", in->locus,
                                   static_cast<unsigned long long>(shortest), static_cast<unsigned long long>(AFFIX));
        for (uint32_t a = 1; a < rec.n_seqs; a++) {
            const uint8_t* s0 = rec.seqs; const uint64_t l0 = rec.seq_off[1];
            const uint8_t* s = rec.seqs + rec.seq_off[a]; const uint64_t l = rec.seq_off[a + 1] - rec.seq_off[a];
            if (memcmp(s, s0, AFFIX) || memcmp(s + l - AFFIX, s0 + l0 - AFFIX, AFFIX)) { st.warn_bits |= LCTY_LOCUS_WARN_BOUNDARY_DIFFERS; break; }
        }
        lcty_locus_vcf_out o{}; Handoff h;
        // the names of the reconstructed haplotypes' columns, for the caller who maps files.kept back: kept indexes the surviving haplotypes
        o.hap_cols = h.copy(rec.kept_cols, rec.n_seqs); o.n_hap_cols = rec.n_seqs;
        const std::string bed = std::string(in->contig) + "\t" + std::to_string(ex.start) + "\t" + std::to_string(ex.end) + "\t" + in->locus + "\n";   // bed_fmt
        o.ref_bed = h.copy(bed.data(), bed.size()); o.ref_bed_len = bed.size();
        const double tb = now_ms();
        const int32_t brc = lcty_db_build_locus(ctx, rec.n_seqs, rec.names, rec.seqs, rec.seq_off, ref_seq, ref_len, in->hap_counts, in->hap_cnt_off, in->k,
                                                in->counter_bytes, params, &o.files);          // the last thing that can fail: its files are not h's
        if (brc != LCTY_OK) throw Error(brc, lcty_last_error());
        st.build_ms = now_ms() - tb;
        st.n_identical = rec.n_seqs - o.files.n_kept;
        st.total_ms = now_ms() - t0;
        o.stats = st;
        *out = o; h.commit();
    });
}

void lcty_locus_vcf_out_free(lcty_locus_vcf_out* out) {
    if (!out) return;
    lcty_db_files_free(&out->files);
    free(out->ref_bed); free(out->hap_cols);
    memset(out, 0, sizeof(*out));
}

}  // extern "C"
