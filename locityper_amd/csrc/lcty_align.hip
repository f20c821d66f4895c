// lcty_align.hip — pairwise alignments of a locus's haplotypes, the backbone strategy of `locityper align` (what `--transitive 0`
// runs): src/seq/align.rs process_pair 627-679, precompute_kmers / get_kmer_matches 102-120 and 202-224, align_from_backbone 246-292,
// align_multik 294-318; smart_align src/seq/wfa.rs:280-321. The result is the content of DB/loci/<locus>/haplotypes.paf.gz.
//   index    per (sequence, k): a 64-bit hash per window out of prefix sums (align_prefix_kernel, align_keys_kernel), one segmented
//            sort per k (rocPRIM) — once per call
//   stage A  per (pair, k): every window of the reference looks its hash up in the query's sorted list; every candidate is compared
//            base by base before it counts (align_join_kernel, counting pass, scan, emitting pass). The matches leave sorted by
//            (pos1, pos2) because a reference position writes its own run in ascending pos2.
//   stage B  per (pair, k): LCSk++ (Pavetic, Zuzic, Sikic 2014; rust-bio's bio::alignment::sparse::lcskpp): one lane per task,
//            a prefix-maximum (Fenwick) tree over the query coordinate, a binary search for the diagonal predecessor
//   stage C  per (pair, k): the walk of align_from_backbone with smart_align; routing, align_simple and the exact aligner's cell,
//            tie rule and walk back are those of lcty_gotoh.hpp, which alignment recovery (lcty_transfer_device.hpp) calls too; here
//            on plain bytes and WITHOUT recovery's step limit, which belongs to accuracy level 6: `locityper align` runs level 9.
//   per pair the best k (first wins a tie) and the counts are taken on the device; only the winner's CIGAR is downloaded.
#include "lcty_common.hpp"
#include "lcty_seq.hpp"
#include "lcty_gotoh.hpp"
#include "lcty_transfer_device.hpp"                 // xfer::DP_SMALL, the size class of the statistics; double_move and the operation classes
#include "lcty_align_internal.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <array>
#include <cmath>

namespace {
using namespace lcty;
using gotoh::OP_I; using gotoh::OP_D; using gotoh::OP_EQ; using gotoh::OP_X; using gotoh::PEN_X; using gotoh::PEN_O; using gotoh::PEN_E; using gotoh::INF32;

constexpr uint64_t kHashBase = 0x9E3779B97F4A7C15ull;          // odd: invertible modulo 2^64
constexpr uint64_t kNoKey = ~0ull;                               // key of a window that is not a k-mer (sorts behind every hash)
constexpr uint64_t kMaxMatches = 1ull << 24;                     // matches of one (pair, k); beyond: LCTY_ERR_UNSUPPORTED
constexpr uint32_t kLevels = 3;
constexpr uint32_t kLevelDim[kLevels] = {255, 2047, 16383};      // longest side of a stretch the exact aligner takes at a level
constexpr uint32_t kLevelCells[kLevels] = {1u << 16, 1u << 22, 1u << 26};
constexpr uint32_t kLevelLanes[kLevels] = {8192, 128, 8};        // lanes in flight (their scratch: 0.6 GB, 0.5 GB, 0.5 GB)
enum : uint32_t { ST_TRIVIAL = 0, ST_SIMPLE, ST_SMALL, ST_GENERAL, ST_DROPPED, ST_CELLS, ST_POINTS, ST_OVERFLOW, ST_COUNT };

__host__ __device__ inline uint64_t powu(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1, b *= b) if (e & 1) r *= b;
    return r;
}

// P[i] = sum over t < i of (code(t) + 1) * B^t, NP[i] = bytes outside ACGT before i; sequence s has len + 1 entries from off[s] + s on.
// One block per sequence: a run of consecutive bases per thread, a scan over the threads' sums.
__global__ __launch_bounds__(256) void align_prefix_kernel(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off,
                                                           uint64_t* __restrict__ P, uint32_t* __restrict__ NP) {
    __shared__ uint64_t sh[256];
    __shared__ uint32_t sn[256];
    __shared__ uint64_t tot_h;
    __shared__ uint32_t tot_n;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint64_t base = off[s], L = off[s + 1] - base, pb = base + s;
    const uint64_t chunk = (L + 255) / 256, lo = min(t * chunk, L), hi = min(lo + chunk, L);
    uint64_t sum = 0, pw = powu(kHashBase, lo);
    uint32_t nn = 0;
    for (uint64_t i = lo; i < hi; i++) {
        uint32_t c = base_enc(seq[base + i]);
        if (c > 3u) { nn++; c = 0; }
        sum += (c + 1) * pw; pw *= kHashBase;
    }
    sh[t] = sum; sn[t] = nn;
    __syncthreads();
    if (t == 0) {
        uint64_t a = 0; uint32_t b = 0;
        for (uint32_t x = 0; x < 256; x++) { const uint64_t v = sh[x]; const uint32_t w = sn[x]; sh[x] = a; sn[x] = b; a += v; b += w; }
        tot_h = a; tot_n = b;
    }
    __syncthreads();
    uint64_t acc = sh[t]; uint32_t n = sn[t];
    pw = powu(kHashBase, lo);
    for (uint64_t i = lo; i < hi; i++) {
        P[pb + i] = acc; NP[pb + i] = n;
        uint32_t c = base_enc(seq[base + i]);
        if (c > 3u) { n++; c = 0; }
        acc += (c + 1) * pw; pw *= kHashBase;
    }
    if (t == 0) { P[pb + L] = tot_h; NP[pb + L] = tot_n; }
}

// key of window p of every sequence: the hash of its k bases (independent of p), or kNoKey: the window runs over the end or holds a
// byte outside ACGT. hash_mask: the knob align_hash_bits (all ones by default; then the one value that equals kNoKey is moved).
__global__ __launch_bounds__(256) void align_keys_kernel(const uint64_t* __restrict__ off, const uint64_t* __restrict__ P, const uint32_t* __restrict__ NP,
                                                         uint32_t k, uint64_t base_inv, uint64_t hash_mask, uint64_t* __restrict__ keys,
                                                         uint32_t* __restrict__ vals) {
    const uint32_t s = blockIdx.x;
    const uint64_t base = off[s], L = off[s + 1] - base, pb = base + s;
    for (uint64_t p = threadIdx.x; p < L; p += 256) {
        uint64_t key = kNoKey;
        if (p + k <= L && NP[pb + p + k] == NP[pb + p]) {
            uint64_t h = (P[pb + p + k] - P[pb + p]) * powu(base_inv, p);
            h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27; h *= 0x94D049BB133111EBull; h ^= h >> 31;
            h &= hash_mask;
            key = h == kNoKey ? kNoKey - 1 : h;
        }
        keys[base + p] = key; vals[base + p] = static_cast<uint32_t>(p);
    }
}

struct Task { uint32_t ref, qry, ki, k; };

// Stage A, both passes. One block per (pair, k); a thread per reference window p1. EMIT = false: cnt[slot] = verified matches of p1.
// EMIT = true: they are written from mo[slot] on, in ascending pos2 (a bucket of equal keys is put in order here: the segmented sort
// is not relied on to keep equal keys in input order).
template <bool EMIT>
__global__ __launch_bounds__(256) void align_join_kernel(const Task* __restrict__ tasks, const uint64_t* __restrict__ slot_off,
                                                         const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off, uint64_t total,
                                                         const uint64_t* __restrict__ keys_in, const uint64_t* __restrict__ keys_sorted,
                                                         const uint32_t* __restrict__ vals_sorted, uint32_t* __restrict__ cnt,
                                                         const uint64_t* __restrict__ mo, uint2* __restrict__ matches) {
    const Task tk = tasks[blockIdx.x];
    const uint64_t rb = off[tk.ref], Lr = off[tk.ref + 1] - rb, qb = off[tk.qry], Lq = off[tk.qry + 1] - qb;
    const uint64_t* kr = keys_in + static_cast<uint64_t>(tk.ki) * total + rb;
    const uint64_t* kq = keys_sorted + static_cast<uint64_t>(tk.ki) * total + qb;
    const uint32_t* vq = vals_sorted + static_cast<uint64_t>(tk.ki) * total + qb;
    const uint64_t slot0 = slot_off[blockIdx.x];
    for (uint64_t p1 = threadIdx.x; p1 < Lr; p1 += 256) {
        const uint64_t h = kr[p1];
        uint32_t c = 0;
        uint2* dst = EMIT ? matches + mo[slot0 + p1] : nullptr;
        if (h != kNoKey) {
            uint64_t lo = 0, hi = Lq;
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (kq[mid] < h) lo = mid + 1; else hi = mid; }
            for (; lo < Lq && kq[lo] == h; lo++) {
                const uint32_t p2 = vq[lo];
                bool eq = true;
                for (uint32_t i = 0; i < tk.k && eq; i++) eq = seq[rb + p1 + i] == seq[qb + p2 + i];
                if (!eq) continue;
                if (EMIT) {
                    uint32_t at = c;                                          // insertion by pos2
                    while (at > 0 && dst[at - 1].y > p2) { dst[at] = dst[at - 1]; at--; }
                    dst[at] = make_uint2(static_cast<uint32_t>(p1), p2);
                }
                c++;
            }
        }
        if (!EMIT) cnt[slot0 + p1] = c;
    }
}

__global__ void align_task_offsets_kernel(const uint64_t* __restrict__ slot_off, const uint64_t* __restrict__ mo, uint32_t n_tasks, uint64_t* __restrict__ tm) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_tasks) tm[t] = mo[slot_off[t]];
}

// Stage B. dp(m) = max(k, dp(m') + 1 for m' = (i - 1, j - 1) a match, k + max dp(m'') over matches with i'' + k <= i and j'' + k <= j).
// The matches are sorted, so their start events (i, j) and their end events (i + k, j + k) are two sorted sequences: merged on the fly,
// an end before a start at the same point. A start asks the tree for the best dp among ends at columns <= j; an end takes the diagonal
// predecessor (whose own end came earlier) and enters the tree at column j + k. Ties: the lowest match index (tree entries are
// value << 32 | ~index; the argmax is taken with a strict >, ends come in index order); a jump is kept over an equal continuation.
__device__ inline uint64_t fen_query(const uint64_t* f, uint32_t pos) {
    uint64_t r = 0;
    for (; pos > 0; pos -= pos & (0u - pos)) r = max(r, f[pos]);
    return r;
}
__device__ inline void fen_update(uint64_t* f, uint32_t n, uint32_t pos, uint64_t v) {
    for (; pos <= n; pos += pos & (0u - pos)) if (f[pos] < v) f[pos] = v;
}
__global__ __launch_bounds__(64) void align_chain_kernel(const Task* __restrict__ tasks, uint32_t n_tasks, const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ tm, const uint2* __restrict__ matches, uint32_t* __restrict__ dp,
                                                         uint32_t* __restrict__ prev, uint32_t* __restrict__ path, const uint64_t* __restrict__ fen_off,
                                                         uint64_t* __restrict__ fen, uint32_t* __restrict__ chain, uint32_t* __restrict__ path_start,
                                                         unsigned long long* __restrict__ stats) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_tasks) return;
    const Task tk = tasks[t];
    const uint64_t m0 = tm[t];
    const uint32_t m = static_cast<uint32_t>(tm[t + 1] - m0), k = tk.k;
    const uint2* M = matches + m0;
    uint32_t* D = dp + m0; uint32_t* PV = prev + m0; uint32_t* PT = path + m0;
    uint64_t* F = fen + fen_off[t];
    const uint32_t fn = static_cast<uint32_t>(off[tk.qry + 1] - off[tk.qry]);           // columns 1..qlen (j + k <= qlen)
    uint32_t s = 0, e = 0, best = 0, best_ix = 0;
    while (e < m) {
        bool start = false;
        if (s < m) { const uint2 a = M[s], b = M[e]; start = a.x < b.x + k || (a.x == b.x + k && a.y < b.y + k); }
        if (start) {
            const uint64_t q = fen_query(F, M[s].y);
            if (q >> 32) { D[s] = k + static_cast<uint32_t>(q >> 32); PV[s] = ~static_cast<uint32_t>(q); }
            else { D[s] = k; PV[s] = 0xFFFFFFFFu; }
            s++;
        } else {
            const uint2 b = M[e];
            if (b.x > 0 && b.y > 0) {
                uint32_t lo = 0, hi = m;
                const uint32_t wx = b.x - 1, wy = b.y - 1;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; const uint2 c = M[mid]; if (c.x < wx || (c.x == wx && c.y < wy)) lo = mid + 1; else hi = mid; }
                if (lo < m && M[lo].x == wx && M[lo].y == wy && D[lo] + 1 > D[e]) { D[e] = D[lo] + 1; PV[e] = lo; }
            }
            fen_update(F, fn, b.y + k, (static_cast<uint64_t>(D[e]) << 32) | (~e));
            if (D[e] > best) { best = D[e]; best_ix = e; }
            e++;
        }
    }
    uint32_t n = 0;
    if (m) for (uint32_t x = best_ix; x != 0xFFFFFFFFu; x = PV[x]) { n++; PT[m - n] = x; }
    chain[t] = best; path_start[t] = m - n;
    atomicAdd(&stats[ST_POINTS], static_cast<unsigned long long>(n));
}

// Stage C -------------------------------------------------------------------------------------------------------------------------------
struct Lim { uint32_t dim, cells; };                            // what the exact aligner takes (a level's scratch, or the largest level)
__host__ __device__ inline bool lim_takes(const Lim& l, uint32_t n, uint32_t m) {
    return n <= l.dim && m <= l.dim && (static_cast<uint64_t>(n) + 1) * (static_cast<uint64_t>(m) + 1) <= l.cells;
}
__host__ __device__ inline size_t lane_bytes(const Lim& l) { return (2 * (static_cast<size_t>(l.dim) + 1) * sizeof(gotoh::Cell) + l.cells + 15) & ~size_t(15); }

struct PairSeq {
    const uint8_t* r; const uint8_t* q;                          // any byte outside ACGT is N, and N equals N
    __device__ __forceinline__ uint8_t R(uint32_t i) const { return base_norm(r[i]); }
    __device__ __forceinline__ uint8_t Q(uint32_t j) const { return base_norm(q[j]); }
};
// the CIGAR of a task: raw BAM words; equal neighbours merge (the reference's push_unchecked can leave `a=b=`: same alignment, same score)
struct CigOut {
    uint32_t* w; uint32_t n, cap; bool overflow;
    __device__ __forceinline__ void push(uint32_t op, uint32_t len) {
        if (!len) return;
        if (n && (w[n - 1] & 15u) == op) { w[n - 1] += len << 4; return; }
        if (n < cap) w[n++] = (len << 4) | op; else overflow = true;
    }
};

// the walk of align_from_backbone (align.rs:262-286): v.anchor(len) for a finished '=' run, v.stretch(i1, i2, j1, j2) for smart_align
template <class V>
__device__ inline void walk_backbone(const uint2* M, const uint32_t* path, uint32_t n_path, uint32_t k, uint32_t n1, uint32_t n2, V& v) {
    uint32_t i1 = 0, j1 = 0, cur = 0;
    for (uint32_t x = 0; x < n_path; x++) {
        const uint2 a = M[path[x]];
        if (i1 > a.x) { cur++; i1++; j1++; continue; }
        if (cur) { v.anchor(cur); cur = 0; }
        v.stretch(i1, a.x, j1, a.y);
        cur += k; i1 = a.x + k; j1 = a.y + k;
    }
    if (cur) v.anchor(cur);
    v.stretch(i1, n1, j1, n2);
}

// which scratch level the task needs and an upper bound of its CIGAR's items
struct Levels { Lim l[kLevels]; };                              // the levels' limits, already cut to the knob align_dp_cells
struct PlanVisitor {
    uint32_t max_gap; Lim top; Levels lv; uint32_t level; uint64_t bound;
    __device__ void anchor(uint32_t) { bound++; }
    __device__ void item(uint32_t, uint32_t) { bound++; }
    __device__ void stretch(uint32_t i1, uint32_t i2, uint32_t j1, uint32_t j2) {
        const uint32_t n = i2 - i1, m = j2 - j1;
        const gotoh::Route route = gotoh::route(n, m, max_gap);
        if (route == gotoh::ROUTE_STRAIGHT) { bound += n; return; }
        if (route == gotoh::ROUTE_SIMPLE || (route == gotoh::ROUTE_EXACT && !lim_takes(top, n, m))) { bound += min(n, m) + 1; return; }
        if (route != gotoh::ROUTE_EXACT) { bound++; return; }                 // one gap, or nothing
        bound += static_cast<uint64_t>(n) + m;
        for (uint32_t l = 0; l < kLevels; l++)
            if (lim_takes(lv.l[l], n, m)) { level = max(level, l); return; }
        level = kLevels - 1;
    }
};

struct FillVisitor {
    PairSeq S; CigOut cg; uint32_t max_gap; Lim top, mine; gotoh::Cell* rows; uint8_t* dirs; int score; uint32_t dropped;
    unsigned long long n_route[4], cells;

    __device__ bool same(uint32_t i, uint32_t j) const { return S.R(i) == S.Q(j); }
    __device__ int simple(uint32_t i1, uint32_t n, uint32_t j1, uint32_t m) {
        return gotoh::align_simple(n, m, [&](uint32_t i, uint32_t j) { return same(i1 + i, j1 + j); }, [&](uint32_t op, uint32_t len) { cg.push(op, len); });
    }
    // the end-to-end gap-affine optimum of reference [i1, +n) and query [j1, +m), no match bonus, no step limit: two rolling rows of
    // cells and a direction byte per cell, unstrided, in the lane's own scratch. The caller has checked lim_takes(mine, n, m).
    __device__ int exact(uint32_t i1, uint32_t n, uint32_t j1, uint32_t m) {
        const uint32_t W = m + 1;
        cells += static_cast<unsigned long long>(n + 1) * W;
        gotoh::Cell* prev = rows;
        gotoh::Cell* cur = rows + mine.dim + 1;
        const gotoh::Cell none{INF32, INF32, INF32};
        for (uint32_t a = 0; a <= n; a++) {
            const uint8_t rbase = a > 0 ? S.R(i1 + a - 1) : 0;
            gotoh::Cell left = none, diag = none;
            for (uint32_t b = 0; b <= m; b++) {
                const gotoh::Cell up = a > 0 ? prev[b] : none;
                const int32_t sub = (a > 0 && b > 0 && rbase != S.Q(j1 + b - 1)) ? PEN_X : 0;
                uint32_t dir;
                const gotoh::Cell c = gotoh::cell(up, left, diag, sub, a > 0, b > 0, a == 0 && b == 0, &dir);
                cur[b] = c;
                dirs[static_cast<size_t>(a) * W + b] = static_cast<uint8_t>(dir);
                left = c; diag = up;
            }
            gotoh::Cell* x = prev; prev = cur; cur = x;
        }
        // walk back: the runs arrive last first, behind the items the CIGAR has; then they are turned round and joined to them
        const uint32_t r0 = cg.n;
        CigOut rev{cg.w + r0, 0, cg.cap - r0, false};
        uint32_t a = n, b = m;
        const gotoh::Cell end = prev[m];
        uint32_t st = gotoh::end_state(end);
        while (a > 0 || b > 0) {
            const uint32_t d = dirs[static_cast<size_t>(a) * W + b];
            if (st == gotoh::ST_M) { rev.push(same(i1 + a - 1, j1 + b - 1) ? OP_EQ : OP_X, 1); a--; b--; }
            else if (st == gotoh::ST_D) { rev.push(OP_D, 1); a--; }
            else { rev.push(OP_I, 1); b--; }
            st = gotoh::back_step(st, d);
        }
        cg.overflow |= rev.overflow;
        for (uint32_t x = 0, y = rev.n; x + 1 < y; x++, y--) { const uint32_t w = rev.w[x]; rev.w[x] = rev.w[y - 1]; rev.w[y - 1] = w; }
        cg.n = r0;
        for (uint32_t x = 0; x < rev.n; x++) { const uint32_t w = cg.w[r0 + x]; cg.push(w & 15u, w >> 4); }     // (reads at or ahead of what it writes)
        return -gotoh::best_of(end);
    }
    __device__ void anchor(uint32_t len) { cg.push(OP_EQ, len); }
    __device__ void item(uint32_t op, uint32_t len) { cg.push(op, len); }
    // smart_align (wfa.rs:280-321) with max_gap as the threshold
    __device__ void stretch(uint32_t i1, uint32_t i2, uint32_t j1, uint32_t j2) {
        const uint32_t n = i2 - i1, m = j2 - j1;
        switch (gotoh::route(n, m, max_gap)) {
        case gotoh::ROUTE_SIMPLE: n_route[ST_SIMPLE]++; score += simple(i1, n, j1, m); break;
        case gotoh::ROUTE_STRAIGHT:
            n_route[ST_TRIVIAL]++;
            score += gotoh::align_straight(n, [&](uint32_t i, uint32_t j) { return same(i1 + i, j1 + j); }, [&](uint32_t op, uint32_t len) { cg.push(op, len); });
            break;
        case gotoh::ROUTE_EXACT:
            // beyond the largest scratch level the stretch is dropped, as the reference does when WFA drops an alignment (wfa.rs:234-237)
            if (!lim_takes(top, n, m) || !lim_takes(mine, n, m)) { dropped++; n_route[ST_SIMPLE]++; score += simple(i1, n, j1, m); break; }
            n_route[(n <= xfer::DP_SMALL && m <= xfer::DP_SMALL) ? ST_SMALL : ST_GENERAL]++;      // a size class: one aligner serves both
            score += exact(i1, n, j1, m);
            break;
        case gotoh::ROUTE_DEL: n_route[ST_TRIVIAL]++; cg.push(OP_D, n); score += gotoh::gap_score(n); break;
        case gotoh::ROUTE_INS: n_route[ST_TRIVIAL]++; cg.push(OP_I, m); score += gotoh::gap_score(m); break;
        default: break;
        }
    }
};

// the visitor of lane memory `mem` (lane_bytes(mine): two rows of mine.dim + 1 cells, then the direction bytes) that writes into cg
__device__ inline FillVisitor fill_visitor(PairSeq S, CigOut cg, uint32_t max_gap, Lim top, Lim mine, uint8_t* mem) {
    FillVisitor v;
    v.S = S; v.cg = cg;
    v.max_gap = max_gap; v.top = top; v.mine = mine;
    v.rows = reinterpret_cast<gotoh::Cell*>(mem); v.dirs = mem + 2 * (static_cast<size_t>(mine.dim) + 1) * sizeof(gotoh::Cell);
    v.score = 0; v.dropped = 0; v.cells = 0;
    for (uint32_t r = 0; r < 4; r++) v.n_route[r] = 0;
    return v;
}

// Task sources. Stage C has two kinds of task: a (pair, k) whose walk follows the chain of stage B, and a transitive pair whose walk
// reads finished CIGARs. A source is a small struct the plan and the fill kernel take by value: walk(t, v) leads the visitor through
// task t (true: the task turned out a shortcut), pair(t) names the two sequences it aligns, max_gap() is the threshold of its stretches;
// planned() and filled() write the per-task outputs that only this route reads.
struct BackboneSrc {
    const Task* tasks; const uint64_t* tm; const uint2* matches; const uint32_t* path; const uint32_t* path_start; const uint64_t* off;
    uint32_t gap; int32_t* t_score; uint32_t* t_dropped;
    __device__ uint32_t max_gap() const { return gap; }
    __device__ uint2 pair(uint32_t t) const { return make_uint2(tasks[t].ref, tasks[t].qry); }
    template <class V> __device__ bool walk(uint32_t t, V& v) const {
        const Task tk = tasks[t];
        const uint64_t m0 = tm[t];
        const uint32_t m = static_cast<uint32_t>(tm[t + 1] - m0);
        walk_backbone(matches + m0, path + m0 + path_start[t], m - path_start[t], tk.k, static_cast<uint32_t>(off[tk.ref + 1] - off[tk.ref]),
                      static_cast<uint32_t>(off[tk.qry + 1] - off[tk.qry]), v);
        return false;
    }
    __device__ void planned(uint32_t, bool) const {}
    __device__ void filled(uint32_t t, const FillVisitor& v) const { t_score[t] = v.score; t_dropped[t] = v.dropped; }
};

// Transitive route -----------------------------------------------------------------------------------------------------------------------
// Cigar::find_transitive_alignment (cigar.rs:1389-1414) = transfer_alignment::<true> (1248-1368): the alignment of query i to reference
// k out of the finished alignments i-j and j-k. The two CIGARs are walked side by side (double_move of lcty_cigar_walk.hpp);
// where both stand in a long enough '=' the operation is copied, what lies between two such anchors goes to smart_align — the very
// stretch() of stage C. Then Cigar::optimize (1167-1237; lcty_transfer_device.hpp holds its resumable form for wavefronts that
// carry 64 reads; here a lane has one pair and walks straight through; the predicates are shared). Both walks are templates of
// lcty_cigar_walk.hpp over the visitors of stage C: v.item() for a copied operation, v.stretch() for smart_align. One lane per task.
struct TrTaskDev { uint64_t ij_off, jk_off; uint32_t ij_n, jk_n, ref, qry, inv, _pad; };      // inv: bit 0 i-j is read inverted, bit 1 j-k
using trwalk::TrCig; using trwalk::walk_transitive; using trwalk::walk_optimize;          // lcty_cigar_walk.hpp: the host probe instantiates them too

// PASS 0: the walk of the two CIGARs out of the store, with the caller's max_gap; it finds out which tasks are shortcuts. PASS 1: optimize
// (no maximum gap) over the CIGAR pass 0 left at src + src_off[t], a plain copy for a shortcut
template <int PASS>
struct TrSrc {
    const TrTaskDev* tasks; const uint64_t* off; const uint32_t* store; uint32_t anchor_size, gap;
    const uint64_t* src_off; const uint32_t* src; const uint32_t* src_words; uint8_t* shortcut;
    __device__ uint32_t max_gap() const { return PASS == 0 ? gap : 0xFFFFFFFFu; }
    __device__ uint2 pair(uint32_t t) const { return make_uint2(tasks[t].ref, tasks[t].qry); }
    template <class V> __device__ bool walk(uint32_t t, V& v) const {
        if (PASS == 0) {
            const TrTaskDev tk = tasks[t];
            const TrCig ij{store + tk.ij_off, tk.ij_n, (tk.inv & 1u) != 0}, jk{store + tk.jk_off, tk.jk_n, (tk.inv & 2u) != 0};
            return walk_transitive(ij, jk, static_cast<uint32_t>(off[tk.qry + 1] - off[tk.qry]), static_cast<uint32_t>(off[tk.ref + 1] - off[tk.ref]), anchor_size, v);
        }
        const uint32_t* w = src + src_off[t];
        const uint32_t n = src_words[t];
        const bool sc = shortcut[t] != 0;
        if (sc) for (uint32_t x = 0; x < n; x++) v.item(w[x] & 15u, w[x] >> 4);
        else walk_optimize(w, n, trwalk::kOptGap, trwalk::kOptAnchor, v);
        return sc;
    }
    __device__ void planned(uint32_t t, bool sc) const { if (PASS == 0) shortcut[t] = sc ? 1 : 0; }
    __device__ void filled(uint32_t, const FillVisitor&) const {}
};

// The two kernels of stage C, instantiated for BackboneSrc (the backbone route), TrSrc<0> (the transitive walk) and TrSrc<1> (optimize).
// The plan is the walk without aligning: the scratch level the task needs and an upper bound of the items it writes, by which its slice
// is reserved.
template <class Src>
__global__ __launch_bounds__(64) void align_plan_kernel(Src src, uint32_t n_tasks, Lim top, Levels lv, uint32_t* __restrict__ level, uint32_t* __restrict__ cig_cap) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_tasks) return;
    PlanVisitor v{src.max_gap(), top, lv, 0, 2};
    src.planned(t, src.walk(t, v));
    level[t] = v.level;
    cig_cap[t] = static_cast<uint32_t>(min(v.bound, static_cast<uint64_t>(0xFFFFFFFFu)));
}

// one lane per task of the level's list; lane g works in scratch + g * lane_bytes(mine); the CIGAR goes to cig + cig_off[t]
template <class Src>
__global__ __launch_bounds__(64) void align_fill_kernel(Src src, const uint32_t* __restrict__ list, uint32_t n_list, uint32_t n_lanes, const uint8_t* __restrict__ seq,
                                                        Lim top, Lim mine, uint8_t* __restrict__ scratch, const uint64_t* __restrict__ cig_off,
                                                        uint32_t* __restrict__ cig, uint32_t* __restrict__ t_words, unsigned long long* __restrict__ stats) {
    const uint32_t g = blockIdx.x * 64 + threadIdx.x;
    if (g >= n_lanes) return;
    uint8_t* mem = scratch + static_cast<size_t>(g) * lane_bytes(mine);
    for (uint32_t x = g; x < n_list; x += n_lanes) {
        const uint32_t t = list[x];
        const uint2 p = src.pair(t);
        FillVisitor v = fill_visitor(PairSeq{seq + src.off[p.x], seq + src.off[p.y]},
                                     CigOut{cig + cig_off[t], 0, static_cast<uint32_t>(cig_off[t + 1] - cig_off[t]), false}, src.max_gap(), top, mine, mem);
        src.walk(t, v);
        t_words[t] = v.cg.n;
        src.filled(t, v);
        for (uint32_t r = 0; r < 4; r++) if (v.n_route[r]) atomicAdd(&stats[r], v.n_route[r]);
        if (v.dropped) atomicAdd(&stats[ST_DROPPED], static_cast<unsigned long long>(v.dropped));
        if (v.cells) atomicAdd(&stats[ST_CELLS], v.cells);
        if (v.cg.overflow) atomicAdd(&stats[ST_OVERFLOW], 1ull);
    }
}

// the '=' bases and the others of a finished CIGAR (the counts of process_pair 652-660); err(op, len) sees every item that is not '=',
// so that a caller with a sum of its own reads the words once
struct CigCounts { uint32_t n_matches, nerrs; };
template <class F>
__device__ inline CigCounts cig_counts(const uint32_t* w, uint32_t nw, F err) {
    CigCounts c{0, 0};
    for (uint32_t x = 0; x < nw; x++) {
        const uint32_t op = w[x] & 15u, len = w[x] >> 4;
        if (op == OP_EQ) c.n_matches += len;
        else { c.nerrs += len; err(op, len); }
    }
    return c;
}

// align_multik (align.rs:294-318): the best score over the ks, the first k on a tie
struct PairRes { int32_t score; uint32_t best_ki, n_matches, nerrs, n_words, _pad; };
__global__ __launch_bounds__(64) void align_select_kernel(uint32_t n_pairs, uint32_t nk, const int32_t* __restrict__ t_score, const uint32_t* __restrict__ t_words,
                                                          const uint64_t* __restrict__ cig_off, const uint32_t* __restrict__ cig, PairRes* __restrict__ res) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_pairs) return;
    uint32_t bk = 0;
    for (uint32_t ki = 1; ki < nk; ki++) if (t_score[p * nk + ki] > t_score[p * nk + bk]) bk = ki;
    const uint32_t t = p * nk + bk, nw = t_words[t];
    const CigCounts c = cig_counts(cig + cig_off[t], nw, [](uint32_t, uint32_t) {});
    res[p] = PairRes{t_score[t], bk, c.n_matches, c.nerrs, nw, 0};
}
// a finished transitive CIGAR: its score is Penalties::calculate_score (wfa.rs:87-99) of its items; best_ki stays 0
__global__ __launch_bounds__(64) void tr_count_kernel(uint32_t n_tasks, const uint64_t* __restrict__ cig_off, const uint32_t* __restrict__ cig,
                                                      const uint32_t* __restrict__ t_words, PairRes* __restrict__ res) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_tasks) return;
    const uint32_t nw = t_words[t];
    int32_t score = 0;
    const CigCounts c = cig_counts(cig + cig_off[t], nw, [&](uint32_t op, uint32_t len) {
        score -= op == OP_X ? PEN_X * static_cast<int32_t>(len) : PEN_O + PEN_E * static_cast<int32_t>(len);
    });
    res[t] = PairRes{score, 0, c.n_matches, c.nerrs, nw, 0};
}
// the CIGAR of pair p's best k to out + out_off[p]; a transitive task is a pair with one k
__global__ __launch_bounds__(64) void align_gather_kernel(uint32_t nk, const PairRes* __restrict__ res, const uint64_t* __restrict__ cig_off,
                                                          const uint32_t* __restrict__ cig, const uint64_t* __restrict__ out_off, uint32_t* __restrict__ out) {
    const uint32_t p = blockIdx.x;
    const uint32_t* w = cig + cig_off[p * nk + res[p].best_ki];
    for (uint32_t x = threadIdx.x; x < res[p].n_words; x += 64) out[out_off[p] + x] = w[x];
}

// Host ---------------------------------------------------------------------------------------------------------------------------------
struct Index {
    DevHaps haps; DevBuf<uint64_t> keys_in, keys_sorted; DevBuf<uint32_t> vals_sorted;
    uint64_t total = 0; uint32_t n_seqs = 0;
    std::vector<uint32_t> ks;
};

void build_index(lcty_ctx* ctx, const HapSet& hs, const uint8_t* seqs, const uint64_t* seq_off, const std::vector<uint32_t>& ks, Index& ix, lcty_align_stats& st) {
    hipStream_t s = ctx->stream;
    const double t0 = now_ms();
    const uint32_t n_seqs = hs.n;
    ix.total = hs.total; ix.n_seqs = n_seqs; ix.ks = ks;
    if (ix.total >= 0xFFFFFFFFull) fail(LCTY_ERR_UNSUPPORTED, "%llu bases: the k-mer index holds at most 2^32 - 2", static_cast<unsigned long long>(ix.total));
    const uint64_t T = ix.total, nk = ks.size();
    st.bytes_h2d += ix.haps.upload(ctx, hs, seqs, seq_off, 1);
    ix.keys_in.alloc(std::max<uint64_t>(nk * T, 1)); ix.keys_sorted.alloc(std::max<uint64_t>(nk * T, 1)); ix.vals_sorted.alloc(std::max<uint64_t>(nk * T, 1));
    if (nk && T) {
        DevBuf<uint64_t> P, seg; DevBuf<uint32_t> NP, vals_in; DevBuf<uint8_t> tmp;
        P.alloc(T + n_seqs); NP.alloc(T + n_seqs); vals_in.alloc(T);
        hipLaunchKernelGGL(align_prefix_kernel, dim3(n_seqs), dim3(256), 0, s, ix.haps.seqs.p, ix.haps.off.p, P.p, NP.p);
        LCTY_HIP(hipGetLastError());
        uint64_t inv = kHashBase;                                  // Newton: x <- x (2 - b x) doubles the correct low bits (3 to begin with)
        for (int it = 0; it < 6; it++) inv *= 2 - kHashBase * inv;
        const int64_t bits = ctx->knob("align_hash_bits", 64);
        const uint64_t mask = bits >= 64 ? ~0ull : ((1ull << std::max<int64_t>(bits, 1)) - 1);
        for (uint64_t ki = 0; ki < nk; ki++) {
            uint64_t* kin = ix.keys_in.p + ki * T;
            hipLaunchKernelGGL(align_keys_kernel, dim3(n_seqs), dim3(256), 0, s, ix.haps.off.p, P.p, NP.p, ks[ki], inv, mask, kin, vals_in.p);
            LCTY_HIP(hipGetLastError());
            size_t bytes = 0;
            LCTY_HIP(rocprim::segmented_radix_sort_pairs(nullptr, bytes, kin, ix.keys_sorted.p + ki * T, vals_in.p, ix.vals_sorted.p + ki * T,
                                                         static_cast<unsigned int>(T), n_seqs, ix.haps.off.p, ix.haps.off.p + 1, 0, 64, s));
            if (tmp.n < bytes) tmp.alloc(bytes + 16);
            LCTY_HIP(rocprim::segmented_radix_sort_pairs(tmp.p, bytes, kin, ix.keys_sorted.p + ki * T, vals_in.p, ix.vals_sorted.p + ki * T,
                                                         static_cast<unsigned int>(T), n_seqs, ix.haps.off.p, ix.haps.off.p + 1, 0, 64, s));
        }
        LCTY_HIP(hipStreamSynchronize(s));
    }
    LCTY_HIP(hipStreamSynchronize(s));
    st.index_ms += now_ms() - t0;
}

// the finished CIGARs of a call that keeps them on the device (lcty_align_haplotypes_transitive): one arena of raw BAM words, a slice per
// input pair. reserve() is the bounds check, on the host, in front of every launch that writes into it.
struct Store {
    DevBuf<uint32_t> buf; uint64_t used = 0;
    std::vector<uint64_t> off; std::vector<uint32_t> len;
    void reserve(uint64_t words) const {
        if (used + words > buf.n)
            fail(LCTY_ERR_UNSUPPORTED, "the finished CIGARs outgrow their store of %llu bytes: raise the knob align_cigar_store_mb",
                 static_cast<unsigned long long>(buf.n * 4));
    }
};

struct Prepared { std::vector<uint32_t> ks; Lim top; Levels lv; uint32_t max_gap; bool never; };

// the buffers of one pass of stage C: per task the level and the bound the plan gives (level, cap), the slices reserved by the bounds
// (off, cig) and the words the fill wrote into them, a level's task list and its lanes' scratch. slack: the owner keeps the workspace
// for passes to come, so it grows with head-room; without it every buffer gets the exact size.
struct StageC {
    DevBuf<uint32_t> level, cap, list, cig, words; DevBuf<uint64_t> off; DevBuf<uint8_t> scratch;
    bool slack = false;
    template <typename T> void fit(DevBuf<T>& b, size_t n) const { if (slack) b.ensure_slack(n); else b.ensure(n); }
};

// one pass of stage C over the nt tasks of a source: plan, reserve the slices by the bounds, fill level by level. Returns the tasks per level.
template <class Src>
std::array<uint64_t, kLevels> stage_c(lcty_ctx* ctx, const Src& src, uint32_t nt, const uint8_t* seq, const Prepared& pr, StageC& ws, unsigned long long* stats,
                                      lcty_align_stats& st, double& plan_ms, double& fill_ms) {
    hipStream_t s = ctx->stream;
    double t0 = now_ms();
    ws.fit(ws.level, nt); ws.fit(ws.cap, nt); ws.fit(ws.list, nt);
    hipLaunchKernelGGL(align_plan_kernel<Src>, dim3((nt + 63) / 64), dim3(64), 0, s, src, nt, pr.top, pr.lv, ws.level.p, ws.cap.p);
    LCTY_HIP(hipGetLastError());
    std::vector<uint32_t> level(nt), ccap(nt);
    ws.level.download(level.data(), nt, s); ws.cap.download(ccap.data(), nt, s);
    LCTY_HIP(hipStreamSynchronize(s));
    st.bytes_d2h += 8ull * nt;
    std::vector<uint64_t> cig_off(nt + 1, 0);
    for (uint32_t t = 0; t < nt; t++) cig_off[t + 1] = cig_off[t] + ccap[t];
    ws.fit(ws.off, nt + 1); ws.fit(ws.cig, cig_off[nt] + 1); ws.fit(ws.words, nt);
    ws.off.upload(cig_off.data(), nt + 1, s);
    st.bytes_h2d += 8ull * (nt + 1);
    plan_ms += now_ms() - t0; t0 = now_ms();
    std::array<uint64_t, kLevels> n_level{};
    std::vector<uint32_t> list;
    for (uint32_t l = 0; l < kLevels; l++) {
        list.clear();
        for (uint32_t t = 0; t < nt; t++) if (level[t] == l) list.push_back(t);
        if (list.empty()) continue;
        const Lim mine = pr.lv.l[l];
        const uint32_t lanes = static_cast<uint32_t>(std::min<size_t>(list.size(), kLevelLanes[l]));
        ws.scratch.ensure(lanes * lane_bytes(mine));
        ws.list.upload(list.data(), list.size(), s);
        st.bytes_h2d += 4ull * list.size();
        hipLaunchKernelGGL(align_fill_kernel<Src>, dim3((lanes + 63) / 64), dim3(64), 0, s, src, ws.list.p, static_cast<uint32_t>(list.size()), lanes, seq, pr.top, mine,
                           ws.scratch.p, ws.off.p, ws.cig.p, ws.words.p, stats);
        LCTY_HIP(hipGetLastError());
        LCTY_HIP(hipStreamSynchronize(s));                                    // `list` is filled again
        n_level[l] = list.size();
    }
    fill_ms += now_ms() - t0;
    return n_level;
}

struct Capture {                                               // lcty_align_backbone: every stage's output of the one task
    std::vector<uint2> matches; std::vector<uint32_t> path, cigar; uint32_t chain = 0; int32_t score = 0; uint32_t dropped = 0;
};
constexpr uint32_t kNoK = 0xFFFFFFFFu;                           // best_ki of a pair no backbone k made: a transitive alignment (best_k 0)
struct PairOut { int32_t score; uint32_t best_ki, n_matches, nerrs; std::vector<uint32_t> cigar; };

// the pairs [a, b) of refs / qrys through stages A to C; returns 0, or — the matches of the batch do not fit `budget` and the batch holds
// more than one pair — the number of leading pairs whose matches do fit (at least 1): the caller comes back with those, so the counting
// pass is repeated once, not once per halving
uint64_t run_batch(lcty_ctx* ctx, const Index& ix, const uint64_t* seq_off, const uint32_t* refs, const uint32_t* qrys, uint64_t a, uint64_t b, const Prepared& pr,
               uint64_t budget, PairOut* out, lcty_align_stats& st, Capture* cap, Store* store = nullptr, const uint64_t* pair_ix = nullptr) {
    hipStream_t s = ctx->stream;
    const uint32_t nk = static_cast<uint32_t>(ix.ks.size()), np = static_cast<uint32_t>(b - a), nt = np * nk;
    double t0 = now_ms();
    std::vector<Task> tasks(nt);
    std::vector<uint64_t> slot_off(nt + 1, 0), fen_off(nt + 1, 0);
    for (uint32_t p = 0; p < np; p++) for (uint32_t ki = 0; ki < nk; ki++) {
        const uint32_t t = p * nk + ki, r = refs[a + p], q = qrys[a + p];
        tasks[t] = Task{r, q, ki, ix.ks[ki]};
        slot_off[t + 1] = slot_off[t] + (seq_off[r + 1] - seq_off[r]);
        fen_off[t + 1] = fen_off[t] + (seq_off[q + 1] - seq_off[q]) + 2;
    }
    const uint64_t n_slots = slot_off[nt];
    DevBuf<Task> d_tasks; DevBuf<uint64_t> d_slot, d_fen_off, d_mo, d_tm; DevBuf<uint32_t> d_cnt; DevBuf<uint8_t> d_tmp;
    d_tasks.alloc(nt); d_slot.alloc(nt + 1); d_fen_off.alloc(nt + 1); d_cnt.alloc(n_slots + 1); d_mo.alloc(n_slots + 1); d_tm.alloc(nt + 1);
    d_tasks.upload(tasks.data(), nt, s); d_slot.upload(slot_off.data(), nt + 1, s); d_fen_off.upload(fen_off.data(), nt + 1, s);
    st.bytes_h2d += 16ull * nt + 16ull * (nt + 1);
    d_cnt.zero(s);
    hipLaunchKernelGGL(align_join_kernel<false>, dim3(nt), dim3(256), 0, s, d_tasks.p, d_slot.p, ix.haps.seqs.p, ix.haps.off.p, ix.total, ix.keys_in.p, ix.keys_sorted.p,
                       ix.vals_sorted.p, d_cnt.p, static_cast<const uint64_t*>(nullptr), static_cast<uint2*>(nullptr));
    LCTY_HIP(hipGetLastError());
    // 32-bit counts, 64-bit offsets: rocPRIM accumulates in the type of the operator applied to the initial value, uint64_t here
    size_t bytes = 0;
    LCTY_HIP(rocprim::exclusive_scan(nullptr, bytes, d_cnt.p, d_mo.p, uint64_t(0), n_slots + 1, rocprim::plus<uint64_t>(), s));
    d_tmp.alloc(bytes + 16);
    LCTY_HIP(rocprim::exclusive_scan(d_tmp.p, bytes, d_cnt.p, d_mo.p, uint64_t(0), n_slots + 1, rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL(align_task_offsets_kernel, dim3((nt + 256) / 256), dim3(256), 0, s, d_slot.p, d_mo.p, nt, d_tm.p);
    LCTY_HIP(hipGetLastError());
    std::vector<uint64_t> tm(nt + 1);
    d_tm.download(tm.data(), nt + 1, s);
    LCTY_HIP(hipStreamSynchronize(s));
    st.bytes_d2h += 8ull * (nt + 1);
    const uint64_t n_m = tm[nt];
    for (uint32_t t = 0; t < nt; t++)
        if (tm[t + 1] - tm[t] > kMaxMatches)
            fail(LCTY_ERR_UNSUPPORTED, "sequences %u and %u share %llu %u-mer matches: more than %llu per pair and k", tasks[t].ref, tasks[t].qry,
                 static_cast<unsigned long long>(tm[t + 1] - tm[t]), tasks[t].k, static_cast<unsigned long long>(kMaxMatches));
    if (np > 1 && n_m * 20 > budget) {
        uint64_t fit = 1;
        while (fit < np && tm[(fit + 1) * nk] * 20 <= budget) fit++;
        st.match_ms += now_ms() - t0;
        return fit;
    }
    DevBuf<uint2> d_m; DevBuf<uint32_t> d_dp, d_prev, d_path, d_chain, d_pstart, d_drop; DevBuf<int32_t> d_score; DevBuf<uint64_t> d_fen; DevBuf<unsigned long long> d_stats;
    d_m.alloc(n_m + 1); d_dp.alloc(n_m + 1); d_prev.alloc(n_m + 1); d_path.alloc(n_m + 1); d_chain.alloc(nt); d_pstart.alloc(nt); d_fen.alloc(fen_off[nt]);
    d_score.alloc(nt); d_drop.alloc(nt);
    d_stats.alloc(ST_COUNT); d_stats.zero(s); d_fen.zero(s);
    hipLaunchKernelGGL(align_join_kernel<true>, dim3(nt), dim3(256), 0, s, d_tasks.p, d_slot.p, ix.haps.seqs.p, ix.haps.off.p, ix.total, ix.keys_in.p, ix.keys_sorted.p,
                       ix.vals_sorted.p, static_cast<uint32_t*>(nullptr), d_mo.p, d_m.p);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));
    d_cnt.release(); d_mo.release(); d_tmp.release();
    st.n_kmer_matches += n_m;
    st.match_ms += now_ms() - t0; t0 = now_ms();

    hipLaunchKernelGGL(align_chain_kernel, dim3((nt + 63) / 64), dim3(64), 0, s, d_tasks.p, nt, ix.haps.off.p, d_tm.p, d_m.p, d_dp.p, d_prev.p, d_path.p, d_fen_off.p,
                       d_fen.p, d_chain.p, d_pstart.p, d_stats.p);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));
    d_fen.release(); d_dp.release(); d_prev.release();
    st.chain_ms += now_ms() - t0; t0 = now_ms();

    StageC ws;                                                                // fresh per batch: exact sizes
    const BackboneSrc src{d_tasks.p, d_tm.p, d_m.p, d_path.p, d_pstart.p, ix.haps.off.p, pr.max_gap, d_score.p, d_drop.p};
    const std::array<uint64_t, kLevels> n_level = stage_c(ctx, src, nt, ix.haps.seqs.p, pr, ws, d_stats.p, st, st.fill_ms, st.fill_ms);
    for (uint32_t l = 0; l < kLevels; l++) st.n_level[l] += n_level[l];
    t0 = now_ms();

    DevBuf<PairRes> d_res; DevBuf<uint64_t> d_out_off; DevBuf<uint32_t> d_out;
    d_res.alloc(np);
    hipLaunchKernelGGL(align_select_kernel, dim3((np + 63) / 64), dim3(64), 0, s, np, nk, d_score.p, ws.words.p, ws.off.p, ws.cig.p, d_res.p);
    LCTY_HIP(hipGetLastError());
    std::vector<PairRes> res(np);
    std::vector<unsigned long long> hs(ST_COUNT);
    d_res.download(res.data(), np, s); d_stats.download(hs.data(), ST_COUNT, s);
    LCTY_HIP(hipStreamSynchronize(s));
    if (hs[ST_OVERFLOW]) fail(LCTY_ERR_RUNTIME, "a CIGAR outgrew its bound (%llu tasks)", hs[ST_OVERFLOW]);
    std::vector<uint64_t> out_off(np + 1, 0);
    for (uint32_t p = 0; p < np; p++) out_off[p + 1] = out_off[p] + res[p].n_words;
    // with a store the winners stay on the device: gathered behind what the store holds, downloaded once when the call ends
    if (store) store->reserve(out_off[np]);
    std::vector<uint64_t> dst_off(out_off);
    if (store) for (uint32_t p = 0; p <= np; p++) dst_off[p] += store->used;
    d_out_off.alloc(np + 1);
    if (!store) d_out.alloc(out_off[np] + 1);
    d_out_off.upload(dst_off.data(), np + 1, s);
    hipLaunchKernelGGL(align_gather_kernel, dim3(np), dim3(64), 0, s, nk, d_res.p, ws.off.p, ws.cig.p, d_out_off.p, store ? store->buf.p : d_out.p);
    LCTY_HIP(hipGetLastError());
    std::vector<uint32_t> words(store ? 1 : out_off[np] + 1);
    if (!store) d_out.download(words.data(), out_off[np], s);
    LCTY_HIP(hipStreamSynchronize(s));
    if (store) {
        for (uint32_t p = 0; p < np; p++) { store->off[pair_ix[a + p]] = dst_off[p]; store->len[pair_ix[a + p]] = res[p].n_words; }
        store->used += out_off[np];
    }
    st.bytes_h2d += 8ull * (np + 1); st.bytes_d2h += sizeof(PairRes) * np + (store ? 0 : 4ull * out_off[np]) + 8ull * ST_COUNT;
    for (uint32_t p = 0; p < np; p++) {
        out[a + p].score = res[p].score; out[a + p].best_ki = res[p].best_ki; out[a + p].n_matches = res[p].n_matches; out[a + p].nerrs = res[p].nerrs;
        if (!store) out[a + p].cigar.assign(words.begin() + out_off[p], words.begin() + out_off[p + 1]);
    }
    st.n_trivial += hs[ST_TRIVIAL]; st.n_simple += hs[ST_SIMPLE]; st.n_small_dp += hs[ST_SMALL]; st.n_general_dp += hs[ST_GENERAL];
    st.n_dropped += hs[ST_DROPPED]; st.dp_cells += hs[ST_CELLS]; st.n_chain_points += hs[ST_POINTS];
    if (cap) {                                                                // one pair, one k
        cap->matches.resize(n_m); cap->path.resize(n_m);
        uint32_t ps = 0;
        if (n_m) { LCTY_HIP(hipMemcpyAsync(cap->matches.data(), d_m.p, 8 * n_m, hipMemcpyDeviceToHost, s)); d_path.download(cap->path.data(), n_m, s); }
        d_chain.download(&cap->chain, 1, s); d_pstart.download(&ps, 1, s); d_drop.download(&cap->dropped, 1, s);
        LCTY_HIP(hipStreamSynchronize(s));
        cap->path.erase(cap->path.begin(), cap->path.begin() + ps);
        cap->cigar = out[a].cigar; cap->score = out[a].score;
    }
    st.select_ms += now_ms() - t0;
    st.n_batches++;
    return 0;
}

Prepared validate(lcty_ctx* ctx, const lcty_align_params* p) {                // Params::validate, align.rs:67-89
    if (!(p->div_k >= 1 && p->div_k <= 31)) fail(LCTY_ERR_INVALID_INPUT, "k-mer size (%u) must be between 1 and 31", p->div_k);
    if (!(p->div_w >= 1 && p->div_w <= 63)) fail(LCTY_ERR_INVALID_INPUT, "Minimizer window (%u) must be between 1 and 63", p->div_w);
    if (!(p->thresh_div >= 0.0 && p->thresh_div <= 1.0)) fail(LCTY_ERR_INVALID_INPUT, "Maximum divergence (%g) must be within [0, 1]", p->thresh_div);
    if (p->mismatch != PEN_X || p->gap_open != PEN_O || p->gap_extend != PEN_E)
        fail(LCTY_ERR_UNSUPPORTED, "penalties %d/%d/%d: the aligner is built for %d/%d/%d", p->mismatch, p->gap_open, p->gap_extend, PEN_X, PEN_O, PEN_E);
    Prepared r;
    r.never = p->thresh_div == 0.0;
    if (!r.never) {
        if (p->n_backbone_ks < 1 || p->n_backbone_ks > 8) fail(LCTY_ERR_INVALID_INPUT, "Expect at least one backbone k-mer (and at most 8)");
        for (uint32_t i = 0; i < p->n_backbone_ks; i++) {
            if (p->backbone_ks[i] < 5 || p->backbone_ks[i] > LCTY_ALIGN_MAX_K) fail(LCTY_ERR_INVALID_INPUT, "Backbone k-mer sizes must be between 5 and %u (%u)", LCTY_ALIGN_MAX_K, p->backbone_ks[i]);
            r.ks.push_back(p->backbone_ks[i]);
        }
    }
    r.max_gap = p->max_gap;
    const int64_t cells = ctx->knob("align_dp_cells", kLevelCells[kLevels - 1]);
    r.top = Lim{kLevelDim[kLevels - 1], static_cast<uint32_t>(std::min<int64_t>(std::max<int64_t>(cells, 1), kLevelCells[kLevels - 1]))};
    for (uint32_t l = 0; l < kLevels; l++) r.lv.l[l] = Lim{std::min(kLevelDim[l], r.top.dim), std::min(kLevelCells[l], r.top.cells)};
    return r;
}

constexpr HapLimits kAlignHaps{2, UINT32_MAX, 1ull << 28};                    // a CIGAR word holds a run of fewer than 2^28 bases

std::string fmt_f(double v, int prec) {                                      // Rust's {:.N} of an f64
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char b[64];
    snprintf(b, sizeof(b), "%.*f", prec, v);
    return b;
}

// what lcty_align_haplotypes decides before it aligns: the input checks, the divergences (process_pair 642-648) and which pairs are taken
struct Selection {
    HapSet hs; Prepared pr;
    std::vector<uint32_t> um; std::vector<double> md; std::vector<uint8_t> aligned;
    std::vector<uint32_t> refs, qrys; std::vector<uint64_t> which;            // the taken pairs, in input order; which = their input index
};
void select_pairs(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref_id, const uint32_t* query_id,
                  const uint8_t* against, const lcty_align_params* params, lcty_align_stats& st, Selection& sel) {
    sel.hs = check_haps(n_seqs, seqs, seq_off, kAlignHaps);
    sel.pr = validate(ctx, params);
    const Prepared& pr = sel.pr;
    std::vector<std::pair<uint64_t, uint64_t>> seen(n_pairs);              // (smaller id << 32 | larger id, index)
    for (uint64_t x = 0; x < n_pairs; x++) {
        const uint32_t r = ref_id[x], q = query_id[x];
        if (r >= n_seqs || q >= n_seqs) fail(LCTY_ERR_INVALID_INPUT, "pair %llu names sequence %u of %u", static_cast<unsigned long long>(x), std::max(r, q), n_seqs);
        if (r == q) fail(LCTY_ERR_INVALID_INPUT, "pair %llu aligns sequence %u to itself", static_cast<unsigned long long>(x), r);
        seen[x] = {(static_cast<uint64_t>(std::min(r, q)) << 32) | std::max(r, q), x};
    }
    std::sort(seen.begin(), seen.end());
    for (uint64_t x = 1; x < n_pairs; x++)
        if (seen[x].first == seen[x - 1].first)
            fail(LCTY_ERR_INVALID_INPUT, "pair %llu (%u, %u) is given twice", static_cast<unsigned long long>(seen[x].second), ref_id[seen[x].second], query_id[seen[x].second]);
    seen = {};
    ctx->activate();
    // divergences (process_pair 642-648): the triangle of lcty_db_divergences, rows i, then j > i
    sel.um.assign(n_pairs, 0); sel.md.assign(n_pairs, 0.0); sel.aligned.assign(n_pairs, 0);
    double t0 = now_ms();
    if (!params->skip_div) {
        const uint64_t ntri = static_cast<uint64_t>(n_seqs) * (n_seqs - 1) / 2;
        std::vector<uint32_t> uniq(ntri); std::vector<double> dv(ntri);
        lcty_db_stats ds{};
        const int32_t rc = lcty_db_divergences(ctx, n_seqs, seqs, seq_off, params->div_k, params->div_w, uniq.data(), dv.data(), nullptr, &ds);
        if (rc != LCTY_OK) fail(rc, "%s", lcty_last_error());
        st.bytes_h2d += ds.bytes_h2d; st.bytes_d2h += ds.bytes_d2h;
        for (uint64_t x = 0; x < n_pairs; x++) {
            const uint64_t i = std::min(ref_id[x], query_id[x]), j = std::max(ref_id[x], query_id[x]);
            const uint64_t at = i * n_seqs - i * (i + 1) / 2 + (j - i - 1);
            sel.um[x] = uniq[at]; sel.md[x] = dv[at];
        }
    }
    st.div_ms = now_ms() - t0;
    for (uint64_t x = 0; x < n_pairs; x++) {
        const double lim = against && (against[ref_id[x]] || against[query_id[x]]) ? params->against_div : (pr.never ? -1.0 : params->thresh_div);
        const bool take = params->skip_div || sel.md[x] <= lim;
        // thresh_div == 0 has cleared the ks (Params::validate): a pair that passes all the same — skip_div, or an `against` pair under
        // against_div — ends align_multik without an alignment (align.rs:316)
        if (take && pr.ks.empty()) fail(LCTY_ERR_RUNTIME, "No alignment found between sequences %u and %u", ref_id[x], query_id[x]);
        if (take) { sel.refs.push_back(ref_id[x]); sel.qrys.push_back(query_id[x]); sel.which.push_back(x); sel.aligned[x] = 1; }
    }
}

struct Batching { uint64_t budget, per_batch; };
Batching batching(lcty_ctx* ctx, const HapSet& hs, const Prepared& pr) {
    size_t free_b = 0, total_b = 0;
    LCTY_HIP(hipMemGetInfo(&free_b, &total_b));
    // bytes for the matches of a batch (20 a match); knob align_match_budget: a test reaches the "do not fit" return of run_batch
    const uint64_t budget = static_cast<uint64_t>(ctx->knob("align_match_budget", static_cast<int64_t>(std::max<uint64_t>(free_b / 4, 64ull << 20))));
    // a pair: per k 12 bytes a reference window (counts, offsets), 8 a query column (tree), and about 20 a match
    uint64_t per_batch = std::max<uint64_t>(budget / (pr.ks.size() * (hs.max_len + 2) * 40 + 1), 1);
    const int64_t knob = ctx->knob("align_batch_pairs", 0);
    if (knob > 0) per_batch = static_cast<uint64_t>(knob);
    per_batch = std::min<uint64_t>(per_batch, (1u << 30) / pr.ks.size());
    return Batching{budget, per_batch};
}

// po[y]: the result of taken pair y; words_of(y): its CIGAR, as (first word, number of words)
template <class W>
void write_out(Handoff& h, lcty_align_out& o, uint64_t n_pairs, const Selection& sel, const std::vector<PairOut>& po, W words_of) {
    std::vector<uint64_t> coff(n_pairs + 1, 0);
    for (uint64_t y = 0; y < sel.which.size(); y++) coff[sel.which[y] + 1] = words_of(y).second;
    for (uint64_t x = 0; x < n_pairs; x++) coff[x + 1] += coff[x];
    std::vector<uint32_t> words(coff[n_pairs]);
    for (uint64_t y = 0; y < sel.which.size(); y++) { const auto w = words_of(y); std::copy(w.first, w.first + w.second, words.begin() + coff[sel.which[y]]); }
    std::vector<uint32_t> nm(n_pairs, 0), al(n_pairs, 0), ne(n_pairs, 0), bk(n_pairs, 0); std::vector<int32_t> sc(n_pairs, 0);
    for (uint64_t y = 0; y < sel.which.size(); y++) {
        const uint64_t x = sel.which[y];
        nm[x] = po[y].n_matches; ne[x] = po[y].nerrs; al[x] = po[y].n_matches + po[y].nerrs; sc[x] = po[y].score;
        bk[x] = po[y].best_ki == kNoK ? 0 : sel.pr.ks[po[y].best_ki];
    }
    o.n_pairs = n_pairs;
    o.aligned = h.copy(sel.aligned); o.n_matches = h.copy(nm); o.aln_len = h.copy(al); o.nerrs = h.copy(ne); o.score = h.copy(sc); o.best_k = h.copy(bk);
    o.um = h.copy(sel.um); o.md = h.copy(sel.md); o.cigar_off = h.copy(coff); o.cigar = h.copy(words);
}

// the pairs [0, n) of refs / qrys in batches of bt.per_batch; a batch whose matches do not fit comes back as its prefix that does
void run_batches(lcty_ctx* ctx, const Index& ix, const uint64_t* seq_off, const uint32_t* refs, const uint32_t* qrys, uint64_t n, const Prepared& pr, const Batching& bt,
                 PairOut* out, lcty_align_stats& st, Store* store = nullptr, const uint64_t* pair_ix = nullptr) {
    for (uint64_t at = 0; at < n;) {
        uint64_t m = std::min<uint64_t>(bt.per_batch, n - at);
        for (uint64_t fit; (fit = run_batch(ctx, ix, seq_off, refs, qrys, at, at + m, pr, bt.budget, out, st, nullptr, store, pair_ix)) != 0;) m = fit;
        at += m;
    }
}
}  // namespace

// the device side of lcty_align_haplotypes_transitive (lcty_align_transitive.hip decides the rounds; lcty_align_internal.hpp)
namespace lcty {
namespace align {
struct Session::Impl {
    lcty_ctx* ctx; uint32_t n_seqs; const uint8_t* seqs; const uint64_t* seq_off; uint64_t n_pairs; const uint32_t* ref_id; const uint32_t* query_id;
    Selection sel; Index ix; Batching bt{0, 1}; Store store; std::vector<PairOut> res;      // res: per INPUT pair
    // grow-only workspaces of the transitive rounds: a call has a round per row of the triangle, and nothing is allocated per round
    // once the widest row has been seen
    StageC ws[2];                                                              // of the walk and of optimize; one scratch serves both
    DevBuf<uint8_t> d_short; DevBuf<TrTaskDev> d_tasks; DevBuf<uint64_t> d_dst; DevBuf<PairRes> d_res; DevBuf<unsigned long long> d_stats;
    lcty_align_stats st{}; lcty_align_tr_stats tr{};
    double t_all = 0;
};

Session::Session(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref_id, const uint32_t* query_id,
                 const uint8_t* against, const lcty_align_params* params) : im(new Impl) {
    try {
        im->ctx = ctx; im->n_seqs = n_seqs; im->seqs = seqs; im->seq_off = seq_off; im->n_pairs = n_pairs; im->ref_id = ref_id; im->query_id = query_id;
        im->t_all = now_ms();
        select_pairs(ctx, n_seqs, seqs, seq_off, n_pairs, ref_id, query_id, against, params, im->st, im->sel);
        im->res.assign(n_pairs, PairOut{0, kNoK, 0, 0, {}});
        im->ws[0].slack = im->ws[1].slack = true;
        im->store.off.assign(n_pairs, 0); im->store.len.assign(n_pairs, 0);
    } catch (...) { delete im; throw; }
}
Session::~Session() { delete im; }
const uint8_t* Session::aligned() const { return im->sel.aligned.data(); }
uint32_t Session::nerrs(uint64_t pair) const { return im->res[pair].nerrs; }
uint32_t Session::aln_len(uint64_t pair) const { return im->res[pair].n_matches + im->res[pair].nerrs; }

void Session::open(uint64_t store_words) {
    if (im->sel.which.empty()) return;
    build_index(im->ctx, im->sel.hs, im->seqs, im->seq_off, im->sel.pr.ks, im->ix, im->st);
    im->bt = batching(im->ctx, im->sel.hs, im->sel.pr);
    im->store.buf.alloc(store_words);
}

void Session::backbone(const uint64_t* pairs, uint64_t n) {
    if (!n) return;
    std::vector<uint32_t> refs(n), qrys(n);
    for (uint64_t y = 0; y < n; y++) { refs[y] = im->ref_id[pairs[y]]; qrys[y] = im->query_id[pairs[y]]; }
    std::vector<PairOut> po(n);
    run_batches(im->ctx, im->ix, im->seq_off, refs.data(), qrys.data(), n, im->sel.pr, im->bt, po.data(), im->st, &im->store, pairs);
    for (uint64_t y = 0; y < n; y++) im->res[pairs[y]] = po[y];
}

void Session::transitive(const TrTask* tasks, uint64_t n, uint32_t anchor_size) {
    if (!n) return;
    if (n > 0x7FFFFFFFull) fail(LCTY_ERR_UNSUPPORTED, "%llu transitive tasks in one round", static_cast<unsigned long long>(n));
    lcty_ctx* ctx = im->ctx;
    hipStream_t s = ctx->stream;
    const Prepared& pr = im->sel.pr;
    Store& store = im->store;
    const uint32_t nt = static_cast<uint32_t>(n);
    std::vector<TrTaskDev> h(nt);
    for (uint32_t t = 0; t < nt; t++) {
        const TrTask& k = tasks[t];
        h[t] = TrTaskDev{store.off[k.ij], store.off[k.jk], store.len[k.ij], store.len[k.jk], im->ref_id[k.pair], im->query_id[k.pair],
                         (k.inv_ij ? 1u : 0u) | (k.inv_jk ? 2u : 0u), 0};
    }
    DevBuf<TrTaskDev>& d_tasks = im->d_tasks; DevBuf<uint8_t>& d_short = im->d_short; DevBuf<unsigned long long>& d_stats = im->d_stats;
    StageC& walk = im->ws[0]; StageC& opt = im->ws[1];
    d_tasks.ensure_slack(nt); d_short.ensure_slack(nt); d_stats.ensure(ST_COUNT);
    d_tasks.upload(h.data(), nt, s); d_stats.zero(s);
    LCTY_HIP(hipStreamSynchronize(s));
    im->st.bytes_h2d += sizeof(TrTaskDev) * nt;
    // two passes of stage C (the upload is not planning). The CIGARs of a pass are per-round temporaries sized by the bounds, beside the
    // store (not part of its budget); optimize reads what the walk left.
    stage_c(ctx, TrSrc<0>{d_tasks.p, im->ix.haps.off.p, store.buf.p, anchor_size, pr.max_gap, nullptr, nullptr, nullptr, d_short.p}, nt, im->ix.haps.seqs.p, pr, walk, d_stats.p,
            im->st, im->tr.plan_ms, im->tr.tr_fill_ms);
    std::swap(walk.scratch, opt.scratch);                                     // the lanes' scratch goes along and comes back
    stage_c(ctx, TrSrc<1>{d_tasks.p, im->ix.haps.off.p, store.buf.p, anchor_size, pr.max_gap, walk.off.p, walk.cig.p, walk.words.p, d_short.p}, nt, im->ix.haps.seqs.p, pr, opt, d_stats.p,
            im->st, im->tr.plan_ms, im->tr.optimize_ms);
    std::swap(walk.scratch, opt.scratch);
    const double t0 = now_ms();
    DevBuf<PairRes>& d_res = im->d_res; DevBuf<uint64_t>& d_dst = im->d_dst;
    d_res.ensure_slack(nt); d_dst.ensure_slack(nt);
    hipLaunchKernelGGL(tr_count_kernel, dim3((nt + 63) / 64), dim3(64), 0, s, nt, opt.off.p, opt.cig.p, opt.words.p, d_res.p);
    LCTY_HIP(hipGetLastError());
    std::vector<PairRes> res(nt); std::vector<unsigned long long> hs(ST_COUNT); std::vector<uint8_t> shortcut(nt);
    d_res.download(res.data(), nt, s); d_stats.download(hs.data(), ST_COUNT, s); d_short.download(shortcut.data(), nt, s);
    LCTY_HIP(hipStreamSynchronize(s));
    im->st.bytes_d2h += (sizeof(PairRes) + 1) * nt + 8ull * ST_COUNT;
    if (hs[ST_OVERFLOW]) fail(LCTY_ERR_RUNTIME, "a transitive CIGAR outgrew its bound (%llu tasks)", hs[ST_OVERFLOW]);
    std::vector<uint64_t> dst(nt);
    uint64_t total = 0;
    for (uint32_t t = 0; t < nt; t++) { dst[t] = store.used + total; total += res[t].n_words; }
    store.reserve(total);
    d_dst.upload(dst.data(), nt, s);
    hipLaunchKernelGGL(align_gather_kernel, dim3(nt), dim3(64), 0, s, 1u, d_res.p, opt.off.p, opt.cig.p, d_dst.p, store.buf.p);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));
    im->st.bytes_h2d += 8ull * nt;
    store.used += total;
    for (uint32_t t = 0; t < nt; t++) {
        const uint64_t x = tasks[t].pair;
        store.off[x] = dst[t]; store.len[x] = res[t].n_words;
        im->res[x] = PairOut{res[t].score, kNoK, res[t].n_matches, res[t].nerrs, {}};
        im->tr.n_shortcut += shortcut[t];
    }
    im->tr.n_accelerated += nt;
    im->tr.n_tr_stretches += hs[ST_TRIVIAL] + hs[ST_SIMPLE] + hs[ST_SMALL] + hs[ST_GENERAL];
    im->tr.tr_dp_cells += hs[ST_CELLS];
    im->st.n_dropped += hs[ST_DROPPED];
    im->tr.count_ms += now_ms() - t0;
}

void Session::finish(uint64_t n_rounds, Handoff& h, lcty_align_out& out, lcty_align_stats* stats, lcty_align_tr_stats* tr_stats) {
    hipStream_t s = im->ctx->stream;
    Store& store = im->store;
    const uint64_t n_pairs = im->n_pairs;
    const double t0 = now_ms();
    std::vector<uint32_t> arena(store.used + 1);
    store.buf.download(arena.data(), store.used, s);                           // the one download of the CIGARs
    LCTY_HIP(hipStreamSynchronize(s));
    im->st.bytes_d2h += 4ull * store.used;
    const std::vector<uint64_t>& which = im->sel.which;
    std::vector<PairOut> po(which.size());
    for (uint64_t y = 0; y < which.size(); y++) po[y] = im->res[which[y]];
    write_out(h, out, n_pairs, im->sel, po, [&](uint64_t y) { return std::make_pair(arena.data() + store.off[which[y]], static_cast<size_t>(store.len[which[y]])); });
    im->st.select_ms += now_ms() - t0;
    im->st.n_aligned = im->sel.which.size(); im->st.n_skipped = n_pairs - im->sel.which.size();
    im->st.total_ms = now_ms() - im->t_all;
    im->tr.n_rounds = n_rounds; im->tr.store_bytes = 4ull * store.used;
    if (stats) *stats = im->st;
    if (tr_stats) *tr_stats = im->tr;
}
}  // namespace align
}  // namespace lcty

extern "C" {

void lcty_align_params_default(lcty_align_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->div_k = 15; p->div_w = 15; p->skip_div = 0; p->thresh_div = 1.0; p->against_div = 1.0;
    p->backbone_ks[0] = 25; p->backbone_ks[1] = 51; p->backbone_ks[2] = 101; p->n_backbone_ks = 3;
    p->max_gap = 10000; p->mismatch = PEN_X; p->gap_open = PEN_O; p->gap_extend = PEN_E;
}

int32_t lcty_align_all_pairs(uint32_t n_seqs, uint32_t* ref_id, uint32_t* query_id) {
    return guarded([&] {
        if (!ref_id || !query_id) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        uint64_t x = 0;
        for (uint32_t i = 0; i < n_seqs; i++) for (uint32_t j = i + 1; j < n_seqs; j++) { ref_id[x] = i; query_id[x] = j; x++; }
    });
}

void lcty_align_out_free(lcty_align_out* o) {
    if (!o) return;
    free(o->aligned); free(o->n_matches); free(o->aln_len); free(o->nerrs); free(o->score); free(o->best_k); free(o->um); free(o->md);
    free(o->cigar_off); free(o->cigar);
    memset(o, 0, sizeof(*o));
}

void lcty_align_backbone_out_free(lcty_align_backbone_out* o) {
    if (!o) return;
    free(o->matches); free(o->path); free(o->cigar);
    memset(o, 0, sizeof(*o));
}

int32_t lcty_align_haplotypes(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref_id,
                              const uint32_t* query_id, const uint8_t* against, const lcty_align_params* params, lcty_align_out* out, lcty_align_stats* stats) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !params || !out || (n_pairs && (!ref_id || !query_id))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_align_stats st{};
        const double t_all = now_ms();
        Selection sel;
        select_pairs(ctx, n_seqs, seqs, seq_off, n_pairs, ref_id, query_id, against, params, st, sel);
        const Prepared& pr = sel.pr;
        const std::vector<uint32_t>& refs = sel.refs; const std::vector<uint32_t>& qrys = sel.qrys; const std::vector<uint64_t>& which = sel.which;
        std::vector<PairOut> po(refs.size());
        if (!refs.empty()) {
            Index ix;
            build_index(ctx, sel.hs, seqs, seq_off, pr.ks, ix, st);
            run_batches(ctx, ix, seq_off, refs.data(), qrys.data(), refs.size(), pr, batching(ctx, sel.hs, pr), po.data(), st);
        }
        lcty_align_out o{}; Handoff h;
        write_out(h, o, n_pairs, sel, po, [&](uint64_t y) { return std::make_pair(po[y].cigar.data(), po[y].cigar.size()); });
        *out = o; h.commit();
        st.n_aligned = which.size(); st.n_skipped = n_pairs - which.size();
        st.total_ms = now_ms() - t_all;
        if (stats) *stats = st;
    });
}

int32_t lcty_align_backbone(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref, uint32_t query, uint32_t k,
                            const lcty_align_params* params, lcty_align_backbone_out* out, lcty_align_stats* stats) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !params || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_align_stats st{};
        const double t_all = now_ms();
        const HapSet hs = check_haps(n_seqs, seqs, seq_off, kAlignHaps);
        lcty_align_params one = *params;
        one.backbone_ks[0] = k; one.n_backbone_ks = 1;
        if (one.thresh_div == 0.0) one.thresh_div = 1.0;
        const Prepared pr = validate(ctx, &one);
        if (ref >= n_seqs || query >= n_seqs || ref == query) fail(LCTY_ERR_INVALID_INPUT, "pair (%u, %u) of %u sequences", ref, query, n_seqs);
        ctx->activate();
        Index ix;
        build_index(ctx, hs, seqs, seq_off, pr.ks, ix, st);
        PairOut po; Capture cap;
        run_batch(ctx, ix, seq_off, &ref, &query, 0, 1, pr, ~0ull, &po, st, &cap);
        lcty_align_backbone_out o{}; Handoff h;
        o.n_matches = cap.matches.size(); o.matches = reinterpret_cast<uint32_t*>(h.copy(cap.matches));
        o.chain_score = cap.chain;
        o.path_len = static_cast<uint32_t>(cap.path.size()); o.path = h.copy(cap.path);
        o.n_cigar = static_cast<uint32_t>(cap.cigar.size()); o.cigar = h.copy(cap.cigar);
        o.score = cap.score; o.n_dropped = cap.dropped;
        *out = o; h.commit();
        st.n_aligned = 1;
        st.total_ms = now_ms() - t_all;
        if (stats) *stats = st;
    });
}

int32_t lcty_paf_write_text(const lcty_align_params* params, uint32_t n_seqs, const char* names, const uint64_t* seq_off, uint64_t n_pairs,
                            const uint32_t* ref_id, const uint32_t* query_id, const lcty_align_out* res, char* out, uint64_t cap, uint64_t* needed) {
    return guarded([&] {
        if (!params || !names || !seq_off || !res || !needed || (n_pairs && (!ref_id || !query_id))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (res->n_pairs != n_pairs) fail(LCTY_ERR_INVALID_INPUT, "the result holds %llu pairs, not %llu", static_cast<unsigned long long>(res->n_pairs), static_cast<unsigned long long>(n_pairs));
        std::vector<const char*> nm(n_seqs);
        const char* c = names;
        for (uint32_t i = 0; i < n_seqs; i++) { nm[i] = c; c += strlen(c) + 1; }
        std::string t;
        // command/align.rs:385-387, after Params::validate (thresh_div 0 has become -1 and the ks are gone)
        const bool never = params->thresh_div == 0.0;
        std::string ks;
        for (uint32_t i = 0; !never && i < params->n_backbone_ks && i < 8; i++) ks += (i ? "," : "") + std::to_string(params->backbone_ks[i]);
        t += "# minimizers=" + std::to_string(params->div_k) + "," + std::to_string(params->div_w) + "; max_divergence=" + fmt_f(never ? -1.0 : params->thresh_div, 5) +
             "; backbone-ks=" + ks + "; accuracy=9; max-gap=" + std::to_string(params->max_gap) + "\n";
        static const char kOps[] = "MIDNSHP=X";
        for (uint64_t x = 0; x < n_pairs; x++) {
            const uint32_t r = ref_id[x], q = query_id[x];
            if (r >= n_seqs || q >= n_seqs) fail(LCTY_ERR_INVALID_INPUT, "pair %llu names sequence %u of %u", static_cast<unsigned long long>(x), std::max(r, q), n_seqs);
            const std::string lq = std::to_string(seq_off[q + 1] - seq_off[q]), lr = std::to_string(seq_off[r + 1] - seq_off[r]);
            t += std::string(nm[q]) + "\t" + lq + "\t0\t" + lq + "\t+\t" + nm[r] + "\t" + lr + "\t0\t" + lr + "\t";
            if (res->aligned[x]) {
                const double dv = static_cast<double>(res->nerrs[x]) / static_cast<double>(res->aln_len[x]);
                const double qv = std::isfinite(dv) ? -10.0 * std::log10(dv) : INFINITY;
                t += std::to_string(res->n_matches[x]) + "\t" + std::to_string(res->aln_len[x]) + "\t255\tNM:i:" + std::to_string(res->nerrs[x]) + "\tAS:i:" +
                     std::to_string(res->score[x]) + "\tdv:f:" + fmt_f(dv, 9) + "\tqv:f:" + fmt_f(qv, 6);
            } else t += "0\t0\t255";
            if (!params->skip_div) t += "\tum:i:" + std::to_string(res->um[x]) + "\tmd:f:" + fmt_f(res->md[x], 9);
            if (res->aligned[x]) {
                t += "\tcg:Z:";
                for (uint64_t w = res->cigar_off[x]; w < res->cigar_off[x + 1]; w++) {
                    const uint32_t op = res->cigar[w] & 15u;
                    if (op > 8) fail(LCTY_ERR_INVALID_INPUT, "pair %llu: operation code %u", static_cast<unsigned long long>(x), op);
                    t += std::to_string(res->cigar[w] >> 4) + kOps[op];
                }
            }
            t += "\n";
        }
        *needed = t.size();
        if (out) {
            if (cap < t.size()) fail(LCTY_ERR_INVALID_INPUT, "buffer of %llu bytes, %llu needed", static_cast<unsigned long long>(cap), static_cast<unsigned long long>(t.size()));
            memcpy(out, t.data(), t.size());
        }
    });
}

}  // extern "C"
