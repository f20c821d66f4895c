// lcty_pafvcf.hip — a locus's haplotypes as a VCF (`locityper paf-vcf`, src/command/paf_vcf.rs): the samples of the header
// (group_haplotypes, 569-621), the variants of every haplotype against the reference haplotype (process_paf 362-415, process_haplotype
// 276-332, move_all_left 242-271), the unique and the merged reference ranges (combine_variants 525-563), the allele of every haplotype
// in every range (get_hap_ranges 420-460, write_vcf 473-494) and the text of the records (495-517). The contract of every entry point
// is stated in the header and in DESIGN.md 5l. Positions are 0-based inside the reference haplotype. The scans (wave_scan_incl,
// launch_scan, ScanTotal: lcty_scan.hpp) and the sort of the ranges (RadixSort: lcty_sort.hpp) are the shared ones of DESIGN.md 4.18.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "lcty_common.hpp"
#include "lcty_device.hpp"
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"
#include "lcty_text.hpp"

namespace {

using namespace lcty;

constexpr int WG = 256;                                 // threads of every workgroup here; wave-per-item kernels take four items
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int32_t CELL_NONE = -1, CELL_PENDING = -2;    // allele_ix before the alleles are numbered: None, equal to the reference (0), to be numbered
constexpr uint32_t MAX_HAPS = 65535;

// words of the flag block: the first haplotype (or range) of every kind of failure, and two counters
enum { F_BADOP = 0, F_LYING = 1, F_RANGE = 2, F_SLICE = 3, F_BADID = 4, F_LONGLINE = 5, F_BADCELL = 6, F_BADLEN = 8, F_SHIFTED = 9, F_LINES = 10, F_MISSING = 11, F_COUNT = 12 };

struct Seqs { const uint8_t* seqs; const uint64_t* off; uint32_t n, ref_id; };
struct Paf { const uint32_t* id1; const uint32_t* id2; const uint64_t* cigar_off; const uint32_t* cigar; uint64_t n; };
struct Vars { const uint32_t* off; const uint32_t* rs; const uint32_t* re; const uint32_t* hs; const uint32_t* he; const uint8_t* has; };

// One CIGAR item (length << 4 | operation, BAM numbering) of an alignment of the haplotype (query) to the reference (target), or of the
// reference to the haplotype with the item inverted (Operation::invert, cigar.rs:147-158: I and S become D, D becomes I).
// kind: 0 '=', 1 an edit (X, I, D, S), 2 what process_haplotype refuses (M, H) or the reader never gives (N, P).
__device__ inline void item_diffs(uint32_t w, bool inv, uint32_t* rd, uint32_t* qd, uint32_t* kind) {
    const uint32_t op = w & 15u, len = w >> 4;
    *rd = 0; *qd = 0; *kind = 1;
    switch (op) {
    case 7: *rd = len; *qd = len; *kind = 0; break;
    case 8: *rd = len; *qd = len; break;
    case 1: case 4: if (inv) *rd = len; else *qd = len; break;
    case 2: if (inv) *qd = len; else *rd = len; break;
    case 0: *rd = len; *qd = len; *kind = 2; break;
    default: *kind = 2; break;
    }
}

// ---- device: variants -----------------------------------------------------------------------------------------------------------------

// process_paf's choice (382-408), one wavefront per entry: an entry with the reference on one side whose CIGAR covers both sequences is
// a candidate of its haplotype, the LAST candidate in file order stays (entry_of = index + 1, 0 = none); wrong lengths are counted.
__global__ __launch_bounds__(WG) void pafvcf_entry_kernel(Seqs S, Paf P, uint32_t* __restrict__ entry_of, uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t e = uint64_t(blockIdx.x) * (WG / WAVE) + threadIdx.x / WAVE;
    if (e >= P.n) return;
    const uint32_t q = P.id1[e], t = P.id2[e];
    if (q >= S.n || t >= S.n) { if (lane == 0) atomicMin(&flags[F_BADID], uint32_t(e)); return; }
    uint32_t hap; bool inv;
    if (q == S.ref_id) { hap = t; inv = true; } else if (t == S.ref_id) { hap = q; inv = false; } else return;
    const uint64_t c0 = P.cigar_off[e], c1 = P.cigar_off[e + 1];
    uint64_t rl = 0, ql = 0;
    for (uint64_t k = c0 + lane; k < c1; k += WAVE) {
        uint32_t rd, qd, kind;
        item_diffs(P.cigar[k], inv, &rd, &qd, &kind);
        rl += rd; ql += qd;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) { rl += __shfl_xor(rl, off); ql += __shfl_xor(ql, off); }
    if (lane) return;
    if (ql != S.off[hap + 1] - S.off[hap] || rl != S.off[S.ref_id + 1] - S.off[S.ref_id]) atomicAdd(&flags[F_BADLEN], 1u);
    else atomicMax(&entry_of[hap], uint32_t(e) + 1);
}

// process_haplotype (276-329) of one haplotype, one wavefront, 64 items a step. rpos / qpos are prefix sums; an edit item opens a
// variant iff an '=' of positive length lies between it and the edit before it (then `rpos <= last.ref_end` fails, 302), and the end of a
// variant is the end of its last edit. The right-padded form (315-316) keeps one base of slack, so a first variant of that form is walked
// item by item (every lane the same) up to the first edit it does not take, k1; the parallel rule holds from there.
// WRITE == false: the number of variants, has_aln, the missing haplotypes, and every '=' run compared base by base (F_LYING). WRITE == true: the variants, un-shifted.
template <bool WRITE>
__global__ __launch_bounds__(WG) void pafvcf_walk_kernel(Seqs S, Paf P, const uint32_t* __restrict__ entry_of, uint32_t* __restrict__ cnt,
                                                         const uint32_t* __restrict__ voff, uint32_t* __restrict__ rs, uint32_t* __restrict__ re,
                                                         uint32_t* __restrict__ hs, uint32_t* __restrict__ he, uint8_t* __restrict__ has,
                                                         uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t h = blockIdx.x * (WG / WAVE) + threadIdx.x / WAVE;
    if (h >= S.n) return;                                               // whole wavefronts leave; no workgroup barrier below
    const uint32_t e1 = entry_of[h];
    if (!WRITE && lane == 0) {                                          // process_paf 370-371, 410: the reference has an (empty) list, a haplotype without an entry is missing
        has[h] = h == S.ref_id || e1;
        if (h != S.ref_id && !e1) atomicAdd(&flags[F_MISSING], 1u);
    }
    if (h == S.ref_id || !e1) { if (!WRITE && lane == 0) cnt[h] = 0; return; }
    const uint64_t e = e1 - 1;
    const bool inv = P.id1[e] == S.ref_id;
    const uint32_t* cg = P.cigar + P.cigar_off[e];
    const uint64_t n = P.cigar_off[e + 1] - P.cigar_off[e];
    const uint8_t* ref = S.seqs + S.off[S.ref_id]; const uint8_t* hap = S.seqs + S.off[h];
    const uint32_t ref_len = uint32_t(S.off[S.ref_id + 1] - S.off[S.ref_id]), hap_len = uint32_t(S.off[h + 1] - S.off[h]);

    // the first variant, when it is right-padded
    uint32_t rp = 0, v0_rs = 0, v0_re = 0, v0_hs = 0, v0_he = 0;
    uint64_t k1 = 0;
    {
        uint64_t k = 0; uint32_t r = 0, q = 0, rd = 0, qd = 0, kind = 0;
        for (; k < n; k++) {
            item_diffs(cg[k], inv, &rd, &qd, &kind);
            if (kind) break;
            r += rd; q += qd;
        }
        if (k < n && kind == 1 && rd != qd && (r == 0 || q == 0)) {
            rp = 1; v0_rs = r; v0_re = r + rd + 1; v0_hs = q; v0_he = q + qd + 1;
            r += rd; q += qd;
            for (k1 = k + 1; k1 < n; k1++) {
                item_diffs(cg[k1], inv, &rd, &qd, &kind);
                if (kind == 1) {
                    if (!(r <= v0_re && q <= v0_he)) break;
                    v0_re = max(v0_re, r + rd); v0_he = max(v0_he, q + qd);
                }
                r += rd; q += qd;                                       // an M or H in this stretch is reported by the loop below
            }
        }
    }
    const uint32_t base_ix = WRITE ? voff[h] : 0;
    if (WRITE && rp && lane == 0) { rs[base_ix] = v0_rs; re[base_ix] = v0_re; hs[base_ix] = v0_hs; he[base_ix] = v0_he; }

    uint32_t carry_r = 0, carry_q = 0, carry_er = 0, carry_eq = 0, n_starts = 0;
    bool carry_edit = false, lying = false;
    for (uint64_t b = 0; b < n; b += WAVE) {
        const uint64_t k = b + lane;
        uint32_t rd = 0, qd = 0, kind = 0;
        if (k < n) item_diffs(cg[k], inv, &rd, &qd, &kind);
        if (kind == 2) atomicMin(&flags[F_BADOP], h);
        const uint32_t rpos = carry_r + wave_scan_incl(rd, AddOp{}) - rd, qpos = carry_q + wave_scan_incl(qd, AddOp{}) - qd;
        const bool edit = k < n && kind == 1;
        const uint32_t ir = wave_scan_incl(edit ? rpos + rd : 0u, MaxOp{}), iq = wave_scan_incl(edit ? qpos + qd : 0u, MaxOp{});
        uint32_t prev_er = __shfl_up(ir, 1), prev_eq = __shfl_up(iq, 1);
        if (lane == 0) { prev_er = 0; prev_eq = 0; }
        prev_er = max(prev_er, carry_er); prev_eq = max(prev_eq, carry_eq);
        const uint64_t edits = __ballot(edit);
        const bool prior = carry_edit || (edits & ((1ull << lane) - 1));
        const bool start = edit && k >= k1 && (!prior || rpos > prev_er);
        const uint64_t starts = __ballot(start);
        if (WRITE && start) {
            const uint32_t ix = rp + n_starts + __popcll(starts & ((1ull << lane) - 1));      // index inside the haplotype
            const uint32_t pad = rd == qd ? 0u : 1u;                                         // 313-319: left-padded unless a substitution
            rs[base_ix + ix] = rpos - pad; hs[base_ix + ix] = qpos - pad;
            if (ix >= 1 && !(rp && ix == 1)) { re[base_ix + ix - 1] = prev_er; he[base_ix + ix - 1] = prev_eq; }
        }
        if (!WRITE) {                                                   // every '=' run covers equal bases
            uint64_t eq = __ballot(k < n && kind == 0 && rd > 0);
            while (eq) {
                const int bit = __ffsll(static_cast<unsigned long long>(eq)) - 1;
                eq &= eq - 1;
                const uint32_t r0 = __shfl(rpos, bit), q0 = __shfl(qpos, bit), len = __shfl(rd, bit);
                for (uint32_t x = lane; x < len; x += WAVE)
                    if (uint64_t(r0) + x < ref_len && uint64_t(q0) + x < hap_len && ref[r0 + x] != hap[q0 + x]) lying = true;
            }
        }
        n_starts += __popcll(starts);
        carry_r = __shfl(rpos + rd, WAVE - 1); carry_q = __shfl(qpos + qd, WAVE - 1);
        carry_er = max(carry_er, __shfl(ir, WAVE - 1)); carry_eq = max(carry_eq, __shfl(iq, WAVE - 1));
        carry_edit = carry_edit || edits;
    }
    const uint32_t total = rp + n_starts;
    if (!WRITE) {
        if (__ballot(lying) && lane == 0) atomicMin(&flags[F_LYING], h);
        if (lane == 0) cnt[h] = total;
        return;
    }
    if (lane == 0 && total) {
        uint32_t last_re = v0_re, last_he = v0_he;
        if (!(rp && total == 1)) { last_re = carry_er; last_he = carry_eq; re[base_ix + total - 1] = last_re; he[base_ix + total - 1] = last_he; }
        if (last_re > ref_len || last_he > hap_len) atomicMin(&flags[F_RANGE], h);             // 325-329
    }
}

// the haplotype of variant v: voff[h] <= v < voff[h + 1]
__device__ inline uint32_t owner_of(const uint32_t* __restrict__ off, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid + 1] <= v) lo = mid + 1; else hi = mid; }
    return lo;
}

// move_all_left (242-271) with gap_move_left (231-239), one lane per variant: every variant depends on the UN-shifted end of the one
// before it alone, so all of them move at once.
__global__ __launch_bounds__(WG) void pafvcf_shift_kernel(Seqs S, uint32_t n_vars, const uint32_t* __restrict__ voff, const uint32_t* __restrict__ rs,
                                                          const uint32_t* __restrict__ re, const uint32_t* __restrict__ hs, const uint32_t* __restrict__ he,
                                                          uint32_t* __restrict__ o_rs, uint32_t* __restrict__ o_re, uint32_t* __restrict__ o_hs,
                                                          uint32_t* __restrict__ o_he, uint32_t* __restrict__ flags) {
    const uint32_t v = blockIdx.x * WG + threadIdx.x;
    uint32_t shift = 0;
    if (v < n_vars) {
        const uint32_t h = owner_of(voff, S.n, v);
        const uint8_t* ref = S.seqs + S.off[S.ref_id]; const uint8_t* hap = S.seqs + S.off[h];
        const uint32_t a = rs[v], b = re[v], c = hs[v], d = he[v];
        const uint32_t min_start = v == voff[h] ? 0u : re[v - 1];
        const uint32_t rl = b - a, al = d - c, prefix = rl < al ? rl : al;
        if (rl != al) {
            bool same = true;
            for (uint32_t x = 0; x < prefix && same; x++) same = ref[a + x] == hap[c + x];
            if (same) {
                const uint8_t* gap = prefix == rl ? hap + c + prefix : ref + a + prefix;
                const uint32_t last = (rl > al ? rl : al) - prefix - 1;
                uint32_t gs = a + prefix, k = last;
                const uint32_t stop = min_start + prefix;
                while (gs > stop && gap[k] == ref[gs - 1]) { gs--; k = k ? k - 1 : last; }
                shift = a + prefix - gs;
            }
        }
        o_rs[v] = a - shift; o_re[v] = b - shift; o_hs[v] = c - shift; o_he[v] = d - shift;
    }
    const uint64_t m = __ballot(shift != 0);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(&flags[F_SHIFTED], uint32_t(__popcll(m)));
}

// ---- device: ranges -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(WG) void pafvcf_keys_kernel(uint32_t n, const uint32_t* __restrict__ rs, const uint32_t* __restrict__ re, uint64_t* __restrict__ keys) {
    const uint32_t v = blockIdx.x * WG + threadIdx.x;
    if (v < n) keys[v] = uint64_t(rs[v]) << 32 | re[v];
}
__global__ __launch_bounds__(WG) void pafvcf_head_kernel(uint32_t n, const uint64_t* __restrict__ keys, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) head[i] = i == 0 || keys[i] != keys[i - 1];
}
__global__ __launch_bounds__(WG) void pafvcf_unique_kernel(uint32_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head,
                                                           const uint32_t* __restrict__ rank, uint32_t* __restrict__ start, uint32_t* __restrict__ end) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n && head[i]) { start[rank[i]] = uint32_t(keys[i] >> 32); end[rank[i]] = uint32_t(keys[i]); }
}
// combine_variants 544-555: a range opens a merged range iff no range before it ends behind its start (`last.1 <= start`; touching ranges stay apart)
__global__ __launch_bounds__(WG) void pafvcf_mhead_kernel(uint32_t n, const uint32_t* __restrict__ start, const uint32_t* __restrict__ end_max, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i < n) head[i] = i == 0 || end_max[i - 1] <= start[i];
}
__global__ __launch_bounds__(WG) void pafvcf_merged_kernel(uint32_t n, const uint32_t* __restrict__ start, const uint32_t* __restrict__ end_max,
                                                           const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank, uint32_t* __restrict__ m_start,
                                                           uint32_t* __restrict__ m_end) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = rank[i] + head[i] - 1;                           // the merged range of i
    if (head[i]) m_start[g] = start[i];
    if (i + 1 == n || head[i + 1]) m_end[g] = end_max[i];
}

// ---- device: table --------------------------------------------------------------------------------------------------------------------

// get_hap_ranges (420-460) of one range and one haplotype. 0: None; 1: [*hs, *he); 2: the subtraction of 446 / 452 would underflow.
__device__ inline int cell_range(const Vars& V, uint32_t ref_id, uint32_t h, uint32_t start, uint32_t end, uint32_t* hs, uint32_t* he) {
    if (!V.has[h]) return 0;
    const uint32_t v0 = V.off[h], n = V.off[h + 1] - v0;
    if (h == ref_id || n == 0) { *hs = start; *he = end; return 1; }
    uint32_t lo = 0, hi = n;                                            // i: the first variant with ref_end > start
    while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (V.re[v0 + mid] > start) hi = mid; else lo = mid + 1; }
    const uint32_t i = lo;
    hi = n;                                                             // j: the first at or behind i with ref_start >= end
    while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (V.rs[v0 + mid] < end) lo = mid + 1; else hi = mid; }
    const uint32_t j = lo, diff = end - start;
    if (i == n) {
        const uint32_t s = start - V.re[v0 + n - 1];
        *hs = V.he[v0 + n - 1] + s; *he = *hs + diff;
        return 1;
    }
    const uint32_t left = V.rs[v0 + i] - start;                          // wraps only where it is not used
    if (i == j) {
        if (V.hs[v0 + i] < left) return 2;
        *hs = V.hs[v0 + i] - left; *he = *hs + diff;
        return 1;
    }
    if (start <= V.rs[v0 + i] && V.re[v0 + j - 1] <= end) {
        if (V.hs[v0 + i] < left) return 2;
        *hs = V.hs[v0 + i] - left; *he = V.he[v0 + j - 1] + (end - V.re[v0 + j - 1]);
        return 1;
    }
    return 0;
}

__device__ inline bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n) {
    for (uint32_t x = 0; x < n; x++) if (a[x] != b[x]) return false;
    return true;
}

// One lane per (range, haplotype): None, the reference's own slice (allele 0), or another allele (pending, counted per range).
__global__ __launch_bounds__(WG) void pafvcf_cell_kernel(Seqs S, Vars V, uint32_t n_ranges, const uint32_t* __restrict__ r_start, const uint32_t* __restrict__ r_end,
                                                         int32_t* __restrict__ ix, uint32_t* __restrict__ n_pending, uint32_t* __restrict__ flags) {
    const uint32_t r = blockIdx.x, h = blockIdx.y * WG + threadIdx.x;
    int32_t cell = CELL_NONE;
    if (h < S.n) {
        const uint32_t start = r_start[r], end = r_end[r];
        uint32_t hs = 0, he = 0;
        const int rc = cell_range(V, S.ref_id, h, start, end, &hs, &he);
        const uint64_t hap_len = S.off[h + 1] - S.off[h];
        if (rc == 2 || (rc == 1 && (he < hs || he > hap_len))) atomicMin(&flags[F_SLICE], r);    // upstream panics (strict_sub, the slice)
        else if (rc == 1) {
            const uint8_t* a = S.seqs + S.off[h] + hs; const uint8_t* b = S.seqs + S.off[S.ref_id] + start;
            bool has_n = false;
            for (uint32_t x = 0; x < he - hs; x++) has_n |= a[x] == 'N';
            if (!has_n) cell = (he - hs == end - start && same_bytes(a, b, end - start)) ? 0 : CELL_PENDING;
        }
        ix[uint64_t(r) * S.n + h] = cell;
    }
    const uint64_t m = __ballot(cell == CELL_PENDING);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(&n_pending[r], uint32_t(__popcll(m)));
}

__device__ inline uint64_t hash_bytes(const uint8_t* p, uint32_t n, uint64_t mask) {
    uint64_t x = 0xCBF29CE484222325ull ^ n;
    for (uint32_t i = 0; i < n; i++) x = (x ^ p[i]) * 0x100000001B3ull;
    return mix64(x) & mask;
}

// The pending cells of one range in contig order, one wavefront per range: haplotype, slice and hash of the slice.
__global__ __launch_bounds__(WG) void pafvcf_list_kernel(Seqs S, Vars V, uint32_t n_ranges, const uint32_t* __restrict__ r_start, const uint32_t* __restrict__ r_end,
                                                         const int32_t* __restrict__ ix, const uint32_t* __restrict__ poff, uint64_t hash_mask,
                                                         uint32_t* __restrict__ l_hap, uint32_t* __restrict__ l_start, uint32_t* __restrict__ l_len,
                                                         uint64_t* __restrict__ l_hash) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t r = blockIdx.x * (WG / WAVE) + threadIdx.x / WAVE;
    if (r >= n_ranges) return;
    const uint32_t p0 = poff[r], p1 = poff[r + 1];
    if (p0 == p1) return;
    uint32_t at = p0;
    for (uint32_t h0 = 0; h0 < S.n; h0 += WAVE) {
        const uint32_t h = h0 + lane;
        const bool pend = h < S.n && ix[uint64_t(r) * S.n + h] == CELL_PENDING;
        const uint64_t m = __ballot(pend);
        if (pend) {
            const uint32_t slot = at + __popcll(m & ((1ull << lane) - 1));
            uint32_t hs = 0, he = 0;
            cell_range(V, S.ref_id, h, r_start[r], r_end[r], &hs, &he);
            if (slot < p1) { l_hap[slot] = h; l_start[slot] = hs; l_len[slot] = he - hs; l_hash[slot] = hash_bytes(S.seqs + S.off[h] + hs, he - hs, hash_mask); }
        }
        at += __popcll(m);
    }
}

// write_vcf 487-493, one lane per pending cell: the first earlier cell of the range with the same bytes carries the allele (the hash picks
// candidates, the bytes decide), else the cell itself. Carriers are counted per range.
__global__ __launch_bounds__(WG) void pafvcf_carrier_kernel(Seqs S, uint32_t n_ranges, uint32_t n_list, const uint32_t* __restrict__ poff,
                                                            const uint32_t* __restrict__ l_hap, const uint32_t* __restrict__ l_start,
                                                            const uint32_t* __restrict__ l_len, const uint64_t* __restrict__ l_hash,
                                                            uint32_t* __restrict__ l_car, uint32_t* __restrict__ n_car) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= n_list) return;
    const uint32_t r = owner_of(poff, n_ranges, e);
    const uint8_t* mine = S.seqs + S.off[l_hap[e]] + l_start[e];
    const uint32_t len = l_len[e]; const uint64_t hash = l_hash[e];
    uint32_t car = e;
    for (uint32_t f = poff[r]; f < e; f++)
        if (l_hash[f] == hash && l_len[f] == len && same_bytes(S.seqs + S.off[l_hap[f]] + l_start[f], mine, len)) { car = f; break; }
    l_car[e] = car;
    if (car == e) atomicAdd(&n_car[r], 1u);
}

// The alleles of one range numbered by their first carrier in contig order, one wavefront per range.
__global__ __launch_bounds__(WG) void pafvcf_number_kernel(uint32_t n_ranges, const uint32_t* __restrict__ poff, const uint32_t* __restrict__ aoff,
                                                           const uint32_t* __restrict__ l_hap, const uint32_t* __restrict__ l_start,
                                                           const uint32_t* __restrict__ l_len, const uint32_t* __restrict__ l_car, uint32_t* __restrict__ l_num,
                                                           uint32_t* __restrict__ a_hap, uint32_t* __restrict__ a_start, uint32_t* __restrict__ a_len,
                                                           uint32_t* __restrict__ n_alleles) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t r = blockIdx.x * (WG / WAVE) + threadIdx.x / WAVE;
    if (r >= n_ranges) return;
    const uint32_t p0 = poff[r], p1 = poff[r + 1], a0 = aoff[r], a1 = aoff[r + 1];
    if (lane == 0) n_alleles[r] = 1 + (a1 - a0);
    uint32_t seen = 0;
    for (uint32_t b = p0; b < p1; b += WAVE) {
        const uint32_t e = b + lane;
        const bool car = e < p1 && l_car[e] == e;
        const uint64_t m = __ballot(car);
        if (car) {
            const uint32_t k = seen + __popcll(m & ((1ull << lane) - 1));
            l_num[e] = k + 1;
            if (a0 + k < a1) { a_hap[a0 + k] = l_hap[e]; a_start[a0 + k] = l_start[e]; a_len[a0 + k] = l_len[e]; }
        }
        seen += __popcll(m);
    }
}

__global__ __launch_bounds__(WG) void pafvcf_assign_kernel(uint32_t n_seqs, uint32_t n_ranges, uint32_t n_list, const uint32_t* __restrict__ poff,
                                                           const uint32_t* __restrict__ l_hap, const uint32_t* __restrict__ l_car,
                                                           const uint32_t* __restrict__ l_num, int32_t* __restrict__ ix) {
    const uint32_t e = blockIdx.x * WG + threadIdx.x;
    if (e >= n_list) return;
    const uint32_t r = owner_of(poff, n_ranges, e);
    ix[uint64_t(r) * n_seqs + l_hap[e]] = int32_t(l_num[l_car[e]]);
}

// ---- device: text ---------------------------------------------------------------------------------------------------------------------

// digits, the workgroup's sum and the place of a thread's bytes: lcty_text.hpp
struct TextIn {
    const uint32_t* r_start; const uint32_t* r_end; const int32_t* ix; const uint32_t* n_alleles; const uint32_t* aoff;
    const uint32_t* a_hap; const uint32_t* a_start; const uint32_t* a_len;
    const uint32_t* slot_hap; const uint8_t* slot_first; uint32_t n_slots, n_seqs, chrom_len, shift;
};

__device__ inline uint32_t cell_width(const TextIn& T, uint32_t r, uint32_t s, int32_t* value) {
    const uint32_t hap = T.slot_hap[s];
    const int32_t v = hap == NONE ? CELL_NONE : T.ix[uint64_t(r) * T.n_seqs + hap];
    *value = v;
    return 1 + (v < 0 ? 1u : n_digits(uint64_t(v)));                    // the separator and "." or the allele number
}

#define PAFVCF_TAIL "\t60\t.\t.\tGT"
constexpr uint32_t TAIL_LEN = sizeof(PAFVCF_TAIL) - 1;

// the length of the line of one range (write_vcf 495-516), 0 for a range with one allele; one workgroup per range
__global__ __launch_bounds__(WG) void pafvcf_linelen_kernel(TextIn T, uint64_t* __restrict__ line_len, uint32_t* __restrict__ flags) {
    __shared__ uint64_t part[WG / WAVE];
    const uint32_t r = blockIdx.x;
    const uint32_t na = T.n_alleles[r];
    if (na <= 1) { if (threadIdx.x == 0) line_len[r] = 0; return; }     // the whole workgroup leaves
    uint64_t mine = 0;
    for (uint32_t a = threadIdx.x; a + 1 < na; a += WG) mine += 1 + uint64_t(T.a_len[T.aoff[r] + a]);
    for (uint32_t s = threadIdx.x; s < T.n_slots; s += WG) {
        int32_t v;
        mine += cell_width(T, r, s, &v);
        if (v >= int32_t(na)) atomicMin(&flags[F_BADCELL], r);           // a table that is not lcty_pafvcf_table's
    }
    const uint64_t sum = block_sum<WG>(mine, part);
    if (threadIdx.x == 0) {
        const uint64_t len = T.chrom_len + 1 + n_digits(uint64_t(T.r_start[r]) + T.shift + 1) + 2 + 1 + (T.r_end[r] - T.r_start[r]) + sum + TAIL_LEN + 1;
        line_len[r] = len;
        atomicAdd(&flags[F_LINES], 1u);
        if (len > 0xFFFFFFFFull) atomicMin(&flags[F_LONGLINE], r);
    }
}

// the line of one range at its offset; one workgroup per range. The alleles are copied one after the other by all threads, the cells take
// a scan of their widths per 256 slots.
__global__ __launch_bounds__(WG) void pafvcf_write_kernel(TextIn T, Seqs S, const char* __restrict__ chrom, const uint64_t* __restrict__ line_off, char* __restrict__ out) {
    __shared__ uint32_t wsum[WG / WAVE];
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const uint64_t o0 = line_off[r], o1 = line_off[r + 1];
    if (o0 == o1) return;                                               // the whole workgroup leaves
    char* line = out + o0;
    uint64_t at = 0;
    for (uint32_t x = tid; x < T.chrom_len; x += WG) line[x] = chrom[x];
    at += T.chrom_len;
    const uint64_t pos = uint64_t(T.r_start[r]) + T.shift + 1;
    const uint32_t pd = n_digits(pos);
    if (tid == 0) { line[at] = '\t'; put_digits(line + at + 1, pos, pd); line[at + 1 + pd] = '\t'; line[at + 2 + pd] = '.'; }
    at += 3 + pd;
    const uint32_t na = T.n_alleles[r];
    for (uint32_t a = 0; a < na; a++) {
        const uint8_t* src; uint32_t len;
        if (a == 0) { src = S.seqs + S.off[S.ref_id] + T.r_start[r]; len = T.r_end[r] - T.r_start[r]; }
        else { const uint32_t k = T.aoff[r] + a - 1; src = S.seqs + S.off[T.a_hap[k]] + T.a_start[k]; len = T.a_len[k]; }
        if (tid == 0) line[at] = a <= 1 ? '\t' : ',';
        for (uint32_t x = tid; x < len; x += WG) line[at + 1 + x] = char(src[x]);
        at += 1 + uint64_t(len);
    }
    if (tid < TAIL_LEN) line[at + tid] = PAFVCF_TAIL[tid];
    at += TAIL_LEN;
    for (uint32_t s0 = 0; s0 < T.n_slots; s0 += WG) {
        const uint32_t s = s0 + tid;
        int32_t v = CELL_NONE;
        const uint32_t w = s < T.n_slots ? cell_width(T, r, s, &v) : 0u;
        uint32_t all = 0;
        const uint32_t before = block_place<WG>(w, wsum, &all);
        if (s < T.n_slots) {
            char* c = line + at + before;
            c[0] = T.slot_first[s] ? '\t' : '|';
            if (v < 0) c[1] = '.'; else put_digits(c + 1, uint64_t(v), w - 1);
        }
        at += all;
    }
    if (tid == 0) line[at] = '\n';
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------

void sync(lcty_ctx* ctx) { LCTY_HIP(hipStreamSynchronize(ctx->stream)); }
#define LAUNCH(kernel, grid, ...) do { hipLaunchKernelGGL(kernel, dim3 grid, dim3(WG), 0, s, __VA_ARGS__); LCTY_HIP(hipGetLastError()); } while (0)

struct DSeqs {
    DevHaps d;
    uint32_t n = 0, ref_id = 0; uint64_t ref_len = 0;
    Seqs view() const { return Seqs{d.seqs.p, d.off.p, n, ref_id}; }
    // 32-bit positions inside a haplotype, haplotype numbers that fit a grid dimension
    void upload(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* h_seqs, const uint64_t* seq_off, uint32_t ref) {
        const HapSet hs = check_haps(n_seqs, h_seqs, seq_off, HapLimits{1, MAX_HAPS, 0x7FFFFFF0ull});
        if (ref >= n_seqs) fail(LCTY_ERR_INVALID_INPUT, "reference haplotype %u of %u", ref, n_seqs);
        n = n_seqs; ref_id = ref; ref_len = hs.len(ref);
        d.upload(ctx, hs, h_seqs, seq_off, 0);
    }
};

struct DVars {
    DevBuf<uint32_t> off, rs, re, hs, he; DevBuf<uint8_t> has;
    uint32_t n = 0, n_missing = 0, n_bad_len = 0, n_shifted = 0;
    Vars view() const { return Vars{off.p, rs.p, re.p, hs.p, he.p, has.p}; }
};
struct DRanges { DevBuf<uint32_t> u_start, u_end, m_start, m_end; uint32_t nu = 0, nm = 0; };
struct DTable {
    DevBuf<int32_t> ix; DevBuf<uint32_t> n_alleles, aoff, a_hap, a_start, a_len;
    uint32_t n_ranges = 0, n_all = 0;
};

void read_flags(lcty_ctx* ctx, const DevBuf<uint32_t>& d, uint32_t* flags) { d.download(flags, F_COUNT, ctx->stream); sync(ctx); }
void init_flags(lcty_ctx* ctx, DevBuf<uint32_t>& d) {
    const uint32_t init[F_COUNT] = {NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, 0, 0, 0, 0};
    d.alloc(F_COUNT); d.upload(init, F_COUNT, ctx->stream);
    sync(ctx);                                                           // `init` leaves the stack
}

// items 2-4: the entry of every haplotype, a count pass with the check of the '=' runs, a scan, a write pass, the left shift
void variants_dev(lcty_ctx* ctx, const DSeqs& S, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2, const uint64_t* cigar_off, const uint32_t* cigar,
                  DVars& V) {
    if (n_entries && (!id1 || !id2 || !cigar_off)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (n_entries >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%llu PAF entries", static_cast<unsigned long long>(n_entries));
    const uint64_t n_words = n_entries ? cigar_off[n_entries] : 0;
    if (n_words && !cigar) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    for (uint64_t e = 0; e < n_entries; e++) if (cigar_off[e + 1] < cigar_off[e]) fail(LCTY_ERR_INVALID_INPUT, "cigar_off decreases at entry %llu", static_cast<unsigned long long>(e));
    hipStream_t s = ctx->stream;
    const uint32_t H = S.n;
    DevBuf<uint32_t> d_id1, d_id2, d_cigar, d_entry, d_cnt, d_flags, u_rs, u_re, u_hs, u_he;
    DevBuf<uint64_t> d_coff;
    d_id1.alloc(std::max<uint64_t>(n_entries, 1)); d_id2.alloc(std::max<uint64_t>(n_entries, 1)); d_coff.alloc(n_entries + 1); d_cigar.alloc(std::max<uint64_t>(n_words, 1));
    d_id1.upload(id1, n_entries, s); d_id2.upload(id2, n_entries, s); d_cigar.upload(cigar, n_words, s);
    const uint64_t zero = 0;
    if (n_entries) d_coff.upload(cigar_off, n_entries + 1, s); else d_coff.upload(&zero, 1, s);
    d_entry.alloc(H); d_entry.zero(s); d_cnt.alloc(H);
    init_flags(ctx, d_flags);
    const Paf P{d_id1.p, d_id2.p, d_coff.p, d_cigar.p, n_entries};
    if (n_entries) LAUNCH(pafvcf_entry_kernel, (blocks_of(n_entries, WG / WAVE)), S.view(), P, d_entry.p, d_flags.p);
    uint32_t* const null32 = nullptr;
    V.has.alloc(H);
    LAUNCH(pafvcf_walk_kernel<false>, (blocks_of(H, WG / WAVE)), S.view(), P, d_entry.p, d_cnt.p, null32, null32, null32, null32, null32, V.has.p, d_flags.p);
    ScanTotal scan;
    V.n = scan.run(d_cnt, V.off, H, ctx);
    uint32_t flags[F_COUNT];
    read_flags(ctx, d_flags, flags);
    if (flags[F_BADID] != NONE) fail(LCTY_ERR_INVALID_INPUT, "PAF entry %u names a haplotype the locus does not have", flags[F_BADID]);
    if (flags[F_BADOP] != NONE) fail(LCTY_ERR_RUNTIME, "Unexpected operation (M/H) in the CIGAR of haplotype %u", flags[F_BADOP]);
    if (flags[F_LYING] != NONE)
        fail(LCTY_ERR_INVALID_DATA, "the CIGAR of haplotype %u has an '=' run over bases that differ from the reference haplotype", flags[F_LYING]);
    V.n_missing = flags[F_MISSING]; V.n_bad_len = flags[F_BADLEN];
    const size_t nv = std::max(V.n, 1u);
    u_rs.alloc(nv); u_re.alloc(nv); u_hs.alloc(nv); u_he.alloc(nv);
    V.rs.alloc(nv); V.re.alloc(nv); V.hs.alloc(nv); V.he.alloc(nv);
    LAUNCH(pafvcf_walk_kernel<true>, (blocks_of(H, WG / WAVE)), S.view(), P, d_entry.p, null32, V.off.p, u_rs.p, u_re.p, u_hs.p, u_he.p, static_cast<uint8_t*>(nullptr),
           d_flags.p);
    read_flags(ctx, d_flags, flags);
    if (flags[F_RANGE] != NONE) fail(LCTY_ERR_RUNTIME, "CIGAR operation out of range of the sequence (haplotype %u)", flags[F_RANGE]);
    if (V.n) {
        LAUNCH(pafvcf_shift_kernel, (blocks_of(V.n, WG)), S.view(), V.n, V.off.p, u_rs.p, u_re.p, u_hs.p, u_he.p, V.rs.p, V.re.p, V.hs.p, V.he.p, d_flags.p);
        read_flags(ctx, d_flags, flags);
    }
    V.n_shifted = flags[F_SHIFTED];
}

// item 5: keys start << 32 | end, a radix sort over the bytes a position of this reference can differ in, flag + scan + compaction for
// the unique ranges, a running maximum of the ends and a second compaction for the merged ones
void ranges_dev(lcty_ctx* ctx, uint32_t n_vars, const DevBuf<uint32_t>& rs, const DevBuf<uint32_t>& re, uint32_t max_pos, DRanges& R) {
    hipStream_t s = ctx->stream;
    R.nu = R.nm = 0;
    R.u_start.alloc(std::max(n_vars, 1u)); R.u_end.alloc(std::max(n_vars, 1u));
    if (!n_vars) { R.m_start.alloc(1); R.m_end.alloc(1); return; }
    DevBuf<uint64_t> ka, kb; DevBuf<uint32_t> head, rank, end_max;
    ka.alloc(n_vars); kb.alloc(n_vars);
    LAUNCH(pafvcf_keys_kernel, (blocks_of(n_vars, WG)), n_vars, rs.p, re.p, ka.p);
    std::vector<uint32_t> shifts;
    for (uint32_t half = 0; half < 2; half++)
        for (uint32_t b = 0; b < 4 && (b == 0 || (uint64_t(max_pos) >> (8 * b))); b++) shifts.push_back(32 * half + 8 * b);
    RadixSort sort;
    const uint64_t* a = sort.run(ka.p, nullptr, kb.p, nullptr, n_vars, shifts, s) ? kb.p : ka.p;
    ScanTotal scan;
    head.alloc(n_vars);
    LAUNCH(pafvcf_head_kernel, (blocks_of(n_vars, WG)), n_vars, a, head.p);
    R.nu = scan.run(head, rank, n_vars, ctx);
    LAUNCH(pafvcf_unique_kernel, (blocks_of(n_vars, WG)), n_vars, a, head.p, rank.p, R.u_start.p, R.u_end.p);
    end_max.alloc(R.nu);
    launch_scan<uint32_t>(s, R.nu, LoadU32{R.u_end.p}, MaxOp{}, 0u, end_max.p, false);
    LAUNCH(pafvcf_mhead_kernel, (blocks_of(R.nu, WG)), R.nu, R.u_start.p, end_max.p, head.p);
    R.nm = scan.run(head, rank, R.nu, ctx);
    R.m_start.alloc(R.nm); R.m_end.alloc(R.nm);
    LAUNCH(pafvcf_merged_kernel, (blocks_of(R.nu, WG)), R.nu, R.u_start.p, end_max.p, head.p, rank.p, R.m_start.p, R.m_end.p);
    sync(ctx);
}

// items 6-7 up to the allele numbers
void table_dev(lcty_ctx* ctx, const DSeqs& S, const DVars& V, uint32_t n_ranges, const uint32_t* r_start, const uint32_t* r_end, DTable& T) {
    hipStream_t s = ctx->stream;
    const uint32_t H = S.n;
    T.n_ranges = n_ranges; T.n_all = 0;
    const uint64_t cells = uint64_t(n_ranges) * H;
    {   // the table of a call is resident: n_ranges x n_seqs int32, and at most as much again for the lists of its pending cells
        size_t free_b = 0, total_b = 0;
        LCTY_HIP(hipMemGetInfo(&free_b, &total_b));
        const int64_t cap_mb = ctx->knob("pafvcf_table_mb", static_cast<int64_t>(free_b / 4 >> 20));
        if (cells * 4 > static_cast<uint64_t>(cap_mb) << 20)
            fail(LCTY_ERR_UNSUPPORTED, "the allele table of %u ranges x %u haplotypes needs %llu MB, more than pafvcf_table_mb = %lld (default: a quarter of the free "
                 "device memory)", n_ranges, H, static_cast<unsigned long long>(cells * 4 >> 20), static_cast<long long>(cap_mb));
    }
    T.ix.alloc(std::max<uint64_t>(cells, 1)); T.n_alleles.alloc(std::max(n_ranges, 1u));
    if (!n_ranges) { T.aoff.alloc(1); T.aoff.zero(s); T.a_hap.alloc(1); T.a_start.alloc(1); T.a_len.alloc(1); sync(ctx); return; }
    int64_t bits = ctx->knob("pafvcf_hash_bits", 64);
    if (bits < 0 || bits > 64) fail(LCTY_ERR_INVALID_INPUT, "pafvcf_hash_bits = %lld (0 .. 64)", static_cast<long long>(bits));
    const uint64_t hash_mask = bits == 64 ? ~0ull : (1ull << bits) - 1;
    DevBuf<uint32_t> d_flags, n_pend, poff, l_hap, l_start, l_len, l_car, l_num, n_car;
    DevBuf<uint64_t> l_hash;
    init_flags(ctx, d_flags);
    n_pend.alloc(n_ranges); n_pend.zero(s); n_car.alloc(n_ranges); n_car.zero(s);
    LAUNCH(pafvcf_cell_kernel, (n_ranges, blocks_of(H, WG)), S.view(), V.view(), n_ranges, r_start, r_end, T.ix.p, n_pend.p, d_flags.p);
    ScanTotal scan;
    const uint32_t n_list = scan.run(n_pend, poff, n_ranges, ctx);
    uint32_t flags[F_COUNT];
    read_flags(ctx, d_flags, flags);
    if (flags[F_SLICE] != NONE)
        fail(LCTY_ERR_RUNTIME, "range %u: a haplotype's allele lies outside the haplotype (a CIGAR that starts with gaps of two kinds; the reference panics here)", flags[F_SLICE]);
    const size_t nl = std::max(n_list, 1u);
    l_hap.alloc(nl); l_start.alloc(nl); l_len.alloc(nl); l_car.alloc(nl); l_num.alloc(nl); l_hash.alloc(nl);
    if (n_list) {
        LAUNCH(pafvcf_list_kernel, (blocks_of(n_ranges, WG / WAVE)), S.view(), V.view(), n_ranges, r_start, r_end, T.ix.p, poff.p, hash_mask, l_hap.p, l_start.p, l_len.p,
               l_hash.p);
        LAUNCH(pafvcf_carrier_kernel, (blocks_of(n_list, WG)), S.view(), n_ranges, n_list, poff.p, l_hap.p, l_start.p, l_len.p, l_hash.p, l_car.p, n_car.p);
    }
    T.n_all = scan.run(n_car, T.aoff, n_ranges, ctx);
    const size_t na = std::max(T.n_all, 1u);
    T.a_hap.alloc(na); T.a_start.alloc(na); T.a_len.alloc(na);
    LAUNCH(pafvcf_number_kernel, (blocks_of(n_ranges, WG / WAVE)), n_ranges, poff.p, T.aoff.p, l_hap.p, l_start.p, l_len.p, l_car.p, l_num.p, T.a_hap.p, T.a_start.p,
           T.a_len.p, T.n_alleles.p);
    if (n_list) LAUNCH(pafvcf_assign_kernel, (blocks_of(n_list, WG)), H, n_ranges, n_list, poff.p, l_hap.p, l_car.p, l_num.p, T.ix.p);
    sync(ctx);
}

struct Samples {
    std::vector<std::string> names; std::vector<uint32_t> slot_off, slot_hap;
    uint32_t ref_id = 0, warn_bits = 0;
};

struct DSlots {
    DevBuf<uint32_t> hap; DevBuf<uint8_t> first; uint32_t n = 0;
    void upload(lcty_ctx* ctx, uint32_t n_samples, const uint32_t* slot_off, const uint32_t* slot_hap, uint32_t n_seqs) {
        if (n_samples && (!slot_off || !slot_hap)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        n = n_samples ? slot_off[n_samples] : 0;
        std::vector<uint8_t> f(std::max(n, 1u), 0);
        for (uint32_t i = 0; i < n_samples; i++) {
            if (slot_off[i + 1] <= slot_off[i] || slot_off[i + 1] > n) fail(LCTY_ERR_INVALID_INPUT, "sample %u has no slot", i);
            f[slot_off[i]] = 1;
        }
        for (uint32_t k = 0; k < n; k++) if (slot_hap[k] != NONE && slot_hap[k] >= n_seqs) fail(LCTY_ERR_INVALID_INPUT, "slot %u names haplotype %u of %u", k, slot_hap[k], n_seqs);
        hap.alloc(std::max(n, 1u)); first.alloc(std::max(n, 1u));
        hap.upload(slot_hap, n, ctx->stream); first.upload(f.data(), n, ctx->stream);
        sync(ctx);
    }
};

// item 7: line lengths, a scan, every line at its offset. The text lands behind `prefix` in one block of h.
char* text_dev(lcty_ctx* ctx, const DSeqs& S, const DTable& T, const uint32_t* r_start, const uint32_t* r_end, const DSlots& L, const char* chrom, uint32_t shift,
               const std::string& prefix, Handoff& h, uint64_t* len, uint64_t* n_lines) {
    hipStream_t s = ctx->stream;
    const uint32_t R = T.n_ranges;
    const size_t chrom_len = strlen(chrom);
    if (chrom_len > 0xFFFFu) fail(LCTY_ERR_UNSUPPORTED, "a contig name of %zu bytes", chrom_len);
    uint64_t body = 0, lines = 0;
    DevBuf<uint64_t> line_len, line_off; DevBuf<char> d_chrom, d_out; DevBuf<uint32_t> d_flags;
    if (R) {
        init_flags(ctx, d_flags);
        d_chrom.alloc(std::max<size_t>(chrom_len, 1)); d_chrom.upload(chrom, chrom_len, s);
        line_len.alloc(R); line_off.alloc(uint64_t(R) + 1);
        const TextIn in{r_start, r_end, T.ix.p, T.n_alleles.p, T.aoff.p, T.a_hap.p, T.a_start.p, T.a_len.p, L.hap.p, L.first.p, L.n, S.n, uint32_t(chrom_len), shift};
        LAUNCH(pafvcf_linelen_kernel, (R), in, line_len.p, d_flags.p);
        launch_scan<uint64_t>(s, R, LoadU64{line_len.p}, AddOp{}, uint64_t(0), line_off.p, true);
        line_off.download(&body, 1, s, R);
        uint32_t flags[F_COUNT];
        read_flags(ctx, d_flags, flags);
        if (flags[F_BADCELL] != NONE) fail(LCTY_ERR_INVALID_INPUT, "range %u: an allele number the range does not have", flags[F_BADCELL]);
        if (flags[F_LONGLINE] != NONE) fail(LCTY_ERR_UNSUPPORTED, "the line of range %u is longer than 2^32 bytes", flags[F_LONGLINE]);
        lines = flags[F_LINES];
        if (body) {
            d_out.alloc(body);
            LAUNCH(pafvcf_write_kernel, (R), in, S.view(), d_chrom.p, line_off.p, d_out.p);
        }
    }
    char* out = static_cast<char*>(h.raw(prefix.size() + body));
    memcpy(out, prefix.data(), prefix.size());
    if (body) d_out.download(out + prefix.size(), body, s);
    sync(ctx);
    *len = prefix.size() + body; *n_lines = lines;
    return out;
}

// ---- host: samples --------------------------------------------------------------------------------------------------------------------

bool is_alnum(unsigned char c) { return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }
// ^([0-9A-Za-z][0-9A-Za-z+._|~=@^-]*?)([._][1-9])?$ (paf_vcf.rs:577): the lazy group leaves a final [._][1-9] to the suffix whenever a character stands in front of it
bool parse_name(const std::string& name, std::string* sample, int* slot) {
    if (name.empty() || !is_alnum(name[0])) return false;
    for (size_t i = 1; i < name.size(); i++) if (!is_alnum(name[i]) && !strchr("+._|~=@^-", name[i])) return false;
    const size_t n = name.size();
    if (n >= 3 && (name[n - 2] == '.' || name[n - 2] == '_') && name[n - 1] >= '1' && name[n - 1] <= '9') { *sample = name.substr(0, n - 2); *slot = name[n - 1] - '1'; }
    else { *sample = name; *slot = -1; }
    return true;
}

std::vector<std::string> split_ws(const std::string& line) {
    std::vector<std::string> out;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && strchr(" \t\r\n\v\f", line[i])) i++;
        size_t j = i;
        while (j < line.size() && !strchr(" \t\r\n\v\f", line[j])) j++;
        if (j > i) out.push_back(line.substr(i, j - i));
        i = j;
    }
    return out;
}

Samples group_haplotypes(const std::vector<std::string>& names, const char* discarded, uint64_t discarded_len, const std::string& ref_hap) {
    Samples out;
    std::unordered_map<std::string, uint32_t> ids;
    for (uint32_t i = 0; i < names.size(); i++) ids.emplace(names[i], i);
    // DiscardedHaplotypes::load (contigs.rs:488-528)
    std::map<uint32_t, std::vector<std::string>> by_contig;
    std::unordered_map<std::string, std::vector<std::string>> unknown;
    bool all_identical = true;
    for (uint64_t p = 0; discarded && p < discarded_len;) {
        const char* nl = static_cast<const char*>(memchr(discarded + p, '\n', discarded_len - p));
        const uint64_t q = nl ? uint64_t(nl - discarded) : discarded_len;
        const std::vector<std::string> split = split_ws(std::string(discarded + p, q - p));
        p = q + 1;
        if (split.size() < 3) fail(LCTY_ERR_INVALID_INPUT, "Each line in discarded haplotypes must have at least 3 columns");
        all_identical &= split[1] == "=";
        std::vector<std::string> rhs;
        for (size_t c = 2; c < split.size(); c++) {
            std::string contig = split[c];
            if (!contig.empty() && contig.back() == ',') contig.pop_back();
            if (ids.count(contig)) continue;                            // "marked as discarded, but present in the haplotypes fasta"
            rhs.push_back(contig);
            auto it = unknown.find(contig);
            if (it != unknown.end()) { const std::vector<std::string> more = std::move(it->second); unknown.erase(it); rhs.insert(rhs.end(), more.begin(), more.end()); }
        }
        auto id = ids.find(split[0]);
        if (id != ids.end()) by_contig[id->second] = rhs; else unknown[split[0]] = rhs;
    }
    if (!all_identical) out.warn_bits |= LCTY_PAFVCF_WARN_PRUNED;       // paf_vcf.rs:633-635
    // group_haplotypes (569-621)
    std::map<std::string, std::vector<uint32_t>> groups;                 // ordered bytewise, as the final sort
    bool found = false;
    auto add = [&](uint32_t i, const std::string& name) {
        std::string sample; int slot;
        if (!parse_name(name, &sample, &slot)) fail(LCTY_ERR_INVALID_DATA, "Cannot parse contig name `%s`", name.c_str());
        if (name == ref_hap) {
            found = true; out.ref_id = i;
            if (slot >= 0) out.warn_bits |= LCTY_PAFVCF_WARN_REF_SUFFIX; else return;
        }
        std::vector<uint32_t>& vec = groups[sample];
        const size_t hap = slot < 0 ? 0 : size_t(slot);
        const size_t new_len = std::max({vec.size(), hap + 1, size_t(slot < 0 ? 1 : 2)});
        vec.resize(new_len, NONE);
        vec[hap] = i;
    };
    for (uint32_t i = 0; i < names.size(); i++) {
        add(i, names[i]);
        auto it = by_contig.find(i);
        if (it != by_contig.end()) for (const std::string& hap : it->second) add(i, hap);
    }
    if (!found) fail(LCTY_ERR_INVALID_INPUT, "Cannot find reference haplotype %s in neither the fasta file nor among the discarded haplotypes", ref_hap.c_str());
    out.slot_off.push_back(0);
    for (const auto& g : groups) {
        out.names.push_back(g.first);
        out.slot_hap.insert(out.slot_hap.end(), g.second.begin(), g.second.end());
        out.slot_off.push_back(static_cast<uint32_t>(out.slot_hap.size()));
    }
    return out;
}

void free_out(lcty_pafvcf_out* o) {
    free(o->var_off); free(o->ref_start); free(o->ref_end); free(o->hap_start); free(o->hap_end); free(o->has_aln);
    free(o->unique_start); free(o->unique_end); free(o->merged_start); free(o->merged_end);
    free(o->allele_ix); free(o->n_alleles); free(o->allele_off); free(o->allele_hap); free(o->allele_start); free(o->allele_len);
    free(o->merged); free(o->separate);
    memset(o, 0, sizeof(*o));
}

void vars_to_host(lcty_ctx* ctx, const DSeqs& S, const DVars& V, Handoff& h, lcty_pafvcf_out* out) {
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> off(uint64_t(S.n) + 1);
    V.off.download(off.data(), off.size(), s);
    out->ref_start = from(h, V.rs, V.n, s); out->ref_end = from(h, V.re, V.n, s);
    out->hap_start = from(h, V.hs, V.n, s); out->hap_end = from(h, V.he, V.n, s);
    out->has_aln = from(h, V.has, S.n, s);
    sync(ctx);
    std::vector<uint64_t> off64(off.begin(), off.end());
    out->var_off = h.copy(off64);
    out->n_seqs = S.n; out->n_variants = V.n;
    out->stats.n_variants = V.n; out->stats.n_missing = V.n_missing; out->stats.n_bad_len = V.n_bad_len; out->stats.n_shifted = V.n_shifted;
}

void ranges_to_host(lcty_ctx* ctx, const DRanges& R, Handoff& h, lcty_pafvcf_out* out) {
    hipStream_t s = ctx->stream;
    out->unique_start = from(h, R.u_start, R.nu, s); out->unique_end = from(h, R.u_end, R.nu, s);
    out->merged_start = from(h, R.m_start, R.nm, s); out->merged_end = from(h, R.m_end, R.nm, s);
    sync(ctx);
    out->n_unique = R.nu; out->n_merged = R.nm; out->stats.n_unique = R.nu; out->stats.n_merged = R.nm;
}

void upload_vars(lcty_ctx* ctx, const DSeqs& S, const uint64_t* var_off, const uint32_t* rs, const uint32_t* re, const uint32_t* hs, const uint32_t* he,
                 const uint8_t* has_aln, DVars& V) {
    if (!var_off || !has_aln) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> off(uint64_t(S.n) + 1);
    for (uint32_t h = 0; h <= S.n; h++) {
        if (var_off[h] >= 0x7FFFFFF0ull || (h && var_off[h] < var_off[h - 1])) fail(LCTY_ERR_INVALID_INPUT, "var_off is not a list of 32-bit offsets");
        off[h] = static_cast<uint32_t>(var_off[h]);
    }
    if (off[0] != 0) fail(LCTY_ERR_INVALID_INPUT, "var_off does not start at 0");
    V.n = off[S.n];
    if (V.n && (!rs || !re || !hs || !he)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    // what the bisections and the slices rely on: inside a haplotype the variants are ordered and lie inside both sequences
    for (uint32_t h = 0; h < S.n; h++)
        for (uint32_t v = off[h]; v < off[h + 1]; v++)
            if (rs[v] > re[v] || hs[v] > he[v] || (v > off[h] && (rs[v] < rs[v - 1] || re[v] < re[v - 1])) || re[v] >= 0x7FFFFFF0u || he[v] >= 0x7FFFFFF0u)
                fail(LCTY_ERR_INVALID_INPUT, "variant %u of haplotype %u is not ordered", v - off[h], h);
    const size_t nv = std::max(V.n, 1u);
    V.off.alloc(off.size()); V.off.upload(off.data(), off.size(), s);
    V.rs.alloc(nv); V.re.alloc(nv); V.hs.alloc(nv); V.he.alloc(nv); V.has.alloc(S.n);
    V.rs.upload(rs, V.n, s); V.re.upload(re, V.n, s); V.hs.upload(hs, V.n, s); V.he.upload(he, V.n, s); V.has.upload(has_aln, S.n, s);
    sync(ctx);
}

void check_ranges(const DSeqs& S, uint64_t n_ranges, const uint32_t* r_start, const uint32_t* r_end) {
    if (n_ranges >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%llu ranges", static_cast<unsigned long long>(n_ranges));
    if (n_ranges && (!r_start || !r_end)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    for (uint64_t r = 0; r < n_ranges; r++)
        if (r_start[r] > r_end[r] || r_end[r] > S.ref_len) fail(LCTY_ERR_INVALID_INPUT, "range %llu (%u-%u) lies outside the reference haplotype (%llu bases)",
                                                                static_cast<unsigned long long>(r), r_start[r], r_end[r], static_cast<unsigned long long>(S.ref_len));
}

void table_to_host(lcty_ctx* ctx, const DSeqs& S, const DTable& T, Handoff& h, lcty_pafvcf_out* out) {
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> aoff(uint64_t(T.n_ranges) + 1);
    T.aoff.download(aoff.data(), aoff.size(), s);
    out->allele_ix = from(h, T.ix, uint64_t(T.n_ranges) * S.n, s); out->n_alleles = from(h, T.n_alleles, T.n_ranges, s);
    out->allele_hap = from(h, T.a_hap, T.n_all, s); out->allele_start = from(h, T.a_start, T.n_all, s); out->allele_len = from(h, T.a_len, T.n_all, s);
    sync(ctx);
    std::vector<uint64_t> aoff64(aoff.begin(), aoff.end());
    out->allele_off = h.copy(aoff64);
    out->n_ranges = T.n_ranges; out->n_seqs = S.n;
}

std::string header_text(const std::vector<std::string>& samples) {     // create_vcf_writer, paf_vcf.rs:349-357
    std::string h = "##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT";
    for (const std::string& s : samples) { h += '\t'; h += s; }
    h += '\n';
    return h;
}

}  // namespace

extern "C" {

int32_t lcty_pafvcf_samples(uint32_t n_seqs, const char* names, const char* discarded, uint64_t discarded_len, const char* ref_hap, uint32_t cap_samples,
                            uint32_t* n_samples, char* sample_names, uint64_t cap_names, uint64_t* names_len, uint32_t* slot_off, uint32_t cap_slots,
                            uint32_t* n_slots, uint32_t* slot_hap, uint32_t* ref_id, uint32_t* warn_bits) {
    return guarded([&] {
        if (!names || !ref_hap || !n_samples || !names_len || !n_slots || !n_seqs) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const Samples S = group_haplotypes(split_names(names, n_seqs), discarded, discarded_len, ref_hap);
        std::string blob;
        for (const std::string& n : S.names) { blob += n; blob.push_back('\0'); }
        *n_samples = static_cast<uint32_t>(S.names.size()); *names_len = blob.size(); *n_slots = static_cast<uint32_t>(S.slot_hap.size());
        if (ref_id) *ref_id = S.ref_id;
        if (warn_bits) *warn_bits = S.warn_bits;
        if (sample_names || slot_off || slot_hap) {
            if (!sample_names || !slot_off || !slot_hap) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            if (cap_samples < S.names.size() || cap_names < blob.size() || cap_slots < S.slot_hap.size())
                fail(LCTY_ERR_INVALID_INPUT, "output buffers too small (%zu samples, %zu name bytes, %zu slots)", S.names.size(), blob.size(), S.slot_hap.size());
            memcpy(sample_names, blob.data(), blob.size()); memcpy(slot_off, S.slot_off.data(), 4 * S.slot_off.size());
            memcpy(slot_hap, S.slot_hap.data(), 4 * S.slot_hap.size());
        }
    });
}

int32_t lcty_pafvcf_variants(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref_id, uint64_t n_entries, const uint32_t* id1,
                             const uint32_t* id2, const uint64_t* cigar_off, const uint32_t* cigar, lcty_pafvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        ctx->activate();
        const double t0 = now_ms();
        DSeqs S; DVars V;
        S.upload(ctx, n_seqs, seqs, seq_off, ref_id);
        variants_dev(ctx, S, n_entries, id1, id2, cigar_off, cigar, V);
        lcty_pafvcf_out o{}; Handoff h;
        vars_to_host(ctx, S, V, h, &o);
        o.stats.variants_ms = o.stats.total_ms = now_ms() - t0;
        *out = o; h.commit();
    });
}

int32_t lcty_pafvcf_ranges(lcty_ctx* ctx, uint64_t n_variants, const uint32_t* ref_start, const uint32_t* ref_end, lcty_pafvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out || (n_variants && (!ref_start || !ref_end))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_variants >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%llu variants (32-bit offsets)", static_cast<unsigned long long>(n_variants));
        ctx->activate();
        const double t0 = now_ms();
        const uint32_t n = static_cast<uint32_t>(n_variants);
        uint32_t max_pos = 0;
        for (uint32_t v = 0; v < n; v++) max_pos = std::max({max_pos, ref_start[v], ref_end[v]});
        DevBuf<uint32_t> rs, re; DRanges R;
        rs.alloc(std::max(n, 1u)); re.alloc(std::max(n, 1u));
        rs.upload(ref_start, n, ctx->stream); re.upload(ref_end, n, ctx->stream);
        ranges_dev(ctx, n, rs, re, max_pos, R);
        lcty_pafvcf_out o{}; Handoff h;
        ranges_to_host(ctx, R, h, &o);
        o.stats.ranges_ms = o.stats.total_ms = now_ms() - t0;
        *out = o; h.commit();
    });
}

int32_t lcty_pafvcf_table(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref_id, const uint64_t* var_off,
                          const uint32_t* ref_start, const uint32_t* ref_end, const uint32_t* hap_start, const uint32_t* hap_end, const uint8_t* has_aln,
                          uint64_t n_ranges, const uint32_t* range_start, const uint32_t* range_end, lcty_pafvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        ctx->activate();
        const double t0 = now_ms();
        DSeqs S; DVars V; DTable T; DevBuf<uint32_t> r0, r1;
        S.upload(ctx, n_seqs, seqs, seq_off, ref_id);
        upload_vars(ctx, S, var_off, ref_start, ref_end, hap_start, hap_end, has_aln, V);
        check_ranges(S, n_ranges, range_start, range_end);
        const uint32_t R = static_cast<uint32_t>(n_ranges);
        r0.alloc(std::max(R, 1u)); r1.alloc(std::max(R, 1u));
        r0.upload(range_start, R, ctx->stream); r1.upload(range_end, R, ctx->stream);
        table_dev(ctx, S, V, R, r0.p, r1.p, T);
        lcty_pafvcf_out o{}; Handoff h;
        table_to_host(ctx, S, T, h, &o);
        o.stats.table_ms = o.stats.total_ms = now_ms() - t0;
        *out = o; h.commit();
    });
}

int32_t lcty_pafvcf_text(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref_id, uint64_t n_ranges,
                         const uint32_t* range_start, const uint32_t* range_end, const int32_t* allele_ix, const uint32_t* n_alleles, const uint64_t* allele_off,
                         const uint32_t* allele_hap, const uint32_t* allele_start, const uint32_t* allele_len, uint32_t n_samples, const uint32_t* slot_off,
                         const uint32_t* slot_hap, const char* chrom, uint32_t shift, lcty_pafvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out || !chrom) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        ctx->activate();
        const double t0 = now_ms();
        hipStream_t s = ctx->stream;
        DSeqs S; DTable T; DSlots L; DevBuf<uint32_t> r0, r1;
        S.upload(ctx, n_seqs, seqs, seq_off, ref_id);
        check_ranges(S, n_ranges, range_start, range_end);
        const uint32_t R = static_cast<uint32_t>(n_ranges);
        if (R && (!allele_ix || !n_alleles || !allele_off)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        // the table as lcty_pafvcf_table gives it: every number inside its range's alleles, every allele inside its haplotype
        std::vector<uint32_t> aoff(uint64_t(R) + 1, 0);
        for (uint32_t r = 0; r < R; r++) {
            if (allele_off[r + 1] < allele_off[r] || allele_off[r + 1] >= 0x7FFFFFF0ull || n_alleles[r] != 1 + (allele_off[r + 1] - allele_off[r]))
                fail(LCTY_ERR_INVALID_INPUT, "range %u: n_alleles and allele_off disagree", r);
            aoff[r + 1] = static_cast<uint32_t>(allele_off[r + 1]);
        }
        if (R && allele_off[0] != 0) fail(LCTY_ERR_INVALID_INPUT, "allele_off does not start at 0");
        T.n_ranges = R; T.n_all = aoff[R];
        if (T.n_all && (!allele_hap || !allele_start || !allele_len)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        for (uint32_t a = 0; a < T.n_all; a++)
            if (allele_hap[a] >= n_seqs || uint64_t(allele_start[a]) + allele_len[a] > seq_off[allele_hap[a] + 1] - seq_off[allele_hap[a]])
                fail(LCTY_ERR_INVALID_INPUT, "allele %u lies outside haplotype %u", a, allele_hap[a]);
        const uint64_t cells = uint64_t(R) * n_seqs;
        T.ix.alloc(std::max<uint64_t>(cells, 1)); T.n_alleles.alloc(std::max(R, 1u)); T.aoff.alloc(aoff.size());
        T.a_hap.alloc(std::max(T.n_all, 1u)); T.a_start.alloc(std::max(T.n_all, 1u)); T.a_len.alloc(std::max(T.n_all, 1u));
        T.ix.upload(allele_ix, cells, s); T.n_alleles.upload(n_alleles, R, s); T.aoff.upload(aoff.data(), aoff.size(), s);
        T.a_hap.upload(allele_hap, T.n_all, s); T.a_start.upload(allele_start, T.n_all, s); T.a_len.upload(allele_len, T.n_all, s);
        r0.alloc(std::max(R, 1u)); r1.alloc(std::max(R, 1u));
        r0.upload(range_start, R, s); r1.upload(range_end, R, s);
        L.upload(ctx, n_samples, slot_off, slot_hap, n_seqs);
        lcty_pafvcf_out o{}; Handoff h;
        o.merged = text_dev(ctx, S, T, r0.p, r1.p, L, chrom, shift, std::string(), h, &o.merged_len, &o.stats.n_lines_merged);
        o.stats.merged_bytes = o.merged_len;
        o.stats.text_ms = o.stats.total_ms = now_ms() - t0;
        *out = o; h.commit();
    });
}

int32_t lcty_paf_to_vcf(lcty_ctx* ctx, uint32_t n_seqs, const char* names, const uint8_t* seqs, const uint64_t* seq_off, const char* discarded,
                        uint64_t discarded_len, const char* ref_hap, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2, const uint64_t* cigar_off,
                        const uint32_t* cigar, const char* chrom, uint32_t region_start, uint32_t region_end, int32_t with_separate, lcty_pafvcf_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out || !names || !ref_hap || !n_seqs || !seq_off) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double t0 = now_ms();
        const Samples G = group_haplotypes(split_names(names, n_seqs), discarded, discarded_len, ref_hap);
        const uint64_t ref_len = seq_off[G.ref_id + 1] - seq_off[G.ref_id];
        uint32_t shift = 0;
        if (chrom) {                                                    // convert_to_vcf 638-645
            if (region_end < region_start || uint64_t(region_end - region_start) != ref_len)
                fail(LCTY_ERR_INVALID_DATA, "paf-vcf: region %s:%u-%u (len = %lld) does not match reference haplotype (len = %llu)", chrom, region_start + 1, region_end,
                     static_cast<long long>(region_end) - static_cast<long long>(region_start), static_cast<unsigned long long>(ref_len));
            shift = region_start;
        } else chrom = ref_hap;
        ctx->activate();
        lcty_pafvcf_stats st{};
        st.warn_bits = G.warn_bits; st.n_samples = static_cast<uint32_t>(G.names.size());
        DSeqs S; DVars V; DRanges R; DSlots L;
        S.upload(ctx, n_seqs, seqs, seq_off, G.ref_id);
        L.upload(ctx, st.n_samples, G.slot_off.data(), G.slot_hap.data(), n_seqs);
        st.upload_ms = now_ms() - t0;
        double t = now_ms();
        variants_dev(ctx, S, n_entries, id1, id2, cigar_off, cigar, V);
        st.variants_ms = now_ms() - t; t = now_ms();
        ranges_dev(ctx, V.n, V.rs, V.re, static_cast<uint32_t>(ref_len) + 1, R);
        st.ranges_ms = now_ms() - t;
        st.n_variants = V.n; st.n_missing = V.n_missing; st.n_bad_len = V.n_bad_len; st.n_shifted = V.n_shifted; st.n_unique = R.nu; st.n_merged = R.nm;
        const std::string header = header_text(G.names);
        lcty_pafvcf_out o{}; Handoff h;
        for (int pass = 0; pass < (with_separate ? 2 : 1); pass++) {
            DTable T;
            t = now_ms();
            const uint32_t n = pass ? R.nu : R.nm;
            const uint32_t* r0 = pass ? R.u_start.p : R.m_start.p; const uint32_t* r1 = pass ? R.u_end.p : R.m_end.p;
            table_dev(ctx, S, V, n, r0, r1, T);
            st.table_ms += now_ms() - t; t = now_ms();
            if (pass) { o.separate = text_dev(ctx, S, T, r0, r1, L, chrom, shift, header, h, &o.separate_len, &st.n_lines_separate); st.separate_bytes = o.separate_len; }
            else { o.merged = text_dev(ctx, S, T, r0, r1, L, chrom, shift, header, h, &o.merged_len, &st.n_lines_merged); st.merged_bytes = o.merged_len; }
            st.text_ms += now_ms() - t;
        }
        o.n_seqs = n_seqs; o.n_variants = V.n; o.n_unique = R.nu; o.n_merged = R.nm;
        st.total_ms = now_ms() - t0;
        o.stats = st;
        *out = o; h.commit();
    });
}

void lcty_pafvcf_out_free(lcty_pafvcf_out* out) {
    if (out) free_out(out);
}

}  // extern "C"
