// lcty_basis.hip — the basis haplotypes of a locus: the basis step of `locityper augment` (construct_dominant_set ->
// inner_construct_dominant_set -> Cigar::locally_similar -> find_dominating_set; command/augment.rs:258-396, seq/cigar.rs:656-751,
// algo/dom_set.rs) on the entries lcty_paf_read returns.
//   window similarity  -> one bit row per (contig, window): basis_windows_kernel
//   unique rows        -> basis_dedup_kernel (device hash table), canonical order on the host
//   minimal rows       -> basis_subsume_kernel (a presolve of ours, not the reference's)
//   minimum hitting set-> lcty_basis_search.cpp (host branch and bound in the place of SCIP)
//
// locally_similar is a serial two-pointer walk; here it is a closed form over prefix sums. For one side of one entry let run r of the
// CIGAR start at walked coordinate C[r] (only operations that consume the walked sequence move it) and let ED[r] be the total length of
// the runs before r that are not '='. For a coordinate x < len let r(x) be the LAST run with C[r] <= x: it consumes the walked sequence
// and holds x, and every operation that does not consume it (I on the reference side, D on the query side) at a boundary b <= x comes
// before it. Then
//     A(x) = ED[r(x)] + (run r(x) is not '=' ? x - C[r(x)] : 0)
// counts the edits left of x together with every non-consuming operation at a boundary b <= x, and the walk's edit count at window start
// s = t * step < len - window is A(s + window) - A(s): the left pointer has removed what lies at b <= s (a leading gap at b = 0 included)
// before a start inside its run is emitted, the right pointer has added what lies at b <= s + window.
// The LAST window, s = len - window, is emitted after the loop and differs: the walk breaks when the right iterator ends, before the left
// pointer has removed the non-consuming operations AT b = s (total G), except that trailing non-consuming operations (total c, at b = len)
// are added while operations at b = s are removed run against run, so min(G, c) of G is gone. Its edit count is
//     ED[n] - A(s) + max(G - c, 0).
// tests/test_basis_host.py holds this against the walk itself (tests/pyref_basis.py), on designed CIGARs and on random ones.
#include "lcty_common.hpp"
#include "lcty_basis_search.hpp"
#include "lcty_device.hpp"
#include "lcty_seq.hpp"

#include <algorithm>
#include <cmath>

namespace {
using namespace lcty;

constexpr uint32_t kChunk = 1024;                          // CIGAR runs whose prefix sums one wavefront keeps in LDS (8 KB)
constexpr uint32_t kPerLane = kChunk / 64;
constexpr uint32_t kErrOp = 1u, kErrLen = 2u;

// every row starts with the bit of its own contig (augment.rs:324-325)
__global__ __launch_bounds__(256) void basis_init_kernel(const uint64_t* __restrict__ win_off, uint32_t words, uint32_t* __restrict__ bits) {
    const uint32_t a = blockIdx.x;
    for (uint64_t r = win_off[a] + threadIdx.x; r < win_off[a + 1]; r += 256) bits[r * words + (a >> 5)] = 1u << (a & 31);
}

// first index q in [0, n] with C[q] >= x; the caller guarantees C[n] >= x
__device__ inline uint32_t first_ge(const uint32_t* C, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (C[mid] >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ inline uint32_t edits_left_of(const uint32_t* C, const uint32_t* ED, uint32_t n, uint32_t x, uint32_t* run) {
    const uint32_t r = flat_owner(C, n, x);                // the caller guarantees C[0] <= x
    *run = r;
    return ED[r] + (ED[r + 1] != ED[r] ? x - C[r] : 0u);
}

// One wavefront per (entry, side): side 0 walks the query (contig id1, IN_QUERY), side 1 the target (contig id2). The CIGAR is taken in
// chunks of kChunk runs; a window is decided in the chunk that holds its right end s + window, and where its start lies in an earlier
// chunk A(s) waits in `ring` (per wavefront, `ring_len` >= the windows that can straddle a chunk end: ceil(window / step) + 1).
__global__ __launch_bounds__(64) void basis_windows_kernel(const uint32_t* __restrict__ cigar, const uint64_t* __restrict__ cig_off,
                                                           const uint32_t* __restrict__ id1, const uint32_t* __restrict__ id2,
                                                           const uint8_t* __restrict__ short_ok, const uint32_t* __restrict__ lens,
                                                           const uint64_t* __restrict__ win_off, uint32_t window, uint32_t step, uint32_t max_edit,
                                                           uint32_t ring_len, uint32_t* __restrict__ ring, uint32_t words,
                                                           uint32_t* __restrict__ bits, uint32_t* __restrict__ err) {
    __shared__ uint32_t C[kChunk + 1], ED[kChunk + 1];
    const uint32_t e = blockIdx.x >> 1, side = blockIdx.x & 1, lane = threadIdx.x;
    const uint32_t contig = side ? id2[e] : id1[e], other = side ? id1[e] : id2[e];
    const uint32_t len = lens[contig];
    uint32_t* row0 = bits + win_off[contig] * words + (other >> 5);
    const uint32_t mask = 1u << (other & 31);
    if (len <= window) {                                                      // update_bitarray, augment.rs:302-305
        if (lane == 0 && short_ok[e]) atomicOr(row0, mask);
        return;
    }
    const uint32_t s_last = len - window;
    const uint32_t t_last = (s_last + step - 1) / step;                       // index of the last window; the regular ones are t < t_last
    const uint32_t* cg = cigar + cig_off[e];
    const uint64_t n_runs = cig_off[e + 1] - cig_off[e];
    uint32_t* my_ring = ring + uint64_t(blockIdx.x) * ring_len;
    uint32_t base_c = 0, base_e = 0, gap_carry = 0;                            // gap_carry: non-consuming runs of earlier chunks at the boundary base_c
    uint32_t a_last = 0, g_last = 0;
    bool bad_op = false, have_last = false;
    for (uint64_t ch = 0; ch < n_runs; ch += kChunk) {
        const uint32_t kc = static_cast<uint32_t>(n_runs - ch < kChunk ? n_runs - ch : kChunk);
        // prefix sums of the chunk: kPerLane consecutive runs per lane, then a scan over the lanes
        uint32_t mc = 0, me = 0;
        for (uint32_t i = 0; i < kPerLane; i++) {
            const uint32_t q = lane * kPerLane + i;
            if (q >= kc) break;
            const uint32_t w = cg[ch + q], op = w & 15u, ln = w >> 4;
            C[q] = mc; ED[q] = me;
            // M 0, I 1, D 2, = 7, X 8 (consumes_query: M = X I; consumes_ref: M = X D)
            const bool known = op == 0 || op == 1 || op == 2 || op == 7 || op == 8;
            bad_op |= !known;
            const bool moves = known && op != (side ? 1u : 2u);
            mc += moves ? ln : 0u;
            me += op != 7 ? ln : 0u;
        }
        uint32_t sc = mc, se = me;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t uc = __shfl_up(sc, d), ue = __shfl_up(se, d);
            if (lane >= d) { sc += uc; se += ue; }
        }
        const uint32_t off_c = base_c + sc - mc, off_e = base_e + se - me;
        for (uint32_t i = 0; i < kPerLane; i++) {
            const uint32_t q = lane * kPerLane + i;
            if (q >= kc) break;
            C[q] += off_c; ED[q] += off_e;
        }
        if (lane == 63) { C[kc] = base_c + sc; ED[kc] = base_e + se; }
        __syncthreads();
        const uint32_t c0 = base_c, c1 = C[kc] < len ? C[kc] : len;             // a CIGAR longer than the contig is an error below; nothing is written past it
        if (c1 > c0) {
            // windows whose right end s + window lies in [c0, c1)
            if (c1 > window) {
                const uint32_t lo_s = c0 > window ? c0 - window : 0;
                const uint32_t t_lo = (lo_s + step - 1) / step;
                uint32_t t_hi = (c1 - window + step - 1) / step;
                if (t_hi > t_last) t_hi = t_last;
                for (uint64_t t = uint64_t(t_lo) + lane; t < t_hi; t += 64) {
                    const uint32_t s = static_cast<uint32_t>(t * step);
                    uint32_t r;
                    const uint32_t b = edits_left_of(C, ED, kc, s + window, &r);
                    const uint32_t a = s >= c0 ? edits_left_of(C, ED, kc, s, &r) : my_ring[t % ring_len];
                    if (b - a <= max_edit) atomicOr(row0 + t * words, mask);
                }
            }
            __syncthreads();
            // starts in [c0, c1) whose right end lies beyond this chunk
            if (C[kc] < len) {
                const uint32_t lo_s = c1 > window && c1 - window > c0 ? c1 - window : c0;
                const uint32_t t_lo = (lo_s + step - 1) / step;
                uint32_t t_hi = static_cast<uint32_t>((uint64_t(c1) + step - 1) / step);
                if (t_hi > t_last) t_hi = t_last;
                for (uint64_t t = uint64_t(t_lo) + lane; t < t_hi; t += 64) {
                    uint32_t r;
                    my_ring[t % ring_len] = edits_left_of(C, ED, kc, static_cast<uint32_t>(t * step), &r);
                }
            }
            if (s_last >= c0 && s_last < c1) {                                  // the last window's start: A(s) and the gap exactly at s
                uint32_t r;
                a_last = edits_left_of(C, ED, kc, s_last, &r);
                g_last = 0;
                if (C[r] == s_last) {
                    const uint32_t lb = first_ge(C, kc, s_last);
                    g_last = ED[r] - ED[lb] + (lb == 0 ? gap_carry : 0u);
                }
                have_last = true;
            }
            gap_carry = ED[kc] - ED[first_ge(C, kc, C[kc])];
        } else {
            gap_carry += ED[kc] - ED[0];
        }
        base_c = C[kc]; base_e = ED[kc];
        __syncthreads();
    }
    if (__any(bad_op)) { if (lane == 0) atomicOr(err, kErrOp); return; }
    if (base_c != len || !have_last) { if (lane == 0) atomicOr(err, kErrLen); return; }
    if (lane == 0) {
        const uint32_t edit = base_e - a_last + (g_last > gap_carry ? g_last - gap_carry : 0u);
        if (edit <= max_edit) atomicOr(row0 + uint64_t(t_last) * words, mask);
    }
}

// One wavefront per row: the row's hash (a sum over the words, so the order of the reduction does not matter), then linear probing in a
// table of row indices: an empty slot makes the row the representative of its content, a slot whose row has the same words ends the
// probe, any other slot is passed. WHICH of several equal rows becomes the representative depends on timing; the set of contents does not.
__global__ __launch_bounds__(256) void basis_dedup_kernel(const uint32_t* __restrict__ rows, uint64_t n_rows, uint32_t words,
                                                          uint32_t* __restrict__ table, uint64_t cap_mask, uint8_t* __restrict__ keep,
                                                          uint32_t* __restrict__ n_keep) {
    const uint64_t r = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= n_rows) return;
    const uint32_t* mine = rows + r * words;
    uint64_t h = 0;
    for (uint32_t k = lane; k < words; k += 64) h += mix64((uint64_t(k) << 32) | mine[k]);
    for (uint32_t d = 32; d; d >>= 1) h += __shfl_xor(h, d);
    uint64_t slot = mix64(h) & cap_mask;
    for (;;) {
        uint32_t prev = 0;
        if (lane == 0) prev = atomicCAS(&table[slot], 0u, static_cast<uint32_t>(r + 1));
        prev = __shfl(prev, 0);
        if (prev == 0) {
            if (lane == 0) { keep[r] = 1; atomicAdd(n_keep, 1u); }
            return;
        }
        const uint32_t* theirs = rows + uint64_t(prev - 1) * words;
        bool differ = false;
        for (uint32_t k = lane; k < words; k += 64) differ |= mine[k] != theirs[k];
        if (!__any(differ)) return;
        slot = (slot + 1) & cap_mask;
    }
}

__global__ __launch_bounds__(256) void basis_compact_kernel(const uint32_t* __restrict__ rows, uint64_t n_rows, uint32_t words,
                                                            const uint8_t* __restrict__ keep, uint32_t* __restrict__ counter,
                                                            uint32_t* __restrict__ out) {
    const uint64_t r = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= n_rows || !keep[r]) return;
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(counter, 1u);
    at = __shfl(at, 0);
    for (uint32_t k = lane; k < words; k += 64) out[uint64_t(at) * words + k] = rows[r * words + k];
}

// Rows in order of popcount; limit[r] = rows with a smaller popcount. One wavefront per row r: lane l takes the rows q = l, l + 64, ..
// below limit[r] and leaves at the first word of q that has a bit r lacks. A row with a subset among the rows is implied by it
// (whether that subset is itself dropped or not: what drops it is a subset of both).
__global__ __launch_bounds__(256) void basis_subsume_kernel(const uint32_t* __restrict__ rows, uint32_t n_rows, uint32_t words,
                                                            const uint32_t* __restrict__ limit, uint8_t* __restrict__ implied) {
    extern __shared__ uint32_t mine_all[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * 4 + wv;
    uint32_t* mine = mine_all + wv * words;
    if (r < n_rows) for (uint32_t k = lane; k < words; k += 64) mine[k] = rows[uint64_t(r) * words + k];
    __syncthreads();
    if (r >= n_rows) return;
    const uint32_t lim = limit[r];
    bool hit = false;
    for (uint32_t q0 = 0; q0 < lim && !hit; q0 += 64) {
        const uint32_t q = q0 + lane;
        bool sub = q < lim;
        if (sub) {
            const uint32_t* o = rows + uint64_t(q) * words;
            for (uint32_t k = 0; k < words; k++) if (o[k] & ~mine[k]) { sub = false; break; }
        }
        hit = __any(sub);
    }
    if (lane == 0) implied[r] = hit ? 1 : 0;
}

uint32_t popcount_row(const uint32_t* r, uint32_t words) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < words; k++) n += static_cast<uint32_t>(__builtin_popcount(r[k]));
    return n;
}

}  // namespace

namespace lcty {

// the bit rows of every (contig, window) on the device: row win_off[contig] + window, `words` 32-bit words each
struct BasisRows {
    DevBuf<uint32_t> bits;
    std::vector<uint64_t> win_off;
    uint64_t n_rows = 0;
    uint32_t words = 0;
};

void basis_check_params(const lcty_basis_params* p) {
    if (!p) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (!(p->divergence >= 0.0) || !(p->divergence <= 1.0)) fail(LCTY_ERR_INVALID_INPUT, "divergence %g: must be within [0, 1]", p->divergence);
    if (p->window == 0) fail(LCTY_ERR_INVALID_INPUT, "window = 0");
}

// inner_construct_dominant_set up to augment.rs:339 -> the bit rows on the device
void basis_windows_device(lcty_ctx* ctx, uint32_t n_alleles, const uint32_t* lengths, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2,
                          const uint32_t* n_matches, const uint32_t* aln_len, const uint64_t* cigar_off, const uint32_t* cigar, const uint8_t* leave_out,
                          const lcty_basis_params* prm, BasisRows& out, lcty_basis_stats& st) {
    basis_check_params(prm);
    if (!ctx || !lengths || (n_entries && (!id1 || !id2 || !n_matches || !aln_len || !cigar_off || !cigar))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (n_alleles < 1) fail(LCTY_ERR_INVALID_INPUT, "no haplotypes");
    const double t0 = now_ms();
    const uint32_t window = prm->window;
    const uint32_t step = prm->step ? prm->step : std::max(window >> 1, 1u);                       // augment.rs:320
    const uint32_t max_edit = static_cast<uint32_t>(std::floor(double(window) * prm->divergence));   // augment.rs:319
    const uint32_t words = (n_alleles + 31) / 32;
    out.words = words;
    out.win_off.assign(n_alleles + 1, 0);
    for (uint32_t a = 0; a < n_alleles; a++) {
        // augment.rs:323; a contig not longer than the window has one window (there `l - window` underflows), a left-out contig none
        uint64_t nw = lengths[a] <= window ? 1 : (uint64_t(lengths[a] - window) + step - 1) / step + 1;
        if (leave_out && leave_out[a]) nw = 0;
        out.win_off[a + 1] = out.win_off[a] + nw;
    }
    out.n_rows = out.win_off[n_alleles];
    if (out.n_rows >= 0xFFFFFFFFull) fail(LCTY_ERR_UNSUPPORTED, "%llu windows: row indices are 32 bits wide", static_cast<unsigned long long>(out.n_rows));
    // the entries that count (augment.rs:332-336), and their global divergence for sides not longer than the window
    std::vector<uint64_t> take;
    take.reserve(n_entries);
    for (uint64_t t = 0; t < n_entries; t++) {
        if (id1[t] >= n_alleles || id2[t] >= n_alleles) fail(LCTY_ERR_INVALID_INPUT, "entry %llu names contig %u of %u", static_cast<unsigned long long>(t), std::max(id1[t], id2[t]), n_alleles);
        if (cigar_off[t + 1] < cigar_off[t]) fail(LCTY_ERR_INVALID_INPUT, "cigar_off is not ascending at %llu", static_cast<unsigned long long>(t));
        if (id1[t] == id2[t] || cigar_off[t + 1] == cigar_off[t]) continue;
        if (leave_out && (leave_out[id1[t]] || leave_out[id2[t]])) continue;
        take.push_back(t);
    }
    ctx->activate();
    hipStream_t s = ctx->stream;
    out.bits.alloc(std::max<uint64_t>(out.n_rows * words, 1));
    out.bits.zero(s);
    DevBuf<uint64_t> d_win_off; DevBuf<uint32_t> d_lens, d_err;
    d_win_off.alloc(n_alleles + 1); d_lens.alloc(n_alleles); d_err.alloc(1);
    d_win_off.upload(out.win_off.data(), n_alleles + 1, s); d_lens.upload(lengths, n_alleles, s); d_err.zero(s);
    hipLaunchKernelGGL(basis_init_kernel, dim3(n_alleles), dim3(256), 0, s, d_win_off.p, words, out.bits.p);
    LCTY_HIP(hipGetLastError());
    // Batches of entries: the CIGAR words of a batch, 17 bytes of columns and two rings per entry. "basis_batch_words" (knob) caps the words
    // of a batch; by default a batch keeps to a quarter of the free device memory, so a PAF larger than the device streams through.
    const uint32_t ring_len = static_cast<uint32_t>(std::min<uint64_t>((uint64_t(window) + step - 1) / step + 2, 0x7FFFFFFFull));
    size_t free_b = 0, total_b = 0;
    LCTY_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t per_entry = 17 + 8ull * ring_len;
    uint64_t budget = std::max<uint64_t>(free_b / 4, 1ull << 20);
    const int64_t knob_words = ctx->knob("basis_batch_words", 0);
    if (knob_words > 0) budget = uint64_t(knob_words) * 4;
    DevBuf<uint32_t> d_cigar, d_id1, d_id2, d_ring; DevBuf<uint64_t> d_off; DevBuf<uint8_t> d_short;
    std::vector<uint32_t> b_id1, b_id2; std::vector<uint64_t> b_off; std::vector<uint8_t> b_short; std::vector<uint32_t> b_cigar;
    for (size_t at = 0; at < take.size();) {
        b_id1.clear(); b_id2.clear(); b_short.clear(); b_cigar.clear(); b_off.assign(1, 0);
        uint64_t used = 0;
        while (at < take.size() && b_id1.size() < (1u << 30)) {
            const uint64_t t = take[at], nw = cigar_off[t + 1] - cigar_off[t];
            const uint64_t cost = knob_words > 0 ? 4 * nw : 4 * nw + per_entry;
            if (!b_id1.empty() && used + cost > budget) break;                    // an entry larger than the budget has a batch of its own
            used += cost;
            b_id1.push_back(id1[t]); b_id2.push_back(id2[t]);
            // PafEntry::divergence().unwrap_or(1.0) <= args.divergence (paf.rs:201-208, augment.rs:303, 336): one IEEE division
            const double gdiv = aln_len[t] == 0 ? 1.0 : double(aln_len[t] - n_matches[t]) / double(aln_len[t]);
            b_short.push_back(gdiv <= prm->divergence ? 1 : 0);
            b_cigar.insert(b_cigar.end(), cigar + cigar_off[t], cigar + cigar_off[t + 1]);
            b_off.push_back(b_cigar.size());
            at++;
        }
        const uint32_t nb = static_cast<uint32_t>(b_id1.size());
        d_cigar.ensure_slack(b_cigar.size()); d_id1.ensure_slack(nb); d_id2.ensure_slack(nb); d_off.ensure_slack(nb + 1); d_short.ensure_slack(nb);
        d_ring.ensure_slack(2ull * nb * ring_len);
        d_cigar.upload(b_cigar.data(), b_cigar.size(), s); d_id1.upload(b_id1.data(), nb, s); d_id2.upload(b_id2.data(), nb, s);
        d_off.upload(b_off.data(), nb + 1, s); d_short.upload(b_short.data(), nb, s);
        hipLaunchKernelGGL(basis_windows_kernel, dim3(2 * nb), dim3(64), 0, s, d_cigar.p, d_off.p, d_id1.p, d_id2.p, d_short.p, d_lens.p, d_win_off.p,
                           window, step, max_edit, ring_len, d_ring.p, words, out.bits.p, d_err.p);
        LCTY_HIP(hipGetLastError());
        LCTY_HIP(hipStreamSynchronize(s));                                        // the host vectors are filled again
        st.bytes_h2d += 4 * b_cigar.size() + 17ull * nb;
        st.n_batches++;
    }
    uint32_t err = 0;
    d_err.download(&err, 1, s);
    LCTY_HIP(hipStreamSynchronize(s));
    if (err & kErrOp) fail(LCTY_ERR_INVALID_DATA, "a CIGAR holds an operation other than M, =, X, I, D");
    if (err & kErrLen) fail(LCTY_ERR_INVALID_DATA, "a CIGAR does not cover its contig's length");
    st.n_entries += take.size(); st.n_walks += 2 * take.size(); st.n_rows_raw = out.n_rows;
    st.windows_ms += now_ms() - t0;
}

// unique rows in canonical order (popcount, then the words as numbers from the last word down), with `minimal` only those without a
// subset among them. rows: device, [n_rows][words].
void basis_constraints_device(lcty_ctx* ctx, const uint32_t* d_rows, uint64_t n_rows, uint32_t words, bool minimal, std::vector<uint32_t>& out,
                              lcty_basis_stats& st) {
    ctx->activate();
    hipStream_t s = ctx->stream;
    out.clear();
    double t0 = now_ms();
    if (n_rows == 0) { st.n_rows_unique = st.n_rows_minimal = 0; return; }
    if (n_rows >= 0xFFFFFFFFull) fail(LCTY_ERR_UNSUPPORTED, "%llu rows: row indices are 32 bits wide", static_cast<unsigned long long>(n_rows));
    uint64_t cap = 64;
    while (cap < 2 * n_rows) cap <<= 1;
    DevBuf<uint32_t> table, n_keep, uniq; DevBuf<uint8_t> keep;
    table.alloc(cap); keep.alloc(n_rows); n_keep.alloc(2);
    table.zero(s); keep.zero(s); n_keep.zero(s);
    const dim3 grid(static_cast<uint32_t>((n_rows + 3) / 4));
    hipLaunchKernelGGL(basis_dedup_kernel, grid, dim3(256), 0, s, d_rows, n_rows, words, table.p, cap - 1, keep.p, n_keep.p);
    LCTY_HIP(hipGetLastError());
    uint32_t U = 0;
    n_keep.download(&U, 1, s);
    LCTY_HIP(hipStreamSynchronize(s));
    table.release();
    uniq.alloc(uint64_t(U) * words);
    hipLaunchKernelGGL(basis_compact_kernel, grid, dim3(256), 0, s, d_rows, n_rows, words, keep.p, n_keep.p + 1, uniq.p);
    LCTY_HIP(hipGetLastError());
    std::vector<uint32_t> h(uint64_t(U) * words);
    uniq.download(h.data(), h.size(), s);
    LCTY_HIP(hipStreamSynchronize(s));
    st.bytes_d2h += 4 * h.size();
    // canonical order on the host: the compaction's order depends on timing, and the search's answer must not
    std::vector<uint32_t> order(U), pop(U);
    for (uint32_t r = 0; r < U; r++) { order[r] = r; pop[r] = popcount_row(h.data() + uint64_t(r) * words, words); }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (pop[a] != pop[b]) return pop[a] < pop[b];
        const uint32_t* x = h.data() + uint64_t(a) * words; const uint32_t* y = h.data() + uint64_t(b) * words;
        for (uint32_t k = words; k-- > 0;) if (x[k] != y[k]) return x[k] < y[k];
        return false;
    });
    std::vector<uint32_t> sorted(h.size());
    for (uint32_t r = 0; r < U; r++) memcpy(sorted.data() + uint64_t(r) * words, h.data() + uint64_t(order[r]) * words, 4ull * words);
    st.n_rows_unique = U;
    st.dedup_ms += now_ms() - t0;
    if (!minimal) { out.swap(sorted); st.n_rows_minimal = U; return; }
    t0 = now_ms();
    std::vector<uint32_t> limit(U);
    for (uint32_t r = 0, first = 0; r < U; r++) {
        if (r && pop[order[r]] != pop[order[r - 1]]) first = r;
        limit[r] = first;
    }
    if (4ull * words * 4 > 60000) fail(LCTY_ERR_UNSUPPORTED, "%u haplotypes: a row does not fit the subsume kernel's LDS", words * 32);
    DevBuf<uint32_t> d_limit; DevBuf<uint8_t> d_implied;
    d_limit.alloc(U); d_implied.alloc(U);
    uniq.upload(sorted.data(), sorted.size(), s); d_limit.upload(limit.data(), U, s);
    hipLaunchKernelGGL(basis_subsume_kernel, dim3((U + 3) / 4), dim3(256), 4 * words * sizeof(uint32_t), s, uniq.p, U, words, d_limit.p, d_implied.p);
    LCTY_HIP(hipGetLastError());
    std::vector<uint8_t> implied(U);
    d_implied.download(implied.data(), U, s);
    LCTY_HIP(hipStreamSynchronize(s));
    st.bytes_h2d += 4 * sorted.size() + 4ull * U; st.bytes_d2h += U;
    for (uint32_t r = 0; r < U; r++)
        if (!implied[r]) out.insert(out.end(), sorted.begin() + uint64_t(r) * words, sorted.begin() + uint64_t(r + 1) * words);
    st.n_rows_minimal = out.size() / words;
    st.subsume_ms += now_ms() - t0;
}

}  // namespace lcty

extern "C" {

void lcty_basis_params_default(lcty_basis_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->divergence = 0.01; p->window = 250;      // augment.rs:59-60
    p->step = 0;                                // augment.rs:61, 320: not given = max(window >> 1, 1)
    p->minimal = 1;
    p->node_limit = 2000000;
}

int32_t lcty_basis_select(uint32_t n_alleles, uint64_t n_rows, const uint32_t* rows, uint64_t node_limit, uint32_t* ids, uint32_t* n_ids, uint32_t* bound,
                          int32_t* optimal, uint64_t* nodes) {
    return guarded([&] {
        if (!ids || !n_ids || (n_rows && !rows)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_alleles < 1) fail(LCTY_ERR_INVALID_INPUT, "no haplotypes");
        bool empty = false;
        BasisAnswer ans = basis_search(n_alleles, n_rows, rows, node_limit, &empty);
        if (empty) fail(LCTY_ERR_INVALID_INPUT, "a row without a haplotype cannot be hit");
        memcpy(ids, ans.ids.data(), 4 * ans.ids.size());
        *n_ids = static_cast<uint32_t>(ans.ids.size());
        if (bound) *bound = ans.bound;
        if (optimal) *optimal = ans.optimal ? 1 : 0;
        if (nodes) *nodes = ans.nodes;
    });
}

int32_t lcty_basis_tag(const lcty_basis_params* params, const char* leave_out, uint32_t n_leave_out, char* out, uint64_t cap) {
    return guarded([&] {
        if (!out || (n_leave_out && !leave_out)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        basis_check_params(params);
        // math::fmt_signif(divergence, 5) (src/math/mod.rs:140-174)
        std::string tag = "x";
        const double x = params->divergence;
        if (x == 0.0) tag += "0";
        else {
            const int shift = static_cast<int>(std::floor(std::log10(std::fabs(x)))) + 1 - 5;
            char buf[400];
            if (shift < 0) {
                snprintf(buf, sizeof(buf), "%.*f", -shift, x);
                std::string t = buf;
                while (!t.empty() && t.back() == '0') t.pop_back();
                while (!t.empty() && t.back() == '.') t.pop_back();
                tag += t;
            } else {
                const double fct = std::pow(10.0, shift);
                snprintf(buf, sizeof(buf), "%lld", static_cast<long long>(std::round(std::round(x / fct) * fct)));
                tag += buf;
            }
        }
        auto pretty = [](uint32_t v) {                                    // ext::fmt::PrettyU32 (src/ext/fmt.rs:93-113)
            if (v == 0) return std::string("0");
            if (v == UINT32_MAX) return std::string("inf");
            if (v % 1000000000u == 0) return std::to_string(v / 1000000000u) + "G";
            if (v % 1000000u == 0) return std::to_string(v / 1000000u) + "M";
            if (v % 1000u == 0) return std::to_string(v / 1000u) + "k";
            return std::to_string(v);
        };
        if (params->window == UINT32_MAX) tag += "-global";
        else {
            tag += "-w" + pretty(params->window);
            if (params->step) tag += "-s" + pretty(params->step);
        }
        const char* nm = leave_out;
        for (uint32_t i = 0; i < n_leave_out; i++) {
            tag += i ? "," : "-lo";
            tag += nm;
            nm += strlen(nm) + 1;
        }
        if (tag.size() >= 128)                                                // augment.rs:273-275
            fail(LCTY_ERR_RUNTIME, "Automatic tag name is too long (%zu chars.), please provide tag using --tag", tag.size());
        if (cap < tag.size() + 1) fail(LCTY_ERR_INVALID_INPUT, "tag buffer too small (%llu < %zu)", static_cast<unsigned long long>(cap), tag.size() + 1);
        memcpy(out, tag.c_str(), tag.size() + 1);
    });
}

int32_t lcty_basis_windows(lcty_ctx* ctx, uint32_t n_alleles, const uint32_t* lengths, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2,
                           const uint32_t* n_matches, const uint32_t* aln_len, const uint64_t* cigar_off, const uint32_t* cigar, const uint8_t* leave_out,
                           const lcty_basis_params* params, uint64_t* win_off, uint32_t** rows, lcty_basis_stats* stats) {
    return guarded([&] {
        if (rows) *rows = nullptr;
        if (!ctx || !win_off || !rows) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_basis_stats st{};
        const double t0 = now_ms();
        BasisRows R;
        basis_windows_device(ctx, n_alleles, lengths, n_entries, id1, id2, n_matches, aln_len, cigar_off, cigar, leave_out, params, R, st);
        Handoff h;
        uint32_t* bits = from(h, R.bits, R.n_rows * R.words, ctx->stream);
        LCTY_HIP(hipStreamSynchronize(ctx->stream));
        st.bytes_d2h += 4 * R.n_rows * R.words;
        memcpy(win_off, R.win_off.data(), 8ull * (n_alleles + 1));
        *rows = bits; h.commit();
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

int32_t lcty_basis_constraints(lcty_ctx* ctx, uint32_t n_alleles, uint64_t n_rows, const uint32_t* rows, int32_t minimal, uint64_t* n_out, uint32_t** out,
                               lcty_basis_stats* stats) {
    return guarded([&] {
        if (out) *out = nullptr;
        if (n_out) *n_out = 0;
        if (!ctx || !n_out || !out || (n_rows && !rows)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_alleles < 1) fail(LCTY_ERR_INVALID_INPUT, "no haplotypes");
        lcty_basis_stats st{};
        const double t0 = now_ms();
        const uint32_t words = (n_alleles + 31) / 32;
        ctx->activate();
        DevBuf<uint32_t> d;
        d.alloc(std::max<uint64_t>(n_rows * words, 1));
        d.upload(rows, n_rows * words, ctx->stream);
        st.bytes_h2d += 4 * n_rows * words; st.n_rows_raw = n_rows;
        std::vector<uint32_t> res;
        basis_constraints_device(ctx, d.p, n_rows, words, minimal != 0, res, st);
        Handoff h;
        *out = h.copy(res); *n_out = res.size() / words; h.commit();
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

int32_t lcty_basis_build(lcty_ctx* ctx, uint32_t n_alleles, const uint32_t* lengths, uint64_t n_entries, const uint32_t* id1, const uint32_t* id2,
                         const uint32_t* n_matches, const uint32_t* aln_len, const uint64_t* cigar_off, const uint32_t* cigar, const uint8_t* leave_out,
                         const lcty_basis_params* params, uint32_t* ids, uint32_t* n_ids, uint32_t* bound, int32_t* optimal, lcty_basis_stats* stats) {
    return guarded([&] {
        if (!ctx || !ids || !n_ids) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_basis_stats st{};
        const double t0 = now_ms();
        std::vector<uint32_t> res;
        uint32_t words = 0;
        {
            BasisRows R;
            basis_windows_device(ctx, n_alleles, lengths, n_entries, id1, id2, n_matches, aln_len, cigar_off, cigar, leave_out, params, R, st);
            words = R.words;
            basis_constraints_device(ctx, R.bits.p, R.n_rows, R.words, params->minimal != 0, res, st);
        }
        const double t1 = now_ms();
        bool empty = false;
        BasisAnswer ans = basis_search(n_alleles, res.size() / words, res.data(), params->node_limit, &empty);
        if (empty) fail(LCTY_ERR_RUNTIME, "a row without a haplotype");
        st.search_ms = now_ms() - t1;
        st.n_forced = ans.n_forced; st.n_nodes = ans.nodes;
        memcpy(ids, ans.ids.data(), 4 * ans.ids.size());
        *n_ids = static_cast<uint32_t>(ans.ids.size());
        if (bound) *bound = ans.bound;
        if (optimal) *optimal = ans.optimal ? 1 : 0;
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

}  // extern "C"
