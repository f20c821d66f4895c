// lcty_gotoh.hpp — the gap-affine (Gotoh) aligner of Penalties::default and what stands around it in src/seq/wfa.rs, one definition
// each: the penalties and operation codes, the cell of the recurrence with its tie rule, the end state and the step of the walk
// back, align_simple, the straight comparison of a short stretch and the routing of smart_align. No state, no memory layout, no
// sequence type: the callers keep their rows, direction bytes and bases where they are (lane scratch strided by 64, registers,
// plain bytes, host vectors) and hand values in. WFA2-lib computes the same optimum; its choice among co-optimal alignments is not
// pinned anywhere, ours is decided HERE: walking back from the end, diagonal before deletion before insertion, a gap is extended
// before it is opened. A kernel that needs one of these calls it here and does not restate it.
// Compiles without HIP: scripts/align_probe_host.cpp is the host instantiation.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LCTY_GOTOH_FN __host__ __device__ __forceinline__
#else
#define LCTY_GOTOH_FN inline __attribute__((always_inline))
#endif

namespace lcty {
namespace gotoh {

constexpr uint32_t OP_I = 1, OP_D = 2, OP_S = 4, OP_H = 5, OP_EQ = 7, OP_X = 8;         // BAM operation codes
constexpr int PEN_X = 4, PEN_O = 6, PEN_E = 1;                                          // Penalties::default (wfa.rs:30-38)
constexpr int INF32 = 1 << 28;
constexpr uint32_t SAFE_MISMATCH = (2 * PEN_O + 2 * PEN_E) / PEN_X;                     // wfa.rs:212
LCTY_GOTOH_FN int gap_score(uint32_t len) { return -PEN_O - static_cast<int>(len) * PEN_E; }       // a gap of len > 0 bases, as a score

LCTY_GOTOH_FN int32_t min2(int32_t a, int32_t b) { return b < a ? b : a; }

// The three matrices at one cell: the best penalty of an alignment that ends there in a diagonal step (m), a deletion (d: a
// reference base against nothing) or an insertion (i); INF32 = none.
struct Cell { int32_t m, d, i; };
enum : uint32_t { ST_M = 0, ST_D = 1, ST_I = 2 };            // the matrix a walk back stands in

// Cell (a, b) out of `up` (a - 1, b), `left` (a, b - 1) and `diag` (a - 1, b - 1). has_up: a > 0, has_left: b > 0 (what lies beyond
// the border is not looked at); origin: the cell starts an alignment for free (a == 0 && b == 0, or a border cell where a prefix is
// skipped for free); sub: the cost of the diagonal step into this cell (0 or minus the match bonus for equal bases, PEN_X otherwise).
// *dir = dm | dd << 2 | di << 4, the matrix each of the three values came from: ties of m go to m, then d, then i; d and i extend a
// gap before they open one, and open it from m before the other gap.
LCTY_GOTOH_FN Cell cell(const Cell& up, const Cell& left, const Cell& diag, int32_t sub, bool has_up, bool has_left, bool origin, uint32_t* dir) {
    int32_t cm = origin ? 0 : INF32, cd = INF32, ci = INF32;
    uint32_t dm = 3, dd = 0, di = 0;
    if (has_up && has_left) {
        const int32_t best = min2(diag.m, min2(diag.d, diag.i));
        if (best < INF32) {
            const int32_t v = best + sub;
            if (v < cm) { cm = v; dm = diag.m == best ? 0u : (diag.d == best ? 1u : 2u); }
        }
    }
    if (has_up) {
        int32_t v = min2(up.m, up.i) + PEN_O + PEN_E;
        if (up.d + PEN_E < v) v = up.d + PEN_E;
        if (v < INF32) { cd = v; dd = (up.d + PEN_E == v) ? 1u : (up.m <= up.i ? 0u : 2u); }
    }
    if (has_left) {
        int32_t v = min2(left.m, left.d) + PEN_O + PEN_E;
        if (left.i + PEN_E < v) v = left.i + PEN_E;
        if (v < INF32) { ci = v; di = (left.i + PEN_E == v) ? 2u : (left.m <= left.d ? 0u : 1u); }
    }
    *dir = dm | (dd << 2) | (di << 4);
    return Cell{cm, cd, ci};
}

LCTY_GOTOH_FN int32_t best_of(const Cell& c) { return min2(c.m, min2(c.d, c.i)); }
// where the walk back begins at the cell an alignment ends in
LCTY_GOTOH_FN uint32_t end_state(const Cell& e) { return (e.m <= e.d && e.m <= e.i) ? ST_M : (e.d <= e.i ? ST_D : ST_I); }
// One step of the walk back. The state IS the step taken at cell (a, b): ST_M a diagonal one (a--, b--; '=' or 'X' by the caller's
// bases), ST_D a deletion (a--), ST_I an insertion (b--). Returned: the state at the cell the step leads to, out of (a, b)'s byte.
LCTY_GOTOH_FN uint32_t back_step(uint32_t st, uint32_t dir) {
    if (st == ST_M) return dir & 3u;
    if (st == ST_D) { const uint32_t dd = (dir >> 2) & 3u; return dd == 1 ? ST_D : (dd == 0 ? ST_M : ST_I); }
    const uint32_t di = (dir >> 4) & 3u;
    return di == 2 ? ST_I : (di == 0 ? ST_M : ST_D);
}

// Penalties::align_simple (wfa.rs:49-84) of a reference stretch of n and a query stretch of m bases, both at least one: the
// difference of the lengths as one gap in front, then base against base. same(i, j): reference base i equals query base j (counted
// from the start of the stretches); push(op, len) takes the gap and then maximal runs of '=' / 'X'. Returns the score.
template <class Same, class Push>
LCTY_GOTOH_FN int align_simple(uint32_t n, uint32_t m, Same&& same, Push&& push) {
    const uint32_t len = n < m ? n : m, i0 = n - len, j0 = m - len;
    int score = 0;
    if (n < m) { push(OP_I, m - n); score = gap_score(m - n); }
    else if (n > m) { push(OP_D, n - m); score = gap_score(n - m); }
    bool curr_match = same(i0, j0);
    uint32_t curr_len = 1;
    for (uint32_t t = 1; t < len; t++) {
        const bool eq = same(i0 + t, j0 + t);
        if (eq != curr_match) {
            push(curr_match ? OP_EQ : OP_X, curr_len);
            score -= curr_match ? 0 : PEN_X * static_cast<int>(curr_len);
            curr_match = !curr_match; curr_len = 1;
        } else curr_len++;
    }
    push(curr_match ? OP_EQ : OP_X, curr_len);
    score -= curr_match ? 0 : PEN_X * static_cast<int>(curr_len);
    return score;
}

// two stretches of the same n <= SAFE_MISMATCH bases, base against base (wfa.rs:309-317): no gap can pay. push(op, 1) per base.
template <class Same, class Push>
LCTY_GOTOH_FN int align_straight(uint32_t n, Same&& same, Push&& push) {
    int ndiff = 0;
    for (uint32_t t = 0; t < n; t++) {
        const bool eq = same(t, t);
        push(eq ? OP_EQ : OP_X, 1u);
        ndiff -= !eq;
    }
    return ndiff * PEN_X;
}
struct NoPush { LCTY_GOTOH_FN void operator()(uint32_t, uint32_t) const {} };            // the score alone

// smart_align (wfa.rs:280-321) for a reference stretch of n and a query stretch of m bases; max_gap 0xFFFFFFFF = no threshold.
// NONE: nothing to do; DEL / INS: one gap, gap_score(n) / gap_score(m); SIMPLE: align_simple; STRAIGHT: align_straight;
// EXACT: the aligner (a caller whose scratch cannot take the stretch decides that behind this answer).
enum Route : uint32_t { ROUTE_NONE = 0, ROUTE_DEL, ROUTE_INS, ROUTE_SIMPLE, ROUTE_STRAIGHT, ROUTE_EXACT };
LCTY_GOTOH_FN Route route(uint32_t n, uint32_t m, uint32_t max_gap) {
    if (n > 0 && m > 0) {
        if (max_gap < n || max_gap < m) return ROUTE_SIMPLE;
        if (n == m && n <= SAFE_MISMATCH) return ROUTE_STRAIGHT;
        return ROUTE_EXACT;
    }
    return n > 0 ? ROUTE_DEL : (m > 0 ? ROUTE_INS : ROUTE_NONE);
}

}  // namespace gotoh
}  // namespace lcty
