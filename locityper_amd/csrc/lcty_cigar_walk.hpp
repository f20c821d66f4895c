// lcty_cigar_walk.hpp — walks over CIGARs that need no memory layout and no sequence type, one definition each: the operation classes
// and double_cigar_move_and_shift (cigar.rs:1422-1466) that alignment recovery (lcty_transfer_device.hpp) and the transitive route
// (lcty_align.hip) both step with, the three predicates of Cigar::optimize (cigar.rs:1167-1237) that recovery's resumable pass and the
// straight pass below share, and the two walks of the transitive route as templates over a visitor: walk_transitive
// (transfer_alignment::<true>, cigar.rs:1248-1368) and walk_optimize. v.item(op, len) takes a copied operation, v.stretch(i1, i2, j1,
// j2) is smart_align of reference [i1, i2) and query [j1, j2). Compiles without HIP, as lcty_gotoh.hpp does:
// scripts/align_probe_host.cpp is the host instantiation.
#pragma once

#include "lcty_gotoh.hpp"

#ifdef __HIPCC__
#define LCTY_WALK_FN __host__ __device__ inline
#else
#define LCTY_WALK_FN inline
#endif

namespace lcty {
namespace xfer {

using gotoh::OP_I; using gotoh::OP_D; using gotoh::OP_S; using gotoh::OP_H; using gotoh::OP_EQ; using gotoh::OP_X;

// consumes the query: M I S = X; consumes the reference: M D = X (bit `op` of a mask; operations are 4-bit codes)
LCTY_GOTOH_FN bool cons_q(uint32_t op) { return ((0x193u >> (op & 15u)) & 1u) != 0; }
LCTY_GOTOH_FN bool cons_r(uint32_t op) { return ((0x185u >> (op & 15u)) & 1u) != 0; }
LCTY_GOTOH_FN uint32_t op_invert(uint32_t op) {                                // Operation::invert, cigar.rs:147-159
    return (op == OP_I || op == OP_S) ? OP_D : (op == OP_D ? OP_I : op);
}

// double_cigar_move_and_shift (cigar.rs:1422-1466)
LCTY_GOTOH_FN uint32_t cons_class(uint32_t op) { return cons_q(op) && cons_r(op) ? 0u : (cons_q(op) ? 1u : 2u); }
LCTY_WALK_FN uint32_t double_move(uint32_t op1, uint32_t op2, uint32_t& pos1, uint32_t& rem1, uint32_t& pos2, uint32_t& rem2) {
    // bit 0 read moves, 1 read CIGAR shifts, 2 haplotype moves, 3 haplotype CIGAR shifts; index = class(op1) * 3 + class(op2)
    // the nine cases as nibbles of one constant, case 0 lowest: {0xF, 0xB, 0xC, 0x3, 0x3, 0xF, 0xE, 0xA, 0xC}
    const uint32_t f = static_cast<uint32_t>(0xCAEF33CBFull >> (4u * (cons_class(op1) * 3 + cons_class(op2)))) & 0xFu;
    const bool rs = f & 2u, hs = f & 8u;
    const uint32_t shift = (rs && (!hs || rem1 <= rem2)) ? rem1 : rem2;
    pos1 += (f & 1u) ? shift : 0; rem1 -= rs ? shift : 0;
    pos2 += (f & 4u) ? shift : 0; rem2 -= hs ? shift : 0;
    return shift;
}

// Cigar::optimize, the three decisions of its loop: an item is an anchor (1188); what an item between anchors adds to the flag, 1 a
// deletion seen, 2 an insertion (1217); a stretch between anchors is aligned again (1192, 1223)
LCTY_GOTOH_FN bool opt_is_anchor(uint32_t op, uint32_t len, uint32_t anchor_size) { return cons_q(op) && cons_r(op) && len >= anchor_size; }
LCTY_GOTOH_FN uint32_t opt_gap_flag(uint32_t op) { return (cons_q(op) ? 0u : 1u) | ((cons_r(op) ? 0u : 1u) << 1); }
LCTY_GOTOH_FN bool opt_realigns(uint32_t flag, uint32_t qshift, uint32_t rshift, uint32_t max_gap) { return flag == 3 && !(max_gap < qshift) && !(max_gap < rshift); }

}  // namespace xfer

namespace trwalk {
using gotoh::OP_EQ;

struct Item { uint32_t op, len; };
struct TrCig {
    const uint32_t* w; uint32_t n; bool inv;                                   // raw BAM words; inv: CigarDirection RefToQuery (I and D change places)
    LCTY_GOTOH_FN Item item(uint32_t x) const {
        const uint32_t v = w[x];
        return Item{inv ? xfer::op_invert(v & 15u) : (v & 15u), v >> 4};
    }
    LCTY_GOTOH_FN bool full_match() const { return n == 1 && (w[0] & 15u) == OP_EQ; }      // cigar.rs:514-516
};
constexpr uint32_t kAnchorMargin = 5;                                         // ANCHOR_MARGIN, cigar.rs:1305
constexpr uint32_t kOptGap = 1000, kOptAnchor = 51;                           // MAX_OPTIMIZATION_GAP, OPTIMIZATION_ANCHOR, cigar.rs:1358-1359

// true: one of the two alignments is a full match and the other one is the answer as it stands (1274-1278; no optimize follows)
template <class V>
LCTY_WALK_FN bool walk_transitive(const TrCig& ij, const TrCig& jk, uint32_t len_i, uint32_t len_k, uint32_t anchor_size, V& v) {
    if (ij.full_match()) { for (uint32_t x = 0; x < jk.n; x++) { const Item it = jk.item(x); v.item(it.op, it.len); } return true; }
    if (jk.full_match()) { for (uint32_t x = 0; x < ij.n; x++) { const Item it = ij.item(x); v.item(it.op, it.len); } return true; }
    uint32_t last1 = 0, pos1 = 0, last2 = 0, pos2 = 0;
    if (ij.n && jk.n) {
        uint32_t x1 = 0, x2 = 0;
        Item t = jk.item(x2++);
        uint32_t op2 = t.op, len2 = t.len, rem2 = t.len;
        t = ij.item(x1++);
        uint32_t op1 = t.op, len1 = t.len, rem1 = t.len;
        for (;;) {
            int add = -1;
            const bool e1 = op1 == OP_EQ, e2 = op2 == OP_EQ;
            if (e1 && e2) { if ((rem1 < rem2 ? rem1 : rem2) >= anchor_size) add = OP_EQ; }
            else if (e1 && !e2) { if (rem1 >= anchor_size && len1 - rem1 >= kAnchorMargin) add = static_cast<int>(op2); }
            else if (!e1 && e2) { if (rem2 >= anchor_size && len2 - rem2 >= kAnchorMargin) add = static_cast<int>(op1); }
            if (add >= 0) v.stretch(last2, pos2, last1, pos1);
            const uint32_t shift = xfer::double_move(op1, op2, pos1, rem1, pos2, rem2);
            if (add >= 0) { v.item(static_cast<uint32_t>(add), shift); last1 = pos1; last2 = pos2; }
            if (rem1 == 0) {
                if (x1 == ij.n) break;
                t = ij.item(x1++); op1 = t.op; len1 = rem1 = t.len;
            }
            if (rem2 == 0) {
                if (x2 == jk.n) break;
                t = jk.item(x2++); op2 = t.op; len2 = rem2 = t.len;
            }
        }
    }
    if (last1 != len_i || last2 != len_k) v.stretch(last2, len_k, last1, len_i);
    return false;
}

// Cigar::optimize over the items w[0, n) in one straight pass: a stretch between two anchors that holds both an insertion and a
// deletion, neither side longer than max_gap, is aligned again (smart_align without a threshold: the visitor's max_gap is all ones);
// everything else is copied. (lcty_transfer_device.hpp has the resumable form, for wavefronts whose 64 lanes meet at one aligner call.)
template <class V>
LCTY_WALK_FN void walk_optimize(const uint32_t* w, uint32_t n, uint32_t max_gap, uint32_t anchor_size, V& v) {
    uint32_t i = 0, qpos1 = 0, rpos1 = 0, qpos2 = 0, rpos2 = 0, flag = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t op = w[j] & 15u, len = w[j] >> 4;
        if (xfer::opt_is_anchor(op, len, anchor_size)) {
            if (xfer::opt_realigns(flag, qpos2 - qpos1, rpos2 - rpos1, max_gap)) v.stretch(rpos1, rpos2, qpos1, qpos2);
            else for (uint32_t x = i; x < j; x++) v.item(w[x] & 15u, w[x] >> 4);
            v.item(op, len);
            qpos2 += len; rpos2 += len; qpos1 = qpos2; rpos1 = rpos2; flag = 0;
            i = j + 1;
        } else {
            qpos2 += xfer::cons_q(op) ? len : 0; rpos2 += xfer::cons_r(op) ? len : 0;
            flag |= xfer::opt_gap_flag(op);
        }
    }
    if (xfer::opt_realigns(flag, qpos2 - qpos1, rpos2 - rpos1, max_gap)) v.stretch(rpos1, rpos2, qpos1, qpos2);
    else for (uint32_t x = i; x < n; x++) v.item(w[x] & 15u, w[x] >> 4);
}

}  // namespace trwalk
}  // namespace lcty
