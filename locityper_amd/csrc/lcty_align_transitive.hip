// lcty_align_transitive.hip — the schedule of lcty_align_haplotypes_transitive: `locityper align` with --tr-div > 0, the single-thread
// TransitiveStrategy of src/seq/align.rs:452-514 over the pairs in input order. Once a haplotype k has a close neighbour j and i-j is
// aligned, i-k is composed out of i-j and j-k (Cigar::find_transitive_alignment) instead of being aligned along a backbone. Which
// pair goes which way depends on the pairs before it, so the pairs run in ROUNDS: the longest prefix of the remaining pairs in which
// no pair reads what an earlier pair of the prefix writes. The host keeps a mirror of `closest` (id and divergence) and of which
// alignments exist, and decides a whole round from it; the device (lcty_align.hip, through lcty_align_internal.hpp) aligns the round's
// backbone pairs in the usual batches and its transitive pairs with the transitive kernels, every finished CIGAR stays in the store
// on the device, and only the counts of a round come back. Nothing is tried twice; any device error ends the call.
#include "lcty_common.hpp"
#include "lcty_align_internal.hpp"

#include <algorithm>
#include <unordered_map>
#include <unordered_set>

using namespace lcty;

extern "C" {

void lcty_align_tr_params_default(lcty_align_tr_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->transitive_div = 0.01; p->transitive_anchor = 101;                      // align.rs:59-60
}

void lcty_align_tr_out_free(lcty_align_tr_out* o) {
    if (!o) return;
    free(o->route); free(o->via);
    memset(o, 0, sizeof(*o));
}

int32_t lcty_align_haplotypes_transitive(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref_id,
                                         const uint32_t* query_id, const uint8_t* against, const lcty_align_params* params,
                                         const lcty_align_tr_params* tr_params, lcty_align_out* out, lcty_align_tr_out* tr_out, lcty_align_stats* stats,
                                         lcty_align_tr_stats* tr_stats) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (tr_out) memset(tr_out, 0, sizeof(*tr_out));
        if (!ctx || !params || !tr_params || !out || !tr_out || (n_pairs && (!ref_id || !query_id))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (tr_stats) memset(tr_stats, 0, sizeof(*tr_stats));
        if (tr_params->transitive_div != tr_params->transitive_div || tr_params->transitive_div > 1.0)
            fail(LCTY_ERR_INVALID_INPUT, "Transitive divergence (%g) must be at most 1", tr_params->transitive_div);
        if (tr_params->transitive_anchor < 1) fail(LCTY_ERR_INVALID_INPUT, "Transitive anchor size must be at least 1");
        std::vector<uint8_t> route(std::max<uint64_t>(n_pairs, 1), 0);
        std::vector<uint32_t> via(std::max<uint64_t>(n_pairs, 1), 0xFFFFFFFFu);
        lcty_align_out o{}; lcty_align_tr_out t{}; Handoff h;
        // align.rs:784: no acceleration without a positive divergence or below 16 pairs — the backbone route as it stands
        if (!(tr_params->transitive_div > 0.0) || n_pairs < 16) {
            t.route = h.copy(route); t.via = h.copy(via);                     // before the call: nothing fails once it has filled o
            const int32_t rc = lcty_align_haplotypes(ctx, n_seqs, seqs, seq_off, n_pairs, ref_id, query_id, against, params, &o, stats);
            if (rc != LCTY_OK) fail(rc, "%s", lcty_last_error());
            for (uint64_t x = 0; x < n_pairs; x++) t.route[x] = o.aligned[x] ? 1 : 0;
            *out = o; *tr_out = t; h.commit();
            return;
        }
        align::Session ses(ctx, n_seqs, seqs, seq_off, n_pairs, ref_id, query_id, against, params);
        const uint8_t* aligned = ses.aligned();
        size_t free_b = 0, total_b = 0;
        LCTY_HIP(hipMemGetInfo(&free_b, &total_b));
        // the store of finished CIGARs: an eighth of the free device memory, at least 64 MB, unless the knob says otherwise (megabytes)
        const int64_t store_mb = ctx->knob("align_cigar_store_mb", static_cast<int64_t>(std::max<uint64_t>(free_b / 8, 64ull << 20) >> 20));
        ses.open(static_cast<uint64_t>(store_mb) << 18);

        constexpr uint32_t NONE = 0xFFFFFFFFu;
        auto key = [](uint32_t a, uint32_t b) { return (static_cast<uint64_t>(std::min(a, b)) << 32) | std::max(a, b); };
        std::vector<uint32_t> c_id(n_seqs, NONE); std::vector<double> c_dv(n_seqs, 0.0); std::vector<uint64_t> c_pair(n_seqs, 0);     // the mirror of `closest`
        std::unordered_map<uint64_t, uint64_t> cell;                           // {i, j} -> the input pair whose CIGAR it is
        std::vector<uint64_t> w_closest(n_seqs, 0);                            // the round (from 1) that writes closest[q]
        std::unordered_set<uint64_t> w_cell;
        std::vector<uint64_t> bb, members; std::vector<align::TrTask> tr;
        uint64_t n_rounds = 0;
        for (uint64_t x0 = 0, round = 1; x0 < n_pairs; round++) {
            w_cell.clear(); bb.clear(); tr.clear(); members.clear();
            uint64_t x = x0;
            for (; x < n_pairs; x++) {
                if (!aligned[x]) continue;                                     // reads and writes nothing
                const uint32_t k = ref_id[x], i = query_id[x];
                if (w_closest[k] == round || w_closest[i] == round) break;
                uint8_t rt = 1; uint32_t j = NONE; uint64_t ij = 0, jk = 0;
                bool cut = false;
                if (c_id[k] != NONE) {                                         // first clause: closest[k] = j and {i, j} is aligned
                    const uint64_t kk = key(i, c_id[k]);
                    if (w_cell.count(kk)) cut = true;
                    else { const auto it = cell.find(kk); if (it != cell.end()) { rt = 2; j = c_id[k]; ij = it->second; jk = c_pair[k]; } }
                }
                if (!cut && rt == 1 && c_id[i] != NONE) {                      // second clause: closest[i] = j and {k, j} is aligned
                    const uint64_t kk = key(k, c_id[i]);
                    if (w_cell.count(kk)) cut = true;
                    else { const auto it = cell.find(kk); if (it != cell.end()) { rt = 3; j = c_id[i]; ij = c_pair[i]; jk = it->second; } }
                }
                if (cut) break;
                route[x] = rt; via[x] = j;
                // second_is_ref (align.rs:447-449): i-j is read as it is when j is its reference, j-k when k is
                if (rt == 1) bb.push_back(x);
                else tr.push_back(align::TrTask{x, ij, jk, static_cast<uint8_t>(ref_id[ij] != j), static_cast<uint8_t>(ref_id[jk] != k)});
                members.push_back(x);
                w_cell.insert(key(k, i)); w_closest[i] = round;
            }
            ses.backbone(bb.data(), bb.size());
            ses.transitive(tr.data(), tr.size(), tr_params->transitive_anchor);
            for (const uint64_t y : members) {                                 // save_cigar, align.rs:504-513
                const uint32_t k = ref_id[y], i = query_id[y];
                const double dv = static_cast<double>(ses.nerrs(y)) / static_cast<double>(ses.aln_len(y));
                if (dv <= tr_params->transitive_div && !(c_id[i] != NONE && c_dv[i] <= dv)) { c_id[i] = k; c_dv[i] = dv; c_pair[i] = y; }
                cell[key(k, i)] = y;
            }
            n_rounds += members.empty() ? 0 : 1;
            x0 = x;
        }
        ses.finish(n_rounds, h, o, stats, tr_stats);
        t.route = h.copy(route); t.via = h.copy(via);
        *out = o; *tr_out = t; h.commit();
    });
}

}  // extern "C"
