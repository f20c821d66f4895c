// lcty_align_internal.hpp — what lcty_align_transitive.hip (the schedule of lcty_align_haplotypes_transitive: rounds, the mirror of
// `closest`, the routes) asks of lcty_align.hip (the kernels, the batches, the store of finished CIGARs). Not part of the C interface.
#pragma once

#include "lcty_common.hpp"

namespace lcty {
namespace align {

// pair: the input index of the pair to align; ij, jk: the input indices of the finished pairs whose CIGARs are composed;
// inv_ij / inv_jk: the CIGAR is read with I and D changed places (CigarDirection RefToQuery)
struct TrTask { uint64_t pair, ij, jk; uint8_t inv_ij, inv_jk; };

class Session {
public:
    // the checks, divergences and skips of lcty_align_haplotypes
    Session(lcty_ctx* ctx, uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref_id, const uint32_t* query_id,
            const uint8_t* against, const lcty_align_params* params);
    ~Session();
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    const uint8_t* aligned() const;                                           // [n_pairs] 0: skipped by its divergence
    void open(uint64_t store_words);                                          // the k-mer index, the batch sizes, the store
    void backbone(const uint64_t* pairs, uint64_t n);                         // stages A to C in batches; the winners go to the store
    void transitive(const TrTask* tasks, uint64_t n, uint32_t anchor_size);   // plan, fill, optimize, counts; into the store
    uint32_t nerrs(uint64_t pair) const;
    uint32_t aln_len(uint64_t pair) const;
    void finish(uint64_t n_rounds, Handoff& h, lcty_align_out& out, lcty_align_stats* stats, lcty_align_tr_stats* tr_stats);   // the arrays of out: through h
private:
    struct Impl;
    Impl* im;
};

}  // namespace align
}  // namespace lcty
