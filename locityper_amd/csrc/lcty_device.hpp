// lcty_device.hpp — plain views passed by value to the gfx950 kernels, the probes of the UniqueKmers sets, and two things many
// kernels state: the error word (ErrWord, refuse) and the owner of a flat item (flat_owner). The sequence primitives (base codes,
// hashes, k-mer extraction) are in lcty_seq.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/locityper_hip.h"
#include "lcty_common.hpp"
#include "lcty_seq.hpp"

namespace lcty {

constexpr int WAVE = 64;                       // CDNA4 wavefront
// the pair-alignment arena of a scored batch: a wavefront of a large scoring launch reserves PA_CHUNK entries at a time
// (lcty_score.hip); a batch that can hold such a launch gets an eighth more room and a chunk per wavefront (lcty_reads_create)
constexpr uint32_t PA_CHUNK = 8192, PA_POOL_MIN_PAIRS = 32, PA_MAX_GRID = 256 * 16;

// Device record of one PairAlignment (src/model/locs.rs:668-676), 24 B.
struct PairAlnDev {
    double ln_prob;
    uint32_t mid1, mid2;     // LCTY_NONE_U32 = None
    uint16_t contig;
    uint16_t ix1, ix2;       // record index inside the pair, 0xFFFF = None
    uint16_t _pad;
};
static_assert(sizeof(PairAlnDev) == 24, "PairAlnDev layout");

// BayesCalc<NBinom, NBinom> of one GC bin (src/model/distr_cache.rs:61-75): null hypothesis + alternatives, for the
// direct evaluation of depths beyond the 256-entry LinearCache (src/math/distr/lincache.rs:41-48).
struct DepthNB {
    double lnq;                                  // ln(1 - p), shared by all hypotheses (NBinom::mul keeps p)
    double n[LCTY_MAX_ALT_CN + 1];               // [0] = null (cn 1), then the alternatives
    double lnpmf_const[LCTY_MAX_ALT_CN + 1];     // n ln p - lnGamma(n)
};

struct LocusView {
    uint32_t n_alleles, k;
    const uint32_t* allele_len;     // [A]
    const uint32_t* ci_off;         // [A+1] offsets into the per-position ContigInfo arrays
    const uint16_t* compl_cnt;      // linguistic-complexity numerators (src/seq/compl.rs:115-140)
    double compl_mult;              // 1 / min(neighb+1-ck, 4^ck)
    uint32_t half_neighb;
    // UniqueKmers (src/model/locs.rs:915-1003)
    const uint64_t* kset;           // key table (lcty_table.hpp: MixHash, free = UNDEF64)
    uint64_t kset_mask;             // capacity - 1
    uint32_t undef_in_set;          // UNDEF was inserted (an allele window with N has count 0)
    double weight_mult, weight_interc;
    // InsertDistr (src/bg/insertsz.rs)
    const double* ins_lut;
    uint32_t ins_lut_size;
    double ins_n, ins_lnq, ins_lnpmf_const, insert_penalty;
    // ErrorProfile (src/bg/err_prof.rs:212-221)
    double lp[5];
    // EditDistCache (src/bg/err_prof.rs:415-448): (good, passable) per read length
    const uint2* edit_lut;
    uint32_t edit_lut_size;
    // model::Params
    double unmapped_penalty, prob_diff, min_weight, poor_compl, poor_compl_edit;
    uint32_t boundary;              // boundary_size - tweak (locs.rs:1099)
    uint32_t is_paired, short_reads, strict_subset;
    // ExplicitWeights (src/model/windows.rs:196-250), null without --reg-weights: len + 1 values per allele
    const double* ew_val;
    const uint64_t* ew_off;         // [A+1]
    uint32_t half_window;           // window_size / 2 (windows.rs:499)
};

struct ReadsView {
    uint64_t n_pairs;
    const uint32_t* mate_len;
    const uint64_t* mate_off;
    const uint32_t* bases2;
    const uint32_t* nmask;
    const uint64_t* aln_off;
    const lcty_aln_rec* recs;
    const uint64_t* cigar_off;
    const uint32_t* cigar;
    const uint2* pair_meta;         // per pair {index of the mate-2 primary (or n), number of records to look at}
    // products of AllAlignments::load
    uint8_t* status;
    double* weight;
    double* unmapped_prob;
    uint16_t* uniq_kmers;           // [2R]
    double* matrix;                 // [R][A] read-major; rows of non-GOOD pairs are 0.0
    PairAlnDev* pa;                 // arena
    uint64_t pa_cap;
    uint32_t pa_chunk;              // entries a wavefront of the scoring kernel reserves at a time (0: every pair reserves its own)
    unsigned long long* pa_count;   // arena cursor
    uint64_t* pa_off;               // [R]
    uint32_t* pa_cnt;               // [R]
    uint32_t* pa_idx;               // [R][A]: offset of the contig's entries inside the pair's arena segment | count << 24
    uint32_t* err_flag;             // first LCTY_ERR_* raised by a kernel
    double* recover_w;              // per pair: read weight if it reaches recover_and_group_alignments (locs.rs:1255), else -1
    // the lean scoring kernel hands the pairs it does not take (several saved alignments of a read end on one contig, mates
    // beyond the register path of the k-mer windows) to the general kernel: their indices, appended in any order
    uint32_t* defer_list;           // [cap_raw_pairs] or null
    unsigned int* defer_count;      // [1]
    const uint32_t* only_list;      // general kernel: the pairs to score (null: all n_pairs) ...
    const unsigned int* only_count; // ... and how many (device memory: no host round trip between the two launches)
    unsigned long long* dbg;        // lcty_ctx_set_knob "score_timing": shader-clock sums of the lean kernel's phases (else null)
    uint8_t* park;                  // scoring kernel, large pairs: per-workgroup scratch of saved alignments (else null)
    uint64_t park_stride;
};

// ---- the error word of a pipeline of kernels: (ordinal of the offending item << 8 | class of the error), the smallest wins, so
// the first item in input order decides and at one item the class of lowest rank. All bits set: nobody refused anything.
struct ErrWord {
    DevBuf<unsigned long long> d;
    unsigned long long* reset(hipStream_t s) {
        d.ensure(1);
        LCTY_HIP(hipMemsetAsync(d.p, 0xFF, sizeof(unsigned long long), s));
        return d.p;
    }
    // what the kernels launched on s so far left (synchronises s); false: nothing
    bool take(hipStream_t s, uint64_t& ordinal, uint32_t& cls) {
        unsigned long long e = 0;
        d.download(&e, 1, s);
        LCTY_HIP(hipStreamSynchronize(s));
        ordinal = e >> 8; cls = static_cast<uint32_t>(e & 0xFF);
        return e != ~0ull;
    }
};

#ifdef __HIPCC__
__device__ __forceinline__ void refuse(unsigned long long* err, uint64_t ordinal, uint32_t cls) {
    atomicMin(err, (static_cast<unsigned long long>(ordinal) << 8) | cls);
}

// the owner of flat item j: the last k in [0, n) with off[k] <= j (off ascending, off[0] <= j)
template <typename O, typename J>
__device__ __forceinline__ uint32_t flat_owner(const O* __restrict__ off, uint32_t n, J j) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] <= j) lo = mid; else hi = mid; }
    return lo;
}

// ---- set probe. k-mers of 32..63 bases: the set is an open-addressing table of {lo, hi} pairs built on the host (lcty_locus_create),
// free = {~0, ~0}: another key type than that of lcty_table.hpp, which serves k <= 31 ----
__host__ __device__ inline uint64_t kmer128_hash(uint64_t lo, uint64_t hi) { return mix64(lo ^ mix64(hi ^ 0x9E3779B97F4A7C15ull)); }
__device__ inline bool kset128_contains(const uint64_t* kset, uint64_t mask, Kmer128 key) {
    uint64_t slot = kmer128_hash(key.lo, key.hi) & mask;
    while (true) {
        const uint64_t lo = kset[2 * slot], hi = kset[2 * slot + 1];
        if (lo == key.lo && hi == key.hi) return true;
        if (lo == UNDEF64 && hi == UNDEF64) return false;
        slot = (slot + 1) & mask;
    }
}

#endif

}  // namespace lcty
