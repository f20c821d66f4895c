// lcty_map_internal.hpp — what the two routes of candidate generation share (lcty_map.hip: read ends of up to 256 bases on up to 32
// basis alleles; lcty_map_long.hip: read ends of any length on up to 256 basis alleles): the k-mer index of the basis alleles, the
// packed-base accessors, the device buffers of one call, and everything the routes do alike, once each —
//   the view  MapViewCommon (index, parameters, alleles, reads, counters, the two passes) and fill_map_view;
//   seeds     the k-mers of a read end at every `stride`-th position plus the last one (map_n_seeds); map_seed_at reads the canonical
//             k-mer from the packed stream (lcty_seq.hpp), skips one over a base that is not ACGT, probes the table and skips a k-mer
//             with more than max_occ places; map_place decodes an index entry;
//   records   map_emit_read_end<WRITE, Route>: the best score is the primary record (the smallest slot on ties; the slots are in
//             (allele, strand) order), the others with score >= min_score follow it in slot order as secondary records, a read end
//             without a candidate is an unmapped record; map_write_seq: SEQ and N mask reverse-complemented when the primary is on the
//             reverse strand. A route supplies its candidates and their CIGAR words, nothing else;
//   host      MapInput (the read ends of a call: from the host, uploaded, or where they lie on the device), map_fill_arena (a kernel
//             repeated until its arena held what it asked for) and map_emit_two_pass (sizes, prefix sums over the read ends, the
//             reserve, the records).
#pragma once

#include <algorithm>
#include <initializer_list>
#include <memory>

#include "lcty_objects.hpp"
#include "lcty_table.hpp"

namespace lcty {

constexpr uint32_t MAP_MAX_LEN = 256;          // bases per read end on the short route
constexpr uint32_t MAP_MAX_BASIS = 32;         // basis alleles on the short route
constexpr uint32_t MAP_MAX_BAND = 16;          // diagonals on either side in an alignment with gaps
constexpr uint32_t MAP_LONG_MAX_BASIS = 256;   // basis alleles on the long route
constexpr uint32_t MAP_LONG_MAX_LEN = (1u << 20) - 1;
constexpr uint32_t MAP_NO_SLOT = 0xFFFFFFFFu;

// the counters of a call (MapViewCommon::counters); the host reads the first MAPC_HOST
enum : uint32_t {
    MAPC_WORK = 0,       // work items left for the route's second kernel
    MAPC_OPS = 1,        // CIGAR words asked for in `ops`
    MAPC_WIDEST = 2,     // CIGAR words of the widest record
    MAPC_CHAIN = 3,      // long route: chain entries asked for
    MAPC_HOST = 4,
    MAPC_CURSOR = 4,     // long route: next work item of the align kernel
    MAPC_N = 8
};

__device__ __forceinline__ uint32_t base_at(const uint32_t* b2, uint64_t off, uint32_t i) {
    const uint64_t p = off + i;
    return (b2[p >> 4] >> (2 * (p & 15u))) & 3u;
}
__device__ __forceinline__ bool n_at(const uint32_t* nm, uint64_t off, uint32_t i) {
    const uint64_t p = off + i;
    return (nm[p >> 5] >> (p & 31u)) & 1u;
}

struct MapIndex {
    DevBuf<keytable::Slot> table;          // canonical k-mer -> its run of `entries` (lcty_table.hpp: FastHash, free = UNDEF64)
    DevBuf<uint64_t> entries; DevBuf<uint16_t> basis; DevBuf<uint32_t> scratch;
    uint64_t mask = 0; uint32_t k = 0, n_basis = 0;
};

// lcty_map_index.hip: the index of the given basis alleles, made on the device
std::shared_ptr<MapIndex> build_map_index_device(lcty_locus* locus, const uint16_t* basis, uint32_t n_basis, uint32_t k);

// The read ends of a call. The host always has the lengths and the offsets (the routes size their scratch and the prefix sums from
// them). The four sequence arrays come from the host — bases2 / nmask, uploaded into the call's buffers with the lengths and offsets —
// or lie on the device already and are used in place: d_mate_len, d_bases2, d_nmask, and d_mate_off unless the caller's offsets are
// not the device's (a range of a longer chunk, rebased on the host: null, and mate_off is uploaded). map_upload fills in the null ones.
struct MapInput {
    uint64_t n_pairs; const uint32_t* mate_len; const uint64_t* mate_off;                                // host
    const uint32_t* bases2; const uint32_t* nmask;                                                       // host, or
    const uint32_t* d_mate_len; const uint64_t* d_mate_off; const uint32_t* d_bases2; const uint32_t* d_nmask;      // device
};

// both passes of a route; the records stay on the device, the offsets come to the host
struct MapRun {
    DevBuf<uint32_t> d_len, d_b2, d_nm, d_nrec, d_ncig, d_ob2, d_onm, d_cigar, d_nhave, d_work, d_counters, d_ops;
    DevBuf<uint8_t> d_cands;                              // MapCand / LongCand records
    uint32_t max_rec_cigar = 0;
    DevBuf<uint64_t> d_off, d_rec_at, d_cig_at, d_pair_cig;
    DevBuf<lcty_aln_rec> d_recs;
    std::vector<uint32_t> nrec, ncig;
    uint64_t n_recs = 0, n_cigar = 0;
    // scratch of the long route
    DevBuf<uint4> d_anchors; DevBuf<uint2> d_chain; DevBuf<uint8_t> d_dirs; DevBuf<uint32_t> d_opsbuf;
};

// what the kernels of both routes are given; MapView and LongView add their route's candidates and scratch
struct MapViewCommon {
    const keytable::Slot* table; uint64_t mask;
    const uint64_t* entries;               // basis index << 33 | position << 1 | forward-is-canonical
    const uint16_t* basis;                 // basis index -> allele
    uint32_t n_basis, k, stride, min_votes, max_occ, band;
    int32_t match, mismatch, end_bonus, min_score, gap_open, gap_extend;
    const uint8_t* seqs; const uint64_t* seq_off; const uint32_t* allele_len;
    // reads
    uint64_t n_mates;
    const uint32_t* mate_len; const uint64_t* mate_off; const uint32_t* bases2; const uint32_t* nmask;
    int paired;
    // between the kernels
    uint32_t slots;                        // candidates a read end has room for: [read end][slots], in (allele, strand) order
    uint32_t* n_have;                      // per read end
    uint32_t* counters;                    // MAPC_*
    uint32_t* ops; uint32_t ops_cap;       // arena of the CIGAR words of the alignments with gaps
    // pass 1
    uint32_t* n_recs; uint32_t* n_cigar;
    // pass 2
    const uint64_t* rec_at; const uint64_t* cig_at;      // per read end: first record, first CIGAR word
    const uint64_t* pair_cig;                            // per pair: first CIGAR word (records carry offsets relative to it)
    lcty_aln_rec* recs; uint32_t* cigar;
    uint32_t* out_bases2; uint32_t* out_nmask;
};

// ---- seeds
// the seeds of a read end of L bases: positions 0, stride, 2 stride, .. and the last one
__host__ __device__ inline uint32_t map_n_seeds(uint32_t L, uint32_t k, uint32_t stride) {
    return L < k ? 0u : (L - k) / stride + 1 + ((L - k) % stride ? 1u : 0u);
}
// the host's bound on it, by which the short route refuses a read end and the long route sizes its scratch
inline uint32_t map_seed_bound(uint32_t L, uint32_t k, uint32_t stride) { return L < k ? 0u : (L - k) / stride + 2; }

struct MapSeed { uint32_t pr, start, count; bool read_fwd; };      // position on the read end; its run of `entries`; the read's forward k-mer is the canonical one
struct MapPlace { uint32_t b, pos, strand; };                      // basis index, position of the k-mer on the allele, strand of the read on it

// Seed `sidx` (< map_n_seeds) of the read end of L >= k bases at `off`; count 0: nothing to look at. At most `per_seed` places are taken
// (the first ones: by allele, then position). The read end owns whole 32-base words of both streams (run_map checks the offsets),
// which hipMalloc aligns, so the streams are read as lcty_seq.hpp reads them.
__device__ __forceinline__ MapSeed map_seed_at(const MapViewCommon& V, uint64_t off, uint32_t L, uint32_t sidx, uint32_t per_seed = ~0u) {
    const uint32_t span = L - V.k, n0 = span / V.stride + 1;
    MapSeed sd{sidx < n0 ? sidx * V.stride : span, 0u, 0u, false};
    if (window_has_n(V.nmask + (off >> 5), sd.pr, V.k)) return sd;
    const uint64_t canon = canonical_kmer_2bit(reinterpret_cast<const uint64_t*>(V.bases2 + (off >> 4)), sd.pr, V.k, &sd.read_fwd);
    // keytable::find (lcty_table.hpp) written out: through the function the long route's kernels compile to other instructions, and
    // their time left the parent's range on the slow side
    for (uint64_t h = keytable::home<keytable::FastHash>(canon, V.mask);; h = keytable::step(h, V.mask)) {
        const keytable::Slot s = V.table[h];
        if (s.key == UNDEF64) break;
        if (s.key == canon) { sd.start = s.start; sd.count = s.count > V.max_occ ? 0u : min(s.count, per_seed); break; }      // a repetitive k-mer says nothing about the place
    }
    return sd;
}

__device__ __forceinline__ MapPlace map_place(uint64_t entry, bool read_fwd) {
    return MapPlace{static_cast<uint32_t>(entry >> 33), static_cast<uint32_t>(entry >> 1), read_fwd == ((entry & 1ull) != 0) ? 0u : 1u};
}

// ---- records
// SEQ as the BAM has it: reverse-complemented when the primary record is on the reverse strand. The read end owns whole 32-base
// words of the output; lane = output word.
__device__ __forceinline__ void map_write_seq(const MapViewCommon& V, uint64_t off, uint32_t L, bool reverse) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t wi = lane; wi < (L + 15) / 16; wi += 64) {
        uint32_t out = 0;
        for (uint32_t j = 0; j < 16 && wi * 16 + j < L; j++) {
            const uint32_t i = wi * 16 + j, e = base_at(V.bases2, off, reverse ? L - 1 - i : i);
            out |= (reverse ? 3u - e : e) << (2 * j);
        }
        V.out_bases2[(off >> 4) + wi] = out;
    }
    for (uint32_t wi = lane; wi < (L + 31) / 32; wi += 64) {
        uint32_t out = 0;
        for (uint32_t j = 0; j < 32 && wi * 32 + j < L; j++) {
            const uint32_t i = wi * 32 + j;
            out |= static_cast<uint32_t>(n_at(V.nmask, off, reverse ? L - 1 - i : i)) << j;
        }
        V.out_nmask[(off >> 5) + wi] = out;
    }
}

// The records of read end m from its candidates, one wavefront; sizes (WRITE = false: n_recs, n_cigar, the widest record), then the
// records themselves. The slots are taken 64 at a time, lane = slot. A Route is made from (view, m, L, off) and says
//   Cand load(slot); score(c), group(c) = basis index * 2 + strand, pos(c), n_words(c);
//   write_words(keep, c, n, cg0, rel): called by all lanes of a batch; the n words of every kept candidate go to cg0[rel ..].
template <bool WRITE, class Route>
__device__ void map_emit_read_end(const typename Route::View& V, const uint64_t m) {
    const uint32_t lane = threadIdx.x;
    const uint32_t L = V.mate_len[m];
    if (L == 0) {                                                               // absent read end: no record
        if (!WRITE && lane == 0) { V.n_recs[m] = 0; V.n_cigar[m] = 0; }
        return;
    }
    const uint64_t off = V.mate_off[m];
    const uint32_t nh = V.n_have[m];
    const Route R(V, m, L, off);
    // ---- the primary record: best score, the smallest slot on ties
    int32_t mine = INT32_MIN; uint32_t prim = MAP_NO_SLOT;
    for (uint32_t s = lane; s < nh; s += 64) { const int32_t sc = R.score(R.load(s)); if (prim == MAP_NO_SLOT || sc > mine) { mine = sc; prim = s; } }
    int32_t top = mine;
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o));
    if (mine != top) prim = MAP_NO_SLOT;
    for (int o = 32; o > 0; o >>= 1) prim = min(prim, static_cast<uint32_t>(__shfl_xor(static_cast<int>(prim), o)));
    // its CIGAR words come first: counted by its own lane when its batch comes, ahead of that when others are placed before
    uint32_t ops_primary = prim != MAP_NO_SLOT && prim >= 64 ? R.n_words(R.load(prim)) : 0u, g_primary = 0;
    const uint32_t mate2 = V.paired && (m & 1u) ? LCTY_FLAG_MATE2 : 0u;
    uint64_t rec0 = 0, cig0 = 0, rel0 = 0;
    if (WRITE) { rec0 = V.rec_at[m]; cig0 = V.cig_at[m]; rel0 = cig0 - V.pair_cig[m >> 1]; }
    uint32_t n_others = 0, words = 0, widest = 0;                              // the secondary records so far and their words
    for (uint32_t s0 = 0; s0 < nh; s0 += 64) {
        const uint32_t s = s0 + lane;
        typename Route::Cand c{};
        if (s < nh) c = R.load(s);
        const bool keep = s < nh && (s == prim || R.score(c) >= V.min_score);
        const uint32_t n = keep ? R.n_words(c) : 0u;
        if (prim - s0 < 64u) {
            ops_primary = static_cast<uint32_t>(__shfl(static_cast<int>(n), static_cast<int>(prim - s0)));
            g_primary = static_cast<uint32_t>(__shfl(static_cast<int>(R.group(c)), static_cast<int>(prim - s0)));
        }
        const bool other = keep && s != prim;                                   // the others follow the primary in slot order
        const unsigned long long om = __ballot(other);
        uint32_t incl = other ? n : 0u;                                         // written out: wave_scan_incl costs the long-read kernels registers
        for (int o = 1; o < 64; o <<= 1) { const uint32_t up = __shfl_up(incl, o); if (lane >= static_cast<uint32_t>(o)) incl += up; }
        widest = max(widest, n);
        if (WRITE) {
            const uint32_t rank = s == prim ? 0u : 1u + n_others + static_cast<uint32_t>(__popcll(om & ((1ull << lane) - 1ull)));
            const uint32_t cig_rel = s == prim ? 0u : ops_primary + words + incl - n;
            if (keep) {
                const uint32_t g = R.group(c);
                const uint16_t flags = static_cast<uint16_t>((g & 1u ? LCTY_FLAG_REVERSE : 0u) | (s == prim ? 0u : LCTY_FLAG_SECONDARY) | mate2);
                V.recs[rec0 + rank] = lcty_aln_rec{R.pos(c), V.basis[g >> 1], flags, n, static_cast<uint32_t>(rel0 + cig_rel)};
            }
            R.write_words(keep, c, n, V.cigar + cig0, cig_rel);
        }
        n_others += static_cast<uint32_t>(__popcll(om));
        words += static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63));
    }
    if (!WRITE) {
        for (int o = 32; o > 0; o >>= 1) widest = max(widest, static_cast<uint32_t>(__shfl_xor(static_cast<int>(widest), o)));
        if (lane == 0) {
            V.n_recs[m] = n_others + 1;                                         // no candidate: one unmapped record
            V.n_cigar[m] = ops_primary + words;
            if (widest > V.counters[MAPC_WIDEST]) atomicMax(&V.counters[MAPC_WIDEST], widest);
        }
        return;
    }
    if (nh == 0 && lane == 0) V.recs[rec0] = lcty_aln_rec{0u, 0u, static_cast<uint16_t>(LCTY_FLAG_UNMAPPED | mate2), 0u, static_cast<uint32_t>(rel0)};
    map_write_seq(V, off, L, g_primary & 1u);
}

// ---- host
// what of the input is not on the device yet goes into the call's buffers; afterwards every d_ field of `in` is set
inline void map_upload(MapInput& in, MapRun& X, hipStream_t s) {
    const uint64_t n_mates = 2 * in.n_pairs, nb = in.mate_off[n_mates];
    if (!in.d_mate_len) { X.d_len.ensure_slack(n_mates); X.d_len.upload(in.mate_len, n_mates, s); in.d_mate_len = X.d_len.p; }
    if (!in.d_mate_off) { X.d_off.ensure_slack(n_mates + 1); X.d_off.upload(in.mate_off, n_mates + 1, s); in.d_mate_off = X.d_off.p; }
    if (!in.d_bases2) { X.d_b2.ensure_slack(std::max<uint64_t>(nb / 16, 1)); X.d_b2.upload(in.bases2, nb / 16, s); in.d_bases2 = X.d_b2.p; }
    if (!in.d_nmask) { X.d_nm.ensure_slack(std::max<uint64_t>(nb / 32, 1)); X.d_nm.upload(in.nmask, nb / 32, s); in.d_nmask = X.d_nm.p; }
}

// the view of a call over an input that is on the device (map_upload), with room for `slots` candidates of `cand_bytes` per read end
inline void fill_map_view(MapViewCommon& V, lcty_locus* locus, const MapIndex& ix, const lcty_map_params* params, MapRun& X, const MapInput& in,
                          uint32_t slots, size_t cand_bytes) {
    const uint64_t n_mates = 2 * in.n_pairs;
    V.table = ix.table.p; V.mask = ix.mask; V.entries = ix.entries.p; V.basis = ix.basis.p; V.n_basis = ix.n_basis;
    V.k = params->k; V.stride = params->stride; V.min_votes = std::max<uint32_t>(params->min_votes, 1);
    V.max_occ = params->max_occ ? params->max_occ : 4 * ix.n_basis;
    V.match = params->match; V.mismatch = params->mismatch; V.end_bonus = params->end_bonus; V.min_score = params->min_score;
    V.band = params->band; V.gap_open = params->gap_open; V.gap_extend = params->gap_extend;
    V.seqs = locus->d_seqs.p; V.seq_off = locus->d_seq_off.p; V.allele_len = locus->d_allele_len.p;
    V.n_mates = n_mates; V.mate_len = in.d_mate_len; V.mate_off = in.d_mate_off; V.bases2 = in.d_bases2; V.nmask = in.d_nmask;
    V.paired = locus->bg.is_paired;
    V.n_recs = X.d_nrec.p; V.n_cigar = X.d_ncig.p;
    V.slots = slots;
    if (n_mates * slots > 0xFFFFFFFFull) fail(LCTY_ERR_UNSUPPORTED, "chunks of up to %llu read pairs with this basis", (unsigned long long)(0xFFFFFFFFull / slots / 2));
    X.d_cands.ensure_slack(n_mates * slots * cand_bytes); X.d_nhave.ensure_slack(n_mates);
    X.d_counters.ensure_slack(MAPC_N); X.d_counters.zero(locus->ctx->stream);
    V.n_have = X.d_nhave.p; V.counters = X.d_counters.p;
}

// launch(cap) gives the kernel an arena of `cap` entries and starts it; repeated with the room the kernel asked for in counters[asked]
// when that was more, the counters in `clear` (what the kernel counts) zero again
// The first try clears nothing: it relies on fill_map_view having zeroed every counter and on no earlier kernel of the call counting
// into `clear` (the chain kernel counts MAPC_WORK and MAPC_CHAIN only, the seed kernel MAPC_WORK only). A kernel that does must be
// followed by a clear of its own.
template <class Launch>
void map_fill_arena(hipStream_t s, MapRun& X, uint32_t* counters, uint64_t cap, uint32_t asked, std::initializer_list<uint32_t> clear, const char* limit,
                    Launch&& launch) {
    for (;;) {
        if (cap > 0xFFFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "%s", limit);
        launch(cap);
        LCTY_HIP(hipGetLastError());
        X.d_counters.download(counters, MAPC_HOST, s);
        LCTY_HIP(hipStreamSynchronize(s));
        if (counters[asked] <= cap) return;
        cap = static_cast<uint64_t>(counters[asked]) + 1024;
        const uint32_t zero = 0;
        for (const uint32_t c : clear) X.d_counters.upload(&zero, 1, s, c);
    }
}

// The tail of both routes: emit(V, false, workgroups) launches the route's emit kernel for the sizes; prefix sums over the read ends
// give rec_at, cig_at, pair_cig and the caller's aln_off / cigar_off; the outputs are reserved and zeroed and their places put into V;
// emit(V, true, workgroups) writes.
template <class View, class Emit>
void map_emit_two_pass(lcty_ctx* ctx, const MapInput& in, View& V, MapRun& X, uint64_t* aln_off, uint64_t* cigar_off, bool sizes_only,
                       Emit&& emit) {
    hipStream_t s = ctx->stream;
    const uint64_t n = in.n_pairs, n_mates = 2 * n, nb = in.mate_off[n_mates];
    const uint32_t n_wg = static_cast<uint32_t>(std::min<uint64_t>(n_mates, 16ull * static_cast<uint32_t>(ctx->props.multiProcessorCount)));
    uint32_t counters[MAPC_HOST];
    ctx->timed(LCTY_K_MAP, [&] { emit(V, false, n_wg); }, s);
    LCTY_HIP(hipGetLastError());
    X.d_counters.download(counters, MAPC_HOST, s);
    X.nrec.resize(n_mates); X.ncig.resize(n_mates);
    X.d_nrec.download(X.nrec.data(), n_mates, s); X.d_ncig.download(X.ncig.data(), n_mates, s);
    LCTY_HIP(hipStreamSynchronize(s));
    X.max_rec_cigar = counters[MAPC_WIDEST];
    std::vector<uint64_t> rec_at(n_mates), cig_at(n_mates), pair_cig(n);
    uint64_t r = 0, c = 0;
    for (uint64_t p = 0; p < n; p++) {
        pair_cig[p] = c;
        for (uint32_t e = 0; e < 2; e++) { rec_at[2 * p + e] = r; cig_at[2 * p + e] = c; r += X.nrec[2 * p + e]; c += X.ncig[2 * p + e]; }
        aln_off[p + 1] = r; cigar_off[p + 1] = c;
    }
    X.n_recs = r; X.n_cigar = c;
    if (sizes_only) return;
    X.d_rec_at.ensure_slack(n_mates); X.d_rec_at.upload(rec_at.data(), n_mates, s);
    X.d_cig_at.ensure_slack(n_mates); X.d_cig_at.upload(cig_at.data(), n_mates, s);
    X.d_pair_cig.ensure_slack(n); X.d_pair_cig.upload(pair_cig.data(), n, s);
    X.d_recs.ensure_slack(std::max<uint64_t>(r, 1)); X.d_cigar.ensure_slack(std::max<uint64_t>(c, 1));
    X.d_ob2.ensure_slack(std::max<uint64_t>(nb / 16, 1)); X.d_onm.ensure_slack(std::max<uint64_t>(nb / 32, 1));
    X.d_ob2.zero(s); X.d_onm.zero(s);
    V.rec_at = X.d_rec_at.p; V.cig_at = X.d_cig_at.p; V.pair_cig = X.d_pair_cig.p; V.recs = X.d_recs.p; V.cigar = X.d_cigar.p;
    V.out_bases2 = X.d_ob2.p; V.out_nmask = X.d_onm.p;
    ctx->timed(LCTY_K_MAP, [&] { emit(V, true, n_wg); }, s);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));                                          // rec_at & co. are host vectors of this frame
}

// lcty_map_long.hip: the long route over an input that is on the device (map_upload); leaves records, CIGAR words, re-oriented bases
// and the per-read-end counts in X, the offsets in aln_off / cigar_off
void run_map_long(lcty_locus* locus, const MapInput& in, const lcty_map_params* params, const MapIndex& ix, uint32_t max_len,
                  uint64_t* aln_off, uint64_t* cigar_off, bool sizes_only, MapRun& X);
// lcty_map.hip: lcty_reads_map_append on any input (lcty_recruited.hip maps the resident reads of a locus through it)
void map_append_input(lcty_reads* reads, const MapInput& in, const lcty_map_params* params);

}  // namespace lcty
