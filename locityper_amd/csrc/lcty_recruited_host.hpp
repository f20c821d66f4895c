// lcty_recruited_host.hpp — the host's half of a resident set of recruited reads (lcty_recruited.hip): what the set keeps
// per locus on the host (lengths, offsets, names), the plan of an add (what every locus gains, checked against the answers' shape, the
// entry limit and the byte cap before anything is copied), the growth of a locus's capacity and the commit of a planned add. Standard
// library and lcty_host.hpp only: scripts/recruited_probe_host.cpp runs it without HIP.
#pragma once

#include <string>
#include <vector>

#include "lcty_host.hpp"

namespace lcty {
namespace recruited {

// One unit is 32 bases: a 64-bit word of 2-bit codes and a 32-bit word of "not ACGT" bits. A pair adds two lengths, two offsets and an
// ordinal. These are the bytes knob "recruited_max_bytes" counts: the contents of the set, not the capacity behind them (at most
// twice as much, the growth being geometric).
constexpr uint64_t UNIT_BYTES = 8 + 4, PAIR_BYTES = 2 * 4 + 2 * 8 + 8;
constexpr uint64_t INIT_UNITS_DEFAULT = 4096;                 // knob "recruited_init_units": 128 kb of bases, some 400 pairs of 150-base mates
constexpr uint64_t MAX_BYTES_DEFAULT = 1ull << 36;            // knob "recruited_max_bytes"
constexpr uint64_t MAX_ENTRIES = 1ull << 32;                  // (locus, pair) entries of one add: the sort's and the scan's offsets are 32-bit
constexpr uint64_t MAX_UNITS = 0x7FFFFFF0ull;                 // units of one add, for the same reason

inline uint32_t units_of(uint32_t len) { return len / 32 + (len % 32 ? 1u : 0u); }

// what the host keeps of one locus: the fields run_map reads there, the names when asked for, and how much the device arrays hold
struct LocusBook {
    uint64_t n_pairs = 0, n_units = 0;
    uint64_t cap_pairs = 0, cap_units = 0;
    std::vector<uint32_t> mate_len;                           // [2 n_pairs]
    std::vector<uint64_t> mate_off{0};                        // [2 n_pairs + 1], bases
    std::vector<uint64_t> name_off{0};                        // [n_pairs + 1] into names: name i is names[name_off[i] .. name_off[i + 1]), no terminator (lcty_write_bam's form)
    std::string names;
    uint64_t bytes() const { return n_units * UNIT_BYTES + n_pairs * PAIR_BYTES; }
};

// the smallest capacity of the series init, 2 init, 4 init, .. that holds `need` (init 0 counts as 1)
inline uint64_t grown(uint64_t cap, uint64_t need, uint64_t init) {
    if (need <= cap) return cap;
    uint64_t c = cap ? cap : std::max<uint64_t>(init, 1);
    while (c < need) c = c > (~0ull >> 1) ? need : 2 * c;
    return c;
}

struct Plan {
    std::vector<uint64_t> add_pairs, add_units;               // per locus
    uint64_t n_entries = 0, n_units = 0, bytes_after = 0;
};

// What adding a chunk of n pairs with these answers does to every locus. Nothing is changed. Refused: out_cnt[i] > max_out and a locus
// beyond n_loci (LCTY_ERR_INVALID_INPUT), MAX_ENTRIES entries or MAX_UNITS units (LCTY_ERR_UNSUPPORTED), contents above max_bytes
// (LCTY_ERR_UNSUPPORTED naming the knob).
inline Plan plan_add(const std::vector<LocusBook>& books, uint64_t n, const uint32_t* mate_len, uint32_t max_out, const uint32_t* out_cnt,
                     const uint32_t* out_loci, uint64_t max_bytes) {
    const size_t n_loci = books.size();
    Plan P;
    P.add_pairs.assign(n_loci, 0); P.add_units.assign(n_loci, 0);
    // the counts first: the size of an add is decided before a single locus is read
    for (uint64_t i = 0; i < n; i++) {
        if (out_cnt[i] > max_out) fail(LCTY_ERR_INVALID_INPUT, "record %llu is recruited to %u loci, max_out is %u", static_cast<unsigned long long>(i), out_cnt[i], max_out);
        const uint64_t u = static_cast<uint64_t>(units_of(mate_len[2 * i])) + units_of(mate_len[2 * i + 1]);
        P.n_entries += out_cnt[i]; P.n_units += u * out_cnt[i];
        if (P.n_entries >= MAX_ENTRIES) fail(LCTY_ERR_UNSUPPORTED, "2^32 or more (locus, read) entries in one add: add the reads in smaller chunks");
        if (P.n_units >= MAX_UNITS) fail(LCTY_ERR_UNSUPPORTED, "2^31 or more 32-base units in one add: add the reads in smaller chunks");
    }
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t u = static_cast<uint64_t>(units_of(mate_len[2 * i])) + units_of(mate_len[2 * i + 1]);
        for (uint32_t j = 0; j < out_cnt[i]; j++) {
            const uint32_t locus = out_loci[i * max_out + j];
            if (locus >= n_loci) fail(LCTY_ERR_INVALID_INPUT, "record %llu is recruited to locus %u of %zu", static_cast<unsigned long long>(i), locus, n_loci);
            P.add_pairs[locus]++; P.add_units[locus] += u;
        }
    }
    for (const LocusBook& b : books) P.bytes_after += b.bytes();
    P.bytes_after += P.n_units * UNIT_BYTES + P.n_entries * PAIR_BYTES;
    if (P.bytes_after > max_bytes)
        fail(LCTY_ERR_UNSUPPORTED, "the recruited reads would take %llu bytes on the device, knob \"recruited_max_bytes\" is %llu",
             static_cast<unsigned long long>(P.bytes_after), static_cast<unsigned long long>(max_bytes));
    return P;
}

// A planned add on the host's side, after the device's copy has been made: lengths and offsets of every locus in input order, and
// name(i) of every added pair when names are kept (name == nullptr: none).
template <class Name>
void commit_add(std::vector<LocusBook>& books, const Plan& P, uint64_t n, const uint32_t* mate_len, uint32_t max_out, const uint32_t* out_cnt,
                const uint32_t* out_loci, Name* name) {
    for (size_t l = 0; l < books.size(); l++) {
        LocusBook& b = books[l];
        b.mate_len.reserve(2 * (b.n_pairs + P.add_pairs[l])); b.mate_off.reserve(2 * (b.n_pairs + P.add_pairs[l]) + 1);
        if (name) b.name_off.reserve(b.n_pairs + P.add_pairs[l] + 1);
    }
    std::string nm;
    for (uint64_t i = 0; i < n; i++) {
        if (!out_cnt[i]) continue;
        if (name) nm = (*name)(i);
        for (uint32_t j = 0; j < out_cnt[i]; j++) {
            LocusBook& b = books[out_loci[i * max_out + j]];
            for (uint32_t e = 0; e < 2; e++) {
                const uint32_t len = mate_len[2 * i + e];
                b.mate_len.push_back(len);
                b.mate_off.push_back(b.mate_off.back() + 32ull * units_of(len));
                b.n_units += units_of(len);
            }
            b.n_pairs++;
            if (name) { b.names.append(nm); b.name_off.push_back(b.names.size()); }
        }
    }
}

}  // namespace recruited
}  // namespace lcty
