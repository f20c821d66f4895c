// lcty_aln_bam_parse.hpp — the two host passes of lcty_bam_read_device (lcty_aln_bam.hip) over the inflated bytes of an
// aln.bam: the header (parse_header) and the chain of record lengths (walk_records). Standard library and lcty_host.hpp only, no HIP
// call: scripts/aln_bam_probe_host.cpp runs them on the CPU alone. Both keep the checks, their order, the statuses and the message
// texts of the loop of lcty_bam_read (lcty_io.hip).
#pragma once

#include <map>
#include <string>
#include <vector>

#include "lcty_host.hpp"

namespace lcty {
namespace alnbam {

inline uint32_t rd32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | (static_cast<uint32_t>(p[3]) << 24); }

struct Header {
    uint32_t n_ref = 0;
    uint64_t first_record = 0;                 // the byte behind the reference list
    std::vector<uint32_t> tid2contig;          // [n_ref] allele index of every reference (construct_tid_to_contig_map, locs.rs:388-401)
};

// b[0 .. n): the inflated file. The header may lie anywhere in it (the BGZF blocks it spanned are gone by now). n is compared with
// what is left, so no sum wraps: l_text / l_name / n_ref are 32-bit words of the file.
inline Header parse_header(const uint8_t* b, uint64_t n, const char* const* names, uint32_t n_alleles, const char* path) {
    uint64_t i = 0;
    auto need = [&](uint64_t k) { if (k > n - i) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM", path); };
    need(12);
    if (memcmp(b, "BAM\1", 4)) fail(LCTY_ERR_INVALID_DATA, "%s: not a BAM file", path);
    i = 4;
    const uint32_t l_text = rd32(b + i); i += 4; need(static_cast<uint64_t>(l_text) + 4); i += l_text;
    Header H;
    H.n_ref = rd32(b + i); i += 4;
    if (H.n_ref > (n - i) / 8)
        fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM (%u references in %llu bytes)", path, H.n_ref, static_cast<unsigned long long>(n - i));
    std::map<std::string, uint32_t> by_name;
    for (uint32_t a = 0; a < n_alleles; a++) by_name[names[a]] = a;
    H.tid2contig.resize(H.n_ref);
    for (uint32_t r = 0; r < H.n_ref; r++) {
        need(4); const uint32_t l_name = rd32(b + i); i += 4; need(static_cast<uint64_t>(l_name) + 4);
        const std::string nm(reinterpret_cast<const char*>(b + i), l_name ? l_name - 1 : 0);
        i += static_cast<uint64_t>(l_name) + 4;
        const auto it = by_name.find(nm);
        if (it == by_name.end()) fail(LCTY_ERR_INVALID_DATA, "Intermediate BAM file contains unexpected contigs (e.g. %s)", nm.c_str());
        H.tid2contig[r] = it->second;
    }
    H.first_record = i;
    return H;
}

// The chain of block_size words from byte `first` on. rec_off: the byte of every record whose block lies inside b[0 .. n) and has its
// 32 fixed bytes. The walk ends at the first record that does not — `stop` says how (the record's ordinal is rec_off.size()): the
// records before it are still looked at, since an error of theirs comes first in file order.
enum WalkStop : uint32_t { WALK_END = 0, WALK_TRUNCATED = 1, WALK_SHORT_BLOCK = 2 };
inline WalkStop walk_records(const uint8_t* b, uint64_t n, uint64_t first, std::vector<uint64_t>& rec_off) {
    uint64_t i = first;
    while (i < n) {
        if (n - i < 4) return WALK_TRUNCATED;
        const uint32_t block = rd32(b + i);
        if (block > n - i - 4) return WALK_TRUNCATED;
        if (block < 32) return WALK_SHORT_BLOCK;
        rec_off.push_back(i);
        i += 4ull + block;
    }
    return WALK_END;
}

// the name of the record at byte o as the loop of lcty_bam_read holds it: l_read_name - 1 bytes
inline std::string qname_at(const uint8_t* b, uint64_t o) {
    const uint32_t l = b[o + 12];
    return std::string(reinterpret_cast<const char*>(b + o + 36), l ? l - 1 : 0);
}
inline bool is_primary_at(const uint8_t* b, uint64_t o) { return ((b[o + 18] | (b[o + 19] << 8)) & 0x900u) == 0; }

}  // namespace alnbam
}  // namespace lcty
