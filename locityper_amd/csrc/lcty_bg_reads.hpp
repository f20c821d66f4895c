// lcty_bg_reads.hpp — the alignments of a background region as lcty_bg_estimate takes them (include/locityper_hip.h:
// lcty_bg_reads_view). Made by lcty_bg_reads_load (lcty_io.hip: the whole file parsed on the host) or by lcty_bg_reads_fetch
// (lcty_bg_fetch.hip: through the index, records on the device); read by lcty_bg.hip.
#pragma once

#include <vector>

#include "lcty_common.hpp"

struct lcty_bg_reads {
    std::vector<uint32_t> pos, end, qlen, mate; std::vector<uint8_t> flags;
    std::vector<uint64_t> cigar_off, seq_off; std::vector<uint32_t> cigar, bases2, nmask;
    lcty_bg_reads_view view{};
    // lcty_bg_reads_fetch only: the context whose device holds the same arrays, laid out and sized as the host's, which
    // lcty_bg_estimate on that context reads in place of an upload. Null: a handle of lcty_bg_reads_load.
    lcty_ctx* ctx = nullptr;
    lcty::DevBuf<uint32_t> d_pos, d_end, d_cigar, d_bases2, d_nmask; lcty::DevBuf<uint64_t> d_cigar_off, d_seq_off; lcty::DevBuf<uint8_t> d_flags;
};
