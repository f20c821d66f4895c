// lcty_aln_bam.hpp — the handle of an aln.bam, shared by its two readers: lcty_bam_read (lcty_io.hip, host) and lcty_bam_read_device
// (lcty_aln_bam.hip), whose arrays are also resident on the device of `ctx`.
#pragma once

#include <string>
#include <vector>

#include "lcty_common.hpp"
#include "lcty_device.hpp"

// aln.bam as the flat table of the boundary (+ what only file writers need: names, qualities)
struct lcty_bam_table {
    std::vector<uint32_t> mate_len; std::vector<uint64_t> mate_off; std::vector<uint32_t> bases2, nmask;
    std::vector<uint64_t> aln_off; std::vector<lcty_aln_rec> recs; std::vector<uint64_t> cigar_off; std::vector<uint32_t> cigar;
    std::vector<uint64_t> name_off; std::string names;
    std::vector<uint8_t> quals; std::vector<uint64_t> qual_off;       // per mate, BAM orientation (0xFF: absent)
    std::vector<uint8_t> mapq;                                        // per record
    uint32_t n_refs = 0;
    lcty_reads_host view{};
    // lcty_bam_read_device: the device the arrays below live on (null: a handle of lcty_bam_read), whether the host vectors of records,
    // CIGAR words, bases, qualities and MAPQ were filled (host_copy), the totals, and what an append needs beside the offsets
    lcty_ctx* ctx = nullptr;
    bool host_copy = true;
    uint64_t n_recs = 0, n_cigar = 0;
    std::vector<uint32_t> n_recs_mate;                                // [2 n_pairs] records of every read end, its primary first
    std::vector<uint32_t> pair_max_cigar;                             // [n_pairs] the largest CIGAR of one record of the pair
    lcty::DevBuf<lcty_aln_rec> d_recs; lcty::DevBuf<uint32_t> d_cigar, d_bases2, d_nmask;
};
