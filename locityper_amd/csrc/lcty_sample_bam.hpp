// lcty_sample_bam.hpp — what the two readers of an indexed BAM file share: lcty_sample_bam.hip (`genotype -a`: the
// reads of the target regions) and lcty_bg_fetch.hip (`preproc -a`: the alignments of the background region). The opened file with
// its index, and the front half of a fetch of regions: their chunks, the slice (lcty_bgzf_read.hpp) and the chain of record lengths
// (fetch_slice). The record on the device is in lcty_bam_record.hpp. The reads a fetch leaves on the device (lcty_sample_reads) are
// also what the reader of whole files in windows hands out chunk by chunk (lcty_bam_stream.hip), so that the consumers
// of lcty_sample_bam.hip (view, recruit, write_recruited, lcty_recruited_add_sample) serve both.
#pragma once

#include <string>
#include <vector>

#include "lcty_bam_record.hpp"
#include "lcty_bgzf_read.hpp"
#include "lcty_read_chunk.hpp"
#include "lcty_writers.hpp"

struct lcty_sample_bam {
    lcty::BgzfFile file;
    std::string index_path;
    std::vector<uint32_t> lengths; std::vector<uint64_t> name_off; std::string names;
    uint64_t first_record = 0;                   // virtual offset behind the header
    int paired = -1;                             // flag 0x1 of the first record; -1: not looked at yet, -2: no record
    std::vector<lcty::IndexRef> refs;            // bins -> chunks, the linear index (lcty_bgzf_index.hpp)
    uint64_t tail_start = 0;                     // largest chunk end of the index
    uint64_t n_no_coor = 0; bool has_no_coor = false;
};

// The reads of one fetch, or of one window of a stream of whole files (lcty_bam_stream.hip), resident on the device: the chunk
// (lcty_read_chunk.hpp) and what the records are written from.
struct lcty_sample_reads {
    lcty::ReadChunk chunk;
    lcty::Slice F;                               // the inflated blocks of the call and the records walked in them
    std::vector<uint32_t> h_src, h_src_stream;   // h_src: a mate's record among the records walked (rec_off); _stream: in the fetched stream
    lcty_sample_reads(lcty_ctx* ctx, lcty::ReadChunk::Buffers b) : chunk(ctx, b) {}
    void clear() { chunk.clear(); h_src.clear(); h_src_stream.clear(); }
};

namespace lcty {

// The regions of a call must be inside the file's contigs, non-empty, sorted and disjoint: LCTY_ERR_INVALID_INPUT otherwise.
void check_regions(const lcty_sample_bam* b, uint32_t n, const uint32_t* tid, const uint32_t* start, const uint32_t* end);
// The chunks of the regions, their slice (Slice::read with the knob "sample_bam_max_slice_bytes", Slice::inflate) and the walk of
// record lengths of one call, with the errors lcty_sample_bam_fetch documents for them. Fills F and the fields of S up to ms_walk.
void fetch_slice(lcty_ctx* ctx, lcty_sample_bam* bam, uint32_t n_regions, const uint32_t* tid, const uint32_t* start, const uint32_t* end,
                 bool with_unmapped, bool whole_file, Slice& F, lcty_sample_bam_stats& S);

}  // namespace lcty
