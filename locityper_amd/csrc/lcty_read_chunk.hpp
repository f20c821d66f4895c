// lcty_read_chunk.hpp — a chunk of reads resident on the device, the one object behind every source of a sample's reads:
// the sequence fields of lcty_reads_host (mate m owns the units mate_off[m] / 32 .. of bases2, a 64-bit word a unit, and nmask, a 32-bit
// word a unit). A producer makes it between its two kernels (lcty_fastx_device.hip, lcty_sample_bam.hip, lcty_bam_stream.hip), a host
// chunk is uploaded into it (lcty_recruit, lcty_recruited_add); recruitment, the view and lcty_recruited.hip read it where it lies.
#pragma once

#include <string>
#include <vector>

#include "lcty_common.hpp"
#include "lcty_scan.hpp"

namespace lcty {

// Units of zeros behind the last unit of bases2 and nmask, the same for every producer and for a locus of lcty_recruited.hip. A margin,
// not something a kernel of today needs: walk_minimizers, walk_minimizers_acgt and walk_run_acgt (lcty_recruit.hip) load word i >> 5 of
// a mate for a base i < len only, the `any_n` loops stop at the unit of the last base, and canonical_kmer_2bit (lcty_seq.hpp, the
// mapper) takes word + 1 only when the k-mer itself reaches into it: none touches a word past unit (len + 31) / 32 - 1 of a mate.
constexpr uint32_t CHUNK_PAD_UNITS = 2;

struct ReadChunk {
    // the device buffers: OneShot, sized to the chunk exactly (a handle that holds one chunk for its life: a fetch, an uploaded host
    // chunk); Reused, grow-only with a quarter of head-room (a handle that makes chunk after chunk: DevBuf::ensure_slack)
    enum class Buffers { OneShot, Reused };

    lcty_ctx* ctx;
    bool paired = false;
    uint64_t n = 0, n_units = 0;                 // pairs (or single reads: mate 2 of length 0), units of 32 bases
    DevBuf<uint32_t> d_len, d_nm, d_unit_off;    // [2 n], [n_units + CHUNK_PAD_UNITS], [2 n + 1]: a mate's first unit, for the producer's second kernel
    DevBuf<uint64_t> d_off, d_bases;             // [2 n + 1], [n_units + CHUNK_PAD_UNITS]
    const uint32_t* h_len = nullptr;             // [2 n] mate_len on the host (recruitment sorts by it): the chunk's download, or the caller's array behind upload()

    ReadChunk(lcty_ctx* c, Buffers b) : ctx(c), policy(b) {}
    // the empty chunk
    void clear() { n = 0; n_units = 0; have_view = false; len_store.clear(); h_len = nullptr; }
    // a chunk of n_pairs: d_len and d_off sized for the producer's first kernel, which writes d_len and the units of every mate
    void reserve_mates(uint64_t n_pairs) { clear(); n = n_pairs; size(d_len, 2 * n); size(d_off, 2 * n + 1); }
    // Behind that kernel: the scan of d_units[0 .. M) (M = 2 n) into d_unit_off, mate_off, and d_bases / d_nm sized with their pad
    // zeroed on the stream — for every chunk, since a reused buffer holds the words of the chunk before there. Nothing else is zeroed:
    // pack_kernel and unpack_kernel<true> give every unit below n_units to one lane, which writes its whole word of each array. The
    // download of h_len is enqueued: the producer synchronises the stream behind its second kernel. Returns n_units.
    uint32_t place(const DevBuf<uint32_t>& d_units, uint64_t M, ScanTotal& scan);
    // A host chunk, checked and copied with the pad. The copies read the caller's arrays: synchronise the stream before they go.
    void upload(const lcty_reads_host* h);
    // the chunk as host arrays that belong to it; mate_off, bases2 and nmask come down on the first call
    void view(lcty_reads_host* view);
    // lcty_recruit on the arrays where they lie
    void recruit(lcty_targets* targets, uint32_t max_out, uint32_t* out_cnt, uint32_t* out_loci) const;

private:
    Buffers policy;
    std::vector<uint32_t> len_store, h_bases, h_nm; std::vector<uint64_t> h_off, zero_off;      // behind h_len; of view()
    bool have_view = false;
    template <typename T> void size(DevBuf<T>& b, size_t count) { if (policy == Buffers::Reused) b.ensure_slack(count); else b.alloc(count); }
    void size_units(uint64_t units);             // d_bases / d_nm for n_units = units, the pad zeroed
};

// the chunk of the last lcty_fastx_device_next; the names the two write_recruited write for unit i (its first read end's)
const ReadChunk& fastx_device_reads(const lcty_fastx_device* f);
std::string fastx_device_name(lcty_fastx_device* f, uint64_t i);
std::string sample_reads_name(lcty_sample_reads* r, uint64_t i);

}  // namespace lcty
