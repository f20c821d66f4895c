// lcty_writers.hpp — the per-locus read files behind recruitment (lcty_fastx_writers_open / _close, lcty_fastx.hip), one definition for
// every source of recruited reads (lcty_fastx.hip, lcty_fastx_device.hip, lcty_sample_bam.hip for fetched and streamed BAM records): the
// writers, the one loop over the units of a chunk (write_recruited_units) and the text of a BAM record. Host code, no HIP.
#pragma once

#include <zlib.h>

#include <cstdio>
#include <string>
#include <vector>

#include "lcty_host.hpp"

struct lcty_fastx_writers {
    std::vector<gzFile> gz; std::vector<FILE*> plain; std::vector<std::string> paths;
    ~lcty_fastx_writers() {
        for (gzFile g : gz) if (g) gzclose(g);
        for (FILE* f : plain) if (f) fclose(f);
    }
    void put(uint32_t i, const std::string& s) {
        if (gz[i]) { if (gzwrite(gz[i], s.data(), static_cast<unsigned>(s.size())) != static_cast<int>(s.size())) lcty::fail(LCTY_ERR_RUNTIME, "write error on %s", paths[i].c_str()); }
        else if (fwrite(s.data(), 1, s.size(), plain[i]) != s.size()) lcty::fail(LCTY_ERR_RUNTIME, "write error on %s", paths[i].c_str());
    }
};

namespace lcty {

// recruit_single_thread's `record.write_to(writers.get(locus_ix))` (recruit.rs:1000-1030): unit i < n with out_cnt[i] > 0 goes, as the
// text text_of(i, text) appends, to the writers of its first min(out_cnt[i], max_out) loci. Returns the units written.
template <typename TextOf>
uint64_t write_recruited_units(lcty_fastx_writers* w, uint64_t n, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci, TextOf&& text_of) {
    uint64_t written = 0;
    std::string text;
    for (uint64_t i = 0; i < n; i++) {
        if (!out_cnt[i]) continue;
        text.clear();
        text_of(i, text);
        for (uint32_t j = 0; j < std::min(out_cnt[i], max_out); j++) {
            const uint32_t locus = out_loci[static_cast<size_t>(i) * max_out + j];
            if (locus >= w->paths.size()) fail(LCTY_ERR_INVALID_INPUT, "record %llu is recruited to locus %u of %zu writers", static_cast<unsigned long long>(i), locus, w->paths.size());
            w->put(locus, text);
        }
        written++;
    }
    return written;
}

// the name of the BAM record at byte o of a slice (o: its block_size field)
inline std::string record_name(const uint8_t* slice, uint64_t o) {
    const uint32_t l = slice[o + 12];
    const std::string s(reinterpret_cast<const char*>(slice + o + 36), l ? l - 1 : 0);
    return s.substr(0, s.find('\0'));
}

// BamRecord::write_to (fastx.rs:633-668) of the record at byte o, appended to text: FASTA when it has no qualities; a reverse record back to front, complemented
inline void bam_record_text(const uint8_t* slice, uint64_t o, std::string& text) {
    static const char CODES[] = "=ACMGRSVTWYHKDBN";
    const uint8_t* rec = slice + o;
    uint32_t l_seq; uint16_t n_cigar, flag;
    memcpy(&n_cigar, rec + 16, 2); memcpy(&flag, rec + 18, 2); memcpy(&l_seq, rec + 20, 4);
    const uint8_t* seq = rec + 36 + rec[12] + 4ull * n_cigar;
    const uint8_t* qual = seq + (static_cast<uint64_t>(l_seq) + 1) / 2;
    const bool reverse = (flag & 0x10) != 0, fasta = l_seq == 0 || qual[0] == 255;
    text += fasta ? '>' : '@'; text += record_name(slice, o); text += '\n';
    for (uint32_t k = 0; k < l_seq; k++) {
        const uint32_t j = reverse ? l_seq - 1 - k : k;
        const char c = CODES[(seq[j >> 1] >> ((j & 1) ? 0 : 4)) & 15];
        // seq::complement_nt (seq/mod.rs:125-135): IUPAC codes become N ('=' panics there; N here)
        text += !reverse ? c : c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
    }
    text += fasta ? "\n" : "\n+\n";
    for (uint32_t k = 0; k < l_seq && !fasta; k++) text += static_cast<char>(qual[reverse ? l_seq - 1 - k : k] + 33);
    if (!fasta) text += '\n';
}

}  // namespace lcty
