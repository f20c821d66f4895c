// lcty_writers.hpp — the per-locus read files behind recruitment (lcty_fastx_writers_open / _close, lcty_fastx.hip): one definition for
// the two sources of recruited reads, FASTA / FASTQ input (lcty_fastx.hip) and an indexed BAM file (lcty_sample_bam.hip). Host code.
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
