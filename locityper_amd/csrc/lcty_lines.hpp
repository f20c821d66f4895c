// lcty_lines.hpp — the line reader of the text inputs (FASTA / FASTQ records: lcty_fastx.hip; a genome FASTA: lcty_genome.hip) over
// zlib's gzread, which takes plain files, gzip and BGZF (a run of gzip members) alike. Host only.
#pragma once

#include <zlib.h>

#include <cstring>
#include <string>
#include <vector>

#include "lcty_host.hpp"

namespace lcty {

struct LineReader {
    gzFile f = nullptr;
    std::string path;
    std::vector<char> buf;
    size_t at = 0, end = 0;
    bool eof = false;
    ~LineReader() { if (f) gzclose(f); }
    void open(const char* p) {
        path = p;
        const size_t n = path.size();
        if ((n > 4 && path.compare(n - 4, 4, ".lz4") == 0) || (n > 3 && path.compare(n - 3, 3, ".br") == 0))
            fail(LCTY_ERR_UNSUPPORTED, "%s: FASTA / FASTQ input is read plain or gzip-compressed", p);
        f = gzopen(p, "rb");
        if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot open %s", p);
        gzbuffer(f, 1u << 20);
        buf.resize(1u << 20);
    }
    // read_line (fastx.rs:79-99): the line without its end ("\n" or "\r\n"); false at the end of the file with nothing read
    bool line(std::string& out) {
        out.clear();
        bool any = false;
        for (;;) {
            if (at == end) {
                if (eof) break;
                const int n = gzread(f, buf.data(), static_cast<unsigned>(buf.size()));
                if (n < 0) { int e = 0; fail(LCTY_ERR_INVALID_DATA, "%s: %s", path.c_str(), gzerror(f, &e)); }
                if (n == 0) { eof = true; break; }
                at = 0; end = static_cast<size_t>(n);
            }
            const char* nl = static_cast<const char*>(memchr(buf.data() + at, '\n', end - at));
            if (nl) {
                out.append(buf.data() + at, static_cast<size_t>(nl - (buf.data() + at)));
                at = static_cast<size_t>(nl - buf.data()) + 1;
                if (!out.empty() && out.back() == '\r') out.pop_back();
                return true;
            }
            out.append(buf.data() + at, end - at);
            any = true;
            at = end;
        }
        return any || !out.empty();
    }
};

}  // namespace lcty
