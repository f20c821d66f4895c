// lcty_fastx_window.hpp — the host half of the device route for FASTA / FASTQ input (lcty_fastx_device.hip): the
// container of a file (plain, BGZF, any other gzip), windows of text with the tail of one carried to the front of the next, the
// enlarging of a window that holds no complete record, the cursor over a window's records, and which record's error wins (the first
// in input order, as Reader::next and read_unit of lcty_fastx.hip meet them). Host code without HIP: what runs on a window, and where
// its bytes live, is the executor's (Exec), so that scripts/fastx_probe_host.cpp runs all of this with a serial one.
//   Exec::Buffer                      the text of a window: data(), and whatever keeps it (a page-locked slice; a vector)
//   exec.alloc(buf, n)                n bytes (+ pad) the caller fills
//   exec.inflate(buf, comp, blocks, total, path)   `total` bytes, the BGZF blocks inflated to their out_at; bytes before the first stay free
//   exec.put_front(buf, p, n)         the carried tail, written after either of the two
//   exec.parse(file, buf, n, final, fasta, P)   line table, rows, the first (record, class) of the window
//   exec.mismatch(fa, ra, sa, fb, rb, sb, n)   the first i < n whose records ra + sa i of file fa's window and rb + sb i of fb's fail
//                                     equal_names_fast, or n
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <chrono>
#include <string>
#include <vector>

#include "lcty_bgzf.hpp"
#include "lcty_fastx_parse.hpp"

namespace lcty {
namespace fastx {

constexpr uint64_t WINDOW_DEFAULT = 1ull << 28, WINDOW_MIN = 64, WINDOW_LIMIT = (1ull << 31) - 64;   // offsets inside a window are 32-bit
constexpr uint32_t NO_EVENT = 0xFFFFFFFFu;

inline double clock_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// what an executor's parse of one window leaves
struct Parsed {
    uint32_t n_rec = 0;                   // records decided: FASTQ floor(complete lines / 4), FASTA those another header follows; all, when the stream has ended
    uint32_t covered = 0;                 // the bytes they cover
    uint32_t ev_rec = NO_EVENT, ev_cls = 0;   // the smallest (record, class) below n_rec
    std::vector<Row> rows;                // at least n_rec; FASTA: the record that is still open as well
    std::vector<uint32_t> nl, cum;        // FASTA alone: the line table and the bases before every line (a sequence is gathered from its lines)
};

struct Counters { uint64_t bytes_read = 0, bytes_inflated = 0, windows = 0, windows_enlarged = 0, records = 0; double ms_read = 0, ms_inflate = 0; };

// one input file as a stream of text
struct Source {
    enum Kind { PLAIN, BGZF, GZIP } kind = PLAIN;
    std::string path;
    int fd = -1;
    uint64_t fsize = 0, at = 0;           // the next byte of the file
    bool eof = false;                     // no text is left
    z_stream zs; bool zs_open = false; std::vector<uint8_t> zin; size_t zin_at = 0, zin_end = 0;
    Counters* C = nullptr;
    Source() = default;
    Source(const Source&) = delete;
    Source& operator=(const Source&) = delete;
    ~Source() { if (zs_open) inflateEnd(&zs); if (fd >= 0) close(fd); }

    void read_at(void* dst, size_t n, uint64_t off) {
        const double t0 = clock_ms();
        pread_all(fd, dst, n, off, path.c_str());
        C->ms_read += clock_ms() - t0; C->bytes_read += n;
    }
    void open(const char* p, Counters* c) {
        path = p; C = c;
        if (has_suffix(path, ".lz4") || has_suffix(path, ".br")) fail(LCTY_ERR_UNSUPPORTED, "%s: FASTA / FASTQ input is read plain or gzip-compressed", p);
        fd = ::open(p, O_RDONLY | O_CLOEXEC);
        if (fd < 0) fail(LCTY_ERR_INVALID_INPUT, "cannot open %s", p);
        struct stat st;
        if (fstat(fd, &st) != 0) fail(LCTY_ERR_RUNTIME, "cannot stat %s", p);
        fsize = static_cast<uint64_t>(st.st_size);
        uint8_t hd[0x10000];
        const size_t n = static_cast<size_t>(std::min<uint64_t>(sizeof(hd), fsize));
        if (n) pread_all(fd, hd, n, 0, p);
        BgzfHead h;
        if (bgzf_head(hd, n, h) == BGZF_OK) kind = BGZF;
        else if (n >= 2 && hd[0] == 0x1f && hd[1] == 0x8b) {
            kind = GZIP;
            memset(&zs, 0, sizeof(zs));
            if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateInit2");
            zs_open = true;
            zin.resize(1u << 20);
        }
        eof = fsize == 0;
    }
    // plain and gzip: up to `want` bytes of text to dst; fewer only at the end of the stream
    uint64_t fill(uint8_t* dst, uint64_t want) {
        if (kind == PLAIN) {
            const uint64_t n = std::min<uint64_t>(want, fsize - at);
            if (n) read_at(dst, n, at);
            at += n; eof = at >= fsize;
            return n;
        }
        uint64_t got = 0;
        while (got < want && !eof) {
            if (zin_at == zin_end) {
                const size_t n = static_cast<size_t>(std::min<uint64_t>(zin.size(), fsize - at));
                if (!n) fail(LCTY_ERR_INVALID_DATA, "%s: unexpected end of file", path.c_str());
                read_at(zin.data(), n, at);
                at += n; zin_at = 0; zin_end = n;
            }
            const double t0 = clock_ms();
            zs.next_in = zin.data() + zin_at; zs.avail_in = static_cast<uInt>(zin_end - zin_at);
            const uInt room = static_cast<uInt>(std::min<uint64_t>(want - got, 1u << 30));
            zs.next_out = dst + got; zs.avail_out = room;
            const int rc = inflate(&zs, Z_NO_FLUSH);
            zin_at = zin_end - zs.avail_in; got += room - zs.avail_out;
            if (rc == Z_STREAM_END) {                                            // the next member, or the end of the file
                if (zin_at == zin_end && at >= fsize) eof = true;
                else if (zin_at < zin_end && zin[zin_at] != 0x1f) eof = true;     // what follows is no gzip member: gzread ignores it as well
                else if (inflateReset(&zs) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateReset");
            } else if (rc != Z_OK && rc != Z_BUF_ERROR) fail(LCTY_ERR_INVALID_DATA, "%s: %s", path.c_str(), zs.msg ? zs.msg : "corrupt gzip stream");
            C->ms_inflate += clock_ms() - t0;
        }
        C->bytes_inflated += got;
        return got;
    }
    // BGZF: the next whole blocks, at least one and then as long as they inflate to at most `want` bytes: comp grows by their bytes,
    // blocks by them (out_at from out0 on). Returns their inflated size.
    uint64_t take_blocks(uint64_t want, uint64_t out0, std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks) {
        uint64_t total = 0;
        const uint64_t span = std::min<uint64_t>(fsize - at, want + 0x10000);     // blocks seldom grow: the text is at least as long
        const size_t in0 = comp.size();
        comp.resize(in0 + span);
        if (span) read_at(comp.data() + in0, span, at);
        uint64_t used = 0;
        while (used < span) {
            BgzfHead h;
            const BgzfVerdict v = bgzf_head(comp.data() + in0 + used, span - used, h);
            if (v == BGZF_TOO_LARGE) fail(LCTY_ERR_INVALID_DATA, "%s: a BGZF block of %u bytes", path.c_str(), h.isize);
            if (v == BGZF_NOT_A_BLOCK) {
                if (used == 0 || at + span >= fsize) fail(LCTY_ERR_INVALID_DATA, "%s: not a BGZF block at offset %llu", path.c_str(), static_cast<unsigned long long>(at + used));
                break;                                                            // a block cut by the end of what was read
            }
            if (!blocks.empty() && total + h.isize > want && total) break;
            blocks.push_back(BgzfBlock{h.csize, h.isize, out0 + total, in0 + static_cast<size_t>(used), at + used, h.head});
            total += h.isize; used += h.csize;
        }
        comp.resize(in0 + used);
        C->bytes_read -= span - used;
        at += used; eof = at >= fsize;
        C->bytes_inflated += total;
        return total;
    }
};

enum Stop : int { S_NONE = 0, S_EOF = 1, S_END = 2, S_ERR = 3 };

template <class Exec> struct FileWin {
    Source src;
    typename Exec::Buffer buf;
    uint64_t n = 0;                       // bytes of text in buf
    bool started = false, final = false, fasta = false;
    Parsed P;
    uint32_t cur = 0, n_good = 0, covered = 0, stop_cls = 0;
    int stop = S_NONE;                    // what lies behind record n_good - 1: more text to read, the end, or a refused record
    uint32_t left() const { return n_good - cur; }
};

// the records of one call: mate e of unit i is record rec0[e] + stride * i of file[e]
struct Chunk { uint32_t k = 0; int per = 1; int file[2] = {0, 0}; uint32_t rec0[2] = {0, 0}; uint32_t stride = 1; };

template <class Exec> struct Stream {
    Exec& exec;
    FileWin<Exec> f[2];
    bool two_files = false, interleaved = false, paired = false, done = false;
    std::string what;
    uint64_t window_bytes = WINDOW_DEFAULT, window_cap = WINDOW_LIMIT;
    Counters C;
    uint32_t pair_ok = 0; bool pair_bad = false;      // two files: units from the cursors on whose names are known to match; a mismatch behind them

    explicit Stream(Exec& e) : exec(e) {}

    void open(const char* path1, const char* path2, bool inter, uint64_t window, uint64_t cap) {
        if (window < WINDOW_MIN) fail(LCTY_ERR_INVALID_INPUT, "fastx_window_bytes = %llu (at least %llu)", static_cast<unsigned long long>(window), static_cast<unsigned long long>(WINDOW_MIN));
        window_cap = std::min<uint64_t>(cap, WINDOW_LIMIT);
        window_bytes = std::min(window, window_cap);
        f[0].src.open(path1, &C);
        what = path1;
        if (path2) { f[1].src.open(path2, &C); two_files = true; what += std::string(" and ") + path2; }
        interleaved = inter; paired = two_files || interleaved;
    }

    std::string name_of(const FileWin<Exec>& w, uint32_t rec) const {
        const Row& r = w.P.rows[rec];
        return std::string(reinterpret_cast<const char*>(w.buf.data()) + r.name_beg, r.name_len);
    }
    [[noreturn]] void raise(const FileWin<Exec>& w, uint32_t rec, uint32_t cls) const {
        const std::string name = name_of(w, rec);
        if (cls == C_MIXED) fail(LCTY_ERR_UNSUPPORTED, "%s: record %s: FASTA and FASTQ records in one file (the device route reads one format per file)", w.src.path.c_str(), name.c_str());
        if (cls == C_INCOMPLETE) fail(LCTY_ERR_INVALID_DATA, "Fastq record %s is incomplete", name.c_str());
        if (cls == C_FORMAT) fail(LCTY_ERR_INVALID_DATA, "Fastq record %s has incorrect format", name.c_str());
        if (cls == C_NONMATCH) fail(LCTY_ERR_INVALID_DATA, "Fastq record %s has non-matching sequence and qualities", name.c_str());
        if (cls == C_EMPTY_FASTA) fail(LCTY_ERR_INVALID_DATA, "Fasta record %s has an empty sequence.", name.c_str());
        fail(LCTY_ERR_RUNTIME, "%s: unknown class %u of record %s", w.src.path.c_str(), cls, name.c_str());
    }

    // the next window of file w: the tail of the last one, then window_bytes of text; doubled until it holds a complete record
    void refill(int fi) {
        FileWin<Exec>& w = f[fi];
        uint64_t tail_beg = w.started ? w.covered : 0, tail_n = w.n - tail_beg, want = window_bytes;
        for (;;) {
            if (tail_n + want > window_cap) want = window_cap > tail_n ? window_cap - tail_n : 0;
            if (w.src.kind == Source::PLAIN) want = std::min<uint64_t>(want, w.src.fsize - w.src.at);      // no larger buffer than the file fills
            if (!want && !w.src.eof)
                fail(LCTY_ERR_UNSUPPORTED, "%s: a record of more than %llu bytes (windows of text hold at most 2^31 - 64 bytes; knob fastx_window_bytes sets where they start)",
                     w.src.path.c_str(), static_cast<unsigned long long>(window_cap));
            typename Exec::Buffer nb;
            uint64_t got = 0;
            if (w.src.kind == Source::BGZF && !w.src.eof) {
                std::vector<uint8_t> comp; std::vector<BgzfBlock> blocks;
                got = w.src.take_blocks(want, tail_n, comp, blocks);
                if (tail_n + got > window_cap)
                    fail(LCTY_ERR_UNSUPPORTED, "%s: a record of more than %llu bytes (windows of text hold at most 2^31 - 64 bytes; knob fastx_window_bytes sets where they start)",
                         w.src.path.c_str(), static_cast<unsigned long long>(window_cap));
                const double t0 = clock_ms();
                exec.inflate(nb, comp, blocks, tail_n + got, w.src.path.c_str());
                C.ms_inflate += clock_ms() - t0;
            } else {
                exec.alloc(nb, tail_n + want);
                if (!w.src.eof) got = w.src.fill(nb.data() + tail_n, want);
            }
            if (tail_n) exec.put_front(nb, w.buf.data() + tail_beg, tail_n);
            w.buf = std::move(nb);
            w.n = tail_n + got; w.final = w.src.eof;
            if (!w.started) { w.fasta = w.n > 0 && w.buf.data()[0] == '>'; w.started = true; }
            C.windows++;
            w.P = Parsed();
            exec.parse(fi, w.buf, static_cast<uint32_t>(w.n), w.final, w.fasta, w.P);
            w.cur = 0; w.n_good = w.P.n_rec; w.covered = w.P.covered; w.stop = w.final ? S_EOF : S_NONE; w.stop_cls = 0;
            if (interleaved && !w.final && (w.n_good & 1u)) { w.n_good--; w.covered = w.P.rows[w.n_good].name_beg - 1; }
            if (interleaved && w.n_good >= 2) {                                  // the names of the pairs, behind every class of the records themselves
                const uint32_t bad = exec.mismatch(fi, 0, 2, fi, 1, 2, w.n_good / 2);
                if (bad < w.n_good / 2 && (w.P.ev_rec == NO_EVENT || 2 * bad + 1 < w.P.ev_rec)) { w.P.ev_rec = 2 * bad + 1; w.P.ev_cls = C_MISMATCH; }
            }
            if (w.P.ev_rec != NO_EVENT && w.P.ev_rec < w.P.n_rec && w.P.ev_rec <= w.n_good) {
                w.n_good = w.P.ev_rec; w.stop_cls = w.P.ev_cls; w.stop = w.P.ev_cls == C_END ? S_END : S_ERR;
            }
            if (w.n_good > 0 || w.stop != S_NONE) return;
            tail_beg = 0; tail_n = w.n; want = std::max<uint64_t>(w.n, window_bytes);      // no complete record: the window is doubled and read on
            C.windows_enlarged++;
        }
    }

    // up to max_units records (pairs, when paired) of the current windows; k = 0 at the end of the input
    Chunk next(uint64_t max_units) {
        Chunk c;
        c.per = paired ? 2 : 1;
        if (done || max_units == 0) return c;
        for (;;) {
            FileWin<Exec>& a = f[0];
            if (!two_files) {
                const uint32_t per = interleaved ? 2u : 1u;
                if (!a.started || (a.left() < per && a.stop == S_NONE)) { refill(0); continue; }
                if (a.left() >= per) {
                    c.k = static_cast<uint32_t>(std::min<uint64_t>(max_units, a.left() / per));
                    c.rec0[0] = a.cur; c.rec0[1] = a.cur + 1; c.stride = per;
                    a.cur += per * c.k; C.records += static_cast<uint64_t>(per) * c.k;
                    return c;
                }
                if (a.left() == 1) {                                             // interleaved: a first mate, and what stopped the second
                    if (a.stop == S_ERR && a.stop_cls == C_MISMATCH)
                        fail(LCTY_ERR_INVALID_DATA, "Interleaved input file(s) %s contains non matching first and second mate (%s and %s)", what.c_str(),
                             name_of(a, a.cur).c_str(), name_of(a, a.cur + 1).c_str());
                    if (a.stop == S_ERR) raise(a, a.n_good, a.stop_cls);
                    fail(LCTY_ERR_INVALID_DATA, "Odd number of records in an interleaved input file(s) %s", what.c_str());
                }
                if (a.stop == S_ERR) raise(a, a.n_good, a.stop_cls);
                done = true;
                return c;
            }
            FileWin<Exec>& b = f[1];
            if (!a.started || (a.left() == 0 && a.stop == S_NONE)) { refill(0); pair_ok = 0; pair_bad = false; continue; }
            if (!b.started || (b.left() == 0 && b.stop == S_NONE)) { refill(1); pair_ok = 0; pair_bad = false; continue; }
            const uint32_t avail = std::min(a.left(), b.left());
            if (avail) {
                if (!pair_ok && !pair_bad) { pair_ok = exec.mismatch(0, a.cur, 1, 1, b.cur, 1, avail); pair_bad = pair_ok < avail; }
                if (!pair_ok)
                    fail(LCTY_ERR_INVALID_DATA, "Paired-end input files %s have non matching first and second mates (%s and %s)", what.c_str(),
                         name_of(a, a.cur).c_str(), name_of(b, b.cur).c_str());
                c.k = static_cast<uint32_t>(std::min<uint64_t>(max_units, pair_ok));
                c.file[1] = 1; c.rec0[0] = a.cur; c.rec0[1] = b.cur; c.stride = 1;
                a.cur += c.k; b.cur += c.k; pair_ok -= c.k; C.records += 2ull * c.k;
                return c;
            }
            // one of the two has no record here: the first file's refusal, then the second's, then the count (read_unit's order)
            if (a.left() == 0 && a.stop == S_ERR) raise(a, a.n_good, a.stop_cls);
            if (b.left() == 0 && b.stop == S_ERR) raise(b, b.n_good, b.stop_cls);
            if (a.left() == 0 && b.left() == 0) { done = true; return c; }
            fail(LCTY_ERR_INVALID_DATA, "Different number of records in paired-end input files %s", what.c_str());
        }
    }

    // ---- the text of a record of the current windows, for the writers and the tests
    void sequence(const FileWin<Exec>& w, uint32_t rec, std::string& out) const {
        const Row& r = w.P.rows[rec];
        const char* t = reinterpret_cast<const char*>(w.buf.data());
        if (!w.fasta) { out.append(t + r.seq, r.len); return; }
        Text T{w.buf.data(), static_cast<uint32_t>(w.n), w.P.nl.data(), static_cast<uint32_t>(w.P.nl.size()), static_cast<uint32_t>(w.P.cum.size() - 1)};
        uint32_t have = 0;
        for (uint32_t j = r.seq + 1; have < r.len; j++) {
            uint32_t b, e;
            line_span(T, j, b, e);
            out.append(t + b, e - b); have += e - b;
        }
    }
    void qualities(const FileWin<Exec>& w, uint32_t rec, std::string& out) const {
        if (w.fasta) return;
        const Row& r = w.P.rows[rec];
        out.append(reinterpret_cast<const char*>(w.buf.data()) + fastq_qual_begin(w.buf.data(), r), r.len);
    }
    // write_fastq / write_fasta (fastx.rs:46-75, 262-272) as record_text of lcty_fastx.hip: FASTA when there are no qualities
    void record_text(const FileWin<Exec>& w, uint32_t rec, std::string& out) const {
        const Row& r = w.P.rows[rec];
        const bool fasta = w.fasta || r.len == 0;
        out += fasta ? '>' : '@';
        out.append(reinterpret_cast<const char*>(w.buf.data()) + r.name_beg, r.name_len);
        out += '\n';
        sequence(w, rec, out);
        out += '\n';
        if (!fasta) { out += "+\n"; qualities(w, rec, out); out += '\n'; }
    }
};

}  // namespace fastx
}  // namespace lcty
