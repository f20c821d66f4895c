// lcty_bam_stream_window.hpp — the host half of the reader of whole, unindexed BAM files in windows (lcty_bam_stream.hip, DESIGN.md
// 5w): `locityper genotype|recruit -a reads.bam [-a ...] --no-index [-^]`, DirectBamReader (src/seq/fastx.rs:692-729) under
// PairedEndInterleaved (423-453). The files with their headers, windows of whole BGZF blocks of the current file, the chain of record
// lengths, the tail of one window carried to the front of the next (a partial record; with interleaved pairs a first mate that still
// waits, with whatever lies behind it), the enlarging of a window that completes no record, the change of file, and which record's
// error wins (the first in input order; reads completed in front of it are handed out first). Host code without HIP: what runs on the
// records of a window, and where its bytes live, is the executor's (Exec), so that scripts/bam_stream_probe_host.cpp runs all of this
// with a serial one.
//   exec.alloc(n) / exec.inflate(comp, blocks, total, path)   the window's buffer of n (total) bytes, the blocks inflated to their
//                                     out_at; the bytes in front of the first block stay free. Returns the host's bytes.
//   exec.put_front(p, n)              the carried tail, written after either of the two
//   exec.rec_off()                    where the walk leaves the byte of every record of the window
//   exec.scan(interleaved, S)         kept flags, their stream, the name check of its pairs, the first (record, class)
//   exec.emit(n_lim, n_out, interleaved)   the reads of stream places [0, n_lim) laid out and unpacked; returns their bases
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "lcty_bgzf.hpp"

namespace lcty {
namespace bam_stream {

constexpr uint64_t WINDOW_DEFAULT = 1ull << 28, LIMIT_DEFAULT = 1ull << 33;
constexpr uint64_t MAX_RECORDS = 0x7FFFFFF0ull;                      // 2^31 - 16: record ordinals of a window are 32-bit
constexpr uint32_t NO_RECORD = 0xFFFFFFFFu;
// classes of a record's error, by rank at one record; T_*: found by the walk, behind the last record it took
enum : uint32_t { E_SHORT = 1, E_NOSEQ = 4, E_MISMATCH = 7, T_SHORT = 100, T_CUT = 101 };

inline double clock_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// what an executor's scan of one window leaves
struct Scanned {
    uint32_t n_kept = 0, n_primary = 0;
    uint32_t ev_rec = NO_RECORD, ev_cls = 0;          // the smallest (record, class)
    uint32_t kept_before_ev = 0;                      // kept records in front of ev_rec
    uint32_t ev_first = NO_RECORD;                    // E_MISMATCH: the record of the first mate
    uint32_t wait_rec = NO_RECORD;                    // interleaved: the record at an odd last place of the stream
};

struct Counters {
    uint64_t files = 0, file_bytes = 0, bytes_read = 0, blocks_inflated = 0, bytes_inflated = 0, windows = 0, windows_enlarged = 0, bytes_carried = 0;
    uint64_t records_walked = 0, records_primary = 0, records_kept = 0, bases_kept = 0, reads = 0, first_kept = 0;
    double ms_read = 0, ms_inflate = 0, ms_walk = 0;
};

struct File {
    std::string path;
    int fd = -1;
    uint64_t fsize = 0, at = 0;           // the next block of the file
    uint32_t lead = 0;                    // bytes of the header in the block the first record lies in
    bool started = false;
    File() = default;
    File(const File&) = delete;
    File& operator=(const File&) = delete;
    ~File() { if (fd >= 0) close(fd); }

    // DirectBamReader::new: the header is read now; the contigs are ignored, no index is looked for
    void open(const char* p) {
        path = p;
        fd = ::open(p, O_RDONLY | O_CLOEXEC);
        if (fd < 0) fail(LCTY_ERR_INVALID_INPUT, "cannot open %s", p);
        struct stat st;
        if (fstat(fd, &st) != 0) fail(LCTY_ERR_RUNTIME, "cannot stat %s", p);
        fsize = static_cast<uint64_t>(st.st_size);
        if (fsize >= (1ull << 48)) fail(LCTY_ERR_UNSUPPORTED, "%s: a file of 2^48 bytes or more", p);
        std::vector<uint8_t> hd(static_cast<size_t>(std::min<uint64_t>(0x10000, fsize)));
        if (!hd.empty()) pread_all(fd, hd.data(), hd.size(), 0, p);
        if (hd.size() >= 4 && memcmp(hd.data(), "CRAM", 4) == 0) fail(LCTY_ERR_UNSUPPORTED, "%s is a CRAM file (only BAM files are read)", p);
        BgzfHead h;
        if (bgzf_head(hd.data(), hd.size(), h) != BGZF_OK) fail(LCTY_ERR_INVALID_DATA, "%s is not a BAM file", p);
        BgzfSerial in(fd, fsize, p);
        uint8_t head[8];
        if (!in.read(head, 8) || memcmp(head, "BAM\1", 4) != 0) fail(LCTY_ERR_INVALID_DATA, "%s is not a BAM file", p);
        uint32_t l_text, n_ref = 0;
        memcpy(&l_text, head + 4, 4);
        auto skip = [&](uint64_t n) {
            uint8_t buf[4096];
            while (n) {
                const size_t k = static_cast<size_t>(std::min<uint64_t>(n, sizeof(buf)));
                if (!in.read(buf, k)) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM header", p);
                n -= k;
            }
        };
        skip(l_text);
        if (!in.read(&n_ref, 4)) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM header", p);
        for (uint32_t r = 0; r < n_ref; r++) {
            uint32_t l_name = 0;
            if (!in.read(&l_name, 4)) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM header", p);
            skip(static_cast<uint64_t>(l_name) + 4);
        }
        (void)in.load();
        const uint64_t first = in.tell();
        at = std::min(first >> 16, fsize); lead = static_cast<uint32_t>(first & 0xFFFF);
    }
};

inline std::string name_at(const uint8_t* buf, uint64_t o) {
    const uint32_t l = buf[o + 12];
    std::string s(reinterpret_cast<const char*>(buf + o + 36), l ? l - 1 : 0);
    const size_t z = s.find('\0');
    if (z != std::string::npos) s.resize(z);
    return s;
}

struct Chunk { uint64_t n = 0; };

template <class Exec> struct Stream {
    Exec& exec;
    std::vector<std::unique_ptr<File>> files;
    bool interleaved = false;
    uint64_t window_bytes = WINDOW_DEFAULT, window_limit = LIMIT_DEFAULT, want = WINDOW_DEFAULT;
    std::string what;                                 // ext::fmt::paths of the files
    size_t fi = 0;
    std::vector<uint8_t> carry;
    uint32_t carried_recs = 0; bool carried_mate = false;     // complete records at the front of carry; the first of them is a waiting first mate
    bool failed = false, done = false;
    int32_t err_code = LCTY_OK; std::string err_msg;
    Counters C;

    explicit Stream(Exec& e) : exec(e) {}

    void open(const char* const* paths, uint32_t n_paths, bool inter, int64_t window, int64_t limit) {
        if (window < 1) fail(LCTY_ERR_INVALID_INPUT, "bam_stream_window_bytes = %lld (at least 1)", static_cast<long long>(window));
        if (limit < 1) fail(LCTY_ERR_INVALID_INPUT, "bam_stream_window_limit = %lld (at least 1)", static_cast<long long>(limit));
        window_limit = static_cast<uint64_t>(limit);
        window_bytes = std::min<uint64_t>(static_cast<uint64_t>(window), window_limit);
        want = window_bytes;
        interleaved = inter;
        for (uint32_t i = 0; i < n_paths; i++) {
            if (!paths[i]) fail(LCTY_ERR_INVALID_INPUT, "null argument");
            files.emplace_back(new File());
            files.back()->open(paths[i]);
            C.file_bytes += files.back()->fsize;
            if (i) what += ", ";
            what += paths[i];
        }
        C.files = n_paths;
    }

    // whole blocks of f until they inflate to `need` bytes or the file ends: comp grows by their bytes, blocks by them (out_at from out0 on)
    uint64_t take(File& f, uint64_t need, uint64_t out0, std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks) {
        uint64_t total = 0;
        while (total < need && f.at < f.fsize) {
            const uint64_t span = std::min<uint64_t>(f.fsize - f.at, (need - total) + 0x10000);     // a block holds at most 64 KiB either way
            const size_t in0 = comp.size();
            comp.resize(in0 + span);
            const double t0 = clock_ms();
            pread_all(f.fd, comp.data() + in0, span, f.at, f.path.c_str());
            C.ms_read += clock_ms() - t0;
            uint64_t used = 0;
            while (used < span && total < need) {
                BgzfHead h;
                const BgzfVerdict v = bgzf_head(comp.data() + in0 + used, span - used, h);
                if (v == BGZF_TOO_LARGE) fail(LCTY_ERR_INVALID_DATA, "%s: a BGZF block of %u bytes", f.path.c_str(), h.isize);
                if (v == BGZF_NOT_A_BLOCK) {
                    if (used == 0) fail(LCTY_ERR_INVALID_DATA, "%s: truncated or corrupt BGZF block at offset %llu", f.path.c_str(), static_cast<unsigned long long>(f.at));
                    break;                                                        // a block cut by the end of what was read
                }
                blocks.push_back(BgzfBlock{h.csize, h.isize, out0 + total, in0 + static_cast<size_t>(used), f.at + used, h.head});
                total += h.isize; used += h.csize;
            }
            comp.resize(in0 + used);
            C.bytes_read += used; f.at += used;
        }
        C.bytes_inflated += total;
        return total;
    }

    void set_error(int32_t code, const std::string& msg) { failed = true; err_code = code; err_msg = msg; }

    // One window. Returns the reads it completes; an error behind them is kept for the next call.
    uint64_t window() {
        File& f = *files[fi];
        const char* path = f.path.c_str();
        const bool first = !f.started;
        f.started = true;
        const uint64_t carry_n = carry.size();
        uint64_t lead_left = first ? f.lead : 0;
        std::vector<uint8_t> comp; std::vector<BgzfBlock> blocks;
        const uint64_t taken = take(f, want > carry_n ? want - carry_n : 1, carry_n, comp, blocks);
        const uint64_t n = carry_n + taken;
        const bool file_end = f.at >= f.fsize;
        C.blocks_inflated += blocks.size();
        C.windows++;
        const uint8_t* buf = nullptr;
        if (n) {
            const double t0 = clock_ms();
            buf = blocks.empty() ? exec.alloc(n) : exec.inflate(comp, blocks, n, path);
            if (carry_n) exec.put_front(carry.data(), carry_n);
            C.ms_inflate += clock_ms() - t0;
        }
        // ---- the chain of record lengths
        const double t0 = clock_ms();
        std::vector<uint64_t>& rec_off = exec.rec_off();
        rec_off.clear();
        uint64_t p = 0;
        uint32_t tail = 0;
        for (;;) {
            if (p == carry_n && lead_left) { p += lead_left; lead_left = 0; }
            if (p >= n) break;
            uint32_t bs = 0;
            if (p + 4 <= n) memcpy(&bs, buf + p, 4);
            if (p + 4 <= n && bs < 32) { tail = T_SHORT; break; }
            if (p + 4 > n || p + 4 + bs > n) { if (file_end) tail = T_CUT; break; }
            rec_off.push_back(p);
            p += 4ull + bs;
        }
        C.ms_walk += clock_ms() - t0;
        const uint64_t n_rec = rec_off.size();
        if (n_rec >= MAX_RECORDS) fail(LCTY_ERR_UNSUPPORTED, "%s: %llu records in one window (knob bam_stream_window_bytes)", path, static_cast<unsigned long long>(n_rec));

        // ---- the records: kept stream, pairs, the first error
        Scanned S;
        if (n_rec) exec.scan(interleaved, S);
        const bool dev_err = S.ev_rec != NO_RECORD;
        const uint64_t r_err = dev_err ? S.ev_rec : n_rec;
        const uint32_t cls = dev_err ? S.ev_cls : tail;
        const uint32_t n_lim = dev_err ? S.kept_before_ev : S.n_kept;
        const uint64_t n_out = interleaved ? n_lim / 2 : n_lim;
        const uint64_t rec_base = C.records_walked - carried_recs;               // ordinal in the whole input of record 0 of this window
        C.first_kept = C.records_kept - (carried_mate ? 1 : 0);
        C.records_walked += r_err > carried_recs ? r_err - carried_recs : 0;
        C.records_kept += n_lim - (carried_mate && n_lim ? 1 : 0);
        C.records_primary += (cls ? n_lim : S.n_primary) - (carried_mate && n_lim ? 1 : 0);
        if (n_out) { C.bases_kept += exec.emit(n_lim, static_cast<uint32_t>(n_out), interleaved); C.reads += n_out; }

        if (cls) {
            const unsigned long long ord = rec_base + r_err;
            if (cls == E_SHORT || cls == T_SHORT) set_error(LCTY_ERR_INVALID_DATA, std::string(path) + ": record " + std::to_string(ord) + " is shorter than its fields");
            else if (cls == T_CUT) set_error(LCTY_ERR_INVALID_DATA, std::string(path) + ": record " + std::to_string(ord) + " leaves the end of its file");
            else if (cls == E_NOSEQ) set_error(LCTY_ERR_INVALID_DATA, "Primary alignment for read " + name_at(buf, rec_off[r_err]) + " has no sequence");
            else if (cls == E_MISMATCH)
                set_error(LCTY_ERR_INVALID_DATA, "Interleaved input file(s) " + what + " contains non matching first and second mate (" + name_at(buf, rec_off[S.ev_first]) +
                                                     " and " + name_at(buf, rec_off[r_err]) + ")");
            else set_error(LCTY_ERR_RUNTIME, std::string(path) + ": unknown class " + std::to_string(cls));
            return n_out;
        }

        // ---- what goes to the front of the next window
        const bool no_new = n_rec == carried_recs;
        uint64_t from = p;
        const bool waits = interleaved && (n_lim & 1u);
        if (waits) { from = rec_off[S.wait_rec]; carried_recs = static_cast<uint32_t>(n_rec - S.wait_rec); }
        else carried_recs = 0;
        carried_mate = waits;
        const uint64_t upto = file_end ? p : n;                                  // a partial record never continues in the next file
        std::vector<uint8_t> next_carry;
        if (buf && from < upto) {
            const uint64_t lead_end = first ? carry_n + f.lead : 0;              // the header's bytes between what was carried here and the file's records
            if (from < lead_end) { next_carry.assign(buf + from, buf + carry_n); next_carry.insert(next_carry.end(), buf + lead_end, buf + std::max(lead_end, upto)); }
            else next_carry.assign(buf + from, buf + upto);
        }
        carry.swap(next_carry);
        C.bytes_carried += carry.size();
        if (file_end) {
            fi++; want = window_bytes;
            if (fi == files.size()) {
                if (carried_mate) set_error(LCTY_ERR_INVALID_DATA, "Odd number of records in an interleaved input file(s) " + what);
                else done = true;
            }
        } else if (no_new) {                                                     // no complete record: the window is doubled and read on
            if (n >= window_limit)
                fail(LCTY_ERR_UNSUPPORTED, "%s: a record of more than %llu bytes (knob bam_stream_window_limit)", path, static_cast<unsigned long long>(window_limit));
            want = std::min<uint64_t>(2 * std::max(want, n), window_limit);
            C.windows_enlarged++;
        } else want = window_bytes;
        return n_out;
    }

    // the reads (pairs, when interleaved) of the next window that completes any; n = 0 at the end of the last file
    Chunk next() {
        Chunk c;
        for (;;) {
            if (failed) throw Error(err_code, err_msg);
            if (done) return c;
            if (fi >= files.size()) { done = true; continue; }
            try { c.n = window(); } catch (const Error& e) { set_error(e.code, e.what()); throw; }
            if (c.n) return c;
        }
    }
};

}  // namespace bam_stream
}  // namespace lcty
