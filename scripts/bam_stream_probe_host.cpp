// bam_stream_probe_host.cpp — the host half of the reader of whole BAM files in windows (locityper_amd/csrc/lcty_bam_stream_window.hpp:
// containers, windows, the carried tail, enlargement, the change of file, the order of errors) on the CPU (no HIP), with a serial
// executor in place of the kernels of lcty_bam_stream.hip, for tests/test_bam_stream_host.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/bam_stream_probe_host.cpp -lz
//       -o bam_stream_probe_host && ./bam_stream_probe_host DIR/corpus.tsv
// The corpus is what tests/bam_stream_cases.py writes (write_corpus): name, interleaved, the paths joined by ',' per line. Every case
// is read with windows of 1, 64, 777 and 4 096 bytes and the default; a window lives in a buffer of exactly its size, so that a read
// outside it is the sanitizer's to see. The program prints, per case, the reads in front of the first error (ordinals among the kept
// records of the whole input, names, restored sequences), the status with its message and the totals, and exits 1 when two window
// sizes disagree on any of them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "lcty_bam_stream_window.hpp"

using namespace lcty;
using namespace lcty::bam_stream;

namespace {

struct SerialExec {
    std::vector<uint8_t> buf;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> stream;
    std::vector<uint32_t> src, src_stream;                // of the current chunk: record and stream place of mate m (NO_RECORD: absent)

    uint8_t* alloc(uint64_t n) { buf.assign(n, 0); buf.shrink_to_fit(); return buf.data(); }
    uint8_t* inflate(std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks, uint64_t total, const char* path) {
        alloc(total);
        bgzf_inflate_host(comp.data(), blocks, buf.data(), path, 1);
        return buf.data();
    }
    void put_front(const uint8_t* p, uint64_t n) { memcpy(buf.data(), p, n); }
    std::vector<uint64_t>& rec_off() { return offs; }

    uint32_t u32(uint64_t o) const { uint32_t v; memcpy(&v, buf.data() + o, 4); return v; }
    void scan(bool interleaved, Scanned& S) {
        stream.clear();
        uint64_t ev = ~0ull;
        auto refuse = [&](uint32_t r, uint32_t cls) { ev = std::min<uint64_t>(ev, (static_cast<uint64_t>(r) << 8) | cls); };
        std::vector<uint32_t> before(offs.size() + 1, 0);
        for (uint32_t r = 0; r < offs.size(); r++) {
            const uint64_t o = offs[r];
            const uint32_t block = u32(o), l_name = buf[o + 12], nf = u32(o + 16), l_seq = u32(o + 20);
            const bool fits = 32ull + l_name + 4ull * (nf & 0xFFFFu) + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq <= block;
            const bool primary = fits && ((nf >> 16) & 0x900u) == 0;
            if (!fits) refuse(r, E_SHORT);
            else if (primary && l_seq == 0) refuse(r, E_NOSEQ);
            before[r] = static_cast<uint32_t>(stream.size());
            if (primary) { stream.push_back(r); S.n_primary++; }
        }
        before[offs.size()] = static_cast<uint32_t>(stream.size());
        S.n_kept = static_cast<uint32_t>(stream.size());
        if (interleaved) {
            for (size_t i = 0; 2 * i < stream.size(); i++) {
                if (2 * i + 1 == stream.size()) { S.wait_rec = stream[2 * i]; break; }
                const uint64_t oa = offs[stream[2 * i]], ob = offs[stream[2 * i + 1]];
                const uint32_t la = buf[oa + 12], lb = buf[ob + 12], n = la ? la - 1 : 0;
                if (!(la == lb && (n <= 3 || buf[oa + 36 + n - 3] == buf[ob + 36 + n - 3]))) refuse(stream[2 * i + 1], E_MISMATCH);
            }
        }
        if (ev != ~0ull) {
            S.ev_rec = static_cast<uint32_t>(ev >> 8); S.ev_cls = static_cast<uint32_t>(ev & 0xFF);
            S.kept_before_ev = before[S.ev_rec];
            if (S.ev_cls == E_MISMATCH) S.ev_first = stream[S.kept_before_ev - 1];
        }
    }
    uint64_t emit(uint32_t n_lim, uint32_t n_out, bool interleaved) {
        src.assign(2ull * n_out, NO_RECORD); src_stream.assign(2ull * n_out, NO_RECORD);
        uint64_t bases = 0;
        for (uint32_t i = 0; i < n_out; i++)
            for (uint32_t e = 0; e < (interleaved ? 2u : 1u); e++) {
                const uint32_t s = interleaved ? 2 * i + e : i;
                if (s >= n_lim) { fprintf(stderr, "place %u of %u\n", s, n_lim); exit(3); }
                src[2 * i + e] = stream[s]; src_stream[2 * i + e] = s;
                bases += u32(offs[stream[s]] + 20);
            }
        return bases;
    }
    // the sequence as the sequencer gave it
    std::string restored(uint32_t r) const {
        static const char CODES[] = "=ACMGRSVTWYHKDBN";
        const uint64_t o = offs[r];
        const uint32_t nf = u32(o + 16), l_seq = u32(o + 20);
        const uint8_t* seq = buf.data() + o + 36 + buf[o + 12] + 4ull * (nf & 0xFFFFu);
        const bool reverse = ((nf >> 16) & 0x10u) != 0;
        std::string out;
        for (uint32_t k = 0; k < l_seq; k++) {
            const uint32_t j = reverse ? l_seq - 1 - k : k;
            const char c = CODES[(seq[j >> 1] >> ((j & 1) ? 0 : 4)) & 15];
            out += !reverse ? c : c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
        }
        return out;
    }
};

struct Result { int32_t code = LCTY_OK; std::string msg, reads; Counters C; uint64_t chunks = 0; };

Result run(const std::vector<std::string>& paths, bool interleaved, int64_t window, int64_t limit) {
    Result R;
    SerialExec exec;
    Stream<SerialExec> st(exec);
    std::vector<const char*> p;
    for (const std::string& s : paths) p.push_back(s.c_str());
    try {
        st.open(p.data(), static_cast<uint32_t>(p.size()), interleaved, window, limit);
        for (;;) {
            const Chunk c = st.next();
            if (!c.n) break;
            R.chunks++;
            for (uint64_t i = 0; i < c.n; i++) {
                R.reads += "unit";
                for (uint32_t e = 0; e < 2; e++) {
                    const uint32_t r = exec.src[2 * i + e];
                    if (r == NO_RECORD) { R.reads += " -"; continue; }
                    R.reads += " " + std::to_string(st.C.first_kept + exec.src_stream[2 * i + e]) + " [" + name_at(exec.buf.data(), exec.offs[r]) + "] " + exec.restored(r);
                }
                R.reads += "\n";
            }
        }
        // the failure stays: the next call gives the same status
    } catch (const Error& e) {
        R.code = e.code; R.msg = e.what();
        try { st.next(); R.msg += " (and then nothing)"; } catch (const Error& again) { if (again.code != e.code || R.msg != again.what()) R.msg += " (and then another)"; }
    }
    R.C = st.C;
    return R;
}

std::string totals(const Counters& C) {
    return std::to_string(C.records_walked) + " " + std::to_string(C.records_primary) + " " + std::to_string(C.records_kept) + " " + std::to_string(C.bases_kept) + " " +
           std::to_string(C.reads);
}

}  // namespace

namespace lcty { void set_last_error(const std::string&) {} }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: bam_stream_probe_host DIR/corpus.tsv\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    unsigned cases = 0, runs = 0, bad = 0;
    uint64_t enlarged = 0, carried = 0;
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string x; std::getline(ss, x, '\t');) f.push_back(x);
        if (f.size() != 3) { fprintf(stderr, "bad corpus line: %s\n", line.c_str()); return 2; }
        std::vector<std::string> paths;
        std::stringstream ps(f[2]);
        for (std::string x; std::getline(ps, x, ',');) paths.push_back(x);
        const bool interleaved = f[1] == "1";
        const Result want = run(paths, interleaved, static_cast<int64_t>(WINDOW_DEFAULT), static_cast<int64_t>(LIMIT_DEFAULT));
        cases++;
        std::stringstream rs(want.reads);
        for (std::string x; std::getline(rs, x);) printf("%s %s\n", f[0].c_str(), x.c_str());
        printf("%s status %d %s\n", f[0].c_str(), want.code, want.msg.c_str());
        printf("%s totals %s\n", f[0].c_str(), totals(want.C).c_str());
        for (int64_t window : {1ll, 64ll, 777ll, 4096ll}) {
            const Result got = run(paths, interleaved, window, static_cast<int64_t>(LIMIT_DEFAULT));
            runs++; enlarged += got.C.windows_enlarged; carried += got.C.bytes_carried;
            if (got.code != want.code || got.msg != want.msg || got.reads != want.reads || totals(got.C) != totals(want.C)) {
                fprintf(stderr, "%s: window %lld: status %d (%s), totals %s; with one window %d (%s), totals %s; %zu and %zu bytes of reads\n", f[0].c_str(),
                        static_cast<long long>(window), got.code, got.msg.c_str(), totals(got.C).c_str(), want.code, want.msg.c_str(), totals(want.C).c_str(),
                        got.reads.size(), want.reads.size());
                bad++;
            }
        }
    }
    printf("bam_stream_probe_host: %u cases, %u windowed runs, %llu enlarged windows, %llu bytes carried, %u differences\n", cases, runs,
           static_cast<unsigned long long>(enlarged), static_cast<unsigned long long>(carried), bad);
    return bad ? 1 : 0;
}
