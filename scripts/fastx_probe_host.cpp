// fastx_probe_host.cpp — the record rules of locityper_amd/csrc/lcty_fastx_parse.hpp and the windows of lcty_fastx_window.hpp on the CPU
// (no HIP), with a serial executor in place of the kernels of lcty_fastx_device.hip, for tests/test_fastx_parse_host.py:
//   g++ -O2 -std=c++17 -shared -fPIC -I locityper_amd/csrc scripts/fastx_probe_host.cpp -lz -o libfastx_probe_host.so   (ctypes)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/fastx_probe_host.cpp -lz
//       -o fastx_probe_host && ./fastx_probe_host DIR/corpus.tsv                                                        (stand-alone)
// The stand-alone program reads the corpus tests/fastx_cases.py writes (write_corpus): name, kind, interleaved, path 1, path 2 or "-"
// per line. It reads every case with windows of 64, 65, 127 and 4096 bytes and the default, one record a call and without a limit;
// the text of a window lives in a buffer of exactly its size, so that a read outside it is the sanitizer's to see. It exits 1 when
// two window sizes disagree on the records or the error of a case, or the status is not what the kind of the case says.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "lcty_fastx_parse.hpp"
#include "lcty_fastx_window.hpp"

using namespace lcty;
using namespace lcty::fastx;

namespace {

struct SerialExec {
    struct Buffer {
        std::vector<uint8_t> v;
        uint8_t* data() const { return const_cast<uint8_t*>(v.data()); }
    };
    struct FileState { const uint8_t* text = nullptr; const std::vector<Row>* rows = nullptr; } fs[2];

    void alloc(Buffer& b, uint64_t n) { b.v.assign(n, 0); }
    void inflate(Buffer& b, std::vector<uint8_t>& comp, std::vector<BgzfBlock>& blocks, uint64_t total, const char* path) {
        b.v.assign(total, 0);
        bgzf_inflate_host(comp.data(), blocks, b.v.data(), path, 1);
    }
    void put_front(Buffer& b, const uint8_t* p, uint64_t n) { memcpy(b.v.data(), p, n); }

    void parse(int fi, Buffer& buf, uint32_t n, bool final, bool fasta, Parsed& P) {
        const uint8_t* t = buf.data();
        std::vector<uint32_t> nl;
        for (uint32_t p = 0; p < n; p++) if (t[p] == '\n') nl.push_back(p);
        const uint32_t n_nl = static_cast<uint32_t>(nl.size());
        Text T{t, n, nl.data(), n_nl, n_lines_of(n, n_nl, n_nl ? nl.back() : 0, final)};
        uint64_t ev = ~0ull;
        auto refuse = [&](uint32_t r, uint32_t cls) { ev = std::min<uint64_t>(ev, (static_cast<uint64_t>(r) << 8) | cls); };
        if (!fasta) {
            P.n_rec = final ? (T.n_lines + 3) / 4 : n_nl / 4;
            P.rows.resize(P.n_rec);
            for (uint32_t r = 0; r < P.n_rec; r++) { const uint32_t cls = fastq_record(T, r, P.rows[r]); if (cls) refuse(r, cls); }
            P.covered = final ? n : P.n_rec ? nl[4 * P.n_rec - 1] + 1 : 0;
        } else {
            std::vector<uint32_t> hdr_line;
            P.cum.assign(T.n_lines + 1, 0);
            for (uint32_t j = 0; j < T.n_lines; j++) {
                uint32_t h, b;
                fasta_line(T, j, h, b);
                if (h) hdr_line.push_back(j);
                P.cum[j + 1] = P.cum[j] + b;
            }
            const uint32_t n_hdr = static_cast<uint32_t>(hdr_line.size());
            P.n_rec = final ? n_hdr : n_hdr ? n_hdr - 1 : 0;
            P.rows.resize(n_hdr);
            for (uint32_t r = 0; r < n_hdr; r++) {
                const uint32_t cls = fasta_record(T, r, hdr_line.data(), P.cum.data(), n_hdr, final, P.rows[r]);
                if (cls && r < P.n_rec) refuse(r, cls);
            }
            P.covered = final ? n : n_hdr ? P.rows[n_hdr - 1].name_beg - 1 : 0;
            P.nl = nl;
        }
        if (ev != ~0ull) { P.ev_rec = static_cast<uint32_t>(ev >> 8); P.ev_cls = static_cast<uint32_t>(ev & 0xFF); }
        fs[fi].text = t; fs[fi].rows = &P.rows;
    }
    uint32_t mismatch(int fa, uint32_t ra, uint32_t sa, int fb, uint32_t rb, uint32_t sb, uint32_t n) {
        for (uint32_t i = 0; i < n; i++)
            if (!equal_names_fast(fs[fa].text, (*fs[fa].rows)[ra + sa * i], fs[fb].text, (*fs[fb].rows)[rb + sb * i])) return i;
        return n;
    }
};

void put32(std::string& out, uint32_t v) { out.append(reinterpret_cast<const char*>(&v), 4); }
void put_bytes(std::string& out, const std::string& s) { put32(out, static_cast<uint32_t>(s.size())); out += s; }

struct Result { int32_t code = LCTY_OK; std::string msg, records; Counters C; uint64_t units = 0; };

// every record of the input: per record u32 length + bytes of the name, the sequence and the qualities
Result run(const char* p1, const char* p2, bool interleaved, uint64_t window, uint64_t cap, uint64_t max_records) {
    Result R;
    SerialExec exec;
    Stream<SerialExec> st(exec);
    try {
        st.open(p1, p2, interleaved, window, cap);
        for (;;) {
            const Chunk c = st.next(max_records);
            if (!c.k) break;
            R.units += c.k;
            for (uint32_t i = 0; i < c.k; i++)
                for (int e = 0; e < c.per; e++) {
                    const FileWin<SerialExec>& w = st.f[c.file[e]];
                    const uint32_t rec = c.rec0[e] + c.stride * i;
                    std::string seq, qual;
                    st.sequence(w, rec, seq); st.qualities(w, rec, qual);
                    put_bytes(R.records, st.name_of(w, rec)); put_bytes(R.records, seq); put_bytes(R.records, qual);
                }
        }
    } catch (const Error& e) { R.code = e.code; R.msg = e.what(); }
    R.C = st.C;
    return R;
}

}  // namespace

namespace lcty { void set_last_error(const std::string&) {} }

extern "C" {

// -> the status; *out (free with fastx_probe_free) the records in front of the first error, msg (1024 bytes) its message,
// counters: bytes_read, bytes_inflated, windows, windows_enlarged, records
int32_t fastx_probe_run(const char* p1, const char* p2, int interleaved, uint64_t window, uint64_t cap, uint64_t max_records, uint8_t** out,
                        uint64_t* out_len, char* msg, uint64_t* counters) {
    const Result R = run(p1, p2, interleaved != 0, window, cap, max_records);
    *out = static_cast<uint8_t*>(malloc(R.records.size() + 1));
    memcpy(*out, R.records.data(), R.records.size());
    *out_len = R.records.size();
    snprintf(msg, 1024, "%s", R.msg.c_str());
    counters[0] = R.C.bytes_read; counters[1] = R.C.bytes_inflated; counters[2] = R.C.windows; counters[3] = R.C.windows_enlarged; counters[4] = R.C.records;
    return R.code;
}
void fastx_probe_free(uint8_t* p) { free(p); }

}  // extern "C"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: fastx_probe_host DIR/corpus.tsv\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    unsigned cases = 0, runs = 0, bad = 0;
    uint64_t records = 0;
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string x; std::getline(ss, x, '\t');) f.push_back(x);
        if (f.size() != 5) { fprintf(stderr, "bad corpus line: %s\n", line.c_str()); return 2; }
        const char* p2 = f[4] == "-" ? nullptr : f[4].c_str();
        const bool interleaved = f[2] == "1";
        const Result want = run(f[3].c_str(), p2, interleaved, WINDOW_DEFAULT, WINDOW_LIMIT, ~0ull);
        const int32_t status = f[1] == "valid" ? LCTY_OK : f[1] == "mixed" ? LCTY_ERR_UNSUPPORTED : LCTY_ERR_INVALID_DATA;
        if (want.code != status) { fprintf(stderr, "%s: status %d, the corpus says %d (%s)\n", f[0].c_str(), want.code, status, want.msg.c_str()); bad++; }
        cases++; records += want.C.records;
        for (uint64_t window : {64ull, 65ull, 127ull, 4096ull})
            for (uint64_t max_records : {1ull, ~0ull}) {
                const Result got = run(f[3].c_str(), p2, interleaved, window, WINDOW_LIMIT, max_records);
                runs++;
                if (got.code != want.code || got.msg != want.msg || got.records != want.records) {
                    fprintf(stderr, "%s: window %llu, %s: status %d (%s), with one window %d (%s); %zu and %zu bytes of records\n", f[0].c_str(),
                            static_cast<unsigned long long>(window), max_records == 1 ? "one record a call" : "no limit", got.code, got.msg.c_str(), want.code,
                            want.msg.c_str(), got.records.size(), want.records.size());
                    bad++;
                }
            }
    }
    printf("fastx_probe_host: %u cases, %llu records, %u windowed runs, %u differences\n", cases, static_cast<unsigned long long>(records), runs, bad);
    return bad ? 1 : 0;
}
