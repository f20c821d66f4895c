// lcty_io.hip — the file formats at the edges of the path, host code only:
//   containers   gzip / BGZF (zlib), LZ4 frames (own decoder), brotli streams (the system's libbrotlidec, looked up at run time)
//                — what ext::sys::open / create_gzip / the brotli multi-stream reader hide (src/ext/sys.rs, src/ext/sys/brotli.rs:18-86)
//   distr.gz     BgDistr::load (src/bg/mod.rs:147-177; seq_info 349-364, insert_distr insertsz.rs:183-208, error_profile
//                err_prof.rs:307-329, bg_depth depth.rs:387-412) -> lcty_bg
//   res.json.gz  Genotyping::to_json (src/solvers/solve.rs:732-773), written as the reference does (write_pretty(.., 4), gzip)
//   aln.bam      the record stream AllAlignments::load consumes (src/model/locs.rs:405-461, 502-567, 1116-1150) -> the flat table
//                of lcty_reads_append, in the input-order contract of include/locityper_hip.h
#include <dlfcn.h>
#include <zlib.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "lcty_aln_bam.hpp"
#include "lcty_bg_reads.hpp"
#include "lcty_bgzf.hpp"
#include "lcty_common.hpp"
#include "lcty_gtvcf_host.hpp"
#include "lcty_seq.hpp"
#include "lcty_bgzf_index.hpp"

using namespace lcty;

namespace {

// BGZF (the blocks of a BAM / .bgz file: gzip members of <= 64 KB whose extra field "BC" holds the member's size): the members are
// independent, so they inflate on the host's cores straight into their places (bgzf_inflate_host). Returns false when the input is
// not BGZF from end to end (then the serial walk below takes it).
bool inflate_bgzf(const std::vector<uint8_t>& in, const char* what, std::vector<uint8_t>& out) {
    std::vector<BgzfBlock> blocks;
    uint64_t total = 0;
    for (size_t i = 0; i < in.size();) {
        BgzfHead h;
        if (bgzf_head(in.data() + i, in.size() - i, h) != BGZF_OK) return false;
        blocks.push_back(BgzfBlock{h.csize, h.isize, total, i, i, h.head});
        total += h.isize; i += h.csize;
    }
    out.resize(total);
    bgzf_inflate_host(in.data(), blocks, out.data(), what, 32);
    return true;
}

// gzip members one after the other (a .gz written in pieces, or the BGZF blocks of a BAM file)
std::vector<uint8_t> inflate_gzip(const std::vector<uint8_t>& in, const char* what) {
    std::vector<uint8_t> out;
    if (inflate_bgzf(in, what, out)) return out;
    out.clear();
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) fail(LCTY_ERR_RUNTIME, "zlib: inflateInit2");
    zs.next_in = const_cast<Bytef*>(in.data());
    zs.avail_in = static_cast<uInt>(std::min<size_t>(in.size(), 0x7FFFFFFFu));
    size_t fed = zs.avail_in;
    std::vector<uint8_t> chunk(1 << 18);
    for (;;) {
        zs.next_out = chunk.data(); zs.avail_out = static_cast<uInt>(chunk.size());
        const int rc = inflate(&zs, Z_NO_FLUSH);
        out.insert(out.end(), chunk.data(), chunk.data() + (chunk.size() - zs.avail_out));
        if (rc == Z_STREAM_END) {
            if (zs.avail_in == 0 && fed == in.size()) break;
            if (inflateReset(&zs) != Z_OK) { inflateEnd(&zs); fail(LCTY_ERR_RUNTIME, "zlib: inflateReset"); }
        } else if (rc != Z_OK && rc != Z_BUF_ERROR) {
            inflateEnd(&zs);
            fail(LCTY_ERR_INVALID_DATA, "%s: corrupt gzip stream (zlib %d)", what, rc);
        } else if (rc == Z_BUF_ERROR && zs.avail_in == 0 && fed == in.size()) {
            inflateEnd(&zs);
            fail(LCTY_ERR_INVALID_DATA, "%s: truncated gzip stream", what);
        }
        if (zs.avail_in == 0 && fed < in.size()) {
            const size_t more = std::min<size_t>(in.size() - fed, 0x7FFFFFFFu);
            zs.next_in = const_cast<Bytef*>(in.data() + fed); zs.avail_in = static_cast<uInt>(more); fed += more;
        }
    }
    inflateEnd(&zs);
    return out;
}

// LZ4 frame format (magic 0x184D2204; skippable frames 0x184D2A50..5F), frames one after the other. Blocks of a frame may refer
// back into the blocks before them (block-dependent mode): the frame is decoded into one contiguous buffer.
uint32_t rd32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | (static_cast<uint32_t>(p[3]) << 24); }

void lz4_block(const uint8_t* src, size_t n, std::vector<uint8_t>& out, size_t frame_start, const char* what) {
    size_t i = 0;
    while (i < n) {
        const uint8_t token = src[i++];
        size_t lit = token >> 4;
        if (lit == 15) { uint8_t b; do { if (i >= n) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt LZ4 block", what); b = src[i++]; lit += b; } while (b == 255); }
        if (i + lit > n) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt LZ4 block", what);
        out.insert(out.end(), src + i, src + i + lit);
        i += lit;
        if (i >= n) break;                                   // the last sequence of a block has literals only
        if (i + 2 > n) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt LZ4 block", what);
        const size_t offset = src[i] | (src[i + 1] << 8);
        i += 2;
        size_t len = (token & 15u) + 4;
        if ((token & 15u) == 15) { uint8_t b; do { if (i >= n) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt LZ4 block", what); b = src[i++]; len += b; } while (b == 255); }
        if (offset == 0 || offset > out.size() - frame_start) fail(LCTY_ERR_INVALID_DATA, "%s: LZ4 match before the start of the frame", what);
        size_t from = out.size() - offset;
        for (size_t k = 0; k < len; k++) out.push_back(out[from + k]);       // may overlap its own output
    }
}

std::vector<uint8_t> decode_lz4(const std::vector<uint8_t>& in, const char* what) {
    std::vector<uint8_t> out;
    size_t i = 0;
    while (i < in.size()) {
        if (i + 4 > in.size()) fail(LCTY_ERR_INVALID_DATA, "%s: truncated LZ4 frame", what);
        const uint32_t magic = rd32(&in[i]);
        i += 4;
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {          // skippable frame
            if (i + 4 > in.size()) fail(LCTY_ERR_INVALID_DATA, "%s: truncated LZ4 frame", what);
            i += 4 + static_cast<size_t>(rd32(&in[i]));
            continue;
        }
        if (magic != 0x184D2204u) fail(LCTY_ERR_INVALID_DATA, "%s: not an LZ4 frame (magic %08x)", what, magic);
        if (i + 3 > in.size()) fail(LCTY_ERR_INVALID_DATA, "%s: truncated LZ4 frame", what);
        const uint8_t flg = in[i];
        if ((flg >> 6) != 1) fail(LCTY_ERR_INVALID_DATA, "%s: LZ4 frame version %u", what, flg >> 6);
        const bool block_checksum = flg & 0x10, content_size = flg & 0x08, content_checksum = flg & 0x04, dict_id = flg & 0x01;
        i += 2 + (content_size ? 8 : 0) + (dict_id ? 4 : 0) + 1;          // FLG, BD, [size], [dict id], HC
        const size_t frame_start = out.size();
        for (;;) {
            if (i + 4 > in.size()) fail(LCTY_ERR_INVALID_DATA, "%s: truncated LZ4 frame", what);
            const uint32_t bs = rd32(&in[i]);
            i += 4;
            if (bs == 0) break;                              // EndMark
            const size_t n = bs & 0x7FFFFFFFu;
            if (i + n > in.size()) fail(LCTY_ERR_INVALID_DATA, "%s: truncated LZ4 block", what);
            if (bs & 0x80000000u) out.insert(out.end(), in.begin() + i, in.begin() + i + n);
            else lz4_block(&in[i], n, out, frame_start, what);
            i += n + (block_checksum ? 4 : 0);
        }
        if (content_checksum) i += 4;
    }
    return out;
}

// brotli: the decoder of the system's libbrotlidec.so.1 (public C API of google/brotli, c/include/brotli/decode.h), looked up at
// run time; several streams one after the other as the reference's reader accepts them (ext/sys/brotli.rs:18-86)
std::vector<uint8_t> decode_brotli(const std::vector<uint8_t>& in, const char* what) {
    typedef void* (*create_fn)(void*, void*, void*);
    typedef int (*stream_fn)(void*, size_t*, const uint8_t**, size_t*, uint8_t**, size_t*);
    typedef void (*destroy_fn)(void*);
    static void* lib = dlopen("libbrotlidec.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) fail(LCTY_ERR_UNSUPPORTED, "%s: brotli needs libbrotlidec.so.1, which is not on this system (%s); use the .lz4 file", what, dlerror());
    static create_fn create = reinterpret_cast<create_fn>(dlsym(lib, "BrotliDecoderCreateInstance"));
    static stream_fn stream = reinterpret_cast<stream_fn>(dlsym(lib, "BrotliDecoderDecompressStream"));
    static destroy_fn destroy = reinterpret_cast<destroy_fn>(dlsym(lib, "BrotliDecoderDestroyInstance"));
    if (!create || !stream || !destroy) fail(LCTY_ERR_UNSUPPORTED, "%s: libbrotlidec.so.1 lacks the decoder entry points", what);
    std::vector<uint8_t> out, chunk(1 << 18);
    const uint8_t* next_in = in.data();
    size_t avail_in = in.size();
    while (avail_in > 0) {
        void* st = create(nullptr, nullptr, nullptr);
        if (!st) fail(LCTY_ERR_RUNTIME, "brotli: cannot create a decoder");
        for (;;) {
            uint8_t* next_out = chunk.data();
            size_t avail_out = chunk.size();
            const int rc = stream(st, &avail_in, &next_in, &avail_out, &next_out, nullptr);
            out.insert(out.end(), chunk.data(), chunk.data() + (chunk.size() - avail_out));
            if (rc == 1) break;                              // BROTLI_DECODER_RESULT_SUCCESS: this stream is complete
            if (rc == 3) continue;                           // NEEDS_MORE_OUTPUT
            destroy(st);
            fail(LCTY_ERR_INVALID_DATA, rc == 2 ? "%s: truncated brotli stream" : "%s: corrupt brotli stream", what);
        }
        destroy(st);
    }
    return out;
}

// ---------------------------------------------------------------- a JSON value (what the `json` crate parses for JsonSer::load)
struct Json {
    enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
    bool b = false; double num = 0.0; std::string str;
    std::vector<Json> arr;
    std::vector<std::pair<std::string, Json>> obj;
    const Json* get(const char* key) const {
        if (kind != Obj) return nullptr;
        for (const auto& kv : obj) if (kv.first == key) return &kv.second;
        return nullptr;
    }
};

struct JsonParser {
    const char* p; const char* end;
    size_t len;
    [[noreturn]] void bad(const char* what) const { fail(LCTY_ERR_INVALID_DATA, "JSON: %s at byte %zu", what, static_cast<size_t>(p - (end - len))); }
    void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++; }
    Json value(int depth = 0) {
        if (depth > 64) bad("nesting too deep");
        ws();
        if (p >= end) bad("unexpected end");
        Json v;
        if (*p == '{') {
            v.kind = Json::Obj; p++; ws();
            if (p < end && *p == '}') { p++; return v; }
            for (;;) {
                ws();
                if (p >= end || *p != '"') bad("expected a key");
                std::string k = string();
                ws();
                if (p >= end || *p != ':') bad("expected ':'");
                p++;
                v.obj.emplace_back(std::move(k), value(depth + 1));
                ws();
                if (p < end && *p == ',') { p++; continue; }
                if (p < end && *p == '}') { p++; return v; }
                bad("expected ',' or '}'");
            }
        }
        if (*p == '[') {
            v.kind = Json::Arr; p++; ws();
            if (p < end && *p == ']') { p++; return v; }
            for (;;) {
                v.arr.push_back(value(depth + 1));
                ws();
                if (p < end && *p == ',') { p++; continue; }
                if (p < end && *p == ']') { p++; return v; }
                bad("expected ',' or ']'");
            }
        }
        if (*p == '"') { v.kind = Json::Str; v.str = string(); return v; }
        if (end - p >= 4 && !strncmp(p, "true", 4)) { v.kind = Json::Bool; v.b = true; p += 4; return v; }
        if (end - p >= 5 && !strncmp(p, "false", 5)) { v.kind = Json::Bool; p += 5; return v; }
        if (end - p >= 4 && !strncmp(p, "null", 4)) { p += 4; return v; }
        const char* q = p;
        while (q < end && (isdigit(static_cast<unsigned char>(*q)) || *q == '-' || *q == '+' || *q == '.' || *q == 'e' || *q == 'E')) q++;
        if (q == p) bad("unexpected character");
        const std::string num(p, q);
        char* e = nullptr;
        v.kind = Json::Num; v.num = strtod(num.c_str(), &e);
        if (*e) bad("malformed number");
        p = q;
        return v;
    }
    std::string string() {
        std::string s;
        p++;
        while (p < end && *p != '"') {
            if (*p == '\\') {
                if (++p >= end) bad("unterminated string");
                switch (*p) {
                    case 'n': s += '\n'; break; case 't': s += '\t'; break; case 'r': s += '\r'; break;
                    case 'b': s += '\b'; break; case 'f': s += '\f'; break;
                    case 'u': {
                        if (end - p < 5) bad("unterminated string");
                        const unsigned cp = static_cast<unsigned>(strtoul(std::string(p + 1, p + 5).c_str(), nullptr, 16));
                        if (cp < 0x80) s += static_cast<char>(cp);
                        else if (cp < 0x800) { s += static_cast<char>(0xC0 | (cp >> 6)); s += static_cast<char>(0x80 | (cp & 63)); }
                        else { s += static_cast<char>(0xE0 | (cp >> 12)); s += static_cast<char>(0x80 | ((cp >> 6) & 63)); s += static_cast<char>(0x80 | (cp & 63)); }
                        p += 4; break;
                    }
                    default: s += *p;
                }
                p++;
            } else s += *p++;
        }
        if (p >= end) bad("unterminated string");
        p++;
        return s;
    }
};

double need_f64(const Json& o, const char* key, const char* where) {          // json_get!(obj => key (as_f64))
    const Json* v = o.get(key);
    if (!v || v->kind != Json::Num) fail(LCTY_ERR_INVALID_DATA, "%s: Failed to parse: missing or incorrect '%s' field", where, key);
    return v->num;
}

// shortest decimal text that reads back as the same f64; NaN / inf become null as the `json` crate writes them
std::string json_num(double x) {
    if (!std::isfinite(x)) return "null";
    char buf[64];
    int prec = 1;
    for (; prec <= 17; prec++) {
        snprintf(buf, sizeof(buf), "%.*g", prec, x);
        if (strtod(buf, nullptr) == x) break;
    }
    if (strchr(buf, 'e') && x != 0.0 && std::fabs(x) >= 1e-5 && std::fabs(x) < 1e17) {      // positional notation for ordinary magnitudes
        const int e10 = static_cast<int>(std::floor(std::log10(std::fabs(x))));
        snprintf(buf, sizeof(buf), "%.*f", std::max(0, prec - 1 - e10), x);
        if (strtod(buf, nullptr) != x) snprintf(buf, sizeof(buf), "%.*g", prec, x);
    }
    return buf;
}
std::string json_str(const std::string& s) {
    std::string o = "\"";
    for (const char c : s) {
        if (c == '"' || c == '\\') { o += '\\'; o += c; }
        else if (c == '\n') o += "\\n";
        else if (c == '\t') o += "\\t";
        else if (static_cast<unsigned char>(c) < 0x20) { char b[8]; snprintf(b, sizeof(b), "\\u%04x", c); o += b; }
        else o += c;
    }
    return o + "\"";
}

}  // namespace

namespace {

// A brotli stream (RFC 7932) for the files the reference writes through its brotli writer — `sol.csv.br`, `reads.csv.br` and the other
// --debug tables (ext/sys.rs create_brotli; solvers/solve.rs:937-938, model/locs.rs:1062-1065). With the system's libbrotlienc.so.1
// (looked up at run time, like the decoder) the stream is compressed at `quality` (0..11; the reference's writer uses its crate's
// default); without it — or with quality < 0 — the bytes go into UNCOMPRESSED meta-blocks (RFC 7932 §9.2: ISLAST 0, MNIBBLES, MLEN - 1,
// ISUNCOMPRESSED 1, padding, the bytes; at most 65 536 bytes each so that MLEN - 1 takes four nibbles; a last empty meta-block): a
// valid stream every brotli reader takes, the reference's multi-stream reader included — stored, not compressed.
std::vector<uint8_t> brotli_stored(const uint8_t* data, uint64_t len) {
    std::vector<uint8_t> out;
    out.reserve(len + 3 * (len / 65536 + 1) + 2);
    bool first = true;
    for (uint64_t at = 0; at < len;) {
        const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(len - at, 65536));
        // the stream starts with WBITS = 22 (the four bits 1011, least significant first); a meta-block header is ISLAST (0), MNIBBLES
        // (00: four nibbles), MLEN - 1 (16 bits), ISUNCOMPRESSED (1): 20 bits — 24 with WBITS in front, or with four bits of padding
        uint32_t bits = 0, nb = 0;
        auto put = [&](uint32_t v, uint32_t k) { bits |= v << nb; nb += k; };
        if (first) put(0xBu, 4);
        put(0, 1); put(0, 2); put(n - 1, 16); put(1, 1);
        out.push_back(static_cast<uint8_t>(bits)); out.push_back(static_cast<uint8_t>(bits >> 8)); out.push_back(static_cast<uint8_t>(bits >> 16));
        out.insert(out.end(), data + at, data + at + n);
        at += n; first = false;
    }
    out.push_back(first ? 0x3Bu : 0x03u);        // ISLAST 1, ISLASTEMPTY 1 (behind WBITS when the stream is empty), padding
    return out;
}

std::vector<uint8_t> brotli_encode(const uint8_t* data, uint64_t len, int32_t quality, bool* stored) {
    *stored = true;
    if (quality >= 0) {
        using compress_fn = int (*)(int, int, int, size_t, const uint8_t*, size_t*, uint8_t*);
        using bound_fn = size_t (*)(size_t);
        static void* lib = dlopen("libbrotlienc.so.1", RTLD_NOW | RTLD_LOCAL);
        static compress_fn compress = lib ? reinterpret_cast<compress_fn>(dlsym(lib, "BrotliEncoderCompress")) : nullptr;
        static bound_fn bound = lib ? reinterpret_cast<bound_fn>(dlsym(lib, "BrotliEncoderMaxCompressedSize")) : nullptr;
        if (compress && bound) {
            size_t cap = bound(static_cast<size_t>(len));
            if (cap == 0) cap = static_cast<size_t>(len) + (len >> 2) + 1024;
            std::vector<uint8_t> out(cap);
            size_t n = cap;
            if (compress(std::min(quality, 11), 22, 0, static_cast<size_t>(len), data, &n, out.data()) == 1) {
                out.resize(n);
                *stored = false;
                return out;
            }
        }
    }
    return brotli_stored(data, len);
}

}  // namespace

extern "C" {

int32_t lcty_io_read_file(const char* path, uint8_t** data, uint64_t* len) {
    return guarded([&] {
        if (!path || !data || !len) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<uint8_t> raw = read_whole_file(path);
        const std::string p(path);
        std::vector<uint8_t> out;
        if (has_suffix(p, ".gz") || has_suffix(p, ".bgz") || has_suffix(p, ".bam")) out = inflate_gzip(raw, path);
        else if (has_suffix(p, ".lz4")) out = decode_lz4(raw, path);
        else if (has_suffix(p, ".br")) out = decode_brotli(raw, path);
        else out.swap(raw);
        Handoff h;
        *data = h.copy(out); *len = out.size(); h.commit();
    });
}

void lcty_io_free(void* p) { free(p); }

int32_t lcty_io_write_bgzf(const char* path, const uint8_t* data, uint64_t len) {
    return guarded([&] {
        if (!path || (len && !data)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        BgzfOut out(path);
        out.write(data, len);
        out.close();
    });
}

int32_t lcty_io_write_gz(const char* path, const uint8_t* data, uint64_t len) {
    return guarded([&] {
        if (!path || (len && !data)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        gzFile f = gzopen(path, "wb");
        if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot create %s", path);
        uint64_t at = 0;
        while (at < len) {
            const unsigned n = static_cast<unsigned>(std::min<uint64_t>(len - at, 1u << 30));
            if (gzwrite(f, data + at, n) != static_cast<int>(n)) { gzclose(f); fail(LCTY_ERR_RUNTIME, "write error on %s", path); }
            at += n;
        }
        if (gzclose(f) != Z_OK) fail(LCTY_ERR_RUNTIME, "write error on %s", path);
    });
}

int32_t lcty_io_write_br(const char* path, const uint8_t* data, uint64_t len, int32_t quality, int32_t* stored) {
    return guarded([&] {
        if (!path || (len && !data)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        bool st = true;
        const std::vector<uint8_t> out = brotli_encode(data, len, quality, &st);
        FILE* f = fopen(path, "wb");
        if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot create %s", path);
        const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
        if (fclose(f) != 0 || !ok) fail(LCTY_ERR_RUNTIME, "write error on %s", path);
        if (stored) *stored = st ? 1 : 0;
    });
}

// BgDistr::load (bg/mod.rs:159-177). *read_len = seq_info.read_len (mean read length; window sizes derive from it upstream)
int32_t lcty_bg_from_json(const char* text, uint64_t len, lcty_bg* bg, double* read_len) {
    return guarded([&] {
        if (!text || !bg) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        JsonParser P{text, text + len, len};
        const Json root = P.value();
        P.ws();
        if (P.p != P.end) P.bad("trailing characters");
        const Json* seq = root.get("seq_info"); const Json* ins = root.get("insert_distr"); const Json* err = root.get("error_profile");
        if (!seq || !ins || !err)
            fail(LCTY_ERR_INVALID_DATA, "BgDistr: Failed to parse: missing 'seq_info', 'insert_distr' or 'error_profile' keys!");
        memset(bg, 0, sizeof(*bg));
        // SequencingInfo::load (bg/mod.rs:359-363); Technology::from_str (273-281)
        const double rl = need_f64(*seq, "read_len", "SequencingInfo");
        if (read_len) *read_len = rl;
        const Json* tech = seq->get("technology");
        if (!tech || tech->kind != Json::Str) fail(LCTY_ERR_INVALID_DATA, "SequencingInfo: Failed to parse: missing or incorrect 'technology' field");
        std::string t = tech->str;
        for (auto& c : t) c = static_cast<char>(tolower(static_cast<unsigned char>(c)));
        if (t == "illumina" || t == "sr") bg->technology = LCTY_TECH_ILLUMINA;
        else if (t == "hifi") bg->technology = LCTY_TECH_HIFI;
        else if (t == "pacbio" || t == "pb") bg->technology = LCTY_TECH_PACBIO;
        else if (t == "nanopore" || t == "ont") bg->technology = LCTY_TECH_NANOPORE;
        else fail(LCTY_ERR_INVALID_DATA, "Unknown technology \"%s\"", tech->str.c_str());
        // InsertDistr::load (insertsz.rs:195-208): {} = single-end
        if (ins->kind != Json::Obj) fail(LCTY_ERR_INVALID_DATA, "InsertDistr: Failed to parse: not an object");
        bg->is_paired = !ins->obj.empty();
        if (bg->is_paired) { bg->ins_n = need_f64(*ins, "n", "InsertDistr"); bg->ins_p = need_f64(*ins, "p", "InsertDistr"); }
        // ErrorProfile::load (err_prof.rs:321-329)
        static const char* const ops[5] = {"matches", "mismatches", "insertions", "deletions", "clipping"};
        for (int i = 0; i < 5; i++) bg->op_lnprobs[i] = need_f64(*err, ops[i], "ErrorProfile");
        bg->edit_alpha = need_f64(*err, "alpha", "ErrorProfile"); bg->edit_beta = need_f64(*err, "beta", "ErrorProfile");
        // EditThresh::default_for (err_prof.rs:394-399)
        if (bg->technology == LCTY_TECH_ILLUMINA) { bg->edit_kind = LCTY_EDIT_FRACTION; bg->edit_p1 = 0.03; bg->edit_p2 = 0.06; }
        else { bg->edit_kind = LCTY_EDIT_PVALUE; bg->edit_p1 = 0.99; bg->edit_p2 = 0.999; }
        // ReadDepth::load (depth.rs:400-412); `locityper genotype` needs it (BgDistr::depth().expect)
        const Json* dep = root.get("bg_depth");
        if (!dep) fail(LCTY_ERR_INVALID_DATA, "BgDistr: no 'bg_depth' key: the background read depth is required for genotyping");
        (void)need_f64(*dep, "ploidy", "ReadDepth");
        bg->window = static_cast<uint32_t>(need_f64(*dep, "window", "ReadDepth"));
        bg->neighb = static_cast<uint32_t>(need_f64(*dep, "neighb", "ReadDepth"));
        for (int which = 0; which < 2; which++) {
            const char* key = which ? "p" : "n";
            const Json* a = dep->get(key);
            if (!a || a->kind != Json::Arr) fail(LCTY_ERR_INVALID_DATA, "ReadDepth: Failed to parse: missing or incorrect array '%s'", key);
            if (a->arr.size() != LCTY_GC_BINS) fail(LCTY_ERR_INVALID_DATA, "ReadDepth: Failed to parse: incorrect number of elements in array `%s`", key);
            for (size_t i = 0; i < LCTY_GC_BINS; i++) {
                if (a->arr[i].kind != Json::Num) fail(LCTY_ERR_INVALID_DATA, "ReadDepth: element #%zu of array '%s' is not a float", i, key);
                (which ? bg->depth_p : bg->depth_n)[i] = a->arr[i].num;
            }
        }
    });
}

// Genotyping::to_json (solve.rs:732-773) as text, in the reference's layout (write_pretty(.., 4), genotype.rs:1256).
// names[n_alleles]: contig names; lik_mean / lik_var: natural-log values of the reported genotypes, in call->ixs order;
// distances: NULL or one entry per reported genotype (LCTY_NONE_U32 = "unknown"); weighted_dist: NaN = absent.
int32_t lcty_res_to_json(const lcty_call* call, const uint16_t* genotypes, uint32_t ploidy, const char* const* names, uint32_t n_alleles,
                         const double* lik_mean, const double* lik_var, const uint32_t* distances, int32_t true_edit_distances,
                         double weighted_dist, char* out, uint64_t cap, uint64_t* needed) {
    return guarded([&] {
        if (!call || !genotypes || !names || !lik_mean || !lik_var || !needed || ploidy == 0) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double INV_LN10 = 1.0 / std::log(10.0);
        auto gt_name = [&](uint64_t i) {
            std::string s;
            for (uint32_t t = 0; t < ploidy; t++) {
                const uint16_t a = genotypes[i * ploidy + t];
                if (a >= n_alleles) fail(LCTY_ERR_INVALID_INPUT, "genotype refers to allele %u >= %u", a, n_alleles);
                if (t) s += ',';
                s += names[a];
            }
            return s;
        };
        std::string j = "{\n";
        auto field = [&](int indent, const char* key, const std::string& val, bool last = false) {
            j += std::string(static_cast<size_t>(indent), ' ') + "\"" + key + "\": " + val + (last ? "\n" : ",\n");
        };
        std::vector<std::pair<std::string, std::string>> top;
        top.emplace_back("total_reads", std::to_string(call->n_good));
        top.emplace_back("quality", json_num(call->quality));
        if (distances) top.emplace_back("dist_type", true_edit_distances ? "\"edit\"" : "\"minim-div\"");
        if (!std::isnan(weighted_dist)) top.emplace_back("weight_dist", json_num(weighted_dist));
        top.emplace_back("unexpl_reads", std::to_string(call->unexpl_reads));
        if (call->n_out) {
            top.emplace_back("genotype", json_str(gt_name(0)));
            std::string opts = "[\n";
            for (uint64_t i = 0; i < call->n_out; i++) {
                opts += "        {\n";
                std::vector<std::pair<std::string, std::string>> o;
                o.emplace_back("genotype", json_str(gt_name(i)));
                o.emplace_back("lik_mean", json_num(lik_mean[i] * INV_LN10));
                o.emplace_back("lik_sd", json_num(lik_var[i] * INV_LN10));           // as written upstream: the log10-scaled VARIANCE (solve.rs:755)
                o.emplace_back("prob", json_num(std::exp(call->ln_probs[i])));
                o.emplace_back("log10_prob", json_num(call->ln_probs[i] * INV_LN10));
                if (distances) o.emplace_back("dist_to_primary", distances[i] == LCTY_NONE_U32 ? std::string("\"unknown\"") : std::to_string(distances[i]));
                for (size_t t = 0; t < o.size(); t++)
                    opts += "            \"" + o[t].first + "\": " + o[t].second + (t + 1 < o.size() ? ",\n" : "\n");
                opts += i + 1 < call->n_out ? "        },\n" : "        }\n";
            }
            opts += "    ]";
            top.emplace_back("options", opts);
        }
        if (call->warnings) {
            std::string w = "[\n";
            std::vector<std::string> ws;
            if (call->warnings & LCTY_WARN_NO_PROBABLE_GENOTYPE) ws.push_back("NoProbableGenotype");
            if (call->warnings & LCTY_WARN_FEW_READS) ws.push_back("FewReads(" + std::to_string(call->n_good) + ")");
            for (size_t t = 0; t < ws.size(); t++) w += "        \"" + ws[t] + "\"" + (t + 1 < ws.size() ? ",\n" : "\n");
            top.emplace_back("warnings", w + "    ]");
        }
        for (size_t t = 0; t < top.size(); t++) field(4, top[t].first.c_str(), top[t].second, t + 1 == top.size());
        j += "}";
        *needed = j.size() + 1;
        if (out && cap >= *needed) memcpy(out, j.c_str(), j.size() + 1);
        else if (out) fail(LCTY_ERR_INVALID_INPUT, "output buffer too small (%llu < %llu)", static_cast<unsigned long long>(cap), static_cast<unsigned long long>(*needed));
    });
}

// The top level of a res.json.gz as process_sample reads it (extra/into_csv.py:73-96), numbers in the fixed point of lcty_gtvcf_*.
int32_t lcty_res_summary_read(const char* path, lcty_res_summary* out) {
    return guarded([&] {
        if (out) { memset(out, 0, sizeof(*out)); out->qual10 = out->reads = out->unexpl = out->wdist5 = LCTY_GTVCF_ABSENT; out->state = LCTY_RES_UNKNOWN; }
        if (!path || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (access(path, F_OK) != 0) { out->state = LCTY_RES_MISSING; return; }   // 74-77: the `?` row
        const std::vector<uint8_t> raw = read_whole_file(path);
        if (raw.size() < 2 || raw[0] != 0x1f || raw[1] != 0x8b) fail(LCTY_ERR_INVALID_DATA, "%s: not a gzip file", path);
        const std::vector<uint8_t> text = inflate_gzip(raw, path);
        JsonParser jp{reinterpret_cast<const char*>(text.data()), reinterpret_cast<const char*>(text.data()) + text.size(), text.size()};
        const Json root = jp.value();
        if (root.kind != Json::Obj) fail(LCTY_ERR_INVALID_DATA, "%s: not a JSON object", path);
        const Json* gt = root.get("genotype");
        if (!gt) { out->state = LCTY_RES_NO_GENOTYPE; return; }               // 85-87: the `*` row
        if (gt->kind != Json::Str) fail(LCTY_ERR_INVALID_DATA, "%s: `genotype` is not a string", path);
        // get_or_nan (60-62): a missing key or null is NaN
        auto number = [&](const char* key) -> const Json* {
            const Json* v = root.get(key);
            if (!v || v->kind == Json::Null) return nullptr;
            if (v->kind != Json::Num) fail(LCTY_ERR_INVALID_DATA, "%s: `%s` is not a number", path, key);
            return std::isnan(v->num) ? nullptr : v;
        };
        auto in_range = [&](double x, const char* key) { if (!(std::fabs(x) < 9e17)) fail(LCTY_ERR_INVALID_DATA, "%s: `%s` = %g is out of range", path, key, x); };
        const Json* q = root.get("quality");
        if (!q || q->kind != Json::Num) fail(LCTY_ERR_INVALID_DATA, "%s: a genotype without a numeric `quality`", path);      // 91: float(None) raises
        int64_t qual10 = LCTY_GTVCF_ABSENT;
        if (!std::isnan(q->num)) { const double t = std::floor(10.0 * q->num); in_range(t, "quality"); qual10 = static_cast<int64_t>(t); }
        auto count = [&](const char* key) -> int64_t {
            const Json* v = number(key);
            if (!v) return LCTY_GTVCF_ABSENT;
            in_range(v->num, key);
            if (v->num != std::floor(v->num)) fail(LCTY_ERR_INVALID_DATA, "%s: `%s` = %g is not a whole number", path, key, v->num);
            return static_cast<int64_t>(v->num);
        };
        const int64_t reads = count("total_reads"), unexpl = count("unexpl_reads");
        int64_t wdist5 = LCTY_GTVCF_ABSENT;
        if (const Json* w = number("weight_dist")) {                          // 96: `:.5f`, the text read back digit by digit
            in_range(w->num * 1e5, "weight_dist");
            char buf[64];
            snprintf(buf, sizeof(buf), "%.5f", w->num);
            wdist5 = gtvcf::fixed_parse(buf, gtvcf::WDIST_DECIMALS);
        }
        std::string warnings = "*";                                           // 95: ';'.join(res.get('warnings', '*'))
        if (const Json* w = root.get("warnings")) {
            if (w->kind != Json::Arr) fail(LCTY_ERR_INVALID_DATA, "%s: `warnings` is not an array", path);
            warnings.clear();
            for (size_t i = 0; i < w->arr.size(); i++) {
                if (w->arr[i].kind != Json::Str) fail(LCTY_ERR_INVALID_DATA, "%s: a warning is not a string", path);
                if (i) warnings += ';';
                warnings += w->arr[i].str;
            }
        }
        Handoff h;
        out->genotype = h.copy(gt->str.c_str(), gt->str.size() + 1);
        out->warnings = h.copy(warnings.c_str(), warnings.size() + 1);
        out->qual10 = qual10; out->reads = reads; out->unexpl = unexpl; out->wdist5 = wdist5; out->state = LCTY_RES_CALLED;
        h.commit();
    });
}

void lcty_res_summary_free(lcty_res_summary* out) {
    if (!out) return;
    free(out->genotype); free(out->warnings);
    out->genotype = out->warnings = nullptr;
}

int32_t lcty_predictions_csv_write(const char* path, uint64_t n_rows, const char* const* sample, const char* const* locus, const lcty_res_summary* rows) {
    return guarded([&] {
        if (!path || (n_rows && (!sample || !locus || !rows))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const std::string text = gtvcf::predictions_csv_text(n_rows, sample, locus, rows);
        if (has_suffix(path, ".gz")) {
            const int32_t rc = lcty_io_write_gz(path, reinterpret_cast<const uint8_t*>(text.data()), text.size());
            if (rc != LCTY_OK) throw Error(rc, lcty_last_error());
            return;
        }
        FILE* f = fopen(path, "wb");
        if (!f) fail(LCTY_ERR_INVALID_INPUT, "cannot create %s", path);
        const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
        if (fclose(f) != 0 || !ok) fail(LCTY_ERR_RUNTIME, "write error on %s", path);
    });
}

int32_t lcty_predictions_csv_read(const char* path, lcty_predictions* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!path || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<uint8_t> raw = read_whole_file(path);
        if (raw.size() >= 2 && raw[0] == 0x1f && raw[1] == 0x8b) raw = inflate_gzip(raw, path);                              // common.open
        const gtvcf::PredictionTable T = gtvcf::predictions_csv_parse(std::string(raw.begin(), raw.end()), path);
        const size_t n = T.rows.size();
        std::string pool;
        auto keep = [&](const std::string& s) { const uint64_t at = pool.size(); pool += s; pool.push_back('\0'); return at; };
        std::vector<uint64_t> so(n), lo(n), go(n), wo(n), names(T.samples.size());
        std::vector<int64_t> q(n), r(n), u(n), w(n);
        for (size_t i = 0; i < T.samples.size(); i++) names[i] = keep(T.samples[i]);
        for (size_t i = 0; i < n; i++) {
            const gtvcf::PredictionRow& R = T.rows[i];
            so[i] = names[size_t(std::lower_bound(T.samples.begin(), T.samples.end(), R.sample) - T.samples.begin())];
            lo[i] = keep(R.locus); go[i] = keep(R.genotype); wo[i] = keep(R.warnings);
            q[i] = R.qual10; r[i] = R.reads; u[i] = R.unexpl; w[i] = R.wdist5;
        }
        Handoff h;
        out->text = reinterpret_cast<char*>(h.bytes(pool)); out->text_len = pool.size();
        out->sample_off = h.copy(so); out->locus_off = h.copy(lo); out->genotype_off = h.copy(go); out->warn_off = h.copy(wo);
        out->qual10 = h.copy(q); out->reads = h.copy(r); out->unexpl = h.copy(u); out->wdist5 = h.copy(w);
        out->samples_off = h.copy(names); out->n_samples = names.size(); out->n_rows = n;
        h.commit();
    });
}

void lcty_predictions_free(lcty_predictions* out) {
    if (!out) return;
    free(out->text); free(out->sample_off); free(out->locus_off); free(out->genotype_off); free(out->warn_off);
    free(out->qual10); free(out->reads); free(out->unexpl); free(out->wdist5); free(out->samples_off);
    memset(out, 0, sizeof(*out));
}

// The record stream of OUT/loci/<locus>/aln.bam (name-grouped, mates mapped as independent single-end reads, genotype.rs:975-977)
// as AllAlignments::load walks it (locs.rs:1116-1150): a group = a primary record and the non-primary records behind it
// (LaggedReader, 405-461); the first group of a read is ReadEnd::First, for paired-end data the next group — which must carry the
// same name (ReadData::set_name, 147-155) — is ReadEnd::Second. Reference names are mapped to allele indices through `names`
// (construct_tid_to_contig_map, 388-401: an unknown name is an error). Sequences: the primary record's SEQ as stored.
int32_t lcty_bam_read(const char* path, const char* const* names, uint32_t n_alleles, int32_t paired, lcty_bam_table** out) {
    return guarded([&] {
        if (!path || !names || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const std::vector<uint8_t> b = inflate_gzip(read_whole_file(path), path);
        size_t i = 0;
        // i <= b.size() always holds; n is compared with what is left, so no sum can wrap (l_text / l_name / block_size are 32-bit
        // words of the file: 0xFFFFFFFF + 4 must not pass as 3)
        auto need = [&](uint64_t n) { if (n > b.size() - i) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM", path); };
        need(12);
        if (memcmp(&b[0], "BAM\1", 4)) fail(LCTY_ERR_INVALID_DATA, "%s: not a BAM file", path);
        i = 4;
        const uint32_t l_text = rd32(&b[i]); i += 4; need(static_cast<uint64_t>(l_text) + 4); i += l_text;
        const uint32_t n_ref = rd32(&b[i]); i += 4;
        if (n_ref > (b.size() - i) / 8) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM (%u references in %llu bytes)", path, n_ref, static_cast<unsigned long long>(b.size() - i));
        std::map<std::string, uint32_t> by_name;
        for (uint32_t a = 0; a < n_alleles; a++) by_name[names[a]] = a;
        std::vector<uint32_t> tid2contig(n_ref);
        for (uint32_t r = 0; r < n_ref; r++) {
            need(4); const uint32_t l_name = rd32(&b[i]); i += 4; need(static_cast<uint64_t>(l_name) + 4);
            const std::string nm(reinterpret_cast<const char*>(&b[i]), l_name ? l_name - 1 : 0);
            i += static_cast<size_t>(l_name) + 4;
            const auto it = by_name.find(nm);
            if (it == by_name.end()) fail(LCTY_ERR_INVALID_DATA, "Intermediate BAM file contains unexpected contigs (e.g. %s)", nm.c_str());
            tid2contig[r] = it->second;
        }
        auto T = std::make_unique<lcty_bam_table>();
        T->n_refs = n_ref;
        T->mate_off.push_back(0); T->aln_off.push_back(0); T->cigar_off.push_back(0); T->name_off.push_back(0); T->qual_off.push_back(0);
        static const char NT16[] = "=ACMGRSVTWYHKDBN";
        uint64_t base_at = 0;
        int end_expected = 0;                                  // 0: a new read starts; 1: the second end of the current pair
        bool first_record = true;
        std::string cur_name;
        auto push_mate = [&](const uint8_t* seq, const uint8_t* qual, uint32_t l_seq) {
            T->mate_len.push_back(l_seq);
            const uint64_t words16 = (base_at + l_seq + 15) / 16, words32 = (base_at + l_seq + 31) / 32;
            T->bases2.resize(std::max<size_t>(T->bases2.size(), (words16 + 1) & ~1ull), 0);
            T->nmask.resize(std::max<size_t>(T->nmask.size(), words32), 0);
            for (uint32_t k = 0; k < l_seq; k++) {
                pack_base(T->bases2.data(), T->nmask.data(), base_at + k, static_cast<uint8_t>(NT16[(seq[k >> 1] >> ((~k & 1) << 2)) & 15]));
            }
            T->quals.insert(T->quals.end(), qual, qual + l_seq);
            T->qual_off.push_back(T->quals.size());
            base_at = (base_at + l_seq + 31) / 32 * 32;
            T->mate_off.push_back(base_at);
        };
        auto close_pair = [&] {
            if (T->mate_len.size() % 2) { T->mate_len.push_back(0); T->mate_off.push_back(base_at); T->qual_off.push_back(T->quals.size()); }
            T->aln_off.push_back(T->recs.size());
            T->cigar_off.push_back(T->cigar.size());
        };
        while (i < b.size()) {
            need(4); const uint32_t block = rd32(&b[i]); i += 4; need(block);
            if (block < 32) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BAM record", path);
            const uint8_t* r = &b[i];
            i += block;
            const int32_t ref_id = static_cast<int32_t>(rd32(r)), pos = static_cast<int32_t>(rd32(r + 4));
            const uint32_t l_read_name = r[8], mapq = r[9], n_cigar = r[12] | (r[13] << 8), flag = r[14] | (r[15] << 8), l_seq = rd32(r + 16);
            const size_t fixed = 32 + l_read_name + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq;
            if (fixed > block) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BAM record", path);
            const std::string qname(reinterpret_cast<const char*>(r + 32), l_read_name ? l_read_name - 1 : 0);
            const uint8_t* cg = r + 32 + l_read_name;
            const uint8_t* seq = cg + 4ull * n_cigar;
            const uint8_t* qual = seq + (l_seq + 1) / 2;
            const bool primary = (flag & 2304u) == 0;          // is_primary, locs.rs:405-407
            if (first_record && !primary) fail(LCTY_ERR_INVALID_DATA, "First record in the BAM file is secondary/supplementary");
            first_record = false;
            if (primary) {
                if (end_expected == 1 && paired) {
                    if (qname != cur_name) fail(LCTY_ERR_INVALID_DATA, "Read %s does not have a second read end", cur_name.c_str());
                    push_mate(seq, qual, l_seq);
                    end_expected = 0;
                } else {
                    if (!T->mate_len.empty()) close_pair();
                    cur_name = qname;
                    T->names += qname; T->name_off.push_back(T->names.size());
                    push_mate(seq, qual, l_seq);
                    end_expected = paired ? 1 : 0;
                }
            }
            lcty_aln_rec rec;
            rec.pos = pos < 0 ? 0u : static_cast<uint32_t>(pos);
            if (!(flag & 4u) && (ref_id < 0 || static_cast<uint32_t>(ref_id) >= n_ref)) fail(LCTY_ERR_INVALID_DATA, "%s: mapped record without a reference", path);
            rec.contig = static_cast<uint16_t>((flag & 4u) || ref_id < 0 ? 0 : tid2contig[ref_id]);
            rec.flags = static_cast<uint16_t>(flag & (LCTY_FLAG_UNMAPPED | LCTY_FLAG_REVERSE | LCTY_FLAG_MATE2 | LCTY_FLAG_SECONDARY | LCTY_FLAG_SUPPL));
            rec.n_cigar = n_cigar;
            rec.cigar_rel = static_cast<uint32_t>(T->cigar.size() - T->cigar_off.back());
            for (uint32_t k = 0; k < n_cigar; k++) T->cigar.push_back(rd32(cg + 4 * k));
            T->recs.push_back(rec);
            T->mapq.push_back(static_cast<uint8_t>(mapq));
        }
        if (!T->mate_len.empty()) {
            if (end_expected == 1 && paired) fail(LCTY_ERR_INVALID_DATA, "Read %s does not have a second read end", cur_name.c_str());
            close_pair();
        }
        T->bases2.resize(std::max<size_t>(T->bases2.size(), 2), 0); T->nmask.resize(std::max<size_t>(T->nmask.size(), 1), 0);
        T->view.n_pairs = T->aln_off.size() - 1;
        T->view.mate_len = T->mate_len.data(); T->view.mate_off = T->mate_off.data(); T->view.bases2 = T->bases2.data(); T->view.nmask = T->nmask.data();
        T->view.aln_off = T->aln_off.data(); T->view.recs = T->recs.data(); T->view.cigar_off = T->cigar_off.data(); T->view.cigar = T->cigar.data();
        *out = T.release();
    });
}

// the table as lcty_reads_append takes it; names (optional): name_off[n_pairs + 1] into *name_blob; *n_refs: reference sequences in
// the BAM header (fewer than the locus has alleles = Params::strict_subset, locs.rs:486)
int32_t lcty_bam_table_view(const lcty_bam_table* t, lcty_reads_host* view, const uint64_t** name_off, const char** name_blob, uint32_t* n_refs) {
    return guarded([&] {
        if (!t || !view) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (!t->host_copy) fail(LCTY_ERR_INVALID_INPUT, "the table was read on the device without host_copy: there is no host view (lcty_bam_table_sizes, lcty_reads_append_bam)");
        *view = t->view;
        if (name_off) *name_off = t->name_off.data();
        if (name_blob) *name_blob = t->names.data();
        if (n_refs) *n_refs = t->n_refs;
    });
}

void lcty_bam_table_free(lcty_bam_table* t) { delete t; }

// DB/loci/<locus>/haplotypes.fa.gz as ContigSet::load reads it (seq/contigs.rs:295-306 via fastx): names up to the first blank,
// sequences upper-cased and concatenated. Two calls: names / seqs NULL sizes them (*n_seqs, *names_len incl. one 0 per name, *seqs_len).
int32_t lcty_fasta_read(const char* path, uint32_t* n_seqs, char* names, uint64_t* names_len, uint8_t* seqs, uint64_t* seqs_len, uint64_t* seq_off) {
    return guarded([&] {
        if (!path || !n_seqs || !names_len || !seqs_len) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<uint8_t> raw = read_whole_file(path);
        const std::string p(path);
        const std::vector<uint8_t> text = (has_suffix(p, ".gz") || has_suffix(p, ".bgz")) ? inflate_gzip(raw, path) : raw;
        std::string nm; std::vector<uint8_t> sq; std::vector<uint64_t> off{0};
        uint32_t n = 0;
        size_t i = 0;
        while (i < text.size()) {
            size_t e = i;
            while (e < text.size() && text[e] != '\n') e++;
            size_t le = e;
            if (le > i && text[le - 1] == '\r') le--;
            if (le > i && text[i] == '>') {
                if (n) off.push_back(sq.size());
                size_t q = i + 1;
                while (q < le && text[q] != ' ' && text[q] != '\t') q++;
                nm.append(reinterpret_cast<const char*>(&text[i + 1]), q - i - 1); nm.push_back(0);
                n++;
            } else if (le > i) {
                if (!n) fail(LCTY_ERR_INVALID_DATA, "%s: sequence before the first FASTA header", path);
                for (size_t q = i; q < le; q++) sq.push_back(static_cast<uint8_t>(toupper(text[q])));
            }
            i = e + 1;
        }
        if (n) off.push_back(sq.size());
        if (names && *names_len >= nm.size()) memcpy(names, nm.data(), nm.size());
        else if (names) fail(LCTY_ERR_INVALID_INPUT, "names buffer too small");
        if (seqs && *seqs_len >= sq.size()) memcpy(seqs, sq.data(), sq.size());
        else if (seqs) fail(LCTY_ERR_INVALID_INPUT, "sequence buffer too small");
        if (seq_off) memcpy(seq_off, off.data(), sizeof(uint64_t) * off.size());
        *n_seqs = n; *names_len = nm.size(); *seqs_len = sq.size();
    });
}

// DB/loci/<locus>/haplotypes.paf[.gz|.br|.lz4] as process_paf reads it (command/genotype.rs:1131-1160; PafFile::next, seq/paf.rs:31-56;
// PafEntry::parse, 103-144): the entries lcty_locus_set_hap_alns takes. Left out, as there: empty lines and lines that start with '#',
// lines that name a contig the locus does not have, self-alignments, entries without a cg:Z: tag, and entries that do not cover both
// sequences on the forward strand (HapAlns::add drops those without remembering the pair, transfer.rs:48-52). Fewer than 12 columns,
// a number that does not parse, a strand other than + / - or a CIGAR operation outside MIDSH=X: an error, as there.
// Two calls: id1 = NULL sizes it (*n_entries, *n_cigar); with buffers, *n_entries / *n_cigar hold their capacities on entry.
int32_t lcty_paf_read(const char* path, const char* const* names, uint32_t n_alleles, uint64_t* n_entries, uint32_t* id1, uint32_t* id2,
                      uint32_t* n_matches, uint32_t* aln_len, uint64_t* cigar_off, uint32_t* cigar, uint64_t* n_cigar, uint32_t* dist) {
    return guarded([&] {
        if (!path || !names || !n_entries || !n_cigar) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const bool fill = id1 != nullptr;
        if (fill && (!id2 || !n_matches || !aln_len || !cigar_off || !cigar)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<uint8_t> raw = read_whole_file(path);
        const std::string p(path);
        const std::vector<uint8_t> text = (has_suffix(p, ".gz") || has_suffix(p, ".bgz")) ? inflate_gzip(raw, path)
                                          : has_suffix(p, ".lz4") ? decode_lz4(raw, path) : has_suffix(p, ".br") ? decode_brotli(raw, path) : raw;
        std::unordered_map<std::string, uint32_t> ids;
        for (uint32_t a = 0; a < n_alleles; a++) {
            if (!names[a]) fail(LCTY_ERR_INVALID_INPUT, "null contig name");
            ids.emplace(names[a], a);
        }
        if (dist) std::fill(dist, dist + static_cast<size_t>(n_alleles) * n_alleles, LCTY_NONE_U32);
        const uint64_t cap_e = fill ? *n_entries : 0, cap_c = fill ? *n_cigar : 0;
        uint64_t ne = 0, nc = 0;
        std::vector<uint32_t> words;
        size_t i = 0;
        while (i < text.size()) {
            size_t e = i;
            while (e < text.size() && text[e] != '\n') e++;
            size_t le = e;
            if (le > i && text[le - 1] == '\r') le--;
            const size_t line0 = i;
            i = e + 1;
            if (le == line0 || text[line0] == '#') continue;
            std::vector<std::pair<size_t, size_t>> col;                       // [begin, end)
            for (size_t q = line0, b = line0;; q++) {
                if (q == le || text[q] == '\t') { col.emplace_back(b, q); b = q + 1; if (q == le) break; }
            }
            auto str = [&](size_t c) { return std::string(reinterpret_cast<const char*>(&text[col[c].first]), col[c].second - col[c].first); };
            if (col.size() < 12) fail(LCTY_ERR_INVALID_INPUT, "%s: PAF line (%s) has too few columns", path, str(0).c_str());
            const auto q_it = ids.find(str(0));
            if (q_it == ids.end()) continue;
            const auto t_it = ids.find(str(5));
            if (t_it == ids.end()) continue;
            auto num = [&](size_t c) -> uint32_t {                              // str::parse::<u32>: digits only (a leading '+' is accepted there too)
                const std::string v = str(c);
                size_t k = (!v.empty() && v[0] == '+') ? 1 : 0;
                if (k == v.size()) fail(LCTY_ERR_INVALID_DATA, "%s: could not parse PAF line of %s", path, str(0).c_str());
                uint64_t x = 0;
                for (; k < v.size(); k++) {
                    if (v[k] < '0' || v[k] > '9') fail(LCTY_ERR_INVALID_DATA, "%s: could not parse PAF line of %s", path, str(0).c_str());
                    x = x * 10 + static_cast<uint64_t>(v[k] - '0');
                    if (x > 0xFFFFFFFFull) fail(LCTY_ERR_INVALID_DATA, "%s: could not parse PAF line of %s", path, str(0).c_str());
                }
                return static_cast<uint32_t>(x);
            };
            const uint32_t qlen = num(1), qs = num(2), qe = num(3);
            const std::string strand = str(4);
            if (strand != "+" && strand != "-") fail(LCTY_ERR_INVALID_DATA, "%s: strand '%s'", path, strand.c_str());
            const uint32_t tlen = num(6), ts = num(7), te = num(8), nm = num(9), al = num(10);
            bool have_cigar = false;
            words.clear();
            for (size_t c = 12; c < col.size(); c++) {
                if (col[c].second - col[c].first < 5 || memcmp(&text[col[c].first], "cg:Z:", 5) != 0) continue;
                have_cigar = true;
                words.clear();                                                    // a later tag replaces an earlier one
                uint32_t len = 0;
                for (size_t k = col[c].first + 5; k < col[c].second; k++) {
                    const char ch = static_cast<char>(text[k]);
                    if (ch >= '0' && ch <= '9') { len = 10 * len + static_cast<uint32_t>(ch - '0'); continue; }
                    uint32_t op;
                    switch (ch) {
                        case 'M': op = 0; break; case 'I': op = 1; break; case 'D': op = 2; break; case 'S': op = 4; break;
                        case 'H': op = 5; break; case '=': op = 7; break; case 'X': op = 8; break;
                        case 'N': case 'P': fail(LCTY_ERR_RUNTIME, "CIGAR operations N and P are not supported");
                        default: fail(LCTY_ERR_INVALID_DATA, "Unexpected CIGAR operation %c", ch);
                    }
                    words.push_back((len << 4) | op);
                    len = 0;
                }
            }
            if (q_it->second == t_it->second || !have_cigar) continue;
            // contig_distances (genotype.rs:1148-1150): the edit distance of every such entry, whatever it covers; a later line replaces
            if (dist && al != 0) {
                const uint32_t d = al - nm;
                dist[static_cast<size_t>(q_it->second) * n_alleles + t_it->second] = d;
                dist[static_cast<size_t>(t_it->second) * n_alleles + q_it->second] = d;
            }
            if (strand != "+" || qs != 0 || qe != qlen || ts != 0 || te != tlen) continue;      // full_positive_alignment, paf.rs:211-215
            if (fill) {
                if (ne >= cap_e || nc + words.size() > cap_c) fail(LCTY_ERR_INVALID_INPUT, "PAF buffers too small");
                id1[ne] = q_it->second; id2[ne] = t_it->second; n_matches[ne] = nm; aln_len[ne] = al;
                cigar_off[ne] = nc;
                memcpy(cigar + nc, words.data(), words.size() * sizeof(uint32_t));
            }
            ne++; nc += words.size();
        }
        if (fill) cigar_off[ne] = nc;
        *n_entries = ne; *n_cigar = nc;
    });
}

// DB/loci/<locus>/distances.bin (write_divergences / load_divergences_and_convert, src/seq/minim_div.rs:112-149; not compressed):
// u8 k, u8 w, varint n, then the n (n - 1) / 2 numbers of non-shared minimizers of the pairs (i, j), i < j, row by row
// (TriangleMatrix::indices, src/ext/trimat.rs:15-17) as varints. dist[n_alleles x n_alleles]: symmetric, the diagonal LCTY_NONE_U32.
int32_t lcty_distances_parse(const uint8_t* buf, uint64_t len, uint32_t n_alleles, uint32_t* k, uint32_t* w, uint32_t* dist) {
    return guarded([&] {
        if (!buf || !dist) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        uint64_t at = 0;
        auto byte = [&]() -> uint8_t {
            if (at >= len) fail(LCTY_ERR_INVALID_DATA, "distances: unexpected end of data at byte %llu", static_cast<unsigned long long>(at));
            return buf[at++];
        };
        auto varint = [&]() -> uint32_t {
            uint64_t v = 0;
            for (uint32_t i = 0; i < 5; i++) {
                const uint8_t b = byte();
                v |= static_cast<uint64_t>(b & 0x7Fu) << (7 * i);
                if (!(b & 0x80u)) return static_cast<uint32_t>(v);
            }
            fail(LCTY_ERR_INVALID_DATA, "distances: a varint of more than 5 bytes at byte %llu", static_cast<unsigned long long>(at));
            return 0;
        };
        const uint32_t kk = byte(), ww = byte();
        if (k) *k = kk;
        if (w) *w = ww;
        const uint32_t n = varint();
        if (n != n_alleles)
            fail(LCTY_ERR_INVALID_DATA, "Cannot read distances: invalid number of haplotypes (expected %u, found %u)", n_alleles, n);
        std::fill(dist, dist + static_cast<size_t>(n) * n, LCTY_NONE_U32);
        for (uint32_t i = 0; i + 1 < n; i++)
            for (uint32_t j = i + 1; j < n; j++) {
                const uint32_t d = varint();
                dist[static_cast<size_t>(i) * n + j] = d; dist[static_cast<size_t>(j) * n + i] = d;
            }
    });
}

}  // extern "C"

// ---- the writers of a locus directory (locityper target): the parsers above read back what these write ------------------------------
namespace {
void put_varint(std::vector<uint8_t>& out, uint64_t v) {                        // varint_rs: 7 bits per byte, low first, high bit = more
    while (v >= 0x80) { out.push_back(static_cast<uint8_t>(v) | 0x80); v >>= 7; }
    out.push_back(static_cast<uint8_t>(v));
}
void hand_out(const std::vector<uint8_t>& bytes, uint8_t* out, uint64_t cap, uint64_t* needed) {
    *needed = bytes.size();
    if (!out) return;
    if (cap < bytes.size()) fail(LCTY_ERR_INVALID_INPUT, "output buffer too small (%llu < %zu)", static_cast<unsigned long long>(cap), bytes.size());
    if (!bytes.empty()) memcpy(out, bytes.data(), bytes.size());
}
}  // namespace

extern "C" {

// KmerCounts::save (seq/counts.rs:108-124)
int32_t lcty_kmer_counts_write(uint32_t k, uint32_t counter_bytes, uint32_t n_contigs, const uint64_t* cnt_off, const uint16_t* counts, uint8_t* out,
                               uint64_t cap, uint64_t* needed) {
    return guarded([&] {
        if (!cnt_off || !needed || (cnt_off[n_contigs] && !counts)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (k < 1 || k > 255) fail(LCTY_ERR_INVALID_INPUT, "k = %u does not fit the one byte the format gives it", k);
        if (counter_bytes < 1 || counter_bytes > 8) fail(LCTY_ERR_INVALID_INPUT, "counter length %u: must be 1..8 bytes", counter_bytes);
        const uint32_t max_value = counter_bytes >= 2 ? 65535u : 255u;
        std::vector<uint8_t> b;
        b.reserve(8 + cnt_off[n_contigs] + 5ull * n_contigs);
        b.push_back(static_cast<uint8_t>(k)); b.push_back(static_cast<uint8_t>(counter_bytes));
        put_varint(b, n_contigs);
        for (uint32_t c = 0; c < n_contigs; c++) {
            if (cnt_off[c + 1] < cnt_off[c] || cnt_off[c + 1] - cnt_off[c] > 0xFFFFFFFFull) fail(LCTY_ERR_INVALID_INPUT, "cnt_off is not ascending at %u", c);
            put_varint(b, cnt_off[c + 1] - cnt_off[c]);
            for (uint64_t i = cnt_off[c]; i < cnt_off[c + 1]; i++) {
                if (counts[i] > max_value)
                    fail(LCTY_ERR_INVALID_DATA, "count %u of contig %u exceeds the maximum of a %u-byte counter (%u)", counts[i], c, counter_bytes, max_value);
                put_varint(b, counts[i]);
            }
        }
        hand_out(b, out, cap, needed);
    });
}

// write_divergences (seq/minim_div.rs:113-127)
int32_t lcty_distances_write(uint32_t k, uint32_t w, uint32_t n_alleles, const uint32_t* uniq, uint8_t* out, uint64_t cap, uint64_t* needed) {
    return guarded([&] {
        const uint64_t n_pairs = n_alleles ? uint64_t(n_alleles) * (n_alleles - 1) / 2 : 0;
        if (!needed || (n_pairs && !uniq)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (k > 255 || w > 255) fail(LCTY_ERR_INVALID_INPUT, "k = %u, w = %u: one byte each in the format", k, w);
        std::vector<uint8_t> b;
        b.reserve(8 + 2 * n_pairs);
        b.push_back(static_cast<uint8_t>(k)); b.push_back(static_cast<uint8_t>(w));
        put_varint(b, n_alleles);
        for (uint64_t i = 0; i < n_pairs; i++) put_varint(b, uniq[i]);
        hand_out(b, out, cap, needed);
    });
}

// write_multiline_fasta (seq/fastx.rs:27-43) for every sequence
int32_t lcty_fasta_write_text(uint32_t n_seqs, const char* names, const uint8_t* seqs, const uint64_t* seq_off, char* out, uint64_t cap, uint64_t* needed) {
    return guarded([&] {
        if (!needed || !seq_off || (n_seqs && !names) || (seq_off[n_seqs] && !seqs)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<uint8_t> b;
        b.reserve(seq_off[n_seqs] + seq_off[n_seqs] / 120 + 64ull * n_seqs);
        const char* nm = names;
        for (uint32_t a = 0; a < n_seqs; a++) {
            if (seq_off[a + 1] < seq_off[a]) fail(LCTY_ERR_INVALID_INPUT, "seq_off is not ascending at %u", a);
            const size_t nl = strlen(nm);
            b.push_back('>'); b.insert(b.end(), nm, nm + nl); b.push_back('\n');
            nm += nl + 1;
            for (uint64_t i = seq_off[a]; i < seq_off[a + 1]; i += 120) {
                const uint64_t e = std::min<uint64_t>(i + 120, seq_off[a + 1]);
                b.insert(b.end(), seqs + i, seqs + e); b.push_back('\n');
            }
        }
        hand_out(b, reinterpret_cast<uint8_t*>(out), cap, needed);
    });
}

}  // extern "C"

extern "C" {

// ---- background reads: IndexedReader::fetch + load_alns of `preproc -a` (src/command/preproc.rs:988-1028, 1174-1192) --------------
void lcty_bg_params_default(lcty_bg_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->technology = LCTY_TECH_ILLUMINA;
    p->min_mapq = 30; p->max_clipping = 0.02;                          // preproc.rs:275, 294
    p->insert_pval = 0.001; p->edit_pval = 0.01;                       // bg/mod.rs:39-46
    p->ploidy = 2; p->window_size = 0; p->boundary_size = 1000;        // bg/depth.rs:166-180
    p->uniq_kmer_perc = 90.0; p->frac_windows = 0.5; p->min_tail_obs = 100; p->tail_var_mult = 0.02;
    p->subsampling_rate = 1.0;
}

int32_t lcty_bg_reads_load(const char* path, const char* contig, uint32_t start, uint32_t end, uint32_t padded_start, uint32_t padded_len,
                           const lcty_bg_params* params, lcty_bg_reads** out) {
    return guarded([&] {
        if (!path || !contig || !params || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (start >= end || padded_start > start || static_cast<uint64_t>(padded_start) + padded_len < end)
            fail(LCTY_ERR_INVALID_INPUT, "background interval [%u, %u) is not inside the padded sequence [%u, +%u)", start, end, padded_start, padded_len);
        const std::vector<uint8_t> b = inflate_gzip(read_whole_file(path), path);
        size_t i = 0;
        auto need = [&](uint64_t n) { if (n > b.size() - i) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM", path); };
        need(12);
        if (memcmp(&b[0], "BAM\1", 4)) fail(LCTY_ERR_INVALID_DATA, "%s: not a BAM file", path);
        i = 4;
        const uint32_t l_text = rd32(&b[i]); i += 4; need(static_cast<uint64_t>(l_text) + 4); i += l_text;
        const uint32_t n_ref = rd32(&b[i]); i += 4;
        if (n_ref > (b.size() - i) / 8) fail(LCTY_ERR_INVALID_DATA, "%s: truncated BAM header", path);
        int64_t tid = -1;
        for (uint32_t r = 0; r < n_ref; r++) {
            need(4); const uint32_t l_name = rd32(&b[i]); i += 4; need(static_cast<uint64_t>(l_name) + 4);
            const std::string nm(reinterpret_cast<const char*>(&b[i]), l_name ? l_name - 1 : 0);
            i += static_cast<size_t>(l_name) + 4;
            if (tid < 0 && nm == contig) tid = r;
        }
        if (tid < 0) fail(LCTY_ERR_INVALID_INPUT, "%s: no reference sequence %s in the BAM header", path, contig);
        const uint64_t padded_end = static_cast<uint64_t>(padded_start) + padded_len;
        auto T = std::make_unique<lcty_bg_reads>();
        T->cigar_off.push_back(0); T->seq_off.push_back(0);
        std::vector<std::string> names;
        uint64_t paired_counts[2] = {0, 0}, ignored = 0, wo_cigar = 0;
        static const char NT16[] = "=ACMGRSVTWYHKDBN";
        auto consumes_ref = [](uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; };
        while (i < b.size()) {
            need(4); const uint32_t block = rd32(&b[i]); i += 4; need(block);
            if (block < 32) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BAM record", path);
            const uint8_t* r = &b[i];
            i += block;
            const int32_t ref_id = static_cast<int32_t>(rd32(r)), pos = static_cast<int32_t>(rd32(r + 4));
            const uint32_t l_read_name = r[8], mapq = r[9], n_cigar = r[12] | (r[13] << 8), flag = r[14] | (r[15] << 8), l_seq = rd32(r + 16);
            const size_t fixed = 32 + l_read_name + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq;
            if (fixed > block) fail(LCTY_ERR_INVALID_DATA, "%s: corrupt BAM record", path);
            if (ref_id != tid || pos < 0) continue;
            const uint8_t* cg = r + 32 + l_read_name;
            uint64_t ref_len = 0;
            for (uint32_t k = 0; k < n_cigar; k++) { const uint32_t w = rd32(cg + 4 * k); if (consumes_ref(w & 15u)) ref_len += w >> 4; }
            // the records IndexedReader::fetch returns: overlapping [start, end); no reference span counts as one base (bam_endpos)
            const uint64_t rec_end = static_cast<uint64_t>(pos) + ((flag & 4u) || ref_len == 0 ? 1 : ref_len);
            if (static_cast<uint64_t>(pos) >= end || rec_end <= start) continue;
            // load_alns filter (preproc.rs:1006); clipping_rate / raw_clipping (seq/cigar.rs:944-966)
            bool keep = (flag & 3844u) == 0 && mapq >= params->min_mapq;
            if (keep) {
                if (n_cigar == 0) fail(LCTY_ERR_INVALID_DATA, "%s: mapped record without a CIGAR", path);
                const uint32_t first = rd32(cg), last = rd32(cg + 4ull * (n_cigar - 1));
                const uint32_t clip = (consumes_ref(first & 15u) ? 0 : first >> 4) + (consumes_ref(last & 15u) ? 0 : last >> 4);
                const double rate = clip == 0 ? 0.0 : static_cast<double>(clip) / static_cast<double>(l_seq);
                keep = rate <= params->max_clipping;
            }
            if (!keep) { ignored++; continue; }
            // Cigar::infer_ext_cigar (cigar.rs:434-476): an M run outside the padded sequence -> no extended CIGAR
            uint64_t rl = 0, ql = 0;
            bool dropped = false;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t w = rd32(cg + 4 * k), op = w & 15u, len = w >> 4;
                if (op == 0 && (pos + rl < padded_start || pos + rl + len >= padded_end)) { dropped = true; break; }
                if (consumes_ref(op)) rl += len;
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ql += len;
            }
            if (dropped) { wo_cigar++; continue; }
            const std::string qname(reinterpret_cast<const char*>(r + 32), l_read_name ? l_read_name - 1 : 0);
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t op = rd32(cg + 4 * k) & 15u;
                if (op == 3 || op == 5 || op == 6 || op > 8)
                    fail(LCTY_ERR_INVALID_DATA, "Read %s: unsupported CIGAR operation %c in a background alignment", qname.c_str(), "MIDNSHP=X???????"[op]);
            }
            if (ql != l_seq) fail(LCTY_ERR_INVALID_DATA, "Failed to convert CIGAR for read \"%s\" (query length %llu, SEQ length %u)",
                                  qname.c_str(), static_cast<unsigned long long>(ql), l_seq);
            paired_counts[(flag & 1u) ? 1 : 0]++;
            T->pos.push_back(static_cast<uint32_t>(pos)); T->end.push_back(static_cast<uint32_t>(pos + rl)); T->qlen.push_back(l_seq);
            T->flags.push_back(static_cast<uint8_t>(((flag & 0x10u) ? LCTY_BG_REVERSE : 0u) | ((flag & 0x80u) ? LCTY_BG_SECOND : 0u)));
            for (uint32_t k = 0; k < n_cigar; k++) T->cigar.push_back(rd32(cg + 4 * k));
            T->cigar_off.push_back(T->cigar.size());
            const uint8_t* seq = cg + 4ull * n_cigar;
            const uint64_t base_at = T->seq_off.back();
            const uint64_t next = (base_at + l_seq + 31) / 32 * 32;
            T->bases2.resize(next / 16 + 2, 0); T->nmask.resize(next / 32 + 1, 0);
            for (uint32_t k = 0; k < l_seq; k++) {
                pack_base(T->bases2.data(), T->nmask.data(), base_at + k, static_cast<uint8_t>(NT16[(seq[k >> 1] >> ((~k & 1) << 2)) & 15]));
            }
            T->seq_off.push_back(next);
            names.push_back(qname);
        }
        if (paired_counts[0] > 0 && paired_counts[1] > 0) fail(LCTY_ERR_INVALID_DATA, "BAM file contains both paired and unpaired reads");
        if (T->pos.empty()) fail(LCTY_ERR_INVALID_DATA, "BAM file contains no reads in the target region");
        const bool paired = paired_counts[1] > 0;
        if (paired && params->technology != LCTY_TECH_ILLUMINA) fail(LCTY_ERR_INVALID_INPUT, "Paired end reads are not supported by this technology");
        const size_t n = T->pos.size();
        T->bases2.resize(std::max<size_t>(T->bases2.size(), 2), 0); T->nmask.resize(std::max<size_t>(T->nmask.size(), 1), 0);
        T->mate.assign(n, LCTY_NONE_U32);
        if (paired) {                                       // group_mates (bg/insertsz.rs:25-37): both ends inside the loaded set
            std::unordered_map<std::string, std::array<uint32_t, 2>> by_name;
            by_name.reserve(n);
            for (size_t a = 0; a < n; a++) {
                const int e = (T->flags[a] & LCTY_BG_SECOND) ? 1 : 0;
                auto& slot = by_name.try_emplace(names[a], std::array<uint32_t, 2>{LCTY_NONE_U32, LCTY_NONE_U32}).first->second;
                if (slot[e] != LCTY_NONE_U32) fail(LCTY_ERR_INVALID_DATA, "Read %s has several %s mates", names[a].c_str(), e ? "second" : "first");
                slot[e] = static_cast<uint32_t>(a);
            }
            for (const auto& kv : by_name)
                if (kv.second[0] != LCTY_NONE_U32 && kv.second[1] != LCTY_NONE_U32) { T->mate[kv.second[0]] = kv.second[1]; T->mate[kv.second[1]] = kv.second[0]; }
        }
        double sum = 0.0;                                   // read_len_from_alns (preproc.rs:1031-1037)
        const size_t m = std::min<size_t>(n, 10000);
        for (size_t a = 0; a < m; a++) sum += static_cast<double>(T->qlen[a]);
        lcty_bg_reads_view& v = T->view;
        v.n_records = n; v.n_ignored = ignored; v.n_wo_cigar = wo_cigar; v.paired = paired ? 1 : 0;
        v.read_len = sum / static_cast<double>(m);
        v.pos = T->pos.data(); v.end = T->end.data(); v.qlen = T->qlen.data(); v.flags = T->flags.data(); v.mate = T->mate.data();
        v.cigar_off = T->cigar_off.data(); v.cigar = T->cigar.data(); v.seq_off = T->seq_off.data();
        v.bases2 = T->bases2.data(); v.nmask = T->nmask.data();
        *out = T.release();
    });
}

int32_t lcty_bg_reads_view_get(const lcty_bg_reads* reads, lcty_bg_reads_view* view) {
    return guarded([&] {
        if (!reads || !view) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *view = reads->view;
    });
}

void lcty_bg_reads_free(lcty_bg_reads* reads) { delete reads; }

// BgDistr::save (bg/mod.rs:147-158): seq_info (349-357), insert_distr (insertsz.rs:184-193, {} single-end), error_profile
// (err_prof.rs:308-319), bg_depth (depth.rs:387-398)
int32_t lcty_bg_to_json(const lcty_bg* bg, double read_len, uint32_t ploidy, char* out, uint64_t cap, uint64_t* needed) {
    return guarded([&] {
        if (!bg || !needed) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        static const char* const techs[4] = {"illumina", "hifi", "pacbio", "ont"};
        if (bg->technology < 0 || bg->technology > 3) fail(LCTY_ERR_INVALID_INPUT, "unknown technology %d", bg->technology);
        std::string s = "{\"seq_info\":{\"read_len\":" + json_num(read_len) + ",\"technology\":\"" + techs[bg->technology]
                      + "\",\"total_reads\":null,\"file_size\":null},\"insert_distr\":{";
        if (bg->is_paired) s += "\"n\":" + json_num(bg->ins_n) + ",\"p\":" + json_num(bg->ins_p);
        s += "},\"error_profile\":{";
        static const char* const ops[5] = {"matches", "mismatches", "insertions", "deletions", "clipping"};
        for (int k = 0; k < 5; k++) s += std::string("\"") + ops[k] + "\":" + json_num(bg->op_lnprobs[k]) + ",";
        s += "\"alpha\":" + json_num(bg->edit_alpha) + ",\"beta\":" + json_num(bg->edit_beta) + "},\"bg_depth\":{\"ploidy\":"
           + std::to_string(ploidy) + ",\"window\":" + std::to_string(bg->window) + ",\"neighb\":" + std::to_string(bg->neighb);
        for (int which = 0; which < 2; which++) {
            s += which ? ",\"p\":[" : ",\"n\":[";
            for (int g = 0; g < LCTY_GC_BINS; g++) s += (g ? "," : "") + json_num(which ? bg->depth_p[g] : bg->depth_n[g]);
            s += "]";
        }
        s += "}}";
        *needed = s.size() + 1;
        if (out) {
            if (cap < s.size() + 1) fail(LCTY_ERR_INVALID_INPUT, "output buffer of %llu bytes, %zu needed", static_cast<unsigned long long>(cap), s.size() + 1);
            memcpy(out, s.c_str(), s.size() + 1);
        }
    });
}

}  // extern "C"

// ---- pangenome VCF (text: plain, gzip, BGZF; no index, no BCF) --------------------------------------------------------------------------
// What bcf::IndexedReader gives panvcf.rs: the samples of the header, the ploidies of the first record (HaplotypeNames::new, 85-91) and
// the records of a region with their alleles and GT fields (filter_variants, 155-172).
struct lcty_vcf {
    std::vector<uint8_t> text;
    std::vector<std::string> samples;
    std::string sample_blob;
    std::vector<uint32_t> ploidy, hap_off;           // of the first record; hap_off[n_samples + 1]
    struct Line { uint64_t begin, end; uint32_t contig, pos, ref_len; };
    std::vector<Line> lines;                         // the records in file order
    std::vector<std::string> contigs;                // in the order of first appearance
    lcty_vcf_view view{};
};

// the line rules (split_tabs, parse_gt, gt_index, the head of a record, a record of a region) are in lcty_bgzf_index.hpp: the indexed
// reader (lcty_vcf_fetch.hip) raises its errors through the same functions
using namespace lcty::vcfidx;

extern "C" {

int32_t lcty_vcf_open(const char* path, lcty_vcf** out) {
    return guarded([&] {
        if (!path || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *out = nullptr;
        const std::string p(path);
        if (has_suffix(p, ".bcf")) fail(LCTY_ERR_UNSUPPORTED, "%s: BCF is not read here, convert it to a text VCF", path);
        auto V = std::make_unique<lcty_vcf>();
        std::vector<uint8_t> raw = read_whole_file(path);
        if (raw.size() >= 2 && raw[0] == 0x1f && raw[1] == 0x8b) V->text = inflate_gzip(raw, path); else V->text.swap(raw);
        const std::vector<uint8_t>& t = V->text;
        bool have_header = false;
        std::unordered_map<std::string, uint32_t> contig_ix;
        for (uint64_t b = 0; b < t.size();) {
            uint64_t e = b;
            while (e < t.size() && t[e] != '\n') e++;
            uint64_t le = e;
            if (le > b && t[le - 1] == '\r') le--;
            if (le > b) {
                if (t[b] == '#') {
                    if (le - b >= 6 && !memcmp(&t[b], "#CHROM", 6)) {
                        parse_chrom_line(t.data(), b, le, path, V->samples);
                        have_header = true;
                    }
                } else {
                    if (!have_header) fail_record_before_header(path);
                    const LineHead h = parse_line_head(t.data(), b, le, path);                                    // CHROM, POS, len(REF)
                    const std::string& chrom = h.chrom;
                    auto it = contig_ix.find(chrom);
                    if (it == contig_ix.end()) { it = contig_ix.emplace(chrom, static_cast<uint32_t>(V->contigs.size())).first; V->contigs.push_back(chrom); }
                    V->lines.push_back({b, le, it->second, h.pos, h.ref_len});
                }
            }
            b = e + 1;
        }
        if (!have_header) fail_no_header(path);
        if (V->lines.empty()) fail_no_records();
        // the ploidies of the first record
        const uint32_t S = static_cast<uint32_t>(V->samples.size());
        V->ploidy.assign(S, 0); V->hap_off.assign(S + 1, 0);
        if (S) {
            const lcty_vcf::Line& l0 = V->lines[0];
            const std::string where = V->contigs[l0.contig] + ":" + std::to_string(uint64_t(l0.pos) + 1);
            first_record_ploidy(t.data(), l0.begin, l0.end, where, S, V->ploidy);
        }
        for (uint32_t i = 0; i < S; i++) { V->hap_off[i + 1] = V->hap_off[i] + V->ploidy[i]; V->sample_blob += V->samples[i]; V->sample_blob.push_back('\0'); }
        V->view.n_samples = S; V->view.n_haps = V->hap_off[S]; V->view.n_records = V->lines.size();
        V->view.samples = V->sample_blob.data(); V->view.samples_len = V->sample_blob.size();
        V->view.ploidy = V->ploidy.data(); V->view.hap_off = V->hap_off.data();
        *out = V.release();
    });
}

int32_t lcty_vcf_view_get(const lcty_vcf* vcf, lcty_vcf_view* view) {
    return guarded([&] {
        if (!vcf || !view) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *view = vcf->view;
    });
}

void lcty_vcf_free(lcty_vcf* vcf) { delete vcf; }

int32_t lcty_vcf_region(const lcty_vcf* vcf, const char* contig, uint32_t start, uint32_t end, const uint8_t* sample_used, lcty_vcf_records* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!vcf || !contig || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const uint32_t S = vcf->view.n_samples, Hn = vcf->view.n_haps;
        uint32_t cix = LCTY_NONE_U32;
        for (uint32_t i = 0; i < vcf->contigs.size(); i++) if (vcf->contigs[i] == contig) cix = i;
        RecordArrays A;
        std::vector<int32_t> al;
        const uint8_t* t = vcf->text.data();
        for (const lcty_vcf::Line& l : vcf->lines) {
            if (l.contig != cix || !(l.pos < end && uint64_t(l.pos) + l.ref_len > start)) continue;          // htslib's fetch; INFO/END is not looked at
            parse_record_line(t, l.begin, l.end, contig, l.pos, l.ref_len, S, vcf->ploidy.data(), vcf->samples, sample_used, A, al);
        }
        lcty_vcf_records o{}; Handoff h;
        o.n_recs = static_cast<uint32_t>(A.pos.size()); o.n_haps = Hn; o.n_samples = S; o.n_alleles = A.allele_off.size() - 1; o.pool_len = A.pool.size();
        o.pos = h.copy(A.pos); o.ref_len = h.copy(A.rlen); o.rec_allele = h.copy(A.rec_allele);
        o.allele_off = h.copy(A.allele_off); o.allele_bytes = h.copy(A.pool); o.gt = h.copy(A.gt); o.phased = h.copy(A.phased);
        *out = o; h.commit();
    });
}

void lcty_vcf_records_free(lcty_vcf_records* r) {
    if (!r) return;
    free(r->pos); free(r->ref_len); free(r->rec_allele); free(r->allele_off); free(r->allele_bytes); free(r->gt); free(r->phased);
    memset(r, 0, sizeof(*r));
}

}  // extern "C"
