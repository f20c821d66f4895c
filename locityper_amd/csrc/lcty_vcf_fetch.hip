// lcty_vcf_fetch.hip — a locus's window of an indexed pangenome VCF, the input of `locityper target -v`:
//   src/command/add.rs:496-499 the two fetches of the flanks, 802 bcf::IndexedReader
//   src/seq/panvcf.rs:85-91 HaplotypeNames::new, 149-184 filter_variants
// Host: the tabix index and the lines of the file's head (lcty_bgzf_index.hpp), the chunks of the window, pread of their byte
// ranges, the BGZF split and the inflate into one slice (Slice of lcty_bgzf_read.hpp: zlib, or the device with knob
// "sample_bam_inflate" 1). Device, on the text of that slice and one (begin, end) byte range per merged chunk:
//   line_kernel     16 bytes per lane: a line starts at the start of a range and behind every '\n' inside one; counted per workgroup,
//                   scanned (exclusive_scan), then written in file order
//   head_kernel     a wavefront per line: its end (without '\r'), the first nine tabs (256 bytes per step, a scan of the lanes' tab
//                   counts), CHROM against the contig in full, POS, len(REF), the keep rule, the alleles of ALT and their bytes, the
//                   place of GT among the FORMAT keys
//   compact_kernel  kept lines -> records in file order (scan of the kept flags); scans of the allele counts and the allele bytes
//   allele_kernel   a wavefront per record: REF and the ALT alleles into the pool, their offsets
//   gt_kernel       a wavefront per record: the tabs behind the ninth column, 256 bytes per step; the lane that holds the tab in front
//                   of sample i parses its GT subfield (the rules of parse_gt) and writes gt and phased; the column count
// Every error — of a kept record, or a bad position in any line that names the contig — goes to the error word with the line's
// ordinal (refuse, lcty_device.hpp); the host then runs the line functions of lcty_vcf_region over that one line, so status and text are that reader's.
#include <memory>
#include <string>
#include <vector>

#include "lcty_bgzf_read.hpp"
#include "lcty_objects.hpp"
#include "lcty_scan.hpp"

namespace lcty {

constexpr uint32_t LINE_BYTES = 16, LINE_THREADS = 256;            // line_kernel: bytes per lane, lanes per workgroup
enum : uint32_t { E_LONG = 1, E_LINE = 2 };                         // error classes of a line (refuse, lcty_device.hpp)

// the merged chunks as byte ranges of the slice, sorted and disjoint
struct Ranges { const uint64_t* beg; const uint64_t* end; uint32_t n; };
// the last range that begins at or before p; -1: none
__device__ __forceinline__ int range_of(const Ranges& R, uint64_t p) {
    int lo = -1, hi = static_cast<int>(R.n);
    while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (R.beg[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}

// WRITE = false: count[g] = lines that start in the 4 096 bytes of workgroup g. WRITE = true: their starts to line_start, from
// place offs[g] on. A line starts at the first byte of a range and behind every '\n' that has a byte of its range behind it.
template <bool WRITE>
__global__ __launch_bounds__(LINE_THREADS) void line_kernel(const uint8_t* __restrict__ raw, uint64_t total, const Ranges R, uint32_t* __restrict__ count,
                                                            const uint32_t* __restrict__ offs, uint64_t* __restrict__ line_start) {
    __shared__ uint32_t wsum[LINE_THREADS / WAVE];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint64_t base = (static_cast<uint64_t>(blockIdx.x) * LINE_THREADS + tid) * LINE_BYTES;
    uint32_t mask = 0;
    if (base < total) {
        const uint4 w = *reinterpret_cast<const uint4*>(raw + base);           // base + 16 <= total + SLICE_PAD
        const uint32_t words[4] = {w.x, w.y, w.z, w.w};
        uint32_t prev = base ? raw[base - 1] : 0u;
        int r = range_of(R, base);
        for (uint32_t j = 0; j < LINE_BYTES; j++) {
            const uint64_t p = base + j;
            const uint32_t c = (words[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
            if (p < total) {
                while (r + 1 < static_cast<int>(R.n) && R.beg[r + 1] <= p) r++;
                if (r >= 0 && p < R.end[r] && (p == R.beg[r] || prev == '\n')) mask |= 1u << j;
            }
            prev = c;
        }
    }
    const uint32_t cnt = __popc(mask);
    const uint32_t incl = wave_scan_incl(cnt, AddOp{});
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t v = 0; v < LINE_THREADS / WAVE; v++) { if (v < wave) before += wsum[v]; all += wsum[v]; }
    if (!WRITE) { if (tid == 0) count[blockIdx.x] = all; return; }
    uint64_t at = static_cast<uint64_t>(offs[blockIdx.x]) + before + incl - cnt;
    while (mask) {
        const uint32_t j = __ffs(mask) - 1;
        mask &= mask - 1;
        line_start[at++] = base + j;
    }
}

// what head_kernel finds in a kept line
struct LineInfo {
    uint64_t ref_at, tab8, le;                  // first byte of REF, the ninth tab (with samples), the end of the line
    uint32_t pos, rlen, nall, nbytes, alt_len, which;   // 0-based POS, len(REF), alleles, their bytes, len(ALT field), place of GT in FORMAT
};

struct HeadView {
    const uint8_t* raw; Ranges R;
    const uint64_t* line_start; uint32_t n_lines;
    const uint8_t* contig; uint32_t contig_len;
    uint32_t start, end, S;
    uint32_t* kept; LineInfo* info;
    unsigned long long* err;
};

__global__ __launch_bounds__(WAVE) void head_kernel(const HeadView V) {
    __shared__ uint64_t s_tab[9];
    const uint32_t l = blockIdx.x, lane = threadIdx.x;
    const uint8_t* raw = V.raw;
    const uint64_t b = V.line_start[l];
    // ---- the end of the line: the '\n' in front of the next line of this range, else the end of the range; '\r' is no part of it
    const int r = range_of(V.R, b);
    if (lane == 0) V.kept[l] = 0;
    if (r < 0) return;                                                         // a line starts inside a range
    const uint64_t rend = V.R.end[r];
    const uint64_t next = l + 1 < V.n_lines ? V.line_start[l + 1] : ~0ull;
    uint64_t le = next < rend ? next - 1 : rend;
    if (!(next < rend) && le > b && raw[le - 1] == '\n') le--;
    if (le > b && raw[le - 1] == '\r') le--;
    if (le == b || raw[b] == '#') return;
    auto refuse = [&](uint32_t cls) { if (lane == 0) lcty::refuse(V.err, l, cls); };
    if (le - b >= (1ull << 32)) { refuse(E_LONG); return; }
    // ---- the first nine tabs: 256 bytes per step, a dword per lane; nothing assumes they lie in the first step
    uint32_t nt = 0;
    for (uint64_t off = b & ~3ull; off < le && nt < 9; off += 4ull * WAVE) {
        const uint64_t my = off + 4ull * lane;
        const uint32_t w = my < le ? *reinterpret_cast<const uint32_t*>(raw + my) : 0u;    // the dword of a byte before `le` ends inside SLICE_PAD
        uint32_t tabs = 0;
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t p = my + j;
            if (p >= b && p < le && ((w >> (8u * j)) & 0xFFu) == '\t') tabs |= 1u << j;
        }
        const uint32_t cnt = __popc(tabs);
        const uint32_t incl = wave_scan_incl(cnt, AddOp{});
        uint32_t ord = nt + incl - cnt;
        while (tabs) {
            const uint32_t j = __ffs(tabs) - 1;
            tabs &= tabs - 1;
            if (ord < 9) s_tab[ord] = my + j;
            ord++;
        }
        nt += __shfl(incl, WAVE - 1);
    }
    __syncthreads();
    const uint32_t ntab = min(nt, 9u);
    // ---- CHROM, compared with the contig in full
    const uint64_t clen = (ntab ? s_tab[0] : le) - b;
    bool differs = clen != V.contig_len;
    if (!differs) for (uint32_t i = lane; i < V.contig_len; i += WAVE) differs |= raw[b + i] != V.contig[i];
    if (__any(differs)) return;
    if (ntab < 4) { refuse(E_LINE); return; }                                  // fewer than five columns
    // ---- POS: digits only, 1 <= POS <= 2^32 - 1 (every lane walks the same few bytes)
    uint64_t pos = 0;
    bool bad = s_tab[1] == s_tab[0] + 1;
    for (uint64_t i = s_tab[0] + 1; i < s_tab[1] && !bad; i++) {
        const uint32_t c = raw[i];
        if (c < '0' || c > '9' || pos > 0xFFFFFFFFull) bad = true; else pos = pos * 10 + (c - '0');
    }
    if (bad || pos < 1 || pos > 0xFFFFFFFFull) { refuse(E_LINE); return; }
    const uint32_t pos0 = static_cast<uint32_t>(pos - 1), rlen = static_cast<uint32_t>(s_tab[3] - s_tab[2] - 1);
    if (!(pos0 < V.end && static_cast<uint64_t>(pos0) + rlen > V.start)) return;          // htslib's fetch; INFO/END is not looked at
    if (ntab < (V.S ? 9u : 7u)) { refuse(E_LINE); return; }                    // the column count (with samples: gt_kernel counts the rest)
    // ---- ALT: '.' is no allele, else commas separate them
    const uint64_t a_b = s_tab[3] + 1, a_e = s_tab[4];
    const uint32_t alt_len = static_cast<uint32_t>(a_e - a_b);
    uint32_t commas = 0;
    for (uint64_t i = a_b + lane; i < a_e; i += WAVE) commas += raw[i] == ',' ? 1u : 0u;
    commas = wave_reduce(commas, AddOp{});
    const uint32_t n_alt = (alt_len == 1 && raw[a_b] == '.') ? 0u : commas + 1u;
    // ---- the place of GT among the FORMAT keys
    uint32_t which = 0;
    if (V.S) {
        const uint64_t f_b = s_tab[7] + 1, f_e = s_tab[8];
        bool found = false;
        uint64_t s = f_b;
        for (uint64_t i = f_b; i <= f_e && !found; i++)
            if (i == f_e || raw[i] == ':') {
                if (i - s == 2 && raw[s] == 'G' && raw[s + 1] == 'T') found = true; else { which++; s = i + 1; }
            }
        if (!found) { refuse(E_LINE); return; }
    }
    if (lane == 0) {
        LineInfo I;
        I.ref_at = s_tab[2] + 1; I.tab8 = V.S ? s_tab[8] : 0ull; I.le = le;
        I.pos = pos0; I.rlen = rlen; I.nall = 1u + n_alt; I.nbytes = rlen + (n_alt ? alt_len - commas : 0u); I.alt_len = alt_len; I.which = which;
        V.info[l] = I;
        V.kept[l] = 1;
    }
}

// kept line l -> record scan[l], in file order
__global__ __launch_bounds__(256) void compact_kernel(uint32_t n_lines, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ scan,
                                                      const LineInfo* __restrict__ info, LineInfo* __restrict__ rec, uint32_t* __restrict__ rec_line,
                                                      uint32_t* __restrict__ pos, uint32_t* __restrict__ rlen, uint32_t* __restrict__ nall, uint32_t* __restrict__ nbytes) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l >= n_lines || !kept[l]) return;
    const uint32_t k = scan[l];
    const LineInfo I = info[l];
    rec[k] = I; rec_line[k] = l;
    pos[k] = I.pos; rlen[k] = I.rlen; nall[k] = I.nall; nbytes[k] = I.nbytes;
}

// record k: REF and the ALT alleles, verbatim, into pool[byte_off[k] ..), and the start of each in allele_off[rec_allele[k] ..)
__global__ __launch_bounds__(WAVE) void allele_kernel(const uint8_t* __restrict__ raw, uint32_t n_recs, const LineInfo* __restrict__ rec, const uint32_t* __restrict__ rec_allele,
                                                      const uint64_t* __restrict__ byte_off, uint64_t* __restrict__ allele_off, uint8_t* __restrict__ pool) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const LineInfo I = rec[k];
    const uint64_t base = byte_off[k];
    const uint32_t ra = rec_allele[k];
    if (lane == 0) {
        allele_off[ra] = base;
        if (I.nall > 1) allele_off[ra + 1] = base + I.rlen;
        if (k + 1 == n_recs) allele_off[ra + I.nall] = byte_off[n_recs];
    }
    for (uint32_t i = lane; i < I.rlen; i += WAVE) pool[base + i] = raw[I.ref_at + i];
    if (I.nall < 2) return;
    const uint64_t a_b = I.ref_at + I.rlen + 1, dst = base + I.rlen;
    uint32_t carry = 0;                                                        // commas in front of this step
    for (uint32_t j0 = 0; j0 < I.alt_len; j0 += WAVE) {
        const uint32_t j = j0 + lane;
        const bool valid = j < I.alt_len;
        const uint8_t c = valid ? raw[a_b + j] : uint8_t(0);
        const uint32_t comma = valid && c == ',' ? 1u : 0u;
        const uint32_t incl = wave_scan_incl(comma, AddOp{});
        const uint32_t before = carry + incl - comma;
        if (valid && !comma) pool[dst + j - before] = c;
        if (comma) allele_off[ra + 2 + before] = dst + (j + 1) - (before + 1);
        carry += __shfl(incl, WAVE - 1);
    }
}

struct GtView {
    const uint8_t* raw;
    const LineInfo* rec; const uint32_t* rec_line;
    uint32_t S, n_haps;
    const uint32_t* ploidy; const uint32_t* hap_off; const uint8_t* sample_used;   // sample_used null: all
    int16_t* gt; uint8_t* phased;
    unsigned long long* err;
};

// The GT subfield of the sample field that starts at q (it ends at a tab or at le): parse_gt of lcty_bgzf_index.hpp and the two
// checks of a used sample. Writes the ploidy[i] entries of gt and the entry of phased as the host reader does; false: an error.
__device__ inline bool sample_field(const GtView& V, uint64_t k, uint32_t i, uint64_t q, uint64_t le, uint32_t which) {
    const uint8_t* raw = V.raw;
    auto ch = [&](uint64_t p) -> uint32_t { return p < le ? raw[p] : uint32_t('\t'); };
    for (uint32_t skip = 0; skip < which; skip++) {
        uint32_t c = ch(q);
        while (c != '\t' && c != ':') { q++; c = ch(q); }
        if (c == ':') q++; else break;
    }
    const uint32_t pl = V.ploidy[i];
    int16_t* out = V.gt + k * V.n_haps + V.hap_off[i];
    uint32_t n_al = 0;
    bool ph = true, ok = true;
    uint32_t c = ch(q);
    if (c == '\t' || c == ':') { if (pl) out[0] = -1; n_al = 1; }               // a dropped trailing field: one missing allele
    else {
        for (;;) {
            int32_t a = -1;
            if (c == '.') q++;
            else {
                if (c < '0' || c > '9') { ok = false; break; }
                a = 0;
                while (c >= '0' && c <= '9') { a = a * 10 + static_cast<int32_t>(c - '0'); if (a > 32767) break; q++; c = ch(q); }
                if (a > 32767) { ok = false; break; }
            }
            if (n_al < pl) out[n_al] = static_cast<int16_t>(a);
            n_al++;
            c = ch(q);
            if (c == '\t' || c == ':') break;
            if (c != '/' && c != '|') { ok = false; break; }
            ph = c == '|';
            q++; c = ch(q);
            if (c == '\t' || c == ':') { ok = false; break; }
        }
    }
    for (uint32_t h = n_al; h < pl; h++) out[h] = -1;
    V.phased[k * V.S + i] = ph ? 1 : 0;
    const bool used = !V.sample_used || V.sample_used[i];
    if (used && (n_al != pl || (pl > 1 && !ph))) ok = false;
    return ok;
}

__global__ __launch_bounds__(WAVE) void gt_kernel(const GtView V) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const LineInfo I = V.rec[k];
    const uint8_t* raw = V.raw;
    bool ok = true;
    uint32_t seen = 0;                                                         // tabs from the ninth on, in front of this step
    for (uint64_t off = I.tab8 & ~3ull; off < I.le; off += 4ull * WAVE) {
        const uint64_t my = off + 4ull * lane;
        const uint32_t w = my < I.le ? *reinterpret_cast<const uint32_t*>(raw + my) : 0u;
        uint32_t tabs = 0;
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t p = my + j;
            if (p >= I.tab8 && p < I.le && ((w >> (8u * j)) & 0xFFu) == '\t') tabs |= 1u << j;
        }
        const uint32_t cnt = __popc(tabs);
        const uint32_t incl = wave_scan_incl(cnt, AddOp{});
        uint32_t i = seen + incl - cnt;                                        // the sample behind this lane's first tab
        while (tabs) {
            const uint32_t j = __ffs(tabs) - 1;
            tabs &= tabs - 1;
            if (i < V.S) ok &= sample_field(V, k, i, my + j + 1, I.le, I.which);
            i++;
        }
        seen += __shfl(incl, WAVE - 1);
    }
    if (seen != V.S) ok = false;                                               // 9 + S columns
    if (__any(!ok) && lane == 0) refuse(V.err, V.rec_line[k], E_LINE);
}

}  // namespace lcty

using namespace lcty;

struct lcty_vcf_indexed {
    BgzfFile file;
    std::string index_path;
    vcfidx::Tbi tbi;
    std::vector<std::string> samples;
    std::string sample_blob;
    std::vector<uint32_t> ploidy, hap_off;           // of the first record of the file; hap_off[n_samples + 1]
    lcty_vcf_view view{};
    std::vector<std::string> contigs; std::vector<uint64_t> contig_len; std::string contig_blob;      // lcty_vcf_indexed_contigs
};

namespace {

// the .tbi file: BGZF, inflated by zlib block after block
void load_tbi(lcty_vcf_indexed* v) {
    const char* ip = v->index_path.c_str();
    BgzfFile f;
    f.open(ip);
    uint8_t magic[2] = {0, 0};
    if (f.fsize >= 2) pread_all(f.fd, magic, 2, 0, ip);
    if (magic[0] != 0x1f || magic[1] != 0x8b) fail(LCTY_ERR_INVALID_DATA, "%s is not a tabix index (it is not compressed)", ip);
    BgzfSerial in(f.fd, f.fsize, ip);
    std::vector<uint8_t> x;
    while (in.append_block(x)) {}
    v->tbi = vcfidx::parse_tbi(x.data(), x.size(), ip);
}

// one ##contig line behind `##contig=<`: ID=name and length=n among its comma-separated keys (a line without an ID is passed over)
void note_contig(lcty_vcf_indexed* v, std::string body) {
    if (!body.empty() && body.back() == '>') body.pop_back();
    std::string id; uint64_t len = 0;
    for (size_t at = 0; at <= body.size();) {
        size_t e = body.find(',', at);
        if (e == std::string::npos) e = body.size();
        const std::string kv = body.substr(at, e - at);
        if (kv.compare(0, 3, "ID=") == 0) id = kv.substr(3);
        else if (kv.compare(0, 7, "length=") == 0) { len = 0; for (size_t i = 7; i < kv.size() && kv[i] >= '0' && kv[i] <= '9' && len < (uint64_t(1) << 60); i++) len = len * 10 + uint64_t(kv[i] - '0'); }
        at = e + 1;
    }
    if (id.empty() || std::find(v->contigs.begin(), v->contigs.end(), id) != v->contigs.end()) return;
    v->contigs.push_back(id); v->contig_len.push_back(len);
}

// The head of the file: BGZF blocks from offset 0 until the #CHROM line and the first record are complete. The errors of
// lcty_vcf_open, with its texts.
void load_head(lcty_vcf_indexed* v) {
    const char* path = v->file.path.c_str();
    BgzfSerial in(v->file.fd, v->file.fsize, path);
    std::vector<uint8_t> t;
    uint64_t b = 0, searched = 0;                    // the first line not looked at yet; no '\n' in [b, searched)
    bool have_header = false, have_record = false, eof = false;
    while (!have_record && !eof) {
        eof = !in.append_block(t);
        while (!have_record) {
            uint64_t e = std::max(b, searched);
            while (e < t.size() && t[e] != '\n') e++;
            searched = e;
            if (e == t.size() && (!eof || b >= t.size())) break;           // the line is not complete yet; at the end a last line without '\n' is one
            uint64_t le = e;
            if (le > b && t[le - 1] == '\r') le--;
            if (le > b) {
                if (t[b] == '#') {
                    if (le - b >= 6 && !memcmp(&t[b], "#CHROM", 6)) { vcfidx::parse_chrom_line(t.data(), b, le, path, v->samples); have_header = true; }
                    else if (le - b >= 10 && !memcmp(&t[b], "##contig=<", 10)) note_contig(v, std::string(reinterpret_cast<const char*>(&t[b + 10]), le - b - 10));
                } else {
                    if (!have_header) vcfidx::fail_record_before_header(path);
                    const vcfidx::LineHead h = vcfidx::parse_line_head(t.data(), b, le, path);
                    const uint32_t S = static_cast<uint32_t>(v->samples.size());
                    v->ploidy.assign(S, 0);
                    if (S) vcfidx::first_record_ploidy(t.data(), b, le, h.chrom + ":" + std::to_string(uint64_t(h.pos) + 1), S, v->ploidy);
                    have_record = true;
                }
            }
            b = e + 1; searched = b;
        }
    }
    if (!have_header) vcfidx::fail_no_header(path);
    if (!have_record) vcfidx::fail_no_records();
    for (const std::string& name : v->tbi.names)
        if (std::find(v->contigs.begin(), v->contigs.end(), name) == v->contigs.end()) { v->contigs.push_back(name); v->contig_len.push_back(0); }
    for (const std::string& name : v->contigs) { v->contig_blob += name; v->contig_blob.push_back('\0'); }
    const uint32_t S = static_cast<uint32_t>(v->samples.size());
    v->hap_off.assign(S + 1, 0);
    for (uint32_t i = 0; i < S; i++) { v->hap_off[i + 1] = v->hap_off[i] + v->ploidy[i]; v->sample_blob += v->samples[i]; v->sample_blob.push_back('\0'); }
    v->view.n_samples = S; v->view.n_haps = v->hap_off[S]; v->view.n_records = 0;            // the file is not walked
    v->view.samples = v->sample_blob.data(); v->view.samples_len = v->sample_blob.size();
    v->view.ploidy = v->ploidy.data(); v->view.hap_off = v->hap_off.data();
}

}  // namespace

extern "C" {

int32_t lcty_vcf_indexed_open(const char* path, const char* index_path, lcty_vcf_indexed** out) {
    return guarded([&] {
        if (!path || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *out = nullptr;
        const std::string p(path);
        if (has_suffix(p, ".bcf")) fail(LCTY_ERR_UNSUPPORTED, "%s: BCF is not read here, convert it to a text VCF", path);
        std::unique_ptr<lcty_vcf_indexed> v(new lcty_vcf_indexed());
        // ---- the index
        if (index_path) v->index_path = index_path;
        else if (is_regular_file(p + ".tbi")) v->index_path = p + ".tbi";
        else if (is_regular_file(p + ".csi")) fail(LCTY_ERR_UNSUPPORTED, "%s.csi is a CSI index (only tabix indices are read)", path);
        else fail(LCTY_ERR_INVALID_INPUT, "no index for %s (%s.tbi)", path, path);
        if (has_suffix(v->index_path, ".csi")) fail(LCTY_ERR_UNSUPPORTED, "%s is a CSI index (only tabix indices are read)", v->index_path.c_str());
        if (!is_regular_file(v->index_path)) fail(LCTY_ERR_INVALID_INPUT, "no index for %s (%s)", path, v->index_path.c_str());
        // ---- the file
        v->file.open(path);
        uint8_t hd[64];
        const size_t n = static_cast<size_t>(std::min<uint64_t>(sizeof(hd), v->file.fsize));
        if (n) pread_all(v->file.fd, hd, n, 0, path);
        if (!bgzf_block_size(hd, n)) fail(LCTY_ERR_INVALID_INPUT, "%s: an indexed file must be BGZF (bgzip); this one is plain text or plain gzip", path);
        load_tbi(v.get());
        load_head(v.get());
        *out = v.release();
    });
}

int32_t lcty_vcf_indexed_contigs(const lcty_vcf_indexed* vcf, lcty_vcf_contigs* out) {
    return guarded([&] {
        if (!vcf || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        out->n_contigs = static_cast<uint32_t>(vcf->contigs.size()); out->_pad0 = 0;
        out->names = vcf->contig_blob.data(); out->names_len = vcf->contig_blob.size(); out->length = vcf->contig_len.data();
    });
}

int32_t lcty_vcf_indexed_view_get(const lcty_vcf_indexed* vcf, lcty_vcf_view* view) {
    return guarded([&] {
        if (!vcf || !view) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *view = vcf->view;
    });
}

void lcty_vcf_indexed_close(lcty_vcf_indexed* vcf) { delete vcf; }

int32_t lcty_vcf_indexed_plan(lcty_vcf_indexed* vcf, const char* contig, uint32_t start, uint32_t end, uint64_t chunk_cap, uint64_t* n_chunks,
                              uint64_t* chunk_beg, uint64_t* chunk_end, uint64_t* blocks_total) {
    return guarded([&] {
        if (!vcf || !contig || !n_chunks || (chunk_cap && (!chunk_beg || !chunk_end))) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        report_plan(vcf->file, vcfidx::plan(vcf->tbi, contig, start, end), chunk_cap, n_chunks, chunk_beg, chunk_end, blocks_total);
    });
}

int32_t lcty_vcf_indexed_fetch(lcty_ctx* ctx, lcty_vcf_indexed* vcf, const char* contig, uint32_t start, uint32_t end, const uint8_t* sample_used,
                               lcty_vcf_records* out, lcty_vcf_fetch_stats* stats) {
    if (out) memset(out, 0, sizeof(*out));
    if (stats) memset(stats, 0, sizeof(*stats));
    return guarded([&] {
        if (!ctx) {
            if (lcty_device_count() == 0) fail(LCTY_ERR_RUNTIME, "no HIP device is visible: liblocityper_hip has no CPU fallback");
            fail(LCTY_ERR_INVALID_INPUT, "null argument");
        }
        if (!vcf || !contig || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const double t_start = now_ms();
        const char* path = vcf->file.path.c_str();
        const uint32_t S = vcf->view.n_samples, Hn = vcf->view.n_haps;
        lcty_vcf_fetch_stats T{};
        T.file_bytes = vcf->file.fsize;
        lcty_vcf_records o{}; Handoff h;
        o.n_haps = Hn; o.n_samples = S;
        auto finish = [&]() {
            T.ms_total = now_ms() - t_start;
            if (stats) *stats = T;
            *out = o; h.commit();
        };
        auto empty = [&]() {
            const uint32_t zero32 = 0; const uint64_t zero64 = 0;
            o.pos = h.copy(&zero32, 0); o.ref_len = h.copy(&zero32, 0); o.rec_allele = h.copy(&zero32, 1);
            o.allele_off = h.copy(&zero64, 1); o.allele_bytes = h.copy(static_cast<const uint8_t*>(nullptr), 0);
            o.gt = h.copy(static_cast<const int16_t*>(nullptr), 0); o.phased = h.copy(static_cast<const uint8_t*>(nullptr), 0);
            finish();
        };

        // ---- the chunks of the window, their bytes, their blocks
        Slice F;
        SliceStats fs{};
        F.read(ctx, vcf->file, vcfidx::plan(vcf->tbi, contig, start, end), "vcf_max_slice_bytes", fs);
        fs.put(T);
        const uint64_t total = F.total;
        std::vector<uint64_t> rbeg, rend;
        for (const ChunkSpan& sp : F.spans) if (sp.chain_beg < sp.chain_end) { rbeg.push_back(sp.chain_beg); rend.push_back(sp.chain_end); }
        if (rbeg.empty()) { empty(); return; }                                 // nothing of the window's own: nothing is inflated

        T.ms_inflate = F.inflate(ctx, path);
        hipStream_t s = ctx->stream;

        // ---- upload
        double t0 = now_ms();
        const uint32_t n_ranges = static_cast<uint32_t>(rbeg.size()), contig_len = static_cast<uint32_t>(strlen(contig));
        DevBuf<uint64_t> d_rng; DevBuf<uint8_t> d_contig, d_used; DevBuf<uint32_t> d_ploidy, d_hap_off; ErrWord err;
        const uint8_t* d_raw = F.device(s);
        std::vector<uint64_t> rng(rbeg);
        rng.insert(rng.end(), rend.begin(), rend.end());
        d_rng.alloc(rng.size()); d_rng.upload(rng.data(), rng.size(), s);
        d_contig.alloc(std::max<uint32_t>(contig_len, 1)); d_contig.upload(reinterpret_cast<const uint8_t*>(contig), contig_len, s);
        if (S) {
            d_ploidy.alloc(S); d_ploidy.upload(vcf->ploidy.data(), S, s);
            d_hap_off.alloc(S + 1); d_hap_off.upload(vcf->hap_off.data(), S + 1, s);
            if (sample_used) { d_used.alloc(S); d_used.upload(sample_used, S, s); }
        }
        unsigned long long* d_err = err.reset(s);
        LCTY_HIP(hipStreamSynchronize(s));
        T.ms_upload = now_ms() - t0;

        // ---- the lines
        t0 = now_ms();
        const Ranges R{d_rng.p, d_rng.p + n_ranges, n_ranges};
        const uint64_t n_wg = (total + LINE_BYTES * LINE_THREADS - 1) / (LINE_BYTES * LINE_THREADS);
        DevBuf<uint32_t> d_cnt, d_cnt_off;
        d_cnt.alloc(n_wg);
        hipLaunchKernelGGL(line_kernel<false>, dim3(static_cast<uint32_t>(n_wg)), dim3(LINE_THREADS), 0, s, d_raw, total, R, d_cnt.p, nullptr, nullptr);
        LCTY_HIP(hipGetLastError());
        ScanTotal scan;
        const uint32_t n_lines = scan.run(d_cnt, d_cnt_off, n_wg, ctx);           // 2^31 - 16 lines or more: LCTY_ERR_UNSUPPORTED
        T.lines_walked = n_lines;
        if (n_lines == 0) { T.ms_lines = now_ms() - t0; empty(); return; }
        DevBuf<uint64_t> d_line;
        d_line.alloc(n_lines);
        hipLaunchKernelGGL(line_kernel<true>, dim3(static_cast<uint32_t>(n_wg)), dim3(LINE_THREADS), 0, s, d_raw, total, R, nullptr, d_cnt_off.p, d_line.p);
        LCTY_HIP(hipGetLastError());
        LCTY_HIP(hipStreamSynchronize(s));
        T.ms_lines = now_ms() - t0;

        // ---- the heads, the records
        t0 = now_ms();
        DevBuf<uint32_t> d_kept, d_kept_off;
        DevBuf<LineInfo> d_info;
        d_kept.alloc(n_lines); d_info.alloc(n_lines);
        HeadView HV{};
        HV.raw = d_raw; HV.R = R; HV.line_start = d_line.p; HV.n_lines = n_lines; HV.contig = d_contig.p; HV.contig_len = contig_len;
        HV.start = start; HV.end = end; HV.S = S; HV.kept = d_kept.p; HV.info = d_info.p; HV.err = d_err;
        hipLaunchKernelGGL(head_kernel, dim3(n_lines), dim3(WAVE), 0, s, HV);
        LCTY_HIP(hipGetLastError());
        const uint32_t n_recs = scan.run(d_kept, d_kept_off, n_lines, ctx);
        T.records_kept = n_recs;
        DevBuf<LineInfo> d_rec; DevBuf<uint32_t> d_rec_line, d_pos, d_rlen, d_nall, d_nbytes;
        const uint32_t n1 = std::max(n_recs, 1u);
        d_rec.alloc(n1); d_rec_line.alloc(n1); d_pos.alloc(n1); d_rlen.alloc(n1); d_nall.alloc(n1); d_nbytes.alloc(n1);
        if (n_recs) {
            hipLaunchKernelGGL(compact_kernel, dim3(blocks_of(n_lines, 256)), dim3(256), 0, s, n_lines, d_kept.p, d_kept_off.p, d_info.p, d_rec.p, d_rec_line.p,
                               d_pos.p, d_rlen.p, d_nall.p, d_nbytes.p);
            LCTY_HIP(hipGetLastError());
        }
        LCTY_HIP(hipStreamSynchronize(s));
        T.ms_heads = now_ms() - t0;

        // ---- the allele pool
        t0 = now_ms();
        DevBuf<uint32_t> d_rec_allele; DevBuf<uint64_t> d_byte_off, d_allele_off; DevBuf<uint8_t> d_pool;
        uint64_t n_alleles = 0, pool_len = 0;
        if (n_recs) {
            n_alleles = scan.run(d_nall, d_rec_allele, n_recs, ctx);
            d_byte_off.alloc(static_cast<size_t>(n_recs) + 1);
            launch_scan(s, n_recs, LoadU32AsU64{d_nbytes.p}, AddOp{}, uint64_t(0), d_byte_off.p, true);
            d_byte_off.download(&pool_len, 1, s, n_recs);
            LCTY_HIP(hipStreamSynchronize(s));
            d_allele_off.alloc(n_alleles + 1); d_pool.alloc(std::max<uint64_t>(pool_len, 1));
            hipLaunchKernelGGL(allele_kernel, dim3(n_recs), dim3(WAVE), 0, s, d_raw, n_recs, d_rec.p, d_rec_allele.p, d_byte_off.p, d_allele_off.p, d_pool.p);
            LCTY_HIP(hipGetLastError());
            LCTY_HIP(hipStreamSynchronize(s));
        }
        T.ms_alleles = now_ms() - t0;

        // ---- the genotype matrix
        t0 = now_ms();
        DevBuf<int16_t> d_gt; DevBuf<uint8_t> d_phased;
        const size_t n_gt = static_cast<size_t>(n_recs) * Hn, n_ph = static_cast<size_t>(n_recs) * S;
        if (n_recs && S) {
            d_gt.alloc(std::max<size_t>(n_gt, 1)); d_phased.alloc(n_ph);
            GtView GV{};
            GV.raw = d_raw; GV.rec = d_rec.p; GV.rec_line = d_rec_line.p; GV.S = S; GV.n_haps = Hn;
            GV.ploidy = d_ploidy.p; GV.hap_off = d_hap_off.p; GV.sample_used = sample_used ? d_used.p : nullptr;
            GV.gt = d_gt.p; GV.phased = d_phased.p; GV.err = d_err;
            hipLaunchKernelGGL(gt_kernel, dim3(n_recs), dim3(WAVE), 0, s, GV);
            LCTY_HIP(hipGetLastError());
        }
        uint64_t l; uint32_t cls;
        const bool refused = err.take(s, l, cls);
        T.ms_gt = now_ms() - t0;

        // ---- the first offending line in file order, through the line functions of the host reader
        if (refused) {
            uint64_t b = 0;
            d_line.download(&b, 1, s, l);
            LCTY_HIP(hipStreamSynchronize(s));
            uint64_t range_end = total;
            for (uint32_t r = 0; r < n_ranges; r++) if (rbeg[r] <= b && b < rend[r]) range_end = rend[r];
            uint64_t le = b;
            while (le < range_end && F.slice[le] != '\n') le++;
            if (le > b && F.slice[le - 1] == '\r') le--;
            if (cls == E_LONG) fail(LCTY_ERR_UNSUPPORTED, "%s: a line of 2^32 bytes or more", path);
            const vcfidx::LineHead lh = vcfidx::parse_line_head(F.slice, b, le, path);
            vcfidx::RecordArrays A; std::vector<int32_t> al;
            if (lh.chrom == contig) vcfidx::parse_record_line(F.slice, b, le, contig, lh.pos, lh.ref_len, S, vcf->ploidy.data(), vcf->samples, sample_used, A, al);
            fail(LCTY_ERR_RUNTIME, "%s: the device refused line %llu of the fetched slice, the host reader takes it", path, static_cast<unsigned long long>(l));
        }
        if (n_recs == 0) { empty(); return; }

        // ---- download
        t0 = now_ms();
        o.n_recs = n_recs; o.n_alleles = n_alleles; o.pool_len = pool_len;
        o.pos = from(h, d_pos, n_recs, s); o.ref_len = from(h, d_rlen, n_recs, s); o.rec_allele = from(h, d_rec_allele, static_cast<size_t>(n_recs) + 1, s);
        o.allele_off = from(h, d_allele_off, n_alleles + 1, s); o.allele_bytes = from(h, d_pool, pool_len, s);
        o.gt = from(h, d_gt, S ? n_gt : 0, s); o.phased = from(h, d_phased, S ? n_ph : 0, s);
        LCTY_HIP(hipStreamSynchronize(s));
        T.ms_download = now_ms() - t0;
        finish();
    });
}

}  // extern "C"
