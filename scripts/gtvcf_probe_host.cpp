// gtvcf_probe_host.cpp — the host half of a cohort's genotypes as a VCF (locityper_amd/csrc/lcty_gtvcf_host.hpp: the column of a predicted
// allele, fixed-point numbers as text and back, the table of predictions, the header, the tabix writer; no HIP) over a corpus, stand-alone on the CPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/gtvcf_probe_host.cpp
//       -o gtvcf_probe_host && ./gtvcf_probe_host corpus.tsv
// The corpus is written by tests/gtvcf_cases.py (write_corpus), one case per line, tab-separated, answers from tests/pyref_gtvcf.py:
//   view    name:ploidy ...                        the samples of the variants file for the `column` lines that follow
//   column  genome allele status column            lcty_gtvcf_columns' rule for one allele (an empty allele is written as `-`)
//   print   value decimals pad text                the fixed-point printer
//   parse   text decimals status value             the fixed-point parser (an empty text is written as `-`)
// Every text runs from a heap copy of exactly its bytes, so that a read outside it is the sanitizer's to see. After the corpus the tabix
// writer runs over generated records, sorted and not, and every index it writes is parsed back by the reader's parser
// (lcty_bgzf_index.hpp) and asked for every record. It exits 1 when an answer differs from what the corpus says.
// With -DGTVCF_PROBE_SERIAL the file also holds gtvcf_probe_serial, the one-thread twin that scripts/gtvcf_probe.py measures the device against.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "lcty_bgzf_index.hpp"
#include "lcty_gtvcf_host.hpp"

namespace lcty { void set_last_error(const std::string&) {} }

using namespace lcty;
using namespace lcty::gtvcf;

static std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    size_t a = 0;
    for (size_t i = 0; i <= s.size(); i++) if (i == s.size() || s[i] == sep) { out.push_back(s.substr(a, i - a)); a = i + 1; }
    return out;
}
static std::string exact(const std::string& s) {                         // a copy whose buffer ends with the text
    char* p = static_cast<char*>(malloc(s.size() ? s.size() : 1));
    memcpy(p, s.data(), s.size());
    std::string out(p, s.size());
    free(p);
    return out;
}

static uint64_t tbi_round(uint64_t seed, uint32_t n_contigs, uint32_t n_records, bool sorted, uint64_t* wrong) {
    auto next = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return seed >> 33; };
    std::vector<std::string> contigs;
    for (uint32_t c = 0; c < n_contigs; c++) contigs.push_back("chr" + std::to_string(c + 1));
    std::vector<uint32_t> tid(n_records), pos(n_records), rlen(n_records);
    std::vector<uint64_t> line_off(size_t(n_records) + 1);
    uint32_t t = 0, p = 0;
    uint64_t u = 100 + next() % 70000;
    for (uint32_t i = 0; i < n_records; i++) {
        if (n_contigs > 1 && next() % 7 == 0 && t + 1 < n_contigs) { t++; p = 0; }
        p += uint32_t(next() % (next() % 5 == 0 ? 3000000 : 300));
        if (p > (1u << 29) - 70001) p = (1u << 29) - 70001;
        tid[i] = t; pos[i] = p; rlen[i] = uint32_t(next() % 4 == 0 ? next() % 70000 : next() % 3);
        line_off[i] = u; u += 20 + next() % (next() % 9 == 0 ? 200000 : 500);
    }
    line_off[n_records] = u;
    if (!sorted && n_records > 2) std::swap(pos[n_records / 2], pos[n_records / 2 - 1]);
    const uint64_t n_blocks = (u + BGZF_CUT - 1) / BGZF_CUT;
    std::vector<uint64_t> block_off(n_blocks + 1);
    for (uint64_t b = 0, at = 0; b <= n_blocks; b++) { block_off[b] = at; at += 28 + next() % 60000; }
    uint64_t found = 0;
    try {
        const std::string plain = tbi_plain(contigs, n_records, tid.data(), pos.data(), rlen.data(), line_off.data(), block_off.data(), n_blocks);
        std::vector<uint8_t> bytes(plain.begin(), plain.end());
        const vcfidx::Tbi T = vcfidx::parse_tbi(bytes.data(), bytes.size(), "probe.tbi");
        if (T.names != contigs) { (*wrong)++; fprintf(stderr, "tbi: the names differ\n"); }
        for (uint32_t i = 0; i < n_records; i++) {
            const uint64_t v = block_off[line_off[i] / BGZF_CUT] << 16 | line_off[i] % BGZF_CUT;
            bool hit = false;
            for (const Chunk& c : vcfidx::plan(T, contigs[tid[i]].c_str(), pos[i], pos[i] + 1)) hit |= c.beg <= v && v < c.end;
            if (!hit) { (*wrong)++; fprintf(stderr, "tbi: record %u at %u is in no chunk of its window\n", i, pos[i]); }
            found += hit;
        }
        if (!sorted && n_records > 2 && pos[n_records / 2] != pos[n_records / 2 - 1] && tid[n_records / 2] == tid[n_records / 2 - 1]) {
            (*wrong)++; fprintf(stderr, "tbi: unsorted records were taken\n");
        }
    } catch (const Error& e) {
        if (sorted || e.code != LCTY_ERR_INVALID_INPUT) { (*wrong)++; fprintf(stderr, "tbi: status %d (%s)\n", e.code, e.what()); }
    }
    return found;
}

#ifdef GTVCF_PROBE_SERIAL
// ---- the serial twin of scripts/gtvcf_probe.py: lcty_gtvcf_add_locus for every locus and lcty_gtvcf_merge as plain loops in ONE host thread, the
// execution model of extra/into_vcf.py (g++ -O3 -shared -fPIC -DGTVCF_PROBE_SERIAL ... -lz). Stage by stage as the device's stats name them;
// deflate is zlib at level 6 over blocks of 0xff00 bytes, what lcty_io_write_bgzf does. The texts must equal the device's byte for byte.
#include <zlib.h>

#include <chrono>

namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct SerialLocus { const lcty_gtvcf_locus_in* in; uint32_t n_slots; std::vector<int16_t> calls; std::vector<std::string> suffix; };
struct Src { uint32_t l, r; };

uint32_t digits_of(int32_t v) { return v < 0 ? 1u : dec_digits(uint64_t(v)); }

uint64_t field_len(const SerialLocus& L, uint32_t r, uint32_t s) {
    const uint32_t p0 = L.in->pred_off[s], p1 = L.in->pred_off[s + 1];
    if (p0 == p1) return 2;
    uint64_t w = 1 + (p1 - p0 - 1) + L.suffix[s].size();
    for (uint32_t k = p0; k < p1; k++) w += digits_of(L.calls[size_t(r) * L.n_slots + k]);
    return w;
}
char* field_put(char* c, const SerialLocus& L, uint32_t r, uint32_t s) {
    const uint32_t p0 = L.in->pred_off[s], p1 = L.in->pred_off[s + 1];
    *c++ = '\t';
    if (p0 == p1) { *c++ = '.'; return c; }
    for (uint32_t k = p0; k < p1; k++) {
        if (k > p0) *c++ = '|';
        const int32_t v = L.calls[size_t(r) * L.n_slots + k];
        if (v < 0) *c++ = '.';
        else { const uint32_t d = dec_digits(uint64_t(v)); uint64_t x = uint64_t(v); for (uint32_t i = d; i-- > 0;) { c[i] = char('0' + x % 10); x /= 10; } c += d; }
    }
    memcpy(c, L.suffix[s].data(), L.suffix[s].size());
    return c + L.suffix[s].size();
}
// the line of record `own`, sample s shown from choice[s] (null: the record itself)
uint64_t line_len(const std::vector<SerialLocus>& loci, Src own, const Src* choice, uint32_t n_samples, size_t tail_len) {
    const lcty_gtvcf_locus_in& I = *loci[own.l].in;
    const uint32_t a0 = I.rec_allele[own.r], na = I.rec_allele[own.r + 1] - a0;
    uint64_t len = strlen(I.chrom) + 1 + dec_digits(uint64_t(I.pos[own.r]) + 1) + 1 + 1 + 1 + (I.allele_off[a0 + 1] - I.allele_off[a0]) + (na == 1 ? 2 : 0) + tail_len + 1;
    for (uint32_t a = 1; a < na; a++) len += 1 + (I.allele_off[a0 + a + 1] - I.allele_off[a0 + a]);
    for (uint32_t s = 0; s < n_samples; s++) { const Src f = choice ? choice[s] : own; len += field_len(loci[f.l], f.r, s); }
    return len;
}
char* line_put(char* c, const std::vector<SerialLocus>& loci, Src own, const Src* choice, uint32_t n_samples, const std::string& tail) {
    const lcty_gtvcf_locus_in& I = *loci[own.l].in;
    const size_t cl = strlen(I.chrom);
    memcpy(c, I.chrom, cl); c += cl;
    *c++ = '\t';
    const uint64_t pos = uint64_t(I.pos[own.r]) + 1;
    const uint32_t pd = dec_digits(pos);
    { uint64_t x = pos; for (uint32_t i = pd; i-- > 0;) { c[i] = char('0' + x % 10); x /= 10; } c += pd; }
    *c++ = '\t'; *c++ = '.';
    const uint32_t a0 = I.rec_allele[own.r], na = I.rec_allele[own.r + 1] - a0;
    for (uint32_t a = 0; a < na; a++) {
        *c++ = a <= 1 ? '\t' : ',';
        const uint64_t n = I.allele_off[a0 + a + 1] - I.allele_off[a0 + a];
        memcpy(c, I.allele_bytes + I.allele_off[a0 + a], n); c += n;
    }
    if (na == 1) { *c++ = '\t'; *c++ = '.'; }
    memcpy(c, tail.data(), tail.size()); c += tail.size();
    for (uint32_t s = 0; s < n_samples; s++) { const Src f = choice ? choice[s] : own; c = field_put(c, loci[f.l], f.r, s); }
    *c++ = '\n';
    return c;
}
int64_t floor_units(int64_t tenths) { return tenths == LCTY_GTVCF_ABSENT ? tenths : tenths >= 0 ? tenths / 10 : -((-tenths + 9) / 10); }

uint32_t crc_seen = 0;
uint64_t deflate_blocks(const std::string& text) {
    uint64_t total = 28;
    std::vector<uint8_t> out(compressBound(0xff00) + 64);
    for (size_t at = 0; at < text.size(); at += 0xff00) {
        const size_t n = std::min<size_t>(0xff00, text.size() - at);
        z_stream zs{};
        deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        zs.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(text.data() + at)); zs.avail_in = uInt(n);
        zs.next_out = out.data(); zs.avail_out = uInt(out.size());
        deflate(&zs, Z_FINISH);
        crc_seen ^= uint32_t(crc32(0, reinterpret_cast<const Bytef*>(text.data() + at), uInt(n)));     // the trailer of a BGZF block
        total += 26 + zs.total_out;
        deflateEnd(&zs);
    }
    return total;
}

}  // namespace

// ms[5]: cells, widths, write, merge, deflate. texts: the loci's files back to back (text_len[n_loci] each), then the merged one (*merged_len).
extern "C" int gtvcf_probe_serial(uint32_t n_loci, const lcty_gtvcf_locus_in* in, uint32_t n_samples, const char* samples_blob, uint32_t mask, double* ms,
                                  char** texts, uint64_t* text_len, uint64_t* merged_len, uint64_t* n_joined, uint64_t* deflated_bytes) {
    try {
        const std::vector<std::string> samples = split_names(samples_blob, n_samples);
        const std::string tail = "\t.\t.\t.\t" + format_key(mask);
        std::vector<SerialLocus> loci(n_loci);
        std::vector<std::string> files(size_t(n_loci) + 1);
        for (int k = 0; k < 5; k++) ms[k] = 0;
        *deflated_bytes = 0;
        for (uint32_t l = 0; l < n_loci; l++) {
            SerialLocus& L = loci[l];
            const lcty_gtvcf_locus_in& I = in[l];
            L.in = &I; L.n_slots = I.pred_off[n_samples];
            double t = now_ms();
            L.calls.resize(size_t(I.n_recs) * L.n_slots);                 // cells: copy_genotype, record by record, sample by sample
            for (uint32_t r = 0; r < I.n_recs; r++)
                for (uint32_t k = 0; k < L.n_slots; k++) {
                    const uint32_t col = I.pred_col[k];
                    const int32_t v = col == LCTY_GTVCF_REF ? 0 : I.gt[size_t(r) * I.n_haps + col];
                    L.calls[size_t(r) * L.n_slots + k] = int16_t(v < 0 ? -1 : v);
                }
            ms[0] += now_ms() - t; t = now_ms();
            L.suffix.assign(n_samples, std::string());                   // widths: the feature text of every sample, the length of every line
            const int64_t* const num[4] = {I.qual10, I.reads, I.unexpl, I.wdist5};
            for (uint32_t s = 0; s < n_samples; s++) {
                if (I.pred_off[s] == I.pred_off[s + 1]) continue;
                std::string& x = L.suffix[s];
                for (uint32_t f = 0; f < 4; f++) if (mask >> f & 1) { x += ':'; x += fixed_text(num[f] ? num[f][s] : LCTY_GTVCF_ABSENT, f == 0 ? QUAL_DECIMALS : f == 3 ? WDIST_DECIMALS : 0, false); }
                if (mask >> 4 & 1) { x += ':'; const uint64_t w0 = I.warn_off ? I.warn_off[s] : 0, w1 = I.warn_off ? I.warn_off[s + 1] : 0; if (w0 == w1) x += '.'; else x.append(I.warn + w0, w1 - w0); }
            }
            const uint64_t len0 = I.contig_len;
            const std::string header = header_text({I.chrom}, &len0, samples);
            std::vector<uint64_t> off(size_t(I.n_recs) + 1, header.size());
            for (uint32_t r = 0; r < I.n_recs; r++) off[r + 1] = off[r] + line_len(loci, Src{l, r}, nullptr, n_samples, tail.size());
            ms[1] += now_ms() - t; t = now_ms();
            std::string& text = files[l];                                // write
            text.resize(off[I.n_recs]);
            memcpy(&text[0], header.data(), header.size());
            for (uint32_t r = 0; r < I.n_recs; r++) line_put(&text[off[r]], loci, Src{l, r}, nullptr, n_samples, tail);
            ms[2] += now_ms() - t; t = now_ms();
            *deflated_bytes += deflate_blocks(text);
            ms[4] += now_ms() - t;
        }
        // ---- merge_vcfs: the loci by (contig, start, end), the records by (contig, pos, alleles), the join per sample
        double t = now_ms();
        std::vector<uint32_t> by(n_loci);
        for (uint32_t l = 0; l < n_loci; l++) by[l] = l;
        std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) {
            return in[a].contig_ix != in[b].contig_ix ? in[a].contig_ix < in[b].contig_ix : in[a].start != in[b].start ? in[a].start < in[b].start : in[a].end < in[b].end; });
        std::vector<Src> recs;
        std::vector<std::string> contigs; std::vector<uint64_t> lens;
        for (uint32_t k = 0; k < n_loci; k++) {
            const uint32_t l = by[k];
            if (k == 0 || in[l].contig_ix != in[by[k - 1]].contig_ix) { contigs.push_back(in[l].chrom); lens.push_back(in[l].contig_len); }
            for (uint32_t r = 0; r < in[l].n_recs; r++) recs.push_back(Src{l, r});
        }
        auto alleles_cmp = [&](const Src& a, const Src& b) {
            const lcty_gtvcf_locus_in& A = in[a.l]; const lcty_gtvcf_locus_in& B = in[b.l];
            const uint32_t ra = A.rec_allele[a.r], na = A.rec_allele[a.r + 1] - ra, rb = B.rec_allele[b.r], nb = B.rec_allele[b.r + 1] - rb;
            for (uint32_t e = 0; e < na && e < nb; e++) {
                const uint64_t la = A.allele_off[ra + e + 1] - A.allele_off[ra + e], lb = B.allele_off[rb + e + 1] - B.allele_off[rb + e];
                const int c = memcmp(A.allele_bytes + A.allele_off[ra + e], B.allele_bytes + B.allele_off[rb + e], std::min(la, lb));
                if (c) return c;
                if (la != lb) return la < lb ? -1 : 1;
            }
            return na == nb ? 0 : na < nb ? -1 : 1;
        };
        auto key_cmp = [&](const Src& a, const Src& b) {
            if (in[a.l].contig_ix != in[b.l].contig_ix) return in[a.l].contig_ix < in[b.l].contig_ix ? -1 : 1;
            if (in[a.l].pos[a.r] != in[b.l].pos[b.r]) return in[a.l].pos[a.r] < in[b.l].pos[b.r] ? -1 : 1;
            return alleles_cmp(a, b);
        };
        std::stable_sort(recs.begin(), recs.end(), [&](const Src& a, const Src& b) { return key_cmp(a, b) < 0; });
        std::vector<Src> line_own; std::vector<Src> choice;
        for (size_t i = 0; i < recs.size();) {
            size_t j = i + 1;
            while (j < recs.size() && key_cmp(recs[i], recs[j]) == 0) j++;
            line_own.push_back(recs[i]);
            for (uint32_t s = 0; s < n_samples; s++) {
                Src cur = recs[i];
                for (size_t m = i + 1; m < j; m++) {
                    const Src nxt = recs[m];
                    const SerialLocus& A = loci[cur.l]; const SerialLocus& B = loci[nxt.l];
                    const uint32_t a0 = A.in->pred_off[s], an = A.in->pred_off[s + 1] - a0, b0 = B.in->pred_off[s], bn = B.in->pred_off[s + 1] - b0;
                    if (!bn) continue;
                    bool take = an == 0;
                    if (!take) {
                        bool differ = an != bn;
                        for (uint32_t k = 0; k < an && !differ; k++) differ = A.calls[size_t(cur.r) * A.n_slots + a0 + k] != B.calls[size_t(nxt.r) * B.n_slots + b0 + k];
                        take = differ && floor_units(B.in->qual10 ? B.in->qual10[s] : LCTY_GTVCF_ABSENT) > floor_units(A.in->qual10 ? A.in->qual10[s] : LCTY_GTVCF_ABSENT);
                    }
                    if (take) cur = nxt;
                }
                choice.push_back(cur);
            }
            i = j;
        }
        *n_joined = recs.size() - line_own.size();
        ms[3] += now_ms() - t; t = now_ms();
        const std::string header = header_text(contigs, lens.data(), samples);
        std::vector<uint64_t> off(line_own.size() + 1, header.size());
        for (size_t r = 0; r < line_own.size(); r++) off[r + 1] = off[r] + line_len(loci, line_own[r], &choice[r * n_samples], n_samples, tail.size());
        ms[1] += now_ms() - t; t = now_ms();
        std::string& text = files[n_loci];
        text.resize(off.back());
        memcpy(&text[0], header.data(), header.size());
        for (size_t r = 0; r < line_own.size(); r++) line_put(&text[off[r]], loci, line_own[r], &choice[r * n_samples], n_samples, tail);
        ms[2] += now_ms() - t; t = now_ms();
        *deflated_bytes += deflate_blocks(text);
        ms[4] += now_ms() - t;
        uint64_t total = 0;
        for (const std::string& f : files) total += f.size();
        char* out = static_cast<char*>(malloc(total ? total : 1));
        if (!out) return 2;
        uint64_t at = 0;
        for (uint32_t l = 0; l <= n_loci; l++) { memcpy(out + at, files[l].data(), files[l].size()); at += files[l].size(); if (l < n_loci) text_len[l] = files[l].size(); }
        *merged_len = files[n_loci].size();
        *texts = out;
        return 0;
    } catch (const std::exception& e) { fprintf(stderr, "gtvcf_probe_serial: %s\n", e.what()); return 1; }
}
extern "C" void gtvcf_probe_serial_free(char* p) { free(p); }
#endif

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.tsv\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint64_t cases = 0, refused = 0, wrong = 0;
    std::vector<std::string> names; std::vector<uint32_t> ploidy, hap_off; std::string blob;
    lcty_vcf_view view{}; SampleIndex index;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        const std::vector<std::string> f = split(line, '\t');
        auto text_of = [](const std::string& s) { return exact(s == "-" ? std::string() : s); };
        if (f[0] == "view") {
            names.clear(); ploidy.clear(); hap_off.assign(1, 0); blob.clear();
            for (size_t i = 1; i < f.size(); i++) {
                const size_t c = f[i].rfind(':');
                names.push_back(f[i].substr(0, c)); ploidy.push_back(uint32_t(atoi(f[i].c_str() + c + 1)));
                hap_off.push_back(hap_off.back() + ploidy.back()); blob += names.back(); blob.push_back('\0');
            }
            view.n_samples = uint32_t(names.size()); view.n_haps = hap_off.back(); view.samples = blob.data(); view.samples_len = blob.size();
            view.ploidy = ploidy.data(); view.hap_off = hap_off.data();
            index = sample_index(view);
            continue;
        }
        cases++;
        if (f[0] == "column" && f.size() == 5) {
            uint32_t status = 0, col = 0;
            try { col = resolve_column(view, index, text_of(f[1]), text_of(f[2])); } catch (const Error& e) { status = uint32_t(e.code); refused++; }
            if (status != uint32_t(atoi(f[3].c_str())) || (!status && col != uint32_t(strtoul(f[4].c_str(), nullptr, 10)))) {
                wrong++; fprintf(stderr, "column %s: status %u column %u, corpus says %s %s\n", f[2].c_str(), status, col, f[3].c_str(), f[4].c_str());
            }
        } else if (f[0] == "print" && f.size() == 5) {
            const int64_t v = strtoll(f[1].c_str(), nullptr, 10);
            const uint32_t d = uint32_t(atoi(f[2].c_str())); const bool pad = f[3] == "1";
            const std::string got = exact(fixed_text(v, d, pad));
            if (got != f[4]) { wrong++; fprintf(stderr, "print %s / %u: `%s`, corpus says `%s`\n", f[1].c_str(), d, got.c_str(), f[4].c_str()); }
            else if (got != "." && fixed_parse(got, d) != v) { wrong++; fprintf(stderr, "print %s / %u does not parse back\n", f[1].c_str(), d); }
        } else if (f[0] == "parse" && f.size() == 5) {
            uint32_t status = 0; int64_t v = 0;
            try { v = fixed_parse(text_of(f[1]), uint32_t(atoi(f[2].c_str()))); } catch (const Error& e) { status = uint32_t(e.code); refused++; }
            if (status != uint32_t(atoi(f[3].c_str())) || (!status && v != strtoll(f[4].c_str(), nullptr, 10))) {
                wrong++; fprintf(stderr, "parse `%s`: status %u value %lld, corpus says %s %s\n", f[1].c_str(), status, static_cast<long long>(v), f[3].c_str(), f[4].c_str());
            }
        } else { fprintf(stderr, "case %llu: unknown line `%s`\n", static_cast<unsigned long long>(cases), line.c_str()); return 2; }
    }
    // the header of any number of contigs and samples
    const uint64_t lens[3] = {248956422, 0, 5};
    const std::string h = header_text({"chr1", "chrUn", "c"}, lens, {"a", "b"});
    if (h.find("##contig=<ID=chrUn>\n") == std::string::npos || h.find("##contig=<ID=c,length=5>\n") == std::string::npos || h.substr(h.size() - 12) != "\tFORMAT\ta\tb\n") {
        wrong++; fprintf(stderr, "header text\n");
    }
    if (format_key(LCTY_GTVCF_UPSTREAM) != "GT:reads:unexpl:wdist" || format_key(0) != "GT") { wrong++; fprintf(stderr, "FORMAT key\n"); }
    // the table of into_csv.py: written from rows of every state, parsed back from a buffer that ends with the text, also cut short at every
    // byte (a truncated table is refused or gives fewer rows, never a read outside it)
    {
        char gt[] = "HG002.2,chm13", warn[] = "FewReads(9000)", star[] = "*";
        lcty_res_summary rows[4] = {};
        rows[0] = lcty_res_summary{gt, warn, 273, 9000, 17, 123, LCTY_RES_CALLED, 0};
        rows[1].state = LCTY_RES_NO_GENOTYPE; rows[2].state = LCTY_RES_MISSING;
        rows[3] = lcty_res_summary{gt, star, LCTY_GTVCF_ABSENT, LCTY_GTVCF_ABSENT, 0, -5, LCTY_RES_CALLED, 0};
        const char* const sample[4] = {"s2", "s10", "s1", "S9"};
        const char* const locus[4] = {"A", "A", "B", "B"};
        const std::string table = predictions_csv_text(4, sample, locus, rows);
        const PredictionTable T = predictions_csv_parse(exact(table), "probe.csv");
        if (T.rows.size() != 4 || T.samples != std::vector<std::string>({"S9", "s1", "s10", "s2"}) || T.rows[0].qual10 != 273 || T.rows[0].wdist5 != 123 ||
            T.rows[0].warnings != warn || T.rows[1].genotype != "*" || T.rows[2].genotype != "?" || T.rows[2].reads != LCTY_GTVCF_ABSENT ||
            T.rows[3].qual10 != LCTY_GTVCF_ABSENT || T.rows[3].unexpl != 0 || T.rows[3].wdist5 != -5) { wrong++; fprintf(stderr, "table round trip\n"); }
        for (size_t cut = 0; cut < table.size(); cut++) {
            try { if (predictions_csv_parse(exact(table.substr(0, cut)), "probe.csv").rows.size() > 4) wrong++; } catch (const Error&) { refused++; }
        }
    }
    uint64_t found = 0;
    for (uint64_t round = 0; round < 24; round++)
        found += tbi_round(round * 7919 + 1, 1 + uint32_t(round % 4), uint32_t(round % 6 == 0 ? round / 6 : 40 * round), round % 5 != 4, &wrong);
    printf("{\"cases\": %llu, \"refused\": %llu, \"wrong\": %llu, \"tbi_records_found\": %llu}\n", static_cast<unsigned long long>(cases),
           static_cast<unsigned long long>(refused), static_cast<unsigned long long>(wrong), static_cast<unsigned long long>(found));
    return wrong ? 1 : 0;
}
