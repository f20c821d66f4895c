// lcty_fastx_parse.hpp — the record rules of FASTA / FASTQ text (src/seq/fastx.rs:79-110, 319-415 as Reader::next, read_unit and
// LineReader::line of lcty_fastx.hip / lcty_lines.hpp read them), stated once as functions of a line table, the same text for host and
// device as lcty_inflate.hpp is: the kernels of lcty_fastx_device.hip call them with one thread per line or record, the serial
// executor of scripts/fastx_probe_host.cpp in loops. DESIGN.md 5u.
//   lines     a line ends at '\n'; a '\r' directly before it is not part of the line; a last line without '\n' exists iff it has a byte,
//             and keeps a trailing '\r'. The table is the ascending positions of the '\n' bytes.
//   FASTQ     record r is lines 4r .. 4r+3; name = header bytes 1 up to the first ' '; the first empty header line ends the input.
//   FASTA     a record starts at every line that begins with '>' or '@'; its sequence is the lines up to the next such line.
//   classes   what a record may be refused for, in the order the host reader meets them; the smallest (record, class) of a window decides.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define LCTY_FX_FN __host__ __device__ __forceinline__
#else
#define LCTY_FX_FN inline
#endif

namespace lcty {
namespace fastx {

enum Class : uint32_t {
    C_NONE = 0,
    C_END = 1,            // FASTQ: an empty header line: the input ends here
    C_MIXED = 2,          // a '>' header in a FASTQ stream, an '@' header in a FASTA stream
    C_INCOMPLETE = 3,     // "Fastq record .. is incomplete"
    C_FORMAT = 4,         // "Fastq record .. has incorrect format"
    C_NONMATCH = 5,       // "Fastq record .. has non-matching sequence and qualities"
    C_EMPTY_FASTA = 6,    // "Fasta record .. has an empty sequence."
    C_MISMATCH = 7        // the names of two mates do not match (equal_names_fast); after every class of the record itself
};

// one window of text and its line table. n_lines: the lines the rules may look at: every complete line, and the last one without
// '\n' when the stream has ended (n_lines_of).
struct Text { const uint8_t* t; uint32_t n; const uint32_t* nl; uint32_t n_nl; uint32_t n_lines; };
// name begin, name length, sequence begin (FASTQ) or header line (FASTA), sequence length
struct Row { uint32_t name_beg, name_len, seq, len; };

LCTY_FX_FN uint32_t n_lines_of(uint32_t n, uint32_t n_nl, uint32_t last_nl, bool final) {
    const uint32_t behind = n_nl ? last_nl + 1 : 0;
    return n_nl + ((final && behind < n) ? 1u : 0u);
}

// line j < n_lines: [b, e)
LCTY_FX_FN void line_span(const Text& T, uint32_t j, uint32_t& b, uint32_t& e) {
    b = j ? T.nl[j - 1] + 1 : 0;
    if (j < T.n_nl) { e = T.nl[j]; if (e > b && T.t[e - 1] == '\r') e--; }
    else e = T.n;
}

// the name of the header line [b, e), e > b: bytes 1 up to the first ' ' (a space at byte 0 ends nothing: the reader's
// `assign(header, 1, sp - 1)` then takes the rest of the line)
LCTY_FX_FN void name_span(const Text& T, uint32_t b, uint32_t e, Row& row) {
    uint32_t sp = b;
    while (sp < e && T.t[sp] != ' ') sp++;
    if (sp == b) sp = e;
    row.name_beg = b + 1; row.name_len = sp - (b + 1);
}

// FASTQ record r (4r < n_lines): its row and its class
LCTY_FX_FN uint32_t fastq_record(const Text& T, uint32_t r, Row& row) {
    row.name_beg = 0; row.name_len = 0; row.seq = 0; row.len = 0;
    const uint32_t j = 4 * r;
    uint32_t b, e;
    line_span(T, j, b, e);
    row.name_beg = b + 1;
    if (e == b) return C_END;
    name_span(T, b, e, row);
    if (T.t[b] == '>') return C_MIXED;
    uint32_t sb = e, se = e;                                   // a missing line counts as an empty one
    if (j + 1 < T.n_lines) line_span(T, j + 1, sb, se);
    row.seq = sb; row.len = se - sb;
    if (j + 2 >= T.n_lines) return C_INCOMPLETE;
    uint32_t pb, pe;
    line_span(T, j + 2, pb, pe);
    if (pe == pb || T.t[pb] != '+') return C_FORMAT;
    uint32_t qlen = 0;
    if (j + 3 < T.n_lines) { uint32_t qb, qe; line_span(T, j + 3, qb, qe); qlen = qe - qb; }
    return qlen != row.len ? C_NONMATCH : C_NONE;
}
// where the qualities of a FASTQ record without a class begin: behind the '\n' of its third line
LCTY_FX_FN uint32_t fastq_qual_begin(const uint8_t* t, const Row& row) {
    uint32_t p = row.seq + row.len;
    while (t[p] != '\n') p++;                                  // the end of the sequence line ("\n" or "\r\n")
    p++;
    while (t[p] != '\n') p++;                                  // the '+' line
    return p + 1;
}

// FASTA, per line: is it a header, and how many bases does it add to its record
LCTY_FX_FN void fasta_line(const Text& T, uint32_t j, uint32_t& is_header, uint32_t& bases) {
    uint32_t b, e;
    line_span(T, j, b, e);
    is_header = (e > b && (T.t[b] == '>' || T.t[b] == '@')) ? 1u : 0u;
    bases = is_header ? 0u : e - b;
}
// FASTA record r of n_hdr: hdr_line[r] its header line, cum[j] the bases of the lines before line j (headers add none)
LCTY_FX_FN uint32_t fasta_record(const Text& T, uint32_t r, const uint32_t* hdr_line, const uint32_t* cum, uint32_t n_hdr, bool final, Row& row) {
    const uint32_t h = hdr_line[r], next = r + 1 < n_hdr ? hdr_line[r + 1] : T.n_lines;
    uint32_t b, e;
    line_span(T, h, b, e);
    name_span(T, b, e, row);
    row.seq = h; row.len = cum[next] - cum[h];
    if (T.t[b] == '@') return C_MIXED;
    return (row.len == 0 && final && r + 1 == n_hdr) ? C_EMPTY_FASTA : C_NONE;
}
// base k of FASTA record `row` (k < row.len): found in the lines behind its header
LCTY_FX_FN uint32_t fasta_line_of(const uint32_t* cum, const Row& row, uint32_t n_lines, uint32_t k) {
    const uint32_t want = cum[row.seq] + k;                    // the last line j > row.seq with cum[j] <= want
    uint32_t lo = row.seq + 1, hi = n_lines;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (cum[mid] <= want) lo = mid; else hi = mid; }
    return lo;
}

// equal_names_fast (fastx.rs:102-110): the same length and, beyond three bytes, the same third byte from the end
LCTY_FX_FN bool equal_names_fast(const uint8_t* ta, const Row& a, const uint8_t* tb, const Row& b) {
    return a.name_len == b.name_len && (a.name_len <= 3 || ta[a.name_beg + a.name_len - 3] == tb[b.name_beg + b.name_len - 3]);
}

}  // namespace fastx
}  // namespace lcty
