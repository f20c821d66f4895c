"""The FASTA / FASTQ readers of src/seq/fastx.rs restated in Python, independent of the library: read_line (79-100), Reader::new and
read_next (312-317, 396-415), fill_fasta_record (319-338), fill_fastq_record (340-364), equal_names_fast (102-110),
PairedEndInterleaved::read_next (437-453) and PairedEndReaders::read_next (480-498).

Where fastx.rs cannot tell an empty line from the end of the file (read_line returns 0 for both) this follows the project's host
reader, whose rules lcty_fastx_parse.hpp states: an empty third line of a FASTQ record "has incorrect format" (fastx.rs: "is
incomplete"), an empty line inside a FASTA record adds nothing (fastx.rs: ends the input), and a header that begins with a blank keeps
the rest of the line as its name (fastx.rs: panics). Everything works on bytes; nothing is decoded."""

INVALID_DATA = 2                                       # LCTY_ERR_INVALID_DATA


class FastxError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code, self.msg = code, msg


class Lines:
    """read_line over the bytes of a file: a line without its end ("\\n" or "\\r\\n"); None at the end of the file with nothing read"""

    def __init__(self, data):
        self.data, self.at = data, 0

    def line(self):
        if self.at >= len(self.data):
            return None
        nl = self.data.find(b"\n", self.at)
        if nl < 0:                                     # a last line without "\n": it keeps a trailing "\r"
            out, self.at = self.data[self.at:], len(self.data)
            return out
        out, self.at = self.data[self.at:nl], nl + 1
        return out[:-1] if out.endswith(b"\r") else out


class Reader:
    def __init__(self, data):
        self.lines = Lines(data)
        self.header = self.lines.line() or b""        # Reader::new: the first line

    def next(self):
        """(name, seq, qual or None) or None at the end"""
        h = self.header
        if not h:                                      # "If it is empty, the file has ended"
            return None
        sp = h.find(b" ")
        name = h[1:] if sp <= 0 else h[1:sp]
        if h[:1] == b">":                              # fill_fasta_record
            seq, self.header = b"", b""
            while True:
                l = self.lines.line()
                if l is None:
                    break
                if l[:1] in (b">", b"@"):
                    self.header = l
                    break
                seq += l
            if not seq and not self.header:
                raise FastxError(INVALID_DATA, "Fasta record %s has an empty sequence." % name.decode("latin-1"))
            return name, seq, None
        seq = self.lines.line() or b""                 # fill_fastq_record
        plus = self.lines.line()
        if plus is None:
            raise FastxError(INVALID_DATA, "Fastq record %s is incomplete" % name.decode("latin-1"))
        if plus[:1] != b"+":
            raise FastxError(INVALID_DATA, "Fastq record %s has incorrect format" % name.decode("latin-1"))
        qual = self.lines.line() or b""
        if len(seq) != len(qual):
            raise FastxError(INVALID_DATA, "Fastq record %s has non-matching sequence and qualities" % name.decode("latin-1"))
        self.header = self.lines.line() or b""
        return name, seq, qual


def equal_names_fast(a, b):
    return len(a) == len(b) and (len(a) <= 3 or a[-3] == b[-3])


def read_all(datas, interleaved, what):
    """Every unit (a record, or the two mates of a pair) in front of the first error, and that error or None.
    datas: the bytes of one or two files; what: the file name(s) as the messages give them (two: "a and b")."""
    readers = [Reader(d) for d in datas]
    units, err = [], None
    try:
        while True:
            if len(readers) == 2:
                a, b = readers[0].next(), readers[1].next()
                if a is None and b is None:
                    break
                if a is None or b is None:
                    raise FastxError(INVALID_DATA, "Different number of records in paired-end input files %s" % what)
                if not equal_names_fast(a[0], b[0]):
                    raise FastxError(INVALID_DATA, "Paired-end input files %s have non matching first and second mates (%s and %s)"
                                     % (what, a[0].decode("latin-1"), b[0].decode("latin-1")))
                units.append((a, b))
            elif interleaved:
                a = readers[0].next()
                if a is None:
                    break
                b = readers[0].next()
                if b is None:
                    raise FastxError(INVALID_DATA, "Odd number of records in an interleaved input file(s) %s" % what)
                if not equal_names_fast(a[0], b[0]):
                    raise FastxError(INVALID_DATA, "Interleaved input file(s) %s contains non matching first and second mate (%s and %s)"
                                     % (what, a[0].decode("latin-1"), b[0].decode("latin-1")))
                units.append((a, b))
            else:
                a = readers[0].next()
                if a is None:
                    break
                units.append((a,))
    except FastxError as e:
        err = e
    return units, err


def record_text(rec):
    """write_fastq / write_fasta (fastx.rs:46-75, 262-272): FASTA when there are no qualities"""
    name, seq, qual = rec
    if not qual:
        return b">" + name + b"\n" + seq + b"\n"
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def pack(units, per):
    """pack() of lcty_fastx.hip: mate_len [2 n], mate_off [2 n + 1] (mates at multiples of 32 bases, a single read's second mate absent),
    bases2 (2 bits a base, LSB first, 0 where not ACGT) and nmask (1 bit a base where not ACGT) as lists of 32-bit words"""
    mate_len, mate_off, off = [], [], 0
    for u in units:
        for e in range(2):
            mate_off.append(off)
            ln = len(u[e][1]) if e < per else 0
            mate_len.append(ln)
            off += (ln + 31) // 32 * 32
    mate_off.append(off)
    bases2, nmask = [0] * (off // 16 + 1), [0] * (off // 32 + 1)
    for i, u in enumerate(units):
        for e in range(per):
            o = mate_off[2 * i + e]
            for k, c in enumerate(u[e][1]):
                at = o + k
                code = b"ACGT".find(bytes([c]))
                if code >= 0:
                    bases2[at >> 4] |= code << (2 * (at & 15))
                else:
                    nmask[at >> 5] |= 1 << (at & 31)
    return mate_len, mate_off, bases2, nmask
