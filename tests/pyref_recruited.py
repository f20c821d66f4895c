"""The selection and rebasing rule of a resident set of recruited reads (lcty_recruited) in numpy.

A source view is the sequence fields of a chunk: mate_len [2 n], mate_off [2 n + 1] in bases (multiples of 32), bases2 (uint32 words of
sixteen 2-bit codes) and nmask (uint32 words of 32 "not ACGT" bits). One unit is 32 bases: two words of bases2 and one of nmask. The
answers of recruitment are cnt [n] and loci [n, max_out]: pair i goes to exactly loci[i, :cnt[i]].

Rule: within a locus the pairs stand in input order, chunk after chunk and inside a chunk by i. A mate of length L owns ceil(L / 32)
units and is copied unit by unit, padding bits as they were, to consecutive units of the locus; an absent mate (L = 0) takes none.
The ordinal of a pair is its index over every pair of every chunk so far, recruited or not.
"""
import numpy as np

UNIT_BYTES = 12          # a 64-bit word of bases and a 32-bit word of mask
PAIR_BYTES = 32          # two lengths, two offsets, an ordinal


def units_of(length):
    return (int(length) + 31) // 32


def pack_reads(pairs):
    """pairs: list of (seq1, seq2) with str / bytes / None -> (mate_len, mate_off, bases2, nmask) as lcty_fastx_next lays them out."""
    lens, seqs = [], []
    for p in pairs:
        for s in p:
            s = b"" if s is None else (s.encode() if isinstance(s, str) else bytes(s))
            lens.append(len(s)); seqs.append(s)
    mate_len = np.array(lens, dtype=np.uint32)
    mate_off = np.concatenate([[0], np.cumsum((mate_len.astype(np.uint64) + 31) // 32 * 32)]).astype(np.uint64)
    nb = int(mate_off[-1])
    text = np.zeros(nb, dtype=np.uint8)
    valid = np.zeros(nb, dtype=bool)
    for m, s in enumerate(seqs):
        o = int(mate_off[m])
        text[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        valid[o:o + len(s)] = True
    code = np.full(256, 4, dtype=np.uint8)
    for j, c in enumerate(b"ACGT"):
        code[c] = j
    e = code[text]
    two = np.where(e < 4, e, 0).astype(np.uint32).reshape(-1, 16)
    bases2 = (two << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    n_bit = ((e >= 4) & valid).astype(np.uint32).reshape(-1, 32)
    nmask = (n_bit << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return mate_len, mate_off, bases2, nmask


class Expected:
    """what a set over n_loci loci holds after the adds made so far"""

    def __init__(self, n_loci):
        self.n_loci = n_loci
        self.n_seen = 0
        self.loci = [dict(mate_len=[], b2=[], nm=[], ordinal=[]) for _ in range(n_loci)]

    def add(self, view, cnt, loci):
        """view: (mate_len, mate_off, bases2, nmask) or an object with those attributes; cnt [n]; loci [n, max_out]"""
        mate_len, mate_off, bases2, nmask = view if isinstance(view, tuple) else (view.mate_len, view.mate_off, view.bases2, view.nmask)
        n = len(cnt)
        loci = np.asarray(loci).reshape(n, -1) if n else np.zeros((0, 1), dtype=np.uint32)
        for i in range(n):
            for j in range(int(cnt[i])):
                L = self.loci[int(loci[i, j])]
                for e in range(2):
                    ln, u0 = int(mate_len[2 * i + e]), int(mate_off[2 * i + e]) // 32
                    u = units_of(ln)
                    L["mate_len"].append(ln)
                    L["b2"].append(np.asarray(bases2[2 * u0:2 * (u0 + u)], dtype=np.uint32))
                    L["nm"].append(np.asarray(nmask[u0:u0 + u], dtype=np.uint32))
                L["ordinal"].append(self.n_seen + i)
        self.n_seen += n

    def locus(self, l):
        """-> (mate_len, mate_off, bases2, nmask, ordinal) of locus l"""
        L = self.loci[l]
        mate_len = np.array(L["mate_len"], dtype=np.uint32)
        mate_off = np.concatenate([[0], np.cumsum((mate_len.astype(np.uint64) + 31) // 32 * 32)]).astype(np.uint64)
        b2 = np.concatenate(L["b2"]) if L["b2"] else np.zeros(0, dtype=np.uint32)
        nm = np.concatenate(L["nm"]) if L["nm"] else np.zeros(0, dtype=np.uint32)
        return mate_len, mate_off, b2.astype(np.uint32), nm.astype(np.uint32), np.array(L["ordinal"], dtype=np.uint64)

    def bytes(self):
        """the contents knob "recruited_max_bytes" counts"""
        total = 0
        for L in self.loci:
            total += UNIT_BYTES * sum(units_of(x) for x in L["mate_len"]) + PAIR_BYTES * len(L["ordinal"])
        return total
