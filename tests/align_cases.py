"""Designed haplotype sets for the tests of the pairwise haplotype alignments (TEST INFRASTRUCTURE; tests/test_align_host.py checks that
they are fit for purpose, tests/test_gpu_align.py runs them on the device).

"Unique chain" cases: a random sequence plus sparse edits on a common grid at least 2 k apart for the largest k of the case, so every
pair differs by isolated edits; an indel never has a second placement (its first base differs from the base behind it, its last base
from the base in front of it). Then every k-mer match lies on the true diagonal, all of them chain, and the optimal alignment is
unique — the transliteration's answer is the full-DP optimum and any optimal path gives the same CIGAR."""
import functools

import numpy as np

from tests import pyref_align as R

B = b"ACGT"


def rand_seq(rng, n):
    return bytes(B[i] for i in rng.integers(0, 4, n))


def other_base(c, rng):
    return [x for x in B if x != c][int(rng.integers(0, 3))]


def _insert_seq(rng, n, before, after):
    """n random bases whose last differs from `before` (the base in front) and whose first differs from `after` (the base behind)"""
    while True:
        s = bytearray(rand_seq(rng, n))
        if s[-1] != before and s[0] != after:
            return bytes(s)


def apply_edits(base, edits):
    """edits: [(pos, kind, arg)] ascending; 'X' arg = new base; 'I' arg = bytes inserted in front of pos; 'D' arg = bases removed from pos"""
    out, at = bytearray(), 0
    for pos, kind, arg in edits:
        out += base[at:pos]; at = pos
        if kind == "X":
            out.append(arg); at = pos + 1
        elif kind == "I":
            out += arg
        else:
            at = pos + arg
    out += base[at:]
    return bytes(out)


class Case:
    def __init__(self, name, seqs, ks, unique, pairs=None, max_gap=10000, dp_cells=None):
        self.name, self.seqs, self.ks, self.unique, self.max_gap, self.dp_cells = name, [bytes(s) for s in seqs], list(ks), unique, max_gap, dp_cells
        n = len(self.seqs)
        self.pairs = pairs if pairs is not None else [(i, j) for i in range(n) for j in range(i + 1, n)]
        # a set holds at least four haplotypes: variants of haplotype 0 fill it up; they take part in the divergences and the index
        # of every call, the pairs stay the designed ones
        fill = np.random.default_rng(len(name) + 7 * n)
        while len(self.seqs) < 4:
            s0 = self.seqs[0]
            pos = sorted(set(int(x) for x in fill.integers(0, len(s0), 5)))
            self.seqs.append(apply_edits(s0, [(p, "X", other_base(s0[p], fill)) for p in pos]))
        self.names = [f"{name}_h{i}" for i in range(len(self.seqs))]

    def arrays(self):
        seqs = np.frombuffer(b"".join(self.seqs), dtype=np.uint8).copy()
        off = np.zeros(len(self.seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in self.seqs], out=off[1:])
        return seqs, off


def _grid_case(name, seed, length, ks, step, maker, n_haps=4):
    """haplotype 0 is the base; haplotype h > 0 carries the edit maker(rng, base, pos, h) at a random half of the grid positions"""
    rng = np.random.default_rng(seed)
    base = rand_seq(rng, length)
    grid = list(range(step, length - step, step))
    seqs = [base]
    for h in range(1, n_haps):
        take = [p for p in grid if rng.integers(0, 2)] or grid[:1]
        seqs.append(apply_edits(base, [maker(rng, base, p, h) for p in take]))
    return Case(name, seqs, ks, True)


def _sub(rng, base, p, h):
    return (p, "X", B[(B.index(base[p]) + 1) % 4])           # the same substitute in every haplotype: two carriers agree there


def _indel(rng, base, p, h):
    if h % 2:
        n = int(rng.integers(1, 61))
        return (p, "I", _insert_seq(rng, n, base[p - 1], base[p]))
    n = int(rng.integers(1, 61))
    while base[p + n - 1] == base[p - 1] or base[p] == base[p + n]:          # the removed bases must not slide either
        n += 1
    return (p, "D", n)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    out.append(_grid_case("subs", 11, 1500, [25, 51, 101], 210, _sub))
    out.append(_grid_case("indels", 12, 1800, [25, 51], 240, _indel, n_haps=3))
    # every pair of "indels" differs by isolated indels only when at most one of the two carries an edit at a grid position with
    # another content: haplotypes 1 (insertions) and 2 (deletions) may both edit a position — then the pair sees a replacement
    out[-1].pairs = [(0, 1), (0, 2), (1, 0), (2, 0)]
    rng = np.random.default_rng(13)
    base = rand_seq(rng, 700)
    ends = [base,
            apply_edits(base, [(0, "X", other_base(base[0], rng))]),                                   # an edit at position 0
            apply_edits(base, [(len(base) - 1, "X", other_base(base[-1], rng))]),                      # ... and at the last base
            bytes(base),                                                                               # identical: L=
            base[:-37],                                                                                # differs only in length
            apply_edits(base, [(9, "X", other_base(base[9], rng)), (688, "X", other_base(base[688], rng))])]   # inside the first / last k
    out.append(Case("ends", ends, [25, 33], True, pairs=[(0, 1), (0, 2), (0, 3), (0, 4), (4, 0), (0, 5), (1, 2)]))
    rng = np.random.default_rng(14)
    small = rand_seq(rng, 300)
    out.append(Case("k5", [small, apply_edits(small, [(100, "X", other_base(small[100], rng)), (200, "D", 7)])], [5], False))
    # hard cases
    rng = np.random.default_rng(15)
    unit, left, right = rand_seq(rng, 40), rand_seq(rng, 200), rand_seq(rng, 200)
    out.append(Case("tandem", [left + unit * 20 + right, left + unit * 19 + right, left + unit * 20 + right[:150]], [25, 33], False,
                    pairs=[(0, 1), (1, 0), (0, 2)]))
    rng = np.random.default_rng(16)
    out.append(Case("unrelated", [rand_seq(rng, 600), rand_seq(rng, 640)], [25], False))
    rng = np.random.default_rng(17)
    long_one = rand_seq(rng, 400)
    out.append(Case("short", [long_one, long_one[180:200]], [25], False, pairs=[(0, 1), (1, 0)]))
    rng = np.random.default_rng(18)
    base = rand_seq(rng, 900)
    with_n = base[:400] + b"N" * 30 + base[430:]
    out.append(Case("nrun", [base, with_n, with_n[:600] + rand_seq(rng, 5) + with_n[600:]], [25, 51], False))
    rng = np.random.default_rng(19)
    base = rand_seq(rng, 1200)
    ins = apply_edits(base, [(500, "I", _insert_seq(rng, 300, base[499], base[500]))])                # a plain I: one side is empty
    repl = base[:700] + rand_seq(rng, 300) + base[750:]                                               # 50 against 300: align_simple
    out.append(Case("maxgap", [base, ins, repl], [25, 51], False, max_gap=200))
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name, ref, query, k):
    """the transliteration on one pair and one k: (matches, chain score, path)"""
    c = by_name(name)
    m = R.kmer_matches(c.seqs[ref], c.seqs[query], k)
    score, path = R.lcskpp(m, k)
    return m, score, path


@functools.lru_cache(maxsize=None)
def reference_multik(name, ref, query):
    """(normalized items, score, best k) of align_multik on one pair"""
    c = by_name(name)
    best = None
    for k in c.ks:
        m, _, path = reference(name, ref, query, k)
        cig, score = R.align_from_path(c.seqs[ref], c.seqs[query], m, path, k, c.max_gap)
        if best is None or score > best[1]:
            best = (R.normalize(cig), score, k)
    return best


@functools.lru_cache(maxsize=None)
def optimum(name, ref, query):
    c = by_name(name)
    return R.full_dp_score(c.seqs[ref], c.seqs[query])


# ---- stretches whose optimal alignment is not unique: where the aligner's tie rule decides (lcty_gotoh.hpp) --------------------------------
# (name, reference, query, max_gap, more than one optimal alignment). Every sequence is shorter than k = 25, so a pair is one stretch
# of smart_align; tests/test_align_host.py checks the last column against an enumeration and runs the host instantiation,
# tests/test_gpu_align.py the device. Each stretch is also run with reference and query exchanged.
TIE_CASES = [
    ("homopolymer", b"A" * 9, b"A" * 6, 10000, True),                         # where does the gap go
    ("dinucleotide", b"AC" * 6, b"AC" * 5, 10000, True),
    ("sub_next_to_indel", b"TTGCAACGTCAT", b"TTGCAGGTCAT", 10000, True),      # AC against G: X then gap, or gap then X
    ("sub_next_to_indel_in_a_run", b"GATCTTTAGC", b"GATCTGGC", 10000, True),  # TTTA against TG
    ("equal_3", b"ACG", b"TGA", 10000, False),                                # at safe_mismatch: base against base, no aligner
    ("equal_4", b"ACGT", b"TGCA", 10000, False),                              # just beyond it: the aligner, four mismatches beat two gaps
    ("empty_reference", b"", b"ACGT", 10000, False),
    ("empty_query", b"ACGT", b"", 10000, False),
    ("beyond_max_gap", b"ACGTTTTAC", b"ACGTTAC", 8, True),                    # align_simple: the gap in front, whatever is optimal
    # at most 7 bases a side: what alignment recovery gives to its in-register aligner (xfer::dp_align_small) in a batch with long CIGARs
    ("homopolymer_short", b"A" * 6, b"A" * 4, 10000, True),
    ("dinucleotide_short", b"AC" * 3, b"AC" * 2, 10000, True),
    ("sub_next_to_indel_short", b"GCAACG", b"GCAGG", 10000, True),
]


def tie_runs():
    """every stretch of TIE_CASES both ways round: (name, reference, query, max_gap)"""
    return [(name + sfx, a, b, mg) for name, r, q, mg, _ in TIE_CASES for sfx, a, b in (("", r, q), ("_swapped", q, r))]


TIE_FLANK = 215


@functools.lru_cache(maxsize=None)
def tie_transfer_case():
    """The stretches of tie_runs() as work for alignment recovery: (two alleles, the CIGAR of allele 0 as query on allele 1, reads).
    Allele 0 is a row of blocks F G of random flanks, allele 1 has the stretch's reference between them (F R G; the haplotype alignment
    says 215= nD 215=). A read is the end of F, the stretch's query and the start of G, reported on allele 0 as f= mI f=. In its
    transfer to allele 1 the flanks anchor and neither CIGAR has an `=` in between, so smart_align gets exactly (R, Q)
    (cigar.rs:1248-1384). Each stretch comes as a read with flanks of 210 — long enough that its m <= 12 edits on allele 0 are within
    3 % of the read, the threshold of tests/helpers.py::make_bg for a well mapped read, so the read stays in use —
    and as one with flanks of 5 (at most 32 bases; no record of it can stay: with the stretch as an insertion among so few bases it is
    poorly mapped and not transferred, and where it is, the result is below MIN_ALN_SIZE = 50). Both alleles begin with 300 and end
    with 700 equal bases (the boundary of the locus; room for a read with a long CIGAR). reads: [(name, start on allele 0, bases, CIGAR)]."""
    rng = np.random.default_rng(47)
    a0, a1, hap, reads = bytearray(), bytearray(), [], []

    def push(op, n):
        if n and hap and hap[-1][0] == op: hap[-1][1] += n
        elif n: hap.append([op, n])
    head = rand_seq(rng, 300)
    a0 += head; a1 += head; push("=", 300)
    for name, r, q, _ in tie_runs():
        f, g = rand_seq(rng, TIE_FLANK), rand_seq(rng, TIE_FLANK)
        at = len(a0)
        a0 += f + g; a1 += f + r + g
        push("=", TIE_FLANK); push("D", len(r)); push("=", TIE_FLANK)
        for tag, fl in (("", 210), ("/32", 5)):
            cg = f"{fl}={len(q)}I{fl}=" if q else f"{2 * fl}="
            reads.append((name + tag, at + TIE_FLANK - fl, f[TIE_FLANK - fl:] + q + g[:fl], cg))
            assert fl == 210 or len(reads[-1][2]) <= 32
    tail = rand_seq(rng, 700)
    a0 += tail; a1 += tail; push("=", 700)
    return (bytes(a0), bytes(a1)), "".join(f"{n}{op}" for op, n in hap), reads
