"""Designed haplotype sets for the tests of the pairwise haplotype alignments (TEST INFRASTRUCTURE; tests/test_align_host.py checks that
they are fit for purpose, tests/test_gpu_align.py and tests/test_gpu_align_limits.py run them on the device).

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
    return next(c for c in cases() + limit_cases() if c.name == name)


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


# ---- what the device tests of the alignments share (tests/test_gpu_align.py, tests/test_gpu_align_limits.py) -----------------------------------
_bb = {}


def backbone_run(ctx, name, ref, query, k, hash_bits=None):
    """(result, statistics) of lcty_align_backbone of one task of a named case, once per session"""
    from locityper_amd import api
    key = (name, ref, query, k, hash_bits)
    if key not in _bb:
        c = by_name(name)
        seqs, off = c.arrays()
        if hash_bits is not None:
            ctx.set_knob("align_hash_bits", hash_bits)
        try:
            _bb[key] = api.align_backbone(ctx, seqs, off, ref, query, k, api.align_params(max_gap=c.max_gap))
        finally:
            if hash_bits is not None:
                ctx.set_knob("align_hash_bits", -1)
    return _bb[key]


def backbone(ctx, name, ref, query, k, hash_bits=None):
    return backbone_run(ctx, name, ref, query, k, hash_bits)[0]


def check_cigar(items, score, ref, query, optimum=None):
    """the properties every alignment has"""
    ref, query = R.norm(ref), R.norm(query)
    i = j = 0
    for x, (op, ln) in enumerate(items):
        assert ln > 0 and op in "=XID"
        assert x == 0 or items[x - 1][0] != op, "adjacent equal operations"
        if op == "=":
            assert ref[i:i + ln] == query[j:j + ln]
        if op == "X":
            assert all(a != b for a, b in zip(ref[i:i + ln], query[j:j + ln]))
        i += ln if op in "=XD" else 0
        j += ln if op in "=XI" else 0
    assert (i, j) == (len(ref), len(query)), "the CIGAR does not consume both sequences"
    assert score == R.calculate_score(items)
    if optimum is not None:
        assert score <= optimum


def check_stage_a(ctx, name, ref, query, k):
    want = np.array(reference(name, ref, query, k)[0], dtype=np.uint32).reshape(-1, 2)
    assert np.array_equal(backbone(ctx, name, ref, query, k)["matches"], want)
    # eight bits of hash: every bucket is full of collisions, the comparison of the bases has to reject them
    assert np.array_equal(backbone(ctx, name, ref, query, k, hash_bits=8)["matches"], want)


def check_stage_b(ctx, name, ref, query, k):
    matches, score, _ = reference(name, ref, query, k)
    got = backbone(ctx, name, ref, query, k)
    assert got["chain_score"] == score
    path = got["path"].tolist()
    assert all(0 <= x < len(matches) for x in path) and (len(path) > 0) == (len(matches) > 0)
    total = k if path else 0
    for a, b in zip(path, path[1:]):
        assert a < b, "the path is not strictly ordered"
        (i1, j1), (i2, j2) = matches[a], matches[b]
        diagonal = (i2, j2) == (i1 + 1, j1 + 1)
        assert diagonal or (i1 + k <= i2 and j1 + k <= j2), "a step is neither a diagonal + 1 nor clears k in both coordinates"
        # a diagonal neighbour that also clears k cannot exist (k >= 5), so the step's worth is unambiguous
        total += 1 if diagonal else k
    assert total == score, "the path does not add up to the chain score"


def check_stage_c(ctx, name, ref, query, k, optimum_of=None):
    """the gap fill along the DEVICE's path, CIGAR word for word; optimum_of(name, ref, query) bounds the score from above"""
    c = by_name(name)
    matches = reference(name, ref, query, k)[0]
    got = backbone(ctx, name, ref, query, k)
    cig, score = R.align_from_path(c.seqs[ref], c.seqs[query], matches, got["path"].tolist(), k, c.max_gap)
    assert np.array_equal(got["cigar"], R.words(R.normalize(cig)))
    assert got["score"] == score and got["n_dropped"] == 0
    check_cigar(R.items_of(got["cigar"]), got["score"], c.seqs[ref], c.seqs[query], (optimum_of or optimum)(name, ref, query))


# ---- designed sets for the limits of the device aligner (tests/test_gpu_align_limits.py) ----------------------------------------------------
# The block builder: a pair is F + R + G against F + Q + G with random flanks of FLANK bases and k = 25. Q is R with the base rotated
# (A -> C -> G -> T -> A) at every position = phase (mod 17) — 17 < k, so R and Q share no 25-mer — and cut at its end to m bases.
# The first and the last base of Q are then made to differ from the first and the last base of R, so neither flank's run of matches
# reaches into the block: the pair is the anchor F, ONE stretch of exactly len(R) x len(Q), the anchor G.
K, FLANK, PERIOD = 25, 60, 17


def rotated(c):
    return B[(B.index(c) + 1) % 4]


def rotate_at_phase(seq, phase):
    out = bytearray(seq)
    for p in range(phase % PERIOD, len(out), PERIOD):
        out[p] = rotated(out[p])
    return out


def _make_differ(q, p, avoid):
    while q[p] in avoid:
        q[p] = rotated(q[p])


def block(rng, n, m, phase=0):
    """(R, Q) of n >= m >= 1 bases"""
    r = rand_seq(rng, n)
    q = rotate_at_phase(r, phase)[:m]
    _make_differ(q, 0, {r[0]} | ({r[-1]} if m == 1 else set()))
    _make_differ(q, m - 1, {r[-1]} | ({r[0]} if m == 1 else set()))
    return r, bytes(q)


# (name, bases of the longer side (haplotype 0), of the shorter (haplotype 1), pairs as (reference, query), max_gap,
#  expected n_level of one task, expected n_dropped). The shape in the name is reference x query of the first pair.
LEVEL_SHAPES = [
    ("255x255", 255, 255, [(0, 1), (1, 0)], 10000, [1, 0, 0], 0),            # level 0 with dim and cells (256 * 256 = 2^16) at their limit
    ("255x256", 256, 255, [(1, 0), (0, 1)], 10000, [0, 1, 0], 0),            # dim refuses
    ("256x40", 256, 40, [(0, 1), (1, 0)], 10000, [0, 1, 0], 0),
    ("2047x2047", 2047, 2047, [(0, 1)], 10000, [0, 1, 0], 0),                # level 1 at both limits: 2^22 cells in one lane
    ("2048x30", 2048, 30, [(0, 1), (1, 0)], 10000, [0, 0, 1], 0),            # dim refuses
    ("2047x2048", 2048, 2047, [(1, 0)], 10000, [0, 0, 1], 0),                # cells refuse (2048 * 2049 > 2^22)
    ("16383x5", 16383, 5, [(0, 1), (1, 0)], 20000, [0, 0, 1], 0),            # the largest side
    ("16384x5", 16384, 5, [(0, 1), (1, 0)], 20000, [1, 0, 0], 1),            # beyond it: dropped to align_simple, no scratch level
]
# the optimal penalty of these is a gap of about 16 000 columns: beyond the step limit of the oracle's aligner (pyref_align.UnfitCase)
BEYOND_ORACLE = ("16383x5",)


def _level_case(x, name, n, m, pairs, max_gap):
    rng = np.random.default_rng(100 + x)
    f, g = rand_seq(rng, FLANK), rand_seq(rng, FLANK)
    r, q = block(rng, n, m, phase=x)
    c = Case("lv_" + name, [f + r + g, f + q + g], [K], False, pairs=pairs, max_gap=max_gap)
    c.stretch = {(0, 1): (n, m), (1, 0): (m, n)}
    c.middles = (r, q)
    return c


# Two middles agree up to the first rotated position (min(h1, h2) bases) and, by chance, in their last few bases; both join the flank
# anchors. The first seed from 201 on with which every pair's stretch keeps a side of at least 256 bases (tests/test_align_host.py
# checks it): with 201 and 202 a pair falls to 254 x 255, level 0.
REUSE1_SEED = 203


def _reuse1(seed=REUSE1_SEED):
    """17 haplotypes with common flanks; middle h is one random R rotated at phase h and cut to 256 + h bases. Two middles differ at
    two positions of every 17, so no pair has a 25-mer off the flanks' diagonals; every pair is one stretch whose longer side has at
    least 256 bases: 136 tasks of level 1, more than its 128 lanes, with many row widths."""
    rng = np.random.default_rng(seed)
    f, g, r = rand_seq(rng, FLANK), rand_seq(rng, FLANK), rand_seq(rng, 256 + 16)
    return Case("reuse1", [f + bytes(rotate_at_phase(r, h)[:256 + h]) + g for h in range(17)], [K], False)


def _reuse2():
    """one haplotype with a middle of 2 048 bases, twelve with unrelated middles of 8 to 19: twelve tasks of level 2 (eight lanes)"""
    rng = np.random.default_rng(202)
    f, g, big = rand_seq(rng, FLANK), rand_seq(rng, FLANK), rand_seq(rng, 2048)
    seqs = [f + big + g]
    for t in range(12):
        mid = bytearray(rand_seq(rng, 8 + t))
        _make_differ(mid, 0, {big[0]}); _make_differ(mid, len(mid) - 1, {big[-1]})
        seqs.append(f + bytes(mid) + g)
    return Case("reuse2", seqs, [K], False, pairs=[(0, i) for i in range(1, 13)] + [(i, 0) for i in range(1, 13)])


TIGHT_MAX_GAP = 8


def _tight_bound():
    """Pairs whose CIGAR has as many items as PlanVisitor's bound allows, the start of 2 aside. Anchors of exactly k bases (one
    25-mer each: the bases on either side differ, or are N) separate stretches that fill their bound:
      straight (3 x 3, bound n): X=X; and =X= with N against N as the '=' (a window with an N is no k-mer, in the fill N equals N)
      align_simple (max_gap = 8; bound min(n, m) + 1): 9 x 12 and 12 x 9, the common part alternating mismatch and match: 1 + 9 items
      a plain gap (bound 1).
    Pair (0, 1) has no two equal operations next to each other, so its item count IS the sum of the bounds plus the anchors. Pair
    (2, 3) holds the =X= stretches: each joins the anchors on both sides (two items fewer per stretch, as designed)."""
    rng = np.random.default_rng(203)

    def anchor():
        return rand_seq(rng, K)

    def build(kinds):
        ref, qry = bytearray(anchor()), None
        qry = bytearray(ref)
        for kind in kinds:
            nxt = anchor()
            if kind == "X=X":
                a = rand_seq(rng, 3)
                b = bytes([rotated(a[0]), a[1], rotated(a[2])])
            elif kind == "=X=":
                x = rand_seq(rng, 1)
                a, b = b"N" + x + b"N", b"N" + bytes([rotated(x[0])]) + b"N"
            elif kind in ("9x12", "12x9"):
                short = rand_seq(rng, 9)
                extra = bytearray(rand_seq(rng, 3))
                _make_differ(extra, 0, {short[0]})
                long_ = bytes(extra) + bytes(rotated(c) if t % 2 == 0 else c for t, c in enumerate(short))
                a, b = (short, long_) if kind == "9x12" else (long_, short)
            elif kind in ("D", "I"):
                gap = _insert_seq(rng, 5 if kind == "D" else 7, ref[-1], nxt[0])
                a, b = (gap, b"") if kind == "D" else (b"", gap)
            ref += a + nxt; qry += b + nxt
        return bytes(ref), bytes(qry)
    plain = ["X=X", "9x12", "D", "12x9", "X=X", "I", "9x12", "X=X", "12x9", "D", "I", "9x12", "I", "12x9", "D"]
    joined = ["=X=", "X=X", "=X=", "9x12", "D", "=X="]
    c = Case("tight_bound", list(build(plain)) + list(build(joined)), [K], False, pairs=[(0, 1), (1, 0), (2, 3), (3, 2)], max_gap=TIGHT_MAX_GAP)
    c.kinds = {(0, 1): plain, (1, 0): plain, (2, 3): joined, (3, 2): joined}
    return c


def plan_bound(seq1, seq2, matches, path, k, max_gap):
    """(anchors, [(route, n, m, bound of the stretch's items)]) of the walk of align_from_backbone: what PlanVisitor (lcty_align.hip)
    adds up, from the routing rules of gotoh::route as pyref_align.smart_align states them (wfa.rs:280-321); the exact aligner's n + m
    is for a stretch the largest scratch level takes, min(n, m) + 1 the one of align_simple."""
    stretches, anchors, i1, j1, curr = [], 0, 0, 0, 0

    def stretch(n, m):
        if n > 0 and m > 0:
            if max_gap < n or max_gap < m: return ("simple", n, m, min(n, m) + 1)
            if n == m and n <= R.SAFE_MISMATCH: return ("straight", n, m, n)
            if n > R.DP_DIM or m > R.DP_DIM or (n + 1) * (m + 1) > R.DP_CELLS: return ("dropped", n, m, min(n, m) + 1)
            return ("exact", n, m, n + m)
        return ("gap", n, m, 1) if n or m else ("none", 0, 0, 0)
    for ix in path:
        i2, j2 = matches[ix]
        if i1 > i2:
            curr += 1; i1 += 1; j1 += 1
            continue
        if curr > 0:
            anchors += 1; curr = 0
        stretches.append(stretch(i2 - i1, j2 - j1))
        curr += k; i1 = i2 + k; j1 = j2 + k
    if curr > 0:
        anchors += 1
    stretches.append(stretch(len(seq1) - i1, len(seq2) - j1))
    return anchors, [s for s in stretches if s[0] != "none"]


def tight_bound_items(r, q):
    """(items of the transliteration's CIGAR, the count the design gives): the anchors plus the sum of the stretches' bounds, less the
    two joins of every =X= stretch with its anchors"""
    c = by_name("tight_bound")
    matches, _, path = reference("tight_bound", r, q, K)
    anchors, stretches = plan_bound(c.seqs[r], c.seqs[q], matches, path, K, c.max_gap)
    cig, _ = R.align_from_path(c.seqs[r], c.seqs[q], matches, path, K, c.max_gap)
    return R.normalize(cig), anchors + sum(s[3] for s in stretches) - 2 * c.kinds[(r, q)].count("=X=")


LOW_KS = [5, 7]


def _lowcomplexity():
    """homopolymer, dinucleotide and trinucleotide repeats: buckets of hundreds of equal k-mers, about 11 000 matches, ties everywhere"""
    rng = np.random.default_rng(204)
    left, right = rand_seq(rng, 150), rand_seq(rng, 150)
    seqs = [b"A" * 120, b"A" * 100, b"AC" * 80, b"AC" * 70, left + b"CAG" * 40 + right, left + b"CAG" * 33 + right]
    return Case("lowcomplexity", seqs, LOW_KS, False, pairs=[(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4)])


LENGTHS = [0, 1, 24, 25, 26, 255, 256, 257, 511, 512, 513, 1024]


def _lengths():
    """prefixes of one random sequence around k and around the 256 threads of align_prefix_kernel (chunk = ceil(L / 256)), each with
    one substitution at a third of its length where it has three bases; haplotype 0 is the whole sequence"""
    rng = np.random.default_rng(205)
    base = rand_seq(rng, 1024)
    seqs = [base]
    for ln in LENGTHS:
        s = bytearray(base[:ln])
        if ln >= 3:
            s[ln // 3] = rotated(s[ln // 3])
        seqs.append(bytes(s))
    return Case("lengths", seqs, [K], False, pairs=[p for i in range(1, len(LENGTHS) + 1) for p in ((0, i), (i, 0))])


# ---- the random differential run: the only set here that is not designed; it stays last --------------------------------------------------------
RANDOM_KS = [5, 11, 25]
N_RANDOM = 48


def _random_pair(seed):
    """(reference, query): 60 to 400 bases; the query is the reference after substitutions and indels of 1 to 30 bases, a run of N, a
    lower-case stretch and an inserted short tandem repeat, in random order at random places"""
    rng = np.random.default_rng(1000 + seed)
    ref = rand_seq(rng, int(rng.integers(60, 401)))
    q = bytearray(ref)
    events = ["sub"] * int(rng.integers(1, 6)) + ["ins"] * int(rng.integers(0, 3)) + ["del"] * int(rng.integers(0, 3)) + ["n", "lower", "str"]
    for ev in [events[i] for i in rng.permutation(len(events))]:
        p = int(rng.integers(0, len(q) + 1))
        ln = int(rng.integers(1, 31))
        if ev == "sub" and len(q):
            p = min(p, len(q) - 1); q[p] = other_base(q[p], rng) if q[p] in B else B[0]
        elif ev == "ins":
            q[p:p] = rand_seq(rng, ln)
        elif ev == "del":
            del q[p:p + ln]
        elif ev == "n":
            q[p:p + min(ln, 12)] = b"N" * len(q[p:p + min(ln, 12)])
        elif ev == "lower":
            q[p:p + ln] = bytes(q[p:p + ln]).lower()
        elif ev == "str":
            unit = rand_seq(rng, int(rng.integers(1, 5)))
            q[p:p] = unit * int(rng.integers(3, 11))
    return ref, bytes(q)


def _random_cases():
    out = []
    for k in RANDOM_KS:
        seeds = [s for s in range(N_RANDOM) if RANDOM_KS[s % 3] == k]
        seqs = [x for s in seeds for x in _random_pair(s)]
        out.append(Case(f"random_k{k}", seqs, [k], False, pairs=[(2 * t, 2 * t + 1) for t in range(len(seeds))]))
    return out


@functools.lru_cache(maxsize=None)
def limit_cases():
    return [_level_case(x, *sh[:5]) for x, sh in enumerate(LEVEL_SHAPES)] + [_reuse1(), _reuse2(), _tight_bound(), _lowcomplexity(), _lengths()] + _random_cases()
