"""Designed read pairs for the hand-offs between the scoring kernels of a counted batch (lcty_score.hip): the lean kernel, its
two-slot form and the general kernel. Every pair names the route it must take and why, and the facts that make it so (saved
alignments per (read end, contig) group, bins, ties, mate lengths). tests/test_score_route_cases.py holds those facts against
tests/pyref.py on the CPU and derives the route from them; tests/test_gpu_score_routes.py holds the kernels against the routes,
against each other and against the oracle.

The route rule, restated here from the kernels' own rules (never read back from the library):
  - a locus with k >= 32, a record batch or the knob "score_lean" 0: the general kernel takes every pair;
  - a mate of more than 2 016 bases: general;
  - a pair whose first primary is not saved is never looked at: lean, whatever its records hold;
  - a saved alignment is a mapped record on a contig of the locus whose edit distance is at most `passable` of its read end;
  - every (read end, contig) group holds at most one: lean;
  - the two-slot form runs at 309 alleles and fewer (n * 33 + 16 <= 10 240 bytes of LDS), with the knobs "score_lean_keep" and
    "score_lean_two" on; it takes a pair whose groups hold at most two, with at most 64 second alignments in the pair;
  - everything else: general.
"""
import functools

import numpy as np

from locityper_amd import cdefs
from tests import pyref
from tests.helpers import make_bg, random_alleles

LEAN, TWO, GENERAL = 0, 1, 2                  # cdefs.ROUTE_*, restated
LEAN_OVF = 64                                 # second alignments a pair of the two-slot form can hold
REGS_MAX_LEN = 2016                           # the longest mate of the register path of the k-mer windows
KEEP_MAX_ALLELES = 309                        # n * 33 + 16 <= 10 240
TRIP = 256                                    # records per trip of pass 1
M2, REV, SEC = cdefs.FLAG_MATE2, cdefs.FLAG_REVERSE, cdefs.FLAG_SECONDARY
RL, INS = 150, 450                            # read length and insert size of the ordinary pairs
MATE_LENGTHS = (20, 31, 32, 33, 63, 64, 65, 1985, 2015, 2016, 2017)


def keep_runs(n_alleles):
    return n_alleles * 33 + 16 <= 10240


def two_runs(n_alleles, knobs=()):
    return keep_runs(n_alleles) and "score_lean_keep" not in knobs and "score_lean_two" not in knobs


def route_from_facts(facts, n_alleles, k, knobs=(), counted=True):
    """The kernel that takes a pair, from what pyref finds in it (walk) and the knobs set to 0."""
    if not counted or k >= 32 or "score_lean" in knobs:
        return GENERAL
    if max(facts["len"]) > REGS_MAX_LEN:
        return GENERAL
    sizes = [len(g) for g in facts["groups"].values()] if facts["look"] else []
    if all(n <= 1 for n in sizes):
        return LEAN
    if two_runs(n_alleles, knobs) and max(sizes) == 2 and sum(n - 1 for n in sizes) <= LEAN_OVF:
        return TWO
    return GENERAL


def lean_form(n_alleles, k, knobs=(), counted=True):
    if not counted or k >= 32 or "score_lean" in knobs:
        return cdefs.LEAN_FORM_NONE
    return cdefs.LEAN_FORM_KEEP if keep_runs(n_alleles) and "score_lean_keep" not in knobs else cdefs.LEAN_FORM_INDEX


# ---- what pyref sees in a pair ----

class _LazyCompl:
    """complexity_counts of the contigs that are asked for (a primary's contig), not of 310 alleles"""
    def __init__(self, alleles, ck, neighb):
        self.alleles, self.ck, self.neighb, self.done = alleles, ck, neighb, {}

    def __getitem__(self, c):
        if c not in self.done:
            self.done[c] = pyref.complexity_counts(self.alleles[c], self.ck, self.neighb)
        return self.done[c]


class WalkLocus(pyref.PyLocus):
    """The part of pyref.PyLocus that PrelimAlignments::push and _read_next_alns read: thresholds and complexity, no k-mers."""
    def __init__(self, alleles, k, bg, params, edit_thresholds):
        self.alleles, self.k, self.bg, self.prm = alleles, k, bg, params
        self.edit_thresholds = edit_thresholds
        self.half_neighb = bg.neighb // 2
        self.compl_mult = 1.0 / min(bg.neighb + 1 - params.complexity_k, 1 << (2 * params.complexity_k))
        self.compl = _LazyCompl(alleles, params.complexity_k, bg.neighb)


class _LoggingPrelim(pyref._Prelim):
    def __init__(self):
        super().__init__()
        self.pushed = []

    def push(self, aln):
        self.pushed.append(dict(aln, saved=aln["edit"] <= self.passable[aln["read_end"]]))
        return super().push(aln)


def walk(L, pair):
    """One pair (seq1, seq2, recs as pyref._decode_chunk gives them) through pyref's _read_next_alns and push: `look` (the first
    primary is saved), `ok` (both read ends well mapped), the saved alignments of every (read end, contig) group in record order,
    the records that were pushed but not saved, the mates' lengths and the number of records."""
    seq1, seq2, recs = pair
    paired = bool(L.bg.is_paired)
    prelim, state = _LoggingPrelim(), {"weight": 1.0}
    ok, ri = pyref._read_next_alns(L, len(seq1), recs, 0, 0, state, prelim)
    look = bool(prelim.pushed) and prelim.pushed[0]["saved"]
    if paired and look:
        ok2, ri = pyref._read_next_alns(L, len(seq2), recs, ri, 1, state, prelim)
        ok = ok and ok2
    groups, unsaved = {}, []
    for a in prelim.pushed:
        if a["saved"]:
            groups.setdefault((a["read_end"], a["contig"]), []).append(a)
        else:
            unsaved.append(a)
    return {"look": look, "ok": ok, "groups": groups, "unsaved": unsaved, "len": (len(seq1), len(seq2) if paired else 0),
            "n_recs": len(recs), "passable": tuple(prelim.passable)}


# ---- building pairs ----

def cigar_with(n_mism, rl=RL):
    return f"{rl}=" if n_mism == 0 else f"{rl - n_mism}={n_mism}X"


class Design:
    """A locus and the designed cases on it: cases[name] = list of pairs (ReadsChunk.from_pairs dicts with `route`, `why`,
    `sizes` = saved alignments per (read end, contig) group, and what else the case names)."""
    def __init__(self, key, n_alleles, length, k=25, paired=True, seed=3):
        self.key, self.n_alleles, self.length, self.k, self.paired = key, n_alleles, length, k, paired
        self.alleles = random_alleles(n_alleles, length, seed=seed)
        self.counts = None                       # None: every k-mer of the locus is unique (all counts 0)
        self.bg = make_bg(paired=paired)
        self.cases = {}

    def seq(self, a, s, n):
        assert 0 <= s and s + n <= self.length
        return self.alleles[a][s:s + n].decode()

    def pair(self, src, s, sizes, route, why, first_mism=0, unsaved=(), **named):
        """Mate 1 from allele `src` at s, forward; mate 2 INS bases on, reverse. sizes[(end, contig)] saved alignments in that
        group: the primaries lie on `src`; the j-th alignment of a group lies 256 * j bases on (its own bin) and has j mismatches
        more. unsaved: (end, contig) groups that get one more record, beyond `passable` (20 mismatches)."""
        pos = (s, s + INS - RL)
        sizes = dict(sizes)
        for e in range(2 if self.paired else 1):
            sizes.setdefault((e, src), 1)
        recs = []
        for e in range(2 if self.paired else 1):
            fl = (M2 | REV) if e else 0
            recs.append((src, pos[e], fl, cigar_with(first_mism if e == 0 else 0)))
            for (ge, c), n in sizes.items():
                if ge != e:
                    continue
                for j in range(1 if c == src else 0, n):
                    recs.append((c, pos[e] + 256 * j, fl | SEC, cigar_with(j + (c != src))))
            for (ge, c) in unsaved:
                if ge == e:
                    recs.append((c, pos[e] + 128, fl | SEC, cigar_with(20)))
        return dict({"seq1": self.seq(src, pos[0], RL), "seq2": self.seq(src, pos[1], RL) if self.paired else None, "recs": recs,
                     "route": route, "why": why, "sizes": sizes if first_mism < 20 else {}}, **named)


def group_size_pairs(D, contigs, src=None):
    """Groups of 1, 2 and 3 saved alignments on end 0, on end 1 and on both, on each of `contigs`; and the variants."""
    two_ok = two_runs(D.n_alleles)
    by = {1: LEAN, 2: TWO if two_ok else GENERAL, 3: GENERAL}
    out = []
    ends = ((0,), (1,), (0, 1)) if D.paired else ((0,),)
    for c in contigs:
        s0 = src if src is not None else c
        for where in ends:
            for n in (1, 2, 3):
                out.append(D.pair(s0, 260, {(e, c): n for e in where}, by[n], f"groups of {n} on contig {c}, ends {where}"))
        # a second record in the group that is not saved, because its edit distance is beyond `passable`
        out.append(D.pair(s0, 260, {(0, c): 1}, LEAN, f"contig {c}: two records in the group, one of them not saved", unsaved=[(0, c)]))
        # doubled groups in a pair whose first primary is not saved: never looked at
        out.append(D.pair(s0, 260, {(e, c): 2 for e in ends[-1]}, LEAN, f"contig {c}: doubled groups, the first primary not saved", first_mism=20))
        # a third alignment in one group while another group holds two
        other = (c + 1) % D.n_alleles
        out.append(D.pair(s0, 260, {(0, c): 3, (ends[-1][-1], other): 2}, GENERAL, f"a third alignment on contig {c}, two on contig {other}"))
    return out


def inside_group_pairs(D):
    """Two saved alignments of one group on contig 1, in both record orders, on end 0 and on end 1; the primaries lie on contig 0
    and the other end has one alignment on contig 1, so that the group is paired up. (start, mismatches, strand flipped)"""
    base, shift = 512, (0, 384)                  # end 1 lies three bins on: the bins of a group are those of the arrangement
    arrangements = [
        ("one bin", (base + 10, 0, False), (base + 100, 1, False)),
        ("starts 127 and 128", (base + 127, 0, False), (base + 128, 1, False)),
        ("far apart", (base + 10, 0, False), (base + 700, 1, False)),
        ("tie in one bin", (base + 10, 1, False), (base + 100, 1, False)),
        ("tie in two bins", (base + 10, 1, False), (base + 600, 1, False)),
        ("one on the other strand", (base + 10, 0, False), (base + 300, 1, True)),
    ]
    out = []
    for e in (0, 1) if D.paired else (0,):
        for name, x, y in arrangements:
            for order in ((x, y), (y, x)):
                pos = (260, 260 + INS - RL)
                recs = []
                for end in range(2 if D.paired else 1):
                    fl = (M2 | REV) if end else 0
                    recs.append((0, pos[end], fl, cigar_with(0)))
                    if end == e:
                        for start, mism, flip in order:
                            recs.append((1, start + shift[end], (fl ^ REV if flip else fl) | SEC, cigar_with(mism)))
                    else:
                        recs.append((1, base + 50 + shift[end], fl | SEC, cigar_with(1)))
                sizes = {(end, 0): 1 for end in range(2 if D.paired else 1)}
                sizes.update({(end, 1): 2 if end == e else 1 for end in range(2 if D.paired else 1)})
                out.append({"seq1": D.seq(0, pos[0], RL), "seq2": D.seq(0, pos[1], RL) if D.paired else None, "recs": recs,
                            "route": TWO, "why": f"end {e}: {name}, {'better' if order[0][1] < order[1][1] else 'worse or equal'} one first",
                            "sizes": sizes, "group": (e, 1), "one_bin": (order[0][0] >> 7) == (order[1][0] >> 7),
                            "tie": order[0][1] == order[1][1], "better_first": order[0][1] < order[1][1],
                            "strands_differ": order[0][2] != order[1][2]})
    return out


def trip_pairs(D):
    """More than 256 records with one record per allele; the second alignment of a group lies at the last index of the first trip
    of pass 1 (n_eff = 256), at the first index of the second trip (n_eff = 257), or at a few hundred."""
    assert D.n_alleles >= 300 and D.paired
    pos = (260, 260 + INS - RL)
    out = []

    def build(n0, n1, second_of, why, route):
        """end 0: contigs 0 .. n0 - 1, end 1: contigs 0 .. n1 - 1, then the second alignment of group `second_of` as the last record
        (after end 1's records it belongs to end 1; with n1 == 0 it follows end 0's records and the mate-2 records come after it)."""
        recs = [(a, pos[0], SEC if a else 0, cigar_with(0 if a == 0 else 1)) for a in range(n0)]
        mate2 = [(a, pos[1], M2 | REV | (SEC if a else 0), cigar_with(0 if a == 0 else 1)) for a in range(max(n1, 1))]
        sizes = {(0, a): 1 for a in range(n0)}
        sizes.update({(1, a): 1 for a in range(max(n1, 1))})
        p = {"seq1": D.seq(0, pos[0], RL), "seq2": D.seq(0, pos[1], RL), "route": route, "why": why, "sizes": sizes}
        if second_of is None:
            recs += mate2
        else:
            e, c = second_of
            second = (c, pos[e] + 600, ((M2 | REV) if e else 0) | SEC, cigar_with(2))
            recs = recs + [second] + mate2 if e == 0 else recs + mate2 + [second]
            sizes[second_of] = 2
            p.update(group=second_of, first_ix=c if e == 0 else n0 + c, second_ix=n0 if e == 0 else len(recs) - 1)
        out.append(dict(p, recs=recs))

    two = TWO if two_runs(D.n_alleles) else GENERAL
    build(10, 245, (1, 5), "n_eff = 256: the second alignment is the last record of the first trip", two)
    build(10, 246, (1, 5), "n_eff = 257: the second alignment is the first record of the second trip", two)
    build(150, 249, (1, 7), "record index 399 in the 16-bit index field of a saved alignment", two)
    build(300, 0, (0, 3), "end 0: first at index 3, second at index 300, in the second trip", two)
    build(10, 247, None, "257 records, one per group", LEAN)
    return out


def lean_ovf_pairs(D):
    """64 doubled groups stay with the two-slot form, 65 and 64 with a tripled one among them go to the general kernel."""
    assert 66 <= D.n_alleles <= KEEP_MAX_ALLELES and D.paired
    def doubled(n0, n1):
        sizes = {(0, c): 2 for c in range(n0)}
        sizes.update({(1, c): 2 for c in range(n1)})
        return sizes
    out = [D.pair(0, 260, doubled(32, 32), TWO, "64 doubled groups, 32 on either end", doubled=64),
           D.pair(0, 260, doubled(64, 0), TWO, "64 doubled groups on end 0", doubled=64),
           D.pair(0, 260, doubled(33, 32), GENERAL, "65 doubled groups", doubled=65),
           D.pair(0, 260, doubled(0, 65), GENERAL, "65 doubled groups on end 1", doubled=65),
           D.pair(0, 260, doubled(63, 0), TWO, "63 doubled groups", doubled=63)]
    sizes = doubled(32, 32); sizes[(1, 31)] = 3
    out.append(D.pair(0, 260, sizes, GENERAL, "64 doubled groups, one of them tripled", doubled=64))
    sizes = doubled(32, 32); sizes[(0, 40)] = 3
    out.append(D.pair(0, 260, sizes, GENERAL, "64 doubled groups and a tripled group", doubled=65))
    return out


def unique_windows(n, k):
    """The windows of a designed read of n bases that are unique k-mers: the last one, and those at bases 20 and 50 where they end
    before the last one starts (a counted window skips the k - 1 that follow it, locs.rs:968-1002)."""
    return sorted({n - k} | {w for w in (20, 50) if w + k <= n - k}) if n >= k else []


def mate_length_design(paired, long_mate=0, key=None):
    """Reads of MATE_LENGTHS bases from allele 0, each with a twin with an N in its last base and one with an N in base 31, 32 or
    63. The k-mer counts of the locus are 1 everywhere but at the read's last window and at the windows that start at its bases 20
    and 50, so those alone are unique k-mers: the unique-k-mer counts depend on the last word of the mate and its mask."""
    D = Design(key or f"mates-{'paired' if paired else 'single'}-{long_mate}", 3, 10_500, paired=paired, seed=11)
    k = D.k
    counts = [np.ones(D.length + 1 - k, dtype=np.uint16) for _ in range(D.n_alleles)]
    starts, s = {}, 300
    for n in MATE_LENGTHS:
        starts[n] = s
        for w in unique_windows(n, k):
            counts[0][s + w] = 0
        s += n + 64
    assert s + 600 < D.length
    D.counts = counts
    pairs = []
    for n in MATE_LENGTHS:
        s = starts[n]
        read = D.seq(0, s, n)
        twins = [("as it is", None, read), ("N in the last base", n - 1, read[:-1] + "N")]
        for at in [b for b in (31, 32, 63) if b < n - 1] or [n // 2]:
            twins.append((f"N in base {at}", at, read[:at] + "N" + read[at + 1:]))
        for what, at, seq in twins:
            other = D.seq(0, s + 300, RL)
            long_rec = (0, s, 0, f"{n}=")
            if not paired:
                p = {"seq1": seq, "seq2": None, "recs": [long_rec], "sizes": {(0, 0): 1}}
            elif long_mate == 0:
                p = {"seq1": seq, "seq2": other, "recs": [long_rec, (0, s + 300, M2 | REV, f"{RL}=")], "sizes": {(0, 0): 1, (1, 0): 1}}
            else:
                p = {"seq1": other, "seq2": seq, "recs": [(0, s + 300, 0, f"{RL}="), (0, s, M2 | REV, f"{n}=")], "sizes": {(0, 0): 1, (1, 0): 1}}
            p.update(route=LEAN if n <= REGS_MAX_LEN else GENERAL, why=f"a mate of {n} bases, {what}", mate_len=n, twin=what, n_at=at)
            pairs.append(p)
    D.cases["mate lengths"] = pairs
    return D


ALLELE_COUNTS = (63, 64, 65, 128, 129, 309, 310)


@functools.lru_cache(maxsize=None)
def designs():
    """Every locus with its cases, built once."""
    out = []
    D = Design("small", 9, 2000)
    D.cases["group sizes"] = group_size_pairs(D, [2])
    D.cases["inside a doubled group"] = inside_group_pairs(D)
    out.append(D)
    D = Design("small-single-end", 9, 2000, paired=False)
    D.cases["group sizes"] = group_size_pairs(D, [0, 2])
    D.cases["inside a doubled group"] = inside_group_pairs(D)
    out.append(D)
    D = Design("ovf-70", 70, 1500, seed=5)
    D.cases["LEAN_OVF"] = lean_ovf_pairs(D)
    out.append(D)
    for n in ALLELE_COUNTS:
        D = Design(f"alleles-{n}", n, 1500, seed=7)
        D.cases["group sizes"] = group_size_pairs(D, sorted({0, 63, 64, n - 1} & set(range(n))))
        if n in (309, 310):
            D.cases["pass-1 trips"] = trip_pairs(D)
        out.append(D)
    out.append(mate_length_design(True, 0))
    out.append(mate_length_design(True, 1))
    out.append(mate_length_design(False))
    D = Design("k41", 5, 2000, k=41)
    D.cases["k = 41"] = [dict(p, route=GENERAL) for p in group_size_pairs(D, [2])[:9]]
    out.append(D)
    return tuple(out)


def case_ids():
    return [(D.key, name) for D in designs() for name in D.cases]


def design(key):
    return next(D for D in designs() if D.key == key)


def chunk_of(pairs):
    return cdefs.ReadsChunk.from_pairs(pairs)
