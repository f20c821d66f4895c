"""Designed haplotype families for the tests of the transitive haplotype alignments (TEST INFRASTRUCTURE): 6-9 haplotypes of 600-2 000
bases derived from one base along a small tree by SNPs and indels of 1-30 bases, at the smallest sizes that still reach every branch
of the strategy and of transfer_alignment::<true>. tests/test_transitive_host.py asserts on the transliteration's output that each
case still covers the branch it was designed for; tests/test_gpu_transitive.py runs them on the device.

Of the four direction combinations (j_ref_ij, k_ref_jk) three can occur: the CIGAR kept in closest[k] has k as its QUERY
(save_cigar stores closest[query_id]), so the first clause always reads j-k with k_ref_jk = false, and the second clause always reads
i-j out of closest[i] with j_ref_ij = true: (false, true) is reached by neither. test_transitive_host.py runs that combination through
find_transitive_alignment directly; the kernels' path for it (I and D changed places in i-j only) is run by no test."""
import functools

import numpy as np

from tests import pyref_transitive as T
from tests.align_cases import apply_edits, other_base, rand_seq, _insert_seq


class TrCase:
    def __init__(self, name, seqs, pairs=None, ks=(21, 31), max_gap=10000, tr_div=0.05, anchor=11, thresh_div=1.0, against=None, dp_cells=None):
        self.name, self.seqs, self.ks, self.max_gap = name, [bytes(s) for s in seqs], list(ks), max_gap
        self.tr_div, self.anchor, self.thresh_div, self.against, self.dp_cells = tr_div, anchor, thresh_div, against, dp_cells
        n = len(self.seqs)
        self.pairs = pairs if pairs is not None else [(i, j) for i in range(n) for j in range(i + 1, n)]
        self.names = [f"{name}_h{i}" for i in range(n)]

    def arrays(self):
        seqs = np.frombuffer(b"".join(self.seqs), dtype=np.uint8).copy()
        off = np.zeros(len(self.seqs) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in self.seqs], out=off[1:])
        return seqs, off

    def expected(self, **over):
        kw = dict(max_gap=self.max_gap, tr_div=self.tr_div, anchor=self.anchor, thresh_div=self.thresh_div, against=self.against)
        if self.dp_cells is not None:
            kw["dp_cells"] = self.dp_cells
        kw.update(over)
        return T.run(self.seqs, self.pairs, self.ks, **kw)


def snp(s, p, rng):
    return (p, "X", other_base(s[p], rng))


def ins(s, p, n, rng):
    return (p, "I", _insert_seq(rng, n, s[p - 1], s[p]))


def dele(s, p, n):
    while s[p + n - 1] == s[p - 1] or s[p] == s[p + n]:      # the removed bases must not slide
        n += 1
    return (p, "D", n)


def _tree(rng, length):
    """8 haplotypes along a tree with clustered edits (closer together than the anchor, so the walk has stretches of every kind)"""
    h0 = rand_seq(rng, length)
    h1 = apply_edits(h0, [snp(h0, 100, rng), snp(h0, 300, rng), ins(h0, 420, 7, rng), snp(h0, 600, rng)])
    # h2: edits of its own right next to h1's (adjacent to the SNP at 100: a plain D; 3 and 8 bases from others: straight / exact)
    h2 = apply_edits(h1, [dele(h1, 101, 4), snp(h1, 303, rng), snp(h1, 305, rng), dele(h1, 440, 9), snp(h1, 520, rng)])
    h3 = bytes(h1)                                                             # identical to h1: both shortcuts
    h4 = apply_edits(h1, [snp(h1, 200, rng)])                                   # strictly closer to h1 than to h0; as close to h3 as to h1
    h5 = apply_edits(h2, [ins(h2, 96, 5, rng), ins(h2, 250, 30, rng), dele(h2, 272, 12), snp(h2, 560, rng), snp(h2, 566, rng)])
    h6 = apply_edits(h0, [snp(h0, 50, rng), ins(h0, 104, 3, rng), dele(h0, 296, 2), snp(h0, 610, rng), dele(h0, 650, 15), ins(h0, 680, 11, rng)])
    h7 = apply_edits(h6, [snp(h6, 52, rng), snp(h6, 400, rng), ins(h6, 425, 20, rng)])
    return [h0, h1, h2, h3, h4, h5, h6, h7]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    rng = np.random.default_rng(501)
    fam = _tree(rng, 800)
    out.append(TrCase("tree", fam, tr_div=0.08))
    # a small max_gap: stretches with a side above it take align_simple, in the walk and in the backbone alike
    out.append(TrCase("tree_maxgap", fam, tr_div=0.12, max_gap=8))
    # a haplotype unrelated to the others (skipped by thresh_div in the middle of every row) and another one carrying the `against` flag
    rng = np.random.default_rng(502)
    fam2 = _tree(rng, 760)
    fam2 = fam2[:3] + [rand_seq(rng, 760)] + fam2[3:7] + [rand_seq(rng, 600)]
    out.append(TrCase("skips", fam2, tr_div=0.08, thresh_div=0.6, against=[0] * 8 + [1]))
    # hand-ordered pairs: a reader directly behind its writer, (False, False) and (True, True) directions, closest[q2] = q1 inside a row
    rng = np.random.default_rng(503)
    b = rand_seq(rng, 700)
    hand = [b]
    for h in range(1, 7):
        prev = hand[-1]
        pos = 60 + 90 * h
        hand.append(apply_edits(prev, [snp(prev, pos, rng), ins(prev, pos + 6, 2 + h, rng) if h % 2 else dele(prev, pos + 6, 2 + h), snp(prev, pos + 40, rng)]))
    order = [(1, 0), (0, 2), (2, 1), (3, 4), (5, 3), (5, 4), (6, 3), (6, 4), (6, 5), (0, 3), (4, 0), (0, 5), (6, 0), (1, 3), (1, 4), (5, 1), (1, 6), (2, 3),
             (4, 2), (2, 5), (6, 2)]
    out.append(TrCase("hand", hand, pairs=order, tr_div=0.1))
    # 15 pairs: below the 16 of align.rs:784, everything goes the backbone route
    out.append(TrCase("fifteen", fam[:6], tr_div=0.08))
    # the default anchor of 101 on 2 kb, sparse edits
    rng = np.random.default_rng(504)
    b = rand_seq(rng, 2000)
    wide = [b]
    for h in range(1, 7):
        prev = wide[(h - 1) // 2]
        pos = [150 + 37 * h, 700 + 53 * h, 1300 + 41 * h]
        wide.append(apply_edits(prev, [snp(prev, pos[0], rng), ins(prev, pos[1], 3 * h, rng) if h % 2 else dele(prev, pos[1], 3 * h), snp(prev, pos[2], rng), snp(prev, pos[2] + 40, rng)]))
    out.append(TrCase("anchor101", wide, ks=(25, 51), tr_div=0.02, anchor=101))
    return out


def _dense(rng, length, start, end, tail):
    """7 haplotypes, h from (h - 1) // 2: SNPs every 60 bases of [start + 7 h, end), so no '=' run of the anchor (101) lies in the
    region and the walk sees it as one stretch; behind it one indel of 2 + h bases at tail + 11 h"""
    fam = [rand_seq(rng, length)]
    for h in range(1, 7):
        prev = fam[(h - 1) // 2]
        edits = [snp(prev, p, rng) for p in range(start + 7 * h, end, 60)]
        at = tail + 11 * h
        fam.append(apply_edits(prev, edits + [ins(prev, at, 2 + h, rng) if h % 2 else dele(prev, at, 2 + h)]))
    return fam


@functools.lru_cache(maxsize=None)
def level_cases():
    """walk stretches above scratch level 0 (every family of cases() stays below 256 bases a side): 360 to 390 bases a side, level 1,
    and 2 100 to 2 140 a side, level 2. Of the 21 pairs the 6 of row 0 go the backbone route, the other 15 the transitive one, a row
    (5, 4, ... tasks) per round. A list of its own: test_transitive_host.py bounds the sizes of cases()."""
    rng = np.random.default_rng(505)
    kw = dict(ks=(25, 51), tr_div=0.08, anchor=101, max_gap=10000)
    return [TrCase("level1", _dense(rng, 1200, 300, 700, 900), **kw), TrCase("level2", _dense(rng, 2700, 200, 2350, 2500), **kw)]


def by_name(name):
    return next(c for c in cases() + level_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the transliteration's result of a case, computed once and shared by the tests"""
    return by_name(name).expected()
