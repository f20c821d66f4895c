"""Transliteration of the backbone strategy of `locityper align` (TEST INFRASTRUCTURE), written from the Rust in plain Python and
numpy: src/seq/align.rs precompute_kmers / get_kmer_matches (102-120, 202-224), align_from_backbone (246-292), align_multik
(294-318), the PAF line of process_pair (639-677) and the header line of command/align.rs:385-387; smart_align of
src/seq/wfa.rs:280-321 on the aligner primitive tests/pyref_transfer.py already restates (the oracle's exact gap-affine optimum with
its documented tie rule). LCSk++ is the published definition, evaluated in O(m^2). full_dp_score is an independent full-matrix
global gap-affine optimum (4 / 6 / 1) of two whole sequences.

The stated differences of the library are applied here too: a window with a byte outside ACGT is no k-mer, any such byte is N in the
gap fill, a sequence shorter than k has no k-mers, and equal neighbouring CIGAR operations are merged at the very end (normalize)."""
import math

import numpy as np

from tests import oracle_ffi as O
from tests.pyref_transfer import Cig, align_simple, MISMATCH, GAP_OPEN, GAP_EXTEND, SAFE_MISMATCH, DROPPED

OPC = {"I": 1, "D": 2, "=": 7, "X": 8}
OPS = {v: k for k, v in OPC.items()}
DP_DIM, DP_CELLS = 16383, 1 << 26                            # the largest scratch level of the device aligner
_ACGT = frozenset(b"ACGT")


class UnfitCase(Exception):
    """The aligner primitive gave up (its step limit belongs to accuracy level 6): the input is no test case for level 9."""


def norm(seq):
    return bytes(c if c in _ACGT else 78 for c in bytes(seq))


def precompute_kmers(seq, k):                                # align.rs:102-120: k-mer -> positions, ascending
    seq = bytes(seq)
    out = {}
    for p in range(len(seq) - k + 1):
        w = seq[p:p + k]
        if all(c in _ACGT for c in w):
            out.setdefault(w, []).append(p)
    return out


def get_kmer_matches(kmers1, kmers2):                        # align.rs:202-224
    buf = [(p1, p2) for w, ps1 in kmers1.items() if w in kmers2 for p1 in ps1 for p2 in kmers2[w]]
    buf.sort()
    return buf


def kmer_matches(seq1, seq2, k):
    return get_kmer_matches(precompute_kmers(seq1, k), precompute_kmers(seq2, k))


def lcskpp(matches, k):
    """(score, path as match indices). dp(m) = max(k, dp(m') + 1 for m' = (i - 1, j - 1) a match, k + max dp(m'') over the matches
    with i'' + k <= i and j'' + k <= j); matches sorted."""
    m = len(matches)
    if m == 0:
        return 0, []
    I = np.array([a for a, _ in matches], dtype=np.int64); J = np.array([b for _, b in matches], dtype=np.int64)
    index = {mt: x for x, mt in enumerate(matches)}
    dp = np.zeros(m, dtype=np.int64); prev = np.full(m, -1, dtype=np.int64)
    for x in range(m):
        best, pv = k, -1
        d = index.get((int(I[x]) - 1, int(J[x]) - 1))
        if d is not None and dp[d] + 1 > best:
            best, pv = int(dp[d]) + 1, d
        n_before = int(np.searchsorted(I, I[x] - k, side="right"))          # i'' + k <= i: a prefix of the sorted matches
        if n_before:
            ok = J[:n_before] + k <= J[x]
            if ok.any():
                cand = np.where(ok, dp[:n_before], 0)
                c = int(np.argmax(cand))
                if k + int(cand[c]) > best:
                    best, pv = k + int(cand[c]), c
        dp[x], prev[x] = best, pv
    at = int(np.argmax(dp))
    score, path = int(dp[at]), []
    while at >= 0:
        path.append(at); at = int(prev[at])
    return score, path[::-1]


def exact_align(s1, s2, cig, dp_cells, counters):            # Aligner::align of the global aligner, wfa.rs:254-299, at accuracy 9
    n, m = len(s1), len(s2)
    if n > DP_DIM or m > DP_DIM or (n + 1) * (m + 1) > dp_cells:        # "the aligner dropped it" (wfa.rs:234-237)
        counters["dropped"] = counters.get("dropped", 0) + 1
        return align_simple(s1, s2, cig)
    pen, ops = O.dp_align(bytes(s1), bytes(s2), 0, 0)
    if pen == DROPPED:
        raise UnfitCase(f"stretch {n} x {m}")
    for op, ln in Cig.parse(ops).t:
        cig.push_checked(op, ln)
    return -pen


def smart_align(seq1, i1, i2, seq2, j1, j2, max_gap, cig, dp_cells=DP_CELLS, counters=None):       # wfa.rs:280-321
    counters = counters if counters is not None else {}
    jump1, jump2 = i2 - i1, j2 - j1
    if jump1 > 0 and jump2 > 0:
        s1, s2 = seq1[i1:i2], seq2[j1:j2]
        if max_gap < jump1 or max_gap < jump2:
            return align_simple(s1, s2, cig)
        if jump1 == jump2 and jump1 <= SAFE_MISMATCH:
            nd = 0
            for a, b in zip(s1, s2):
                cig.push_checked("=" if a == b else "X", 1); nd -= a != b
            return nd * MISMATCH
        return exact_align(s1, s2, cig, dp_cells, counters)
    if jump1 > 0:
        cig.push_unchecked("D", jump1); return -GAP_OPEN - jump1 * GAP_EXTEND
    if jump2 > 0:
        cig.push_unchecked("I", jump2); return -GAP_OPEN - jump2 * GAP_EXTEND
    return 0


def align_from_path(seq1, seq2, matches, path, k, max_gap, dp_cells=DP_CELLS, counters=None):       # align.rs:256-291
    """(Cig, score) of reference seq1 and query seq2 along `path` (indices into `matches`)."""
    seq1, seq2 = norm(seq1), norm(seq2)
    cig, score, i1, j1, curr = Cig(), 0, 0, 0, 0
    for ix in path:
        i2, j2 = matches[ix]
        if i1 > i2:
            curr += 1; i1 += 1; j1 += 1
            continue
        if curr > 0:
            cig.push_unchecked("=", curr); curr = 0
        score += smart_align(seq1, i1, i2, seq2, j1, j2, max_gap, cig, dp_cells, counters)
        curr += k; i1 = i2 + k; j1 = j2 + k
    if curr > 0:
        cig.push_unchecked("=", curr)
    score += smart_align(seq1, i1, len(seq1), seq2, j1, len(seq2), max_gap, cig, dp_cells, counters)
    assert cig.rlen == len(seq1) and cig.qlen == len(seq2)
    return cig, score


def align_from_backbone(seq1, seq2, k, max_gap, dp_cells=DP_CELLS):
    matches = [(int(a), int(b)) for a, b in kmer_matches(seq1, seq2, k)]
    _, path = lcskpp(matches, k)
    return align_from_path(seq1, seq2, matches, path, k, max_gap, dp_cells)


def align_multik(seq1, seq2, ks, max_gap, dp_cells=DP_CELLS):                # align.rs:294-318: (Cig, score, best k)
    best = None
    for k in ks:
        cig, score = align_from_backbone(seq1, seq2, k, max_gap, dp_cells)
        if best is None or score > best[1]:
            best = (cig, score, k)
    return best


def normalize(cig):
    """[(op, len)] with empty items dropped and equal neighbours merged: the form the library writes."""
    out = []
    for op, ln in cig.t:
        if ln == 0:
            continue
        if out and out[-1][0] == op: out[-1][1] += ln
        else: out.append([op, ln])
    return [(op, ln) for op, ln in out]


def words(items):
    return np.array([(ln << 4) | OPC[op] for op, ln in items], dtype=np.uint32)


def items_of(w):
    return [(OPS[int(x) & 15], int(x) >> 4) for x in w]


def calculate_score(items):                                  # Penalties::calculate_score, wfa.rs:87-99
    s = 0
    for op, ln in items:
        s -= 0 if op == "=" else MISMATCH * ln if op == "X" else GAP_OPEN + GAP_EXTEND * ln
    return s


def counts(items):                                           # process_pair 652-660: (n_matches, nerrs)
    nm = sum(ln for op, ln in items if op == "=")
    return nm, sum(ln for _, ln in items) - nm


def _f(v, prec):                                             # Rust's {:.N}
    if math.isnan(v): return "NaN"
    if math.isinf(v): return "inf" if v > 0 else "-inf"
    return f"{v:.{prec}f}"


def paf_header(div_k=15, div_w=15, thresh_div=1.0, ks=(25, 51, 101), max_gap=10000):                 # command/align.rs:385-387
    if thresh_div == 0.0:                                    # Params::validate, align.rs:77-80
        thresh_div, ks = -1.0, ()
    return f"# minimizers={div_k},{div_w}; max_divergence={thresh_div:.5f}; backbone-ks={','.join(str(k) for k in ks)}; accuracy=9; max-gap={max_gap}\n"


def paf_line(qname, qlen, rname, rlen, aln=None, div=None):                                          # process_pair, 639-677
    """aln: None (skipped) or (items, score); div: None (skip_div) or (um, md)."""
    s = f"{qname}\t{qlen}\t0\t{qlen}\t+\t{rname}\t{rlen}\t0\t{rlen}\t"
    if aln is not None:
        items, score = aln
        nm, ne = counts(items)
        ln = nm + ne
        dv = ne / ln if ln else float("nan")
        qv = (-10.0 * math.log10(dv) if dv > 0 else float("inf")) if math.isfinite(dv) else float("inf")
        s += f"{nm}\t{ln}\t255\tNM:i:{ne}\tAS:i:{score}\tdv:f:{_f(dv, 9)}\tqv:f:{_f(qv, 6)}"
    else:
        s += "0\t0\t255"
    if div is not None:
        s += f"\tum:i:{div[0]}\tmd:f:{_f(div[1], 9)}"
    if aln is not None:
        s += "\tcg:Z:" + "".join(f"{ln}{op}" for op, ln in aln[0])
    return s + "\n"


def full_dp_score(seq1, seq2):
    """The optimum score (<= 0) of a global gap-affine alignment of two whole sequences, mismatch 4, gap open 6, extend 1 (a gap of
    length l costs 6 + l); a row at a time, the horizontal gap as a running minimum."""
    a = np.frombuffer(norm(seq1), dtype=np.uint8); b = np.frombuffer(norm(seq2), dtype=np.uint8)
    n, m = len(a), len(b)
    INF = 1 << 40
    cols = np.arange(m + 1, dtype=np.int64)
    M = np.full(m + 1, INF, dtype=np.int64); D = np.full(m + 1, INF, dtype=np.int64); Ins = np.full(m + 1, INF, dtype=np.int64)
    M[0] = 0
    Ins[1:] = GAP_OPEN + GAP_EXTEND * cols[1:]
    for r in range(1, n + 1):
        H = np.minimum(M, np.minimum(D, Ins))
        nM = np.full(m + 1, INF, dtype=np.int64)
        nM[1:] = H[:-1] + np.where(b == a[r - 1], 0, MISMATCH)
        nD = np.minimum(D + GAP_EXTEND, H + GAP_OPEN + GAP_EXTEND)
        base = np.minimum(nM, nD) - GAP_EXTEND * cols                       # opened behind column b': (value - E b') + O + E b
        run = np.minimum.accumulate(base)
        nI = np.full(m + 1, INF, dtype=np.int64)
        nI[1:] = run[:-1] + GAP_OPEN + GAP_EXTEND * cols[1:]
        M, D, Ins = nM, nD, nI
    return -int(min(M[m], D[m], Ins[m]))
