"""Designed reads for minimizer recruitment (lcty_recruit.hip: recruit_kernel, one lane per read pair or single read of up to 256
bases; recruit_single_kernel, one wavefront per single read beyond). Plain functions that return cases: loci, parameters, reads and
whether they are pairs, with a note of the shape the case is about and one tag per read. Nothing here predicts an answer. Where a
case has to sit on an equality (a fraction equal to match_frac, a count equal to its threshold, a running sum that peaks at
stretch_score) it is searched for on the restatement tests/pyref_recruit.py and the first hit is kept;
tests/test_recruit_cases.py asserts on the restatement's own output that every case still has the shape it claims and that the
restatement and the oracle agree on every read; tests/test_gpu_recruit_designed.py holds the kernels against the oracle.

The facts the searches read (`counts_of`, `short_fraction`, `pair_fractions`, `long_terms`, `stretch_peak`) are the intermediate
values of Targets.recruit / Targets._stretch, put together from the restatement's own parts.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import pyref_recruit as PR

BASE_K = 25
COMP = bytes.maketrans(b"ACGT", b"TGCA")
# the first four fields are the case; reads: [(mate 1, mate 2 or None)] as bytes; tags: one string per read; max_out: what the call
# is given; error: None or the name of the code the call must return; after: reads the same targets must still answer afterwards;
# common: share of the alleles' k-mers whose count is above the threshold (the others are rare)
Case = namedtuple("Case", "loci params reads paired note name tags max_out error after common")

MAX_LOCI_PER_READ, LONG_LOCI = 8, 16                # lcty_recruit.hip, restated
LANE_MAX, SHORT_MAX = 256, PR.READ_LENGTH_THRESH    # which kernel; which rule


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8).tolist())


def _alleles(rng, length, n):
    base = np.frombuffer(_rand(rng, length), dtype=np.uint8)
    out = [bytes(base)]
    for _ in range(n - 1):
        s = base.copy(); m = rng.random(length) < 0.01
        s[m] = rng.choice(list(b"ACGT"), int(m.sum()))
        out.append(bytes(s))
    return out


def _params(k=14, w=10, match_frac=0.5):
    return dict(k=k, w=w, match_frac=match_frac, match_length=200, thresh_kmer_count=50)


def _case(name, note, loci, params, reads, paired, tags=None, max_out=16, error=None, after=(), common=0.1):
    reads = [(bytes(a), None if b is None else bytes(b)) for a, b in reads]
    assert all((b is not None) == paired for _, b in reads)
    tags = list(tags) if tags is not None else [""] * len(reads)
    assert len(tags) == len(reads)
    return Case(loci, params, reads, paired, note, name, tags, max_out, error, list(after), common)


def case_counts(case):
    """k-mer counts of the alleles of a case (base k 25): `common` of them 80, the others 0, from a fixed seed."""
    rng = np.random.default_rng(9)
    return [[np.where(rng.random(len(a) - BASE_K + 1) < case.common, 80, 0).astype(np.uint16) for a in alleles] for alleles in case.loci]


def pyref_targets(case):
    pt = PR.Targets(**case.params)
    for alleles, counts in zip(case.loci, case_counts(case)):
        pt.add(alleles, counts, BASE_K)
    return pt


# ---- the intermediate values of Targets.recruit ----

def counts_of(pt, seq):
    """(minimizers of seq, {locus: [common-bw, common-fw, rare-bw, rare-fw]})"""
    m = PR.canon_minimizers(seq, pt.k, pt.w)
    c = {}
    for _, minim, fw in m:
        for locus, direction, rare in pt.minim_to_loci.get(minim, ()):
            pt._inc(c.setdefault(locus, [0] * 4), fw, direction, rare)
    return m, c


def _fn(a): return PR.WORTH * a[3] + a[1]
def _bn(a): return PR.WORTH * a[2] + a[0]
def _fd(a, t): return PR.WORTH * (t - a[1]) + a[1]
def _bd(a, t): return PR.WORTH * (t - a[0]) + a[0]


def short_fraction(a, total):
    """the fraction recruit_short_read compares with match_frac"""
    return (_fn(a), _fd(a, total)) if _fn(a) >= _bn(a) else (_bn(a), _bd(a, total))


def pair_fractions(a, t1, b, t2):
    """the two fractions of recruit_read_pair, and both sums of better_pair_fraction"""
    s_fw, s_bw = (_fn(a) + _bn(b)) & 0xFFFF, (_bn(a) + _fn(b)) & 0xFFFF
    if s_fw >= s_bw: return (_fn(a), _fd(a, t1)), (_bn(b), _bd(b, t2)), (s_fw, s_bw)
    return (_bn(a), _bd(a, t1)), (_fn(b), _fd(b, t2)), (s_fw, s_bw)


def long_terms(pt, a, total):
    """(num, den, thr) of recruit_long_read"""
    num, den = (a[3], total - a[1]) if a[3] >= a[2] else (a[2], total - a[0])
    return num, den, max(1, int(math.ceil(min(pt.stretch_minims, den) * pt.match_frac)))


def stretch_peak(pt, locus, minims):
    """The largest value either running sum of has_matching_stretch takes, the index of the minimizer at which it takes it first and
    the index at which that sum last left zero: (peak, first, at)."""
    lm = pt.locus_minimizers[locus]
    s = [0, 0]; since = [0, 0]; best = (0, 0, 0)
    for j, (_, minim, fw) in enumerate(minims):
        e = lm.get(minim)
        add = [0, 0]
        if e is not None:
            x = PR.SUBSUM_PENALTY + int(e[1]) * PR.SUBSUM_BONUS
            add = [((e[0] & (1 + fw)) != 0) * x, ((e[0] & (1 + (not fw))) != 0) * x]
        for d in range(2):
            if s[d] == 0: since[d] = j
            s[d] = max(s[d] + add[d] - PR.SUBSUM_PENALTY, 0)
            if s[d] > best[0]: best = (s[d], since[d], j)
    return best


def kmer_hashes(seq, k):
    """canonical k-mer hashes of an A/C/G/T sequence"""
    enc = {65: 0, 67: 1, 71: 2, 84: 3}
    out = []
    for i in range(len(seq) - k + 1):
        f = r = 0
        for c in seq[i:i + k]: f = f * 4 + enc[c]
        for c in reversed(seq[i:i + k]): r = r * 4 + 3 - enc[c]
        out.append(PR.fast_hash(min(f, r)))
    return out


def tied_windows(seq, k, w):
    """windows of w consecutive k-mers whose minimal hash occurs more than once"""
    h = kmer_hashes(seq, k)
    return sum(1 for s in range(len(h) - w + 1) if h[s:s + w].count(min(h[s:s + w])) > 1)


# ---- the loci of classes a, b and c: k = 14 (even: k-mers can be their own reverse complement), w = 10 ----

TIE_FEATURES = ("homopolymer", "period2", "period3", "period_w", "period_w1", "self_rc")


def tie_allele(rng, k, w):
    """An allele with the repeats of class b embedded in random sequence -> (allele, {feature: (start, length)})"""
    parts, feats = [_rand(rng, 300)], {}
    reps = lambda p: -(-(3 * w + k) // p) + 1                                 # at least 3w + k bases
    for name, s in (("homopolymer", b"A" * 80), ("period2", b"AC" * 45), ("period3", b"ACG" * 35),
                    ("period_w", _rand(rng, w) * max(reps(w), -(-80 // w))), ("period_w1", _rand(rng, w + 1) * max(reps(w + 1), -(-80 // (w + 1)))),
                    ("self_rc", b"AT" * 45)):
        feats[name] = (sum(len(p) for p in parts), len(s))
        parts += [s, _rand(rng, 320)]
    return b"".join(parts), feats


@functools.lru_cache(maxsize=None)
def common_loci(k=14, w=10):
    rng = np.random.default_rng(100 + 64 * k + w)
    al, feats = tie_allele(rng, k, w)
    mut = bytearray(al)
    for p in rng.integers(0, len(al), len(al) // 100): mut[int(p)] = b"ACGT"[int(rng.integers(0, 4))]
    return [[al, bytes(mut)], _alleles(rng, 1500, 2), _alleles(rng, 900, 1)], feats


def short_lengths(k, w):
    return (0, k - 1, k, k + w - 2, k + w - 1, k + w, 31, 32, 33, 63, 64, 65, 255, 256)


@functools.lru_cache(maxsize=None)
def length_cases():
    """a. Every length at which a loop of either kernel starts, ends or changes hands."""
    k, w = 14, 10
    loci, _ = common_loci(k, w)
    prm = _params(k, w)
    al = loci[1][0]
    m2 = revcomp(al[500:650])
    out = []
    reads, tags = [], []
    for i, l in enumerate(short_lengths(k, w) + (257, 499, 500, 501, 502)):
        r = al[100:100 + l]
        reads += [(r, None), (revcomp(r), None)]; tags += [f"len={l}", f"len={l}"]
    # 200 bases of the allele and foreign sequence after them: too little for the short-read rule, enough for the long-read rule
    foreign = _rand(np.random.default_rng(131), 320)
    for l in (499, 500, 501, 502):
        r = al[700:900] + foreign[:l - 200]
        reads += [(r, None), (revcomp(r), None)]; tags += [f"switch={l}", f"switch={l}"]
    out.append(_case("lengths/single", "single reads of every switching length, cut from an allele; at 499 to 502 bases also reads that only the long-read rule takes",
                     loci, prm, reads, False, tags))
    reads, tags = [], []
    for l in short_lengths(k, w):
        reads += [(al[100:100 + l], m2), (al[100:250], revcomp(al[500:500 + l])), (al[100:100 + l], revcomp(al[500:500 + l]))]
        tags += [f"mates={l}+150", f"mates=150+{l}", f"mates={l}+{l}"]
    out.append(_case("lengths/pairs", "mates of every switching length beside a mate that matches; a missing second mate", loci, prm, reads, True, tags))
    for n in (1, 63, 64, 65):
        reads = [(al[100 + i:100 + i + 256 - 3 * i], revcomp(al[500 + i:500 + i + 40 + 3 * i])) for i in range(n)]
        out.append(_case(f"lengths/chunk{n}", f"{n} pairs, a different mate length in every lane (the probe loop runs to the longest lane's count)",
                         loci, prm, reads, True, [f"mates={256 - 3 * i}+{40 + 3 * i}" for i in range(n)]))
    ok = (al[100:250], m2)
    out.append(_case("lengths/pair_257_first", "a first mate of 257 bases is refused", loci, prm, [ok, (al[100:357], m2)], True, error="UNSUPPORTED", after=[ok]))
    out.append(_case("lengths/pair_257_second", "a second mate of 257 bases is refused", loci, prm, [(al[100:250], revcomp(al[500:757])), ok], True,
                     error="UNSUPPORTED", after=[ok]))
    return out


def _tie_reads(al, feats):
    singles, pairs, tags_s, tags_p = [], [], [], []
    for name in TIE_FEATURES:
        f, L = feats[name]
        r1, r2 = al[f - 100:f + 50], al[f + L - 50:f + L + 100]
        r3 = al[f - 30:f + L + 30] if L + 60 <= LANE_MAX else al[f - 30:f + 226]
        l1, l2 = al[f - 150:f + L + 150], al[f - 250:f + L + 300]
        assert len(l1) > LANE_MAX and len(l2) > SHORT_MAX
        for r in (r1, r2, r3, l1, l2):
            singles += [(r, None), (revcomp(r), None)]; tags_s += [name, name]
        pairs += [(r1, revcomp(r2)), (revcomp(r2), r1), (r3, revcomp(r3)), (r3, revcomp(r1))]; tags_p += [name] * 4
    return singles, tags_s, pairs, tags_p


def _tie_boundary_case(k, w):
    """Single reads whose answer rests on the minimizers of the repeat: the repeat with 40 bases of the allele on either side, then
    foreign sequence — the longest tail with which the restatement still recruits the read and the next longer one, for the lane
    kernel (up to 256 bases) and the wavefront kernel (257 to 500); and the repeat between 250 bases of foreign sequence on either
    side, for the long-read rule. Every k-mer is rare and match_frac is 0.7: a walk that drops tied minimizers loses the read."""
    loci, feats = common_loci(k, w)
    prm = _params(k, w, 0.7)
    pt = pyref_targets(_case("", "", loci, prm, [], False, common=0.0))
    al = loci[0][0]
    foreign = _rand(np.random.default_rng(230 + k), 600)
    reads, tags = [], []
    for name in TIE_FEATURES:
        f, L = feats[name]
        core = al[f - 40:f + L + 40]
        for kind, lo, hi in (("lane", 0, LANE_MAX - len(core)), ("wave", LANE_MAX + 1 - len(core), SHORT_MAX - len(core))):
            for strand in (bytes, revcomp):                                    # the leftmost-minimum rule is not symmetric: each strand has its own edge
                taken = [F for F in range(lo, hi + 1, 3) if 0 in pt.recruit(strand(core + foreign[:F]))]
                if not taken: continue
                edge = max(taken)
                for F, tag in ((edge, "edge"), (edge + 3, "over")):
                    if F <= hi: reads.append((strand(core + foreign[:F]), None)); tags.append(f"{name}/{kind}/{tag}")
        r = foreign[300:550] + core + foreign[:250]
        reads += [(r, None), (revcomp(r), None)]; tags += [f"{name}/long"] * 2
    return _case(f"ties/k{k}w{w}/boundary", "reads whose answer rests on the tied minimizers of a repeat, at the edge of match_frac", loci, prm, reads, False, tags, common=0.0)


@functools.lru_cache(maxsize=None)
def tie_cases():
    """b. Equal hashes inside a window: reads cut across repeats, both strands, both kernels; and k in 1..3 with w = 2."""
    out = []
    for k, w in ((14, 10), (16, 7)):
        loci, feats = common_loci(k, w)
        singles, tags_s, pairs, tags_p = _tie_reads(loci[0][0], feats)
        out.append(_case(f"ties/k{k}w{w}/single", "single reads across a homopolymer, repeats of period 2, 3, w and w + 1 and a run of k-mers that are their own reverse complement",
                         loci, _params(k, w), singles, False, tags_s))
        out.append(_case(f"ties/k{k}w{w}/pairs", "the same as mates", loci, _params(k, w), pairs, True, tags_p))
    out.append(_tie_boundary_case(14, 10))
    for k in (1, 2, 3):
        rng = np.random.default_rng(210 + k)
        loci = [[_rand(rng, 600)] for _ in range(3)]
        singles = [(_rand(rng, int(l)), None) for l in (2, 3, 40, 64, 150, 256, 257, 400, 501, 700)] + [(loci[1][0][50:350], None), (revcomp(loci[2][0][0:180]), None)]
        pairs = [(_rand(rng, 100 + 13 * i), _rand(rng, 256 - 17 * i)) for i in range(8)] + [(loci[0][0][10:160], revcomp(loci[0][0][300:450]))]
        out.append(_case(f"ties/k{k}w2/single", "every minimizer belongs to every locus", loci, _params(k, 2), singles, False, ["tiny_k"] * len(singles)))
        out.append(_case(f"ties/k{k}w2/pairs", "every minimizer belongs to every locus", loci, _params(k, 2), pairs, True, ["tiny_k"] * len(pairs)))
    return out


def n_variants(r, k, w):
    """[(tag, read)]: the read r with other bases at the places of class c"""
    ln, out = len(r), []
    def put(tag, pos, n=1):
        b = bytearray(r); b[pos:pos + n] = b"N" * n; out.append((tag, bytes(b)))
    put("N@0", 0); put("N@last", ln - 1); put("N@len-k", ln - k)
    for p in (31, 32, 63): put(f"N@{p}", p)
    for n in (w - 1, w, w + 1, k + w - 1): put(f"Nrun={n}", 70, n)
    out.append(("allN", b"N" * ln))
    return out


@functools.lru_cache(maxsize=None)
def other_base_cases():
    """c. Other bases at the places where the walk as written moves first_kmer and first_window, on both sides of 256 bases; a read
    that takes the walk as written stands directly before and directly after reads that take the block-wise walk."""
    k, w = 14, 10
    loci, _ = common_loci(k, w)
    al = loci[1][1]
    singles, tags_s, pairs, tags_p = [], [], [], []
    for ln in (150, 256, 300, 600):
        src = al[200:200 + ln]
        for i, (tag, r) in enumerate(n_variants(src, k, w)):
            if i % 2: r = revcomp(r)
            singles += [(r, None), (src, None)]; tags_s += [tag, "clean"]
            if ln <= LANE_MAX:
                pairs += [(r, revcomp(al[900:1050])), (al[900:1050], revcomp(r))]; tags_p += [tag + "/1", tag + "/2"]
    return [_case("other/single", "N at base 0, the last base, len - k, 31, 32, 63; runs of w - 1, w, w + 1, k + w - 1; all N; between clean reads",
                  loci, _params(k, w), singles, False, tags_s),
            _case("other/pairs", "the same reads as first and as second mates", loci, _params(k, w), pairs, True, tags_p)]


# ---- d. locus slots ----

def slot_loci(rng, n, seg_len):
    shared = _rand(rng, seg_len)
    return [[_rand(rng, 600) + shared + _rand(rng, 300)] for _ in range(n)], shared


@functools.lru_cache(maxsize=None)
def slot_cases():
    """d. A read that matches n loci at n = the number of slots and one more, max_out at n and n - 1, and what the second mate may do
    to a full table."""
    out = []
    prm = _params(15, 10)
    for kind, n_full, seg in (("pairs", MAX_LOCI_PER_READ, 400), ("short", MAX_LOCI_PER_READ, 400), ("long", LONG_LOCI, 700)):
        for n, max_out, error in ((n_full, n_full, None), (n_full + 1, n_full + 1, "UNSUPPORTED"), (n_full, n_full - 1, "INVALID_INPUT")):
            rng = np.random.default_rng(400 + n)
            loci, S = slot_loci(rng, n, seg)
            priv = loci[0][0][:600]
            if kind == "pairs":
                reads = [(S[0:150], revcomp(S[200:350])), (revcomp(S[200:350]), S[0:150]), (priv[100:250], revcomp(priv[300:450])), (S[100:250], revcomp(S[250:400]))]
                tags = ["shared", "shared", "private", "shared"]; after = [reads[2]]
            elif kind == "short":
                reads = [(S[50:250], None), (priv[100:300], None), (revcomp(S[100:356]), None)]
                tags = ["shared", "private", "shared"]; after = [reads[1]]
            else:
                reads = [(S[0:700], None), (priv[0:400], None), (revcomp(S[0:700]), None), (S[100:500], None), (priv[50:600], None), (S[0:600], None)]
                tags = ["shared", "private", "shared", "shared", "private", "shared"]; after = [reads[1], reads[4]]
            out.append(_case(f"slots/{kind}/n{n}/max_out{max_out}", f"reads of a segment shared by {n} loci, max_out {max_out}: " + (error or "answered with all of them"),
                             loci, prm, reads, kind == "pairs", tags, max_out=max_out, error=error, after=after if error else ()))
    # the first mate reaches eight loci, the second mate would reach a ninth: answered, and the ninth is not in the answer
    rng = np.random.default_rng(450)
    S1, S2 = _rand(rng, 400), _rand(rng, 400)
    loci = [[_rand(rng, 500) + S1 + _rand(rng, 200) + S2 + _rand(rng, 200)] for _ in range(8)] + [[_rand(rng, 500) + S2 + _rand(rng, 300)]]
    out.append(_case("slots/pairs/ninth_by_second_mate", "the second mate never inserts a locus, at a full table", loci, prm,
                     [(S1[0:150], revcomp(S2[100:250])), (revcomp(S1[200:350]), S2[0:150])], True, ["ninth", "ninth"], max_out=8))
    rng = np.random.default_rng(451)
    loci = [_alleles(rng, 900, 1), _alleles(rng, 900, 1)]
    A, B = loci[0][0], loci[1][0]
    out.append(_case("slots/pairs/a_then_b", "the first mate matches only locus A, the second only locus B", loci, prm,
                     [(A[100:250], revcomp(B[300:450])), (B[100:250], revcomp(A[300:450])), (A[100:250], revcomp(A[300:450]))], True, ["ab", "ab", "aa"]))
    return out


# ---- e. fractions at equality ----

MATCH_FRACS = (0.25, 0.5, 0.7, 0.3333, 1.0)
_NEXT = bytes.maketrans(b"ACGT", b"CGTA")


def eroded(read, e, from_left):
    """the read with e bases substituted from one end"""
    return read[:e].translate(_NEXT) + read[e:] if from_left else read[:len(read) - e] + read[len(read) - e:].translate(_NEXT)


def _first_equal_and_below(cmp_at, n_steps):
    """cmp_at(e) -> sign of (fraction - match_frac) after e substitutions, or None when the locus is no longer looked at. The first e
    at which it is 0 and the first later e at which it is negative; (None, last e above, first e below) if it is never 0."""
    last_above = 0
    for e in range(n_steps + 1):
        c = cmp_at(e)
        if c is None or c < 0:
            return (None, last_above, e) if e else (None, None, None)
        if c == 0:
            for e2 in range(e + 1, n_steps + 1):
                c2 = cmp_at(e2)
                if c2 is None or c2 < 0: return e, e, e2
            return None, last_above, None
        last_above = e
    return None, last_above, None


def _sign(pt, f):
    return (f[0] & 0xFFFF) * pt.mf[1] - pt.mf[0] * (f[1] & 0xFFFF)


@functools.lru_cache(maxsize=None)
def fraction_cases():
    """e. Reads whose decisive fraction for locus 0 equals match_frac exactly, and the next read of the same series, just below:
    pairs, single reads of up to 256 bases and of 257 to 500 bases (one rule in three places), both strands. Where no read can
    reach the equality (0.3333 = 3333/10000 in u16: a denominator that no read of 500 bases has) the last read above stands in."""
    out = []
    for mf in MATCH_FRACS:
        rng = np.random.default_rng(500 + int(mf * 10000))
        loci = [_alleles(rng, 1500, 2), _alleles(rng, 900, 1)]
        prm = _params(15, 10, mf)
        base = _case("", "", loci, prm, [], False)
        pt = pyref_targets(base)
        al = loci[0][0]
        for place, L in (("pair", 120), ("short", 120), ("mid", 300)):
            reads, tags = [], []
            for strand in (0, 1):
                found = None
                for p in range(100, 1000, 37):
                    src = al[p:p + L]
                    mate = al[p + 250:p + 370]
                    def build(e):
                        r = eroded(src, e, from_left=bool(strand))
                        if place == "pair": return (r, revcomp(mate)) if not strand else (revcomp(r), mate)
                        return (revcomp(r) if strand else r, None)
                    def cmp_at(e):
                        r1, r2 = build(e)
                        m1, c1 = counts_of(pt, r1)
                        if 0 not in c1: return None
                        if place == "pair":
                            m2, c2 = counts_of(pt, r2)
                            f1, f2, _ = pair_fractions(c1[0], len(m1), c2.get(0, [0] * 4), len(m2))
                            assert _sign(pt, f2) >= 0                            # the intact mate passes: the eroded one decides
                            return _sign(pt, f1)
                        return _sign(pt, short_fraction(c1[0], len(m1)))
                    eq, above, below = _first_equal_and_below(cmp_at, L - 20)
                    if below is None: continue
                    if eq is not None:
                        found = (build(eq), build(below), "equal"); break
                    if found is None: found = (build(above), build(below), "above")
                assert found is not None, (mf, place, strand)
                reads += [found[0], found[1]]; tags += [found[2], "below"]
            out.append(_case(f"fractions/mf{mf}/{place}", f"match_frac {mf}: the decisive fraction at equality and just below, both strands", loci, prm, reads, place == "pair", tags))
    out.append(_pair_choice_tie())
    return out


def _pair_choice_tie():
    """A pair for which both sums of better_pair_fraction are equal and the two choices decide differently: each mate is part forward
    strand, part reverse strand of the allele."""
    rng = np.random.default_rng(560)
    loci = [_alleles(rng, 1500, 1), _alleles(rng, 900, 1)]
    prm = _params(15, 10, 0.25)
    pt = pyref_targets(_case("", "", loci, prm, [], False))
    al = loci[0][0]
    firsts = {}
    for x1 in range(30, 121, 3):
        r1 = al[200:200 + x1] + revcomp(al[600:600 + 150 - x1])
        m1, c1 = counts_of(pt, r1)
        if 0 in c1: firsts[x1] = (r1, len(m1), c1[0])
    for x2 in range(30, 121, 3):
        r2 = al[900:900 + x2] + revcomp(al[1200:1200 + 150 - x2])
        m2, c2 = counts_of(pt, r2)
        if 0 not in c2: continue
        b, t2 = c2[0], len(m2)
        for x1, (r1, t1, a) in firsts.items():
            f1, f2, (s_fw, s_bw) = pair_fractions(a, t1, b, t2)
            if s_fw != s_bw: continue
            taken = _sign(pt, f1) >= 0 and _sign(pt, f2) >= 0
            other = _sign(pt, (_bn(a), _bd(a, t1))) >= 0 and _sign(pt, (_fn(b), _fd(b, t2))) >= 0
            if taken != other: return _case("fractions/pair_choice_tie", "forward/backward sums of better_pair_fraction equal, and the two choices decide differently",
                                            loci, prm, [(r1, r2)], True, ["choice_tie_decisive"])
    raise AssertionError("no pair with equal sums whose two choices decide differently")


# ---- f. the long-read rule ----

def _first(it):
    for x in it: return x
    return None


@functools.lru_cache(maxsize=None)
def long_rule_cases():
    """f. recruit_long_read at its four boundaries: den against stretch_minims, num against thr, the running sum against stretch_score
    (inside foreign sequence, at the read's start and end, reverse-complemented, across the lanes' pieces of the minimizer list, in
    two halves) and a read with fewer than 64 minimizers."""
    out = []
    # den just below stretch_minims and at it: most k-mers common, so den = total - (common matches) is small
    rng = np.random.default_rng(600)
    loci = [_alleles(rng, 2500, 1), _alleles(rng, 900, 1)]
    prm = _params(15, 32, 0.5)
    base = _case("", "", loci, prm, [], False, common=0.6)
    pt = pyref_targets(base)
    al = loci[0][0]
    reads, tags = [], []
    for want in (pt.stretch_minims - 1, pt.stretch_minims):
        for with_n in (False, True):
            def cand():
                for p in range(0, 1900, 7):
                    for ln in (range(501, 560, 3) if not with_n else range(120, 400, 5)):
                        r = al[p:p + ln] if not with_n else b"N" * 390 + al[p:p + ln]
                        m, c = counts_of(pt, r)
                        if 0 in c and long_terms(pt, c[0], len(m))[1] == want: return r
            r = cand()
            assert r is not None, (want, with_n)
            reads.append((r, None)); tags.append(f"den={'sm' if want == pt.stretch_minims else 'sm-1'}")
    out.append(_case("long/den", "den one below stretch_minims and at it, with and without other bases", loci, prm, reads, False, tags, common=0.6))
    # num = thr and thr - 1, for match_frac whose product with stretch_minims is an integer (w = 9: 40 minimizers) and for 0.7
    for w, mf in ((9, 0.5), (9, 0.25), (9, 0.7), (10, 0.7)):
        rng = np.random.default_rng(610 + w + int(100 * mf))
        loci = [_alleles(rng, 2500, 2), _alleles(rng, 900, 1)]
        prm = _params(15, w, mf)
        pt = pyref_targets(_case("", "", loci, prm, [], False))
        al = loci[0][0]
        reads, tags = [], []
        for strand in (0, 1):
            src = al[300 + 500 * strand:1100 + 500 * strand]
            @functools.lru_cache(maxsize=None)
            def terms(e):
                r = eroded(src, e, from_left=bool(strand))
                if strand: r = revcomp(r)
                m, c = counts_of(pt, r)
                return r, (long_terms(pt, c[0], len(m)) if 0 in c else (0, len(m), 1))
            e = 0
            while terms(e + 20)[1][0] >= terms(e + 20)[1][2]: e += 20          # coarse, then base by base
            at = _first(x for x in range(e, e + 40) if terms(x)[1][0] == terms(x)[1][2])
            below = _first(x for x in range(at, at + 40) if terms(x)[1][0] == terms(x)[1][2] - 1)
            reads += [(terms(at)[0], None), (terms(below)[0], None)]; tags += ["num=thr", "num=thr-1"]
        out.append(_case(f"long/num/w{w}mf{mf}", "rare matches at the threshold and one below", loci, prm, reads, False, tags))
    # the running sum: a matching stretch whose sum peaks at stretch_score and one short of it; islands elsewhere keep num above thr
    for name, w, layout in (("inside", 10, "iFiFsF"), ("start", 10, "sFiFiF"), ("end", 10, "iFiFs"), ("revcomp", 10, "iFiFsF"), ("few_minimizers", 20, "isF")):
        rng = np.random.default_rng(650 + len(name))
        loci = [_alleles(rng, 2500, 1), _alleles(rng, 900, 1)]
        prm = _params(15, w, 0.5)
        pt = pyref_targets(_case("", "", loci, prm, [], False))
        al = loci[0][0]
        # islands (i): matching pieces too short to reach the score; foreign parts (F) long enough for the sum to return to zero
        if name == "few_minimizers":
            foreign = [_rand(rng, 330)]; isl = [al[2000:2075] + _rand(rng, 60)]
        else:
            isl = [al[1800:1860], al[2100:2160]]; foreign = [_rand(rng, 220) for _ in range(3)]
        def build(p, L, x):
            """the stretch al[p:p + L], with base x substituted (a few minimizers lost inside: the sum moves in steps of three otherwise)"""
            st = al[p:p + L] if x is None else al[p:p + x] + al[p + x:p + x + 1].translate(_NEXT) + al[p + x + 1:p + L]
            parts, i_n, f_n = [], 0, 0
            for ch in layout:
                if ch == "s": parts.append(st)
                elif ch == "i": parts.append(isl[i_n]); i_n += 1
                else: parts.append(foreign[f_n]); f_n += 1
            r = b"".join(parts)
            return revcomp(r) if name == "revcomp" else r
        want = {pt.stretch_score: None, pt.stretch_score - 1: None}
        def look(r):
            m, c = counts_of(pt, r)
            if 0 not in c: return 0
            num, den, thr = long_terms(pt, c[0], len(m))
            peak = stretch_peak(pt, 0, m)[0]
            if peak in want and want[peak] is None and num >= thr and den >= pt.stretch_minims and len(r) > SHORT_MAX: want[peak] = r
            return peak
        for p in (100, 337, 561, 800, 1013, 1250):
            for L in range(40, 260, 2):
                peak = look(build(p, L, None))
                if peak > pt.stretch_score + 20: break                     # a substituted base costs three or four minimizers
                if peak >= pt.stretch_score - 2:
                    for x in range(16, L - 16, 7):
                        look(build(p, L, x))
                        if all(v is not None for v in want.values()): break
                if all(v is not None for v in want.values()): break
            if all(v is not None for v in want.values()): break
        assert all(v is not None for v in want.values()), name
        out.append(_case(f"long/stretch/{name}", f"a matching stretch ({name}) whose running sum peaks at stretch_score, and one that peaks one short", loci, prm,
                         [(want[pt.stretch_score], None), (want[pt.stretch_score - 1], None)], False, ["peak=score", "peak=score-1"]))
        if name == "inside":
            # two halves of the stretch with enough foreign sequence between them for the sum to return to zero
            st = want[pt.stretch_score]
            s0 = len(isl[0]) + 220 + len(isl[1]) + 220
            L = len(st) - s0 - 220
            half = L // 2
            r = st[:s0 + half] + _rand(rng, 330) + st[s0 + half:]
            out.append(_case("long/stretch/halves", "the same stretch in two halves, the sum back at zero between them", loci, prm, [(r, None), (st, None)], False, ["halves", "peak=score"]))
    return out


# ---- g. window sizes ----

WINDOWS, KS = (2, 16, 32, 33, 51, 52, 63), (5, 15, 31)


@functools.lru_cache(maxsize=None)
def window_cases():
    """g. Every w at which the ring, the LDS request or the block length changes, with small, usual and largest k: ordinary pairs,
    single reads of 100 to 256 bases and of 300 to 2 000 bases, some with other bases."""
    out = []
    for w in WINDOWS:
        for k in KS:
            rng = np.random.default_rng(700 + 64 * k + w)
            loci = [_alleles(rng, 2600, 2), _alleles(rng, 1200, 1)]
            prm = _params(k, w, 0.5)
            def cut(ln, i):
                al = loci[i % 2][0]
                p = int(rng.integers(0, len(al) - min(ln, len(al) - 1)))
                r = bytearray(al[p:p + ln]) if i % 5 != 4 else bytearray(_rand(rng, ln))
                for q in rng.integers(0, len(r), (i % 3) * len(r) // 50): r[int(q)] = b"ACGT"[int(rng.integers(0, 4))]
                if i % 7 == 3: r[len(r) // 2] = ord("N")
                return revcomp(bytes(r)) if i % 2 else bytes(r)
            pairs = [(cut(int(rng.integers(100, 251)), i), revcomp(cut(int(rng.integers(100, 251)), i))) for i in range(24)]
            singles = [(cut(int(rng.integers(100, 257)), i), None) for i in range(22)] + [(cut(int(l), i), None) for i, l in enumerate((300, 480, 500, 501, 640, 900, 1100, 1500, 2000, 1234, 777, 333))]
            out.append(_case(f"windows/w{w}k{k}/pairs", f"w = {w}, k = {k}", loci, prm, pairs, True))
            out.append(_case(f"windows/w{w}k{k}/single", f"w = {w}, k = {k}", loci, prm, singles, False))
    return out


# ---- the turn tests: many turns of one workgroup ----

@functools.lru_cache(maxsize=None)
def turn_cases():
    """About 200 pairs of classes a to c shuffled together, and about 40 single reads beyond 256 bases on 16 loci: reads with other
    bases between reads without, on both sides of 500 bases, and reads that match all 16 loci."""
    loci, _ = common_loci(14, 10)
    pairs = [r for c in length_cases() + tie_cases()[:2] + other_base_cases() if c.paired and c.error is None and c.params == _params(14, 10) for r in c.reads]
    rng = np.random.default_rng(800)
    pairs = [pairs[int(i)] for i in rng.permutation(len(pairs))][:200]
    rng = np.random.default_rng(801)
    loci16, S = slot_loci(rng, LONG_LOCI, 700)
    reads, tags = [], []
    for i in range(40):
        priv = loci16[i % LONG_LOCI][0]
        if i % 4 == 0: r, tag = S[(i * 3) % 100:(i * 3) % 100 + (560 if i % 8 else 420)], "shared"
        else: r, tag = priv[i:i + 300 + 37 * (i % 9)], "private"
        if i % 3 == 1: b = bytearray(r); b[40 + i:43 + i] = b"NNN"; r, tag = bytes(b), tag + "/N"
        reads.append((revcomp(r) if i % 2 else r, None)); tags.append(tag)
    return [_case("turns/pairs", "pairs of classes a to c shuffled", loci, _params(14, 10), pairs, True),
            _case("turns/long", "single reads beyond 256 bases on 16 loci", loci16, _params(15, 10), reads, False, tags, max_out=LONG_LOCI)]


def all_cases():
    return length_cases() + tie_cases() + other_base_cases() + slot_cases() + fraction_cases() + long_rule_cases() + window_cases() + turn_cases()
