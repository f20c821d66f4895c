"""The designed recruitment cases (tests/recruit_cases.py) on the CPU: every case has the shape it claims, read off the restatement's
own output (tests/pyref_recruit.py), and the restatement and the oracle — two independent transliterations of the reference — agree
on every read of every case. The device is held against the oracle in tests/test_gpu_recruit_designed.py."""
import functools
import math

import numpy as np
import pytest

from tests import oracle_ffi as O
from tests import pyref_recruit as PR
from tests import recruit_cases as RC


def oracle_targets(case):
    ot = O.OracleTargets(**case.params)
    for alleles, counts in zip(case.loci, RC.case_counts(case)):
        seqs = np.frombuffer(b"".join(alleles), dtype=np.uint8)
        seq_off = np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64)
        cnt_off = np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64)
        ot.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, RC.BASE_K)
    ot.finalize()
    return ot


@functools.lru_cache(maxsize=None)
def _pt(name):
    return RC.pyref_targets(_by_name()[name])


@functools.lru_cache(maxsize=None)
def _by_name():
    cases = RC.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    return {c.name: c for c in cases}


def _named(prefix):
    return [c for n, c in _by_name().items() if n.startswith(prefix)]


def _facts(case, i):
    """(pt, minimizers of mate 1, counts of mate 1, minimizers of mate 2, counts of mate 2)"""
    pt = _pt(case.name)
    r1, r2 = case.reads[i]
    m1, c1 = RC.counts_of(pt, r1)
    m2, c2 = RC.counts_of(pt, r2) if r2 is not None else ([], {})
    return pt, m1, c1, m2, c2


def _answer(case, i):
    return _pt(case.name).recruit(*case.reads[i])


# ---- the two references agree, read by read ----

GROUPS = ("lengths/", "ties/", "other/", "slots/", "fractions/", "long/", "turns/") + tuple(f"windows/w{w}k" for w in RC.WINDOWS)


@pytest.mark.parametrize("prefix", GROUPS)
def test_restatement_and_oracle_agree_on_every_read(prefix):
    cases = _named(prefix)
    assert cases
    for case in cases:
        pt, ot = _pt(case.name), oracle_targets(case)
        assert ot.entries() == sorted((m, l, d, r) for m, v in pt.minim_to_loci.items() for l, d, r in v), case.name
        for i, (r1, r2) in enumerate(case.reads + case.after):
            assert ot.recruit(r1, r2) == pt.recruit(r1, r2), (case.name, i)
            assert O.canon_minimizers(bytearray(r1), pt.k, pt.w) == PR.canon_minimizers(r1, pt.k, pt.w), (case.name, i)


# ---- shapes ----

def test_lengths_are_the_switching_lengths_and_the_cut_reads_recruit():
    k, w = 14, 10
    single = _by_name()["lengths/single"]
    lens = {len(r) for r, _ in single.reads}
    assert lens == {0, k - 1, k, k + w - 2, k + w - 1, k + w, 31, 32, 33, 63, 64, 65, 255, 256, 257, 499, 500, 501, 502}
    for i, (r, _) in enumerate(single.reads):
        ans = _answer(single, i)
        if len(r) < k + w - 1: assert ans == [] and PR.canon_minimizers(r, k, w) == []
        if single.tags[i].startswith("switch="):                              # the rule decides, not the read
            assert ans == ([] if len(r) <= RC.SHORT_MAX else [1]), (i, len(r))
            pt, m, c, _, _ = _facts(single, i)
            assert RC._sign(pt, RC.short_fraction(c[1], len(m))) < 0
        elif len(r) >= 63: assert 1 in ans, (i, len(r))                      # cut from locus 1
    pairs = _by_name()["lengths/pairs"]
    both = {(len(a), len(b)) for a, b in pairs.reads}
    for l in RC.short_lengths(k, w): assert {(l, 150), (150, l), (l, l)} <= both
    assert (256, 256) in both and _answer(pairs, pairs.tags.index("mates=256+256")) == [1]
    # a second mate that is missing or too short for a window has no minimizers beside a first mate that matches
    for l in (0, k - 1, k + w - 2):
        i = pairs.tags.index(f"mates=150+{l}")
        pt, m1, c1, m2, c2 = _facts(pairs, i)
        assert 1 in c1 and m2 == []
    for n in (1, 63, 64, 65):
        c = _by_name()[f"lengths/chunk{n}"]
        assert len(c.reads) == n and len({len(a) for a, _ in c.reads}) == n and len({len(b) for _, b in c.reads}) == n
        assert len({len(PR.canon_minimizers(a, k, w)) for a, _ in c.reads}) > min(n, 10) // 2       # lanes with different counts
        assert sum(bool(_answer(c, i)) for i in range(n)) >= (n + 1) // 2
    for name in ("lengths/pair_257_first", "lengths/pair_257_second"):
        c = _by_name()[name]
        assert c.error == "UNSUPPORTED" and max(max(len(a), len(b)) for a, b in c.reads) == 257 and _pt(name).recruit(*c.after[0]) == [1]


def test_tie_reads_hold_equal_hashes_inside_a_window():
    for k, w in ((14, 10), (16, 7)):
        loci, feats = RC.common_loci(k, w)
        al = loci[0][0]
        h = RC.kmer_hashes(al, k)
        for name, period in (("period_w", w), ("period_w1", w + 1)):
            f, L = feats[name]
            assert L >= 3 * w + k and all(h[t] == h[t + period] for t in range(f, f + L - k + 1 - period))
        for kind in ("single", "pairs"):
            case = _by_name()[f"ties/k{k}w{w}/{kind}"]
            lens = set()
            for name in RC.TIE_FEATURES:
                idx = [i for i, t in enumerate(case.tags) if t == name]
                assert idx
                for i in idx:
                    r = case.reads[i][0]
                    lens.add(len(r))
                    if name in ("homopolymer", "period2", "period3", "self_rc"):
                        assert RC.tied_windows(r, k, w) >= 10, (case.name, name, i)   # the window really holds equal hashes
                    else:
                        f, L = feats[name]
                        assert al[f:f + 2 * w + k] in r or RC.revcomp(al[f:f + 2 * w + k]) in r or al[f + L - 2 * w - k:f + L] in r or RC.revcomp(al[f + L - 2 * w - k:f + L]) in r
                assert any(_answer(case, i) for i in idx), (case.name, name)
            if kind == "single": assert min(lens) <= RC.LANE_MAX < max(lens) and max(lens) > RC.SHORT_MAX     # both kernels, both rules
    # reads that stand or fall with the tied minimizers
    case = _by_name()["ties/k14w10/boundary"]
    for name in ("homopolymer", "period2", "period3", "self_rc"):
        assert f"{name}/wave/edge" in case.tags and f"{name}/lane/edge" in case.tags and f"{name}/long" in case.tags
    assert sum(t.endswith("/over") for t in case.tags) >= 8
    for i, tag in enumerate(case.tags):
        r = case.reads[i][0]
        name, kind = tag.split("/")[0], tag.split("/")[1]
        assert {"lane": len(r) <= RC.LANE_MAX, "wave": RC.LANE_MAX < len(r) <= RC.SHORT_MAX, "long": len(r) > RC.SHORT_MAX}[kind]
        if name in ("homopolymer", "period2", "period3", "self_rc"): assert RC.tied_windows(r.replace(b"N", b"A"), 14, 10) >= 10
        if kind == "long" and name.startswith("period_w"): continue              # one minimizer per period: too few for the long-read rule either way
        assert (0 in _answer(case, i)) == (not tag.endswith("/over")), (i, tag)
    f, L = RC.common_loci(14, 10)[1]["self_rc"]
    s = RC.common_loci(14, 10)[0][0][0][f:f + L]
    assert all(RC.revcomp(s[i:i + 14]) == s[i:i + 14] for i in range(L - 13))
    for k in (1, 2, 3):
        for kind in ("single", "pairs"):
            case = _by_name()[f"ties/k{k}w2/{kind}"]
            pt = _pt(case.name)
            n_tied = 0
            for i, (r1, r2) in enumerate(case.reads):
                for _, minim, _ in PR.canon_minimizers(r1, k, 2):
                    assert {e[0] for e in pt.minim_to_loci[minim]} == {0, 1, 2}   # every minimizer belongs to every locus
                n_tied += len(r1) >= 40 and RC.tied_windows(r1, k, 2) > 0
            assert n_tied >= len(case.reads) // 2


def test_other_bases_stand_where_the_case_says():
    k, w = 14, 10
    case = _by_name()["other/single"]
    assert {len(r) for r, _ in case.reads} == {150, 256, 300, 600}
    for i, ((r, _), tag) in enumerate(zip(case.reads, case.tags)):
        if tag == "clean":
            assert b"N" not in r and b"N" in case.reads[i - 1][0]                 # a block-wise read directly after one as written
            if i + 1 < len(case.reads): assert b"N" in case.reads[i + 1][0]       # ... and directly before the next
            continue
        ns = [j for j, c in enumerate(r if i // 2 % 11 % 2 == 0 else r[::-1]) if c == ord("N")]        # every second variant is reverse-complemented
        ln = len(r)
        want = {"N@0": [0], "N@last": [ln - 1], "N@len-k": [ln - k], "N@31": [31], "N@32": [32], "N@63": [63], "allN": list(range(ln))}
        for n in (w - 1, w, w + 1, k + w - 1): want[f"Nrun={n}"] = list(range(70, 70 + n))
        assert ns == want[tag], (i, tag)
        if tag == "allN": assert _answer(case, i) == []
    assert sum(bool(_answer(case, i)) for i in range(len(case.reads))) > len(case.reads) // 2
    pairs = _by_name()["other/pairs"]
    assert all((b"N" in a) != (b"N" in b) for a, b in pairs.reads)


def test_slot_cases_fill_the_table_and_go_one_over():
    for kind, n_full in (("pairs", 8), ("short", 8), ("long", 16)):
        for n, max_out, error in ((n_full, n_full, None), (n_full + 1, n_full + 1, "UNSUPPORTED"), (n_full, n_full - 1, "INVALID_INPUT")):
            case = _by_name()[f"slots/{kind}/n{n}/max_out{max_out}"]
            assert case.error == error and len(case.loci) == n and case.max_out == max_out
            for i, tag in enumerate(case.tags):
                pt, m1, c1, m2, c2 = _facts(case, i)
                if tag == "shared":
                    assert sorted(c1) == list(range(n))                           # the read really matches n loci
                    assert _answer(case, i) == list(range(n))
                    if kind == "long": assert len(case.reads[i][0]) > RC.LANE_MAX
                    else: assert len(case.reads[i][0]) <= RC.LANE_MAX
                else:
                    assert _answer(case, i) == [0]
            if kind == "long": assert {len(r) > RC.SHORT_MAX for (r, _), t in zip(case.reads, case.tags) if t == "shared"} == {True, False}
            for r in case.after: assert _pt(case.name).recruit(*r) == [0]
    case = _by_name()["slots/pairs/ninth_by_second_mate"]
    for i in range(len(case.reads)):
        pt, m1, c1, m2, c2 = _facts(case, i)
        assert sorted(c1) == list(range(8)) and sorted(c2) == list(range(9)) and _answer(case, i) == list(range(8))
    case = _by_name()["slots/pairs/a_then_b"]
    for i, want in enumerate(([], [], [0])):
        pt, m1, c1, m2, c2 = _facts(case, i)
        assert len(c1) == 1 and len(c2) == 1 and (list(c1) != list(c2)) == (want == []) and _answer(case, i) == want


def test_fractions_sit_on_match_frac_and_just_below():
    for mf in RC.MATCH_FRACS:
        for place in ("pair", "short", "mid"):
            case = _by_name()[f"fractions/mf{mf}/{place}"]
            pt = _pt(case.name)
            assert len(case.reads) == 4
            for i, tag in enumerate(case.tags):
                pt, m1, c1, m2, c2 = _facts(case, i)
                ln = len(case.reads[i][0])
                assert {"pair": ln <= 256, "short": ln <= 256, "mid": 256 < ln <= 500}[place]
                if place == "pair":
                    f1, f2, _ = RC.pair_fractions(c1.get(0, [0] * 4), len(m1), c2.get(0, [0] * 4), len(m2))
                    assert RC._sign(pt, f2) >= 0
                    sign = RC._sign(pt, f1) if 0 in c1 else -1
                else:
                    sign = RC._sign(pt, RC.short_fraction(c1[0], len(m1))) if 0 in c1 else -1
                if tag == "equal": assert sign == 0 and 0 in _answer(case, i)    # the fraction really is equal
                elif tag == "above": assert sign > 0 and 0 in _answer(case, i)
                else: assert sign < 0 and 0 not in _answer(case, i)
            # equality is kept wherever a read of up to 500 bases can reach it: d <= 3 * total < 1 500
            if pt.mf[1] < 1500 // pt.mf[0] or mf in (0.25, 0.5, 0.7, 1.0): assert case.tags == ["equal", "below"] * 2, case.name
            else: assert pt.mf == (3333, 10000) and case.tags == ["above", "below"] * 2
    case = _by_name()["fractions/pair_choice_tie"]
    pt, m1, c1, m2, c2 = _facts(case, 0)
    f1, f2, (s_fw, s_bw) = RC.pair_fractions(c1[0], len(m1), c2[0], len(m2))
    assert s_fw == s_bw and s_fw > 0                                          # the choice really is a tie ...
    a, b = c1[0], c2[0]
    taken = RC._sign(pt, f1) >= 0 and RC._sign(pt, f2) >= 0
    other = RC._sign(pt, (RC._bn(a), RC._bd(a, len(m1)))) >= 0 and RC._sign(pt, (RC._fn(b), RC._fd(b, len(m2)))) >= 0
    assert taken != other and (0 in _answer(case, 0)) == taken                # ... and the answer depends on it


def test_long_rule_cases_sit_on_their_boundaries():
    case = _by_name()["long/den"]
    pt = _pt(case.name)
    seen = set()
    for i, tag in enumerate(case.tags):
        pt, m, c, _, _ = _facts(case, i)
        num, den, thr = RC.long_terms(pt, c[0], len(m))
        assert len(case.reads[i][0]) > RC.SHORT_MAX and den == pt.stretch_minims - (tag == "den=sm-1")
        seen.add((tag, b"N" in case.reads[i][0]))
    assert len(seen) == 4
    for w, mf in ((9, 0.5), (9, 0.25), (9, 0.7), (10, 0.7)):
        case = _by_name()[f"long/num/w{w}mf{mf}"]
        pt = _pt(case.name)
        if w == 9: assert pt.stretch_minims == 40                             # 40 * 0.5, 40 * 0.25 are integers, 40 * 0.7 is 28 in exact arithmetic
        for i, tag in enumerate(case.tags):
            pt, m, c, _, _ = _facts(case, i)
            num, den, thr = RC.long_terms(pt, c[0], len(m))
            assert den >= pt.stretch_minims and thr == max(1, math.ceil(pt.stretch_minims * mf))
            assert num == thr - (tag == "num=thr-1")
            if tag == "num=thr-1": assert 0 not in _answer(case, i)
            else: assert (0 in _answer(case, i)) == pt._stretch(0, m)
        assert any(0 in _answer(case, i) for i, t in enumerate(case.tags) if t == "num=thr")
    for name in ("inside", "start", "end", "revcomp", "few_minimizers", "halves"):
        case = _by_name()[f"long/stretch/{name}"]
        for i, tag in enumerate(case.tags):
            pt, m, c, _, _ = _facts(case, i)
            num, den, thr = RC.long_terms(pt, c[0], len(m))
            peak, first, at = RC.stretch_peak(pt, 0, m)
            assert len(case.reads[i][0]) > RC.SHORT_MAX and num >= thr and den >= pt.stretch_minims      # the stretch alone decides
            assert (peak >= pt.stretch_score) == pt._stretch(0, m) == (0 in _answer(case, i))
            if tag == "peak=score": assert peak == pt.stretch_score
            elif tag == "peak=score-1": assert peak == pt.stretch_score - 1
            else: assert tag == "halves" and pt.stretch_score // 2 - 3 <= peak < pt.stretch_score
            per = (len(m) + 63) // 64                                            # a lane's piece of the minimizer list
            if name in ("inside", "revcomp") and tag == "peak=score": assert first // per != at // per and at - first >= 2 * per   # crosses piece boundaries
            if name == "few_minimizers": assert len(m) < 64
        if name == "start": assert RC.stretch_peak(_pt(case.name), 0, _facts(case, 0)[1])[1] <= 1
        if name == "end": assert RC.stretch_peak(_pt(case.name), 0, _facts(case, 0)[1])[2] >= len(_facts(case, 0)[1]) - 2


def test_window_cases_cover_every_ring_and_both_kernels():
    for w in RC.WINDOWS:
        for k in RC.KS:
            p, s = _by_name()[f"windows/w{w}k{k}/pairs"], _by_name()[f"windows/w{w}k{k}/single"]
            assert p.params["w"] == w and p.params["k"] == k and len(p.reads) + len(s.reads) >= 55
            lens = [len(r) for r, _ in s.reads]
            assert min(lens) <= 256 and any(256 < l <= 500 for l in lens) and max(lens) >= 1500
            assert any(b"N" in a for a, _ in p.reads) and any(b"N" in a for a, _ in s.reads)
            assert sum(bool(_answer(s, i)) for i in range(len(s.reads))) >= 8 and sum(bool(_answer(p, i)) for i in range(len(p.reads))) >= 4


def test_turn_cases_mix_what_a_workgroup_carries():
    pairs, long = _by_name()["turns/pairs"], _by_name()["turns/long"]
    assert 150 <= len(pairs.reads) <= 200
    assert sum(b"N" in a or b"N" in b for a, b in pairs.reads) >= 20
    assert len(long.reads) == 40 and all(len(r) > RC.LANE_MAX for r, _ in long.reads)
    has_n = [b"N" in r for r, _ in long.reads]
    assert any(has_n[i] and not has_n[i - 1] and not has_n[i + 1] for i in range(1, 39))        # other bases between reads without
    assert {len(r) > RC.SHORT_MAX for r, _ in long.reads} == {True, False}
    n16 = 0
    for i, tag in enumerate(long.tags):
        if tag.startswith("shared"):
            assert sorted(_facts(long, i)[2]) == list(range(16))
            n16 += _answer(long, i) == list(range(16))
    assert n16 >= 5
