"""The designed pairs of the scoring hand-offs (tests/score_route_cases.py) on the CPU: tests/pyref.py, which follows the reference's
PrelimAlignments::push and _read_next_alns, counts the saved alignments of every (read end, contig) group of every pair. Each case
must hold the group sizes, bins, ties and mate lengths it names, and the route a pair is expected to take is derived from those
counts alone (route_from_facts): a case cannot turn into something the lean kernel takes anyway without a test here failing. The
GPU tests (tests/test_gpu_score_routes.py) hold the kernels against the same expectations."""
import ctypes as C

import pytest

from locityper_amd import api, cdefs
from tests import oracle_ffi as O
from tests import pyref
from tests import score_route_cases as SC
from tests.helpers import locus_arrays


def walk_locus(D):
    p = api.resolve_params(api.default_params(), D.bg)

    def edit_thr(rl):
        g, q = C.c_uint32(), C.c_uint32()
        O.lib().orc_edit_thresholds(C.byref(D.bg), rl, C.byref(g), C.byref(q))
        return g.value, q.value
    return SC.WalkLocus(D.alleles, D.k, D.bg, p, edit_thr), p, edit_thr


def facts_of(D, pairs):
    L, _, _ = walk_locus(D)
    return [SC.walk(L, q) for q in pyref._decode_chunk(SC.chunk_of(pairs))]


@pytest.fixture(scope="module")
def facts():
    return {(D.key, name): facts_of(D, pairs) for D in SC.designs() for name, pairs in D.cases.items()}


def test_constants_are_the_shared_ones():
    assert (SC.LEAN, SC.TWO, SC.GENERAL) == (cdefs.ROUTE_LEAN, cdefs.ROUTE_TWO, cdefs.ROUTE_GENERAL)
    assert SC.keep_runs(309) and not SC.keep_runs(310)                          # 309 * 33 + 16 = 10 213, 310 * 33 + 16 = 10 246
    assert SC.two_runs(309) and not SC.two_runs(309, ("score_lean_two",)) and not SC.two_runs(309, ("score_lean_keep",))
    assert C.sizeof(cdefs.ScoreRoutes) == 4 * 8 + 2 * 4 + 8
    keys = [D.key for D in SC.designs()]
    assert len(set(keys)) == len(keys) and {f"alleles-{n}" for n in (63, 64, 65, 128, 129, 309, 310)} <= set(keys)


@pytest.mark.parametrize("key,name", SC.case_ids())
def test_every_pair_is_what_it_names(facts, key, name):
    """Group sizes as designed, and the designed route is the one the counts give."""
    D = SC.design(key)
    pairs = D.cases[name]
    assert 0 < len(pairs) <= 80
    for r, (q, f) in enumerate(zip(pairs, facts[key, name])):
        got = {g: len(v) for g, v in f["groups"].items()}
        assert got == q["sizes"], (r, q["why"], got)
        assert f["n_recs"] == len(q["recs"]) and all(c < D.n_alleles for c, _, _, _ in q["recs"])
        assert SC.route_from_facts(f, D.n_alleles, D.k) == q["route"], (r, q["why"])
        if q["sizes"]:
            assert f["look"] and f["ok"], (r, q["why"])                          # a designed pair is well mapped unless it says not
        # under the knobs the routes fold: nothing but the general kernel; no two-slot form
        assert SC.route_from_facts(f, D.n_alleles, D.k, ("score_lean",)) == SC.GENERAL
        for knob in ("score_lean_two", "score_lean_keep"):
            assert SC.route_from_facts(f, D.n_alleles, D.k, (knob,)) == (SC.LEAN if q["route"] == SC.LEAN else SC.GENERAL)


@pytest.mark.parametrize("key", [D.key for D in SC.designs()])
def test_designed_pairs_are_scored(key):
    """By the oracle most pairs of a case are good pairs, some of every route: the routes are about pairs whose products count."""
    import numpy as np
    D = SC.design(key)
    _, p, _ = walk_locus(D)
    seqs, seq_off, cflat, cnt_off, _ = locus_arrays(D.alleles, D.k, D.counts)
    ol = O.OracleLocus(seqs, seq_off, cflat, cnt_off, D.k, D.bg, p)
    for name, pairs in D.cases.items():
        oa = ol.load(SC.chunk_of(pairs))
        good = oa.status == cdefs.READ_GOOD
        routes = np.array([q["route"] for q in pairs])
        assert good.sum() * 2 >= len(pairs) and all((good & (routes == r)).any() for r in set(routes.tolist())), name
        assert int(oa.pa_off[-1]) > len(pairs) // 2


def test_group_size_cases(facts):
    D = SC.design("small")
    pairs, fs = D.cases["group sizes"], facts["small", "group sizes"]
    seen = set()
    for q, f in zip(pairs, fs):
        multi = {g: n for g, n in q["sizes"].items() if n > 1}
        seen.add((tuple(sorted(e for e, _ in multi)), max(q["sizes"].values(), default=0), q["route"]))
    # 2 and 3 on end 0, on end 1 and on both (2 x 2 in registers), each with its route
    for ends in ((0,), (1,), (0, 1)):
        assert (ends, 2, SC.TWO) in seen and (ends, 3, SC.GENERAL) in seen
    assert ((), 1, SC.LEAN) in seen
    unsaved = [(q, f) for q, f in zip(pairs, fs) if "not saved" in q["why"] and "one of them" in q["why"]]
    assert unsaved and all(len(f["unsaved"]) == 1 and f["unsaved"][0]["edit"] > f["passable"][0] and q["route"] == SC.LEAN for q, f in unsaved)
    blind = [(q, f) for q, f in zip(pairs, fs) if "first primary not saved" in q["why"]]
    assert blind
    for q, f in blind:
        assert not f["look"] and q["route"] == SC.LEAN
        doubled = {}
        for c, _, fl, cig in q["recs"][1:]:                                      # on paper its groups are doubled
            if "20X" not in cig:
                doubled[(bool(fl & cdefs.FLAG_MATE2), c)] = doubled.get((bool(fl & cdefs.FLAG_MATE2), c), 0) + 1
        assert max(doubled.values()) >= 2
    mixed = [q for q in pairs if "a third alignment" in q["why"]]
    assert mixed and all(sorted(q["sizes"].values())[-2:] == [2, 3] and q["route"] == SC.GENERAL for q in mixed)
    single = SC.design("small-single-end")
    assert not single.paired and {q["route"] for q in single.cases["group sizes"]} == {SC.LEAN, SC.TWO, SC.GENERAL}
    assert all(e == 0 for q in single.cases["group sizes"] for e, _ in q["sizes"])


@pytest.mark.parametrize("key", ["small", "small-single-end"])
def test_inside_a_doubled_group(facts, key):
    D = SC.design(key)
    pairs, fs = D.cases["inside a doubled group"], facts[key, "inside a doubled group"]
    seen = set()
    for q, f in zip(pairs, fs):
        a, b = f["groups"][q["group"]]                                           # in record order
        assert a["rec_ix"] < b["rec_ix"] and q["route"] == SC.TWO
        assert ((a["start"] >> 7) == (b["start"] >> 7)) == q["one_bin"]
        assert (a["ln_prob"] == b["ln_prob"]) == q["tie"]
        assert (a["ln_prob"] > b["ln_prob"]) == q["better_first"]
        assert (a["rev"] != b["rev"]) == q["strands_differ"]
        seen.add((q["group"][0], q["one_bin"], q["tie"], q["better_first"], q["strands_differ"], tuple(sorted((a["start"] & 127, b["start"] & 127)))))
    ends = (0, 1) if D.paired else (0,)
    for e in ends:
        mine = {s[1:] for s in seen if s[0] == e}
        for one_bin in (True, False):
            assert any(s[0] == one_bin and s[1] for s in mine)                                                # a tie in one bin and in two
            assert any(s[0] == one_bin and not s[1] and s[2] for s in mine) and any(s[0] == one_bin and not s[1] and not s[2] for s in mine)
        assert any(s[4] == (0, 127) and not s[0] for s in mine)                                              # starts at 127 and 128
        assert any(s[3] for s in mine)
    assert len(pairs) == 12 * len(ends)                                          # every arrangement in both record orders


def test_pass1_trip_cases(facts):
    for n in (309, 310):
        D = SC.design(f"alleles-{n}")
        pairs, fs = D.cases["pass-1 trips"], facts[D.key, "pass-1 trips"]
        n_eff = [f["n_recs"] for f in fs]
        assert n_eff[:2] == [SC.TRIP, SC.TRIP + 1] and max(n_eff) >= 400
        for q, f in zip(pairs, fs):
            per_allele = {}
            for c, _, fl, _ in q["recs"]:
                per_allele[(bool(fl & cdefs.FLAG_MATE2), c)] = per_allele.get((bool(fl & cdefs.FLAG_MATE2), c), 0) + 1
            if "group" not in q:
                assert f["n_recs"] > SC.TRIP and set(per_allele.values()) == {1} and q["route"] == SC.LEAN
                continue
            a, b = f["groups"][q["group"]]
            assert (a["rec_ix"], b["rec_ix"]) == (q["first_ix"], q["second_ix"])
            assert a["rec_ix"] < 64 or "16-bit" in q["why"]                      # the first in the first 64 records, the second in a later trip
            assert sorted(per_allele.values())[-2:] == [1, 2] and q["route"] == (SC.TWO if n == 309 else SC.GENERAL)
        second = [q["second_ix"] for q in pairs if "group" in q]
        assert second[0] == SC.TRIP - 1 and second[1] == SC.TRIP and 300 <= max(second) < 65535 and sorted(second)[-2] >= SC.TRIP
        assert {q["group"][0] for q in pairs if "group" in q} == {0, 1}


def test_lean_ovf_cases(facts):
    D = SC.design("ovf-70")
    got = []
    for q, f in zip(D.cases["LEAN_OVF"], facts["ovf-70", "LEAN_OVF"]):
        sizes = [len(g) for g in f["groups"].values()]
        assert sum(n >= 2 for n in sizes) == q["doubled"]
        got.append((sum(n >= 2 for n in sizes), max(sizes), q["route"]))
    assert (64, 2, SC.TWO) in got and (65, 2, SC.GENERAL) in got and (63, 2, SC.TWO) in got
    assert (64, 3, SC.GENERAL) in got and (65, 3, SC.GENERAL) in got
    assert sum(1 for g in got if g == (64, 2, SC.TWO)) == 2 and sum(1 for g in got if g == (65, 2, SC.GENERAL)) == 2


@pytest.mark.parametrize("key", ["mates-paired-0", "mates-paired-1", "mates-single-0"])
def test_mate_length_cases(facts, key):
    """Lengths and routes as named; the last k-mer window of every read is a unique k-mer of the locus, and the twins with an N lose
    exactly the unique k-mers whose windows hold the N: the counts depend on the last word of the mate and its mask."""
    D = SC.design(key)
    pairs, fs = D.cases["mate lengths"], facts[key, "mate lengths"]
    long_end = 1 if key.endswith("-1") else 0
    assert sorted({q["mate_len"] for q in pairs}) == sorted(SC.MATE_LENGTHS) and {20, 31, 32, 33, 63, 64, 65, 1985, 2015, 2016, 2017} <= set(SC.MATE_LENGTHS)
    for q, f in zip(pairs, fs):
        assert f["len"][long_end] == q["mate_len"] and (not D.paired or f["len"][1 - long_end] == SC.RL)
        assert q["route"] == (SC.LEAN if q["mate_len"] <= 2016 else SC.GENERAL)
    # the unique-k-mer counts, by pyref's load on the whole locus (k-mers and all)
    _, p, edit_thr = walk_locus(D)
    seqs, seq_off, cflat, cnt_off, counts = locus_arrays(D.alleles, D.k, D.counts)
    ol = O.OracleLocus(seqs, seq_off, cflat, cnt_off, D.k, D.bg, p)
    L = pyref.PyLocus(D.alleles, counts, D.k, D.bg, p, ol.insert_lnprob if D.paired else (lambda sz: 0.0),
                      ol.insert_penalty() if D.paired else float("nan"), edit_thr)
    uk = {}
    for q in pairs:
        seq = (q["seq2"] if long_end else q["seq1"]).encode()
        km = pyref.kmers(seq, D.k)
        hits = [i for i, x in enumerate(km) if x in L.unique]
        cnt, i = 0, 0
        while i < len(km):                                                       # locs.rs:968-1002: a hit skips the next k - 1 windows
            if km[i] in L.unique:
                cnt += 1; i += D.k
            else:
                i += 1
        uk[q["mate_len"], q["twin"]] = (cnt, hits)
    for n in SC.MATE_LENGTHS:
        base, hits = uk[n, "as it is"]
        if n < D.k:
            assert base == 0
            continue
        assert hits == SC.unique_windows(n, D.k) and hits[-1] == n - D.k and base == len(hits)      # the last window is a unique k-mer, and counted
        last, _ = uk[n, "N in the last base"]
        assert last == base - 1                                                  # only the last window holds the last base
        ats = sorted(q["n_at"] for q in pairs if q["mate_len"] == n and q["n_at"] not in (None, n - 1))
        assert ats == ([b for b in (31, 32, 63) if b < n - 1] or [n // 2])
        for at in ats:
            inner, inner_hits = uk[n, f"N in base {at}"]
            lost = [w for w in hits if w <= at < w + D.k]
            assert inner == base - len(lost) and inner_hits == [w for w in hits if w not in lost]
            if n >= 1985 or (n, at) in ((33, 31), (65, 63)):
                assert len(lost) == 1                                            # the N sits in a unique window: that word's mask decides
    # and pyref's whole load agrees with that count, twin by twin
    res = pyref.load(L, SC.chunk_of(pairs))
    for q, (status, weight, unm, uks, pa) in zip(pairs, res):
        want = uk[q["mate_len"], q["twin"]][0]
        if status in (cdefs.READ_GOOD, cdefs.READ_FEW_KMERS):
            assert uks[long_end] == want, q["why"]
    assert sum(1 for r in res if r[0] == cdefs.READ_GOOD) >= len(pairs) // 2


def test_allele_count_designs():
    for n in SC.ALLELE_COUNTS:
        D = SC.design(f"alleles-{n}")
        pairs = D.cases["group sizes"]
        on = {c for q in pairs for (e, c), k in q["sizes"].items() if k > 1}
        assert {0, n - 1} <= on and (n <= 63 or 63 in on) and (n <= 64 or 64 in on)
        routes = {q["route"] for q in pairs}
        assert routes == ({SC.LEAN, SC.TWO, SC.GENERAL} if n <= 309 else {SC.LEAN, SC.GENERAL})
        assert SC.lean_form(n, D.k) == (cdefs.LEAN_FORM_KEEP if n <= 309 else cdefs.LEAN_FORM_INDEX)
    D = SC.design("k41")
    assert D.k == 41 and all(q["route"] == SC.GENERAL for q in D.cases["k = 41"]) and SC.lean_form(5, 41) == cdefs.LEAN_FORM_NONE
