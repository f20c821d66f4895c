"""CPU-side checks of the transitive haplotype alignments: the designed families of tests/transitive_cases.py cover the branches they
were designed for (asserted on the transliteration's output, so a case cannot silently stop covering its branch), the transliteration
tests/pyref_transitive.py is sound on them (every CIGAR consumes both sequences, '=' runs are equal bases, 'X' runs unequal, the score is
calculate_score), transitive_div 0 is align_multik pair for pair, and the header, cdefs.py and the library agree on the new structs."""
import ctypes as C
import functools
import os
import re

import pytest

from locityper_amd import _lib, api, cdefs
from tests import pyref_align as R
from tests import pyref_transitive as T
from tests import transitive_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in TC.cases()]
LEVEL_NAMES = [c.name for c in TC.level_cases()]


def trace_routes(name, phases):
    return {r for p, r, _, _ in TC.expected(name)["events"]["trace"] if p in phases}


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_sizes_are_the_designed_ones():
    for c in TC.cases():
        assert 6 <= len(c.seqs) <= 9 and all(600 <= len(s) <= 2100 for s in c.seqs), c.name
        assert len(c.pairs) >= 21 or c.name == "fifteen"
    assert len(TC.by_name("fifteen").pairs) == 15
    assert TC.by_name("anchor101").anchor == 101 == api.align_tr_params().transitive_anchor


def test_routes_and_directions_are_covered():
    routes, dirs = set(), set()
    for n in NAMES:
        e = TC.expected(n)
        routes |= set(e["route"]); dirs |= e["events"]["dirs"]
    assert routes == {0, 1, 2, 3}
    # (j_ref_ij, k_ref_jk) = (False, True) cannot occur: closest[k] keeps a CIGAR whose query is k (see tests/transitive_cases.py)
    assert dirs == {(True, False), (True, True), (False, False)}
    hand = TC.expected("hand")
    assert {2, 3} <= set(hand["route"]) and {(True, True), (False, False)} <= hand["events"]["dirs"]


def test_shortcuts_replacements_and_equal_divergences_are_covered():
    ev = TC.expected("tree")["events"]
    assert ev["shortcuts"] == {"ij", "jk"}                                    # a pair of identical haplotypes, from either side
    assert ev["replaced"] >= 1 and ev["kept_equal"] >= 1
    c = TC.by_name("tree")
    assert c.seqs[1] == c.seqs[3]


def test_every_smart_align_route_is_covered():
    walk = trace_routes("tree", ("walk", "tail")) | trace_routes("tree_maxgap", ("walk", "tail"))
    assert {"del", "ins", "straight", "exact", "simple"} <= walk
    assert "simple" in trace_routes("tree_maxgap", ("walk", "tail"))           # via max_gap
    # an optimize stretch: both an insertion and a deletion between two anchors of 51
    assert "exact" in trace_routes("tree", ("optimize",))


def test_skips_against_and_small_calls_are_covered():
    c, e = TC.by_name("skips"), TC.expected("skips")
    row0 = [x for x, (r, q) in enumerate(c.pairs) if r == 0]
    skipped = [x for x in row0 if e["route"][x] == 0]
    assert skipped and row0[0] < skipped[0] < row0[-1]                        # in the middle of a row
    ag = [x for x, (r, q) in enumerate(c.pairs) if c.against[r] or c.against[q]]
    assert ag and all(e["route"][x] >= 1 and e["div"][x][1] > c.thresh_div for x in ag)      # aligned only because of the flag
    f = TC.expected("fifteen")
    assert set(f["route"]) == {1} and f["rounds"] == []


def test_round_boundaries():
    for n in ("tree", "tree_maxgap", "anchor101"):                             # --all order: a round is a row of the triangle
        c, e = TC.by_name(n), TC.expected(n)
        assert e["rounds"] == [x for x, (r, q) in enumerate(c.pairs) if q == r + 1]
    c, e = TC.by_name("hand"), TC.expected("hand")
    # pair 1 reads closest[0], which pair 0 has just written: a reader directly behind its writer
    assert c.pairs[0][1] == c.pairs[1][0] and e["rounds"][:3] == [0, 1, 2]
    # (6, 3) then (6, 4) with closest[4] = 3: the second clause of (6, 4) tests the cell (6, 3) writes, inside what would be one row
    x = c.pairs.index((6, 4))
    assert c.pairs[x - 1] == (6, 3) and x in e["rounds"] and x - 1 not in e["rounds"]
    assert e["route"][x] == 3 and e["via"][x] == 3


@pytest.mark.parametrize("name,level", [("level1", 1), ("level2", 2)])
def test_level_cases_walk_at_their_level(name, level):
    """an exact stretch of the walk at the scratch level the family is named for (every family of cases() stays at level 0), on 21 pairs
    of which 6 go the backbone route and 15 the transitive one"""
    from tests.test_align_host import _level
    c, e = TC.by_name(name), TC.expected(name)
    assert len(c.seqs) == 7 and len(c.pairs) == 21 and e["route"] == [1] * 6 + [2] * 15
    levels = [_level(n, m) for p, r, n, m in e["events"]["trace"] if p == "walk" and r == "exact"]
    assert levels and max(levels) == level and levels.count(level) >= 1


# ---- the transliteration is sound -------------------------------------------------------------------------------------------------------
def check_items(items, score, ref, qry):
    ref, qry = R.norm(ref), R.norm(qry)
    i = j = 0
    for op, ln in items:
        assert ln > 0
        if op in "=X":
            eq = [ref[i + t] == qry[j + t] for t in range(ln)]
            assert all(eq) if op == "=" else not any(eq), (op, ln, i, j)
            i += ln; j += ln
        elif op == "D": i += ln
        else:
            assert op == "I"; j += ln
    assert (i, j) == (len(ref), len(qry))
    assert all(a[0] != b[0] for a, b in zip(items, items[1:]))               # merged
    assert score == R.calculate_score(items)


@pytest.mark.parametrize("name", NAMES + LEVEL_NAMES)
def test_pyref_cigars_are_alignments(name):
    c, e = TC.by_name(name), TC.expected(name)
    for x, (r, q) in enumerate(c.pairs):
        if e["route"][x]:
            check_items(e["items"][x], e["score"][x], c.seqs[r], c.seqs[q])
            assert (e["best_k"][x] == 0) == (e["route"][x] >= 2)
            # no alignment beats the full-matrix optimum of the pair
            assert e["score"][x] <= R.full_dp_score(c.seqs[r], c.seqs[q])


def test_direction_false_true_through_the_walk():
    """the one combination the strategy cannot reach, through find_transitive_alignment itself: i-j with i the reference, j-k with k the
    reference"""
    c = TC.by_name("hand")
    i, j, k = 2, 1, 0
    ij = R.normalize(R.align_multik(c.seqs[i], c.seqs[j], c.ks, c.max_gap)[0])              # reference i, query j
    jk = R.normalize(R.align_multik(c.seqs[k], c.seqs[j], c.ks, c.max_gap)[0])              # reference k, query j
    items, shortcut = T.find_transitive_alignment(ij, False, jk, True, c.seqs[i], c.seqs[k], c.max_gap, c.anchor)
    assert shortcut is None
    check_items(items, R.calculate_score(items), c.seqs[k], c.seqs[i])


def test_tr_div_zero_is_align_multik():
    c = TC.by_name("tree")
    e = c.expected(tr_div=0.0)
    assert set(e["route"]) == {1} and e["rounds"] == []
    for x, (r, q) in enumerate(c.pairs):
        cig, score, bk = R.align_multik(c.seqs[r], c.seqs[q], c.ks, c.max_gap)
        assert (e["items"][x], e["score"][x], e["best_k"][x]) == (R.normalize(cig), score, bk)


@pytest.mark.parametrize("name", NAMES)
def test_host_thread_form_of_the_probe_agrees_with_the_transliteration(name):
    """scripts/align_probe_host.cpp runs the rounds of the library's schedule in host threads and instantiates the very walk templates
    the kernels run (lcty_cigar_walk.hpp): routes, via, scores, best ks and the number of rounds are the transliteration's"""
    import numpy as np
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import align_probe
    c, want = TC.by_name(name), TC.expected(name)
    seqs, off = c.arrays()
    aligned = np.array([r != 0 for r in want["route"]], dtype=np.uint8)
    for threads in (1, 4):
        h = align_probe.host_route_transitive(seqs, off, [p[0] for p in c.pairs], [p[1] for p in c.pairs], aligned, c.ks, c.max_gap, c.tr_div, c.anchor,
                                              threads=threads, lib=_probe_lib())
        assert h["route"].tolist() == want["route"] and h["via"].tolist() == want["via"] and h["n_rounds"] == len(want["rounds"])
        assert h["score"].tolist() == want["score"] and h["best_k"].tolist() == want["best_k"]


@functools.lru_cache(maxsize=None)
def _probe_lib():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import align_probe
    return align_probe.host_lib()


# ---- header, cdefs and library --------------------------------------------------------------------------------------------------------
def header_struct(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locityper_hip.h")).read(), flags=re.S)
    m = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", header, flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"[\s\*]", "", f).split("[")[0] for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
    return fields


def test_new_structs_match_the_header():
    for c_name, cls, size in (("lcty_align_tr_params", cdefs.AlignTrParams, 16), ("lcty_align_tr_out", cdefs.AlignTrOut, 16),
                              ("lcty_align_tr_stats", cdefs.AlignTrStats, 80)):
        assert header_struct(c_name) == [n for n, _ in cls._fields_], c_name
        assert C.sizeof(cls) == size
    p = api.align_tr_params()
    assert (p.transitive_div, p.transitive_anchor) == (0.01, 101)
    L = _lib.lib()
    for s in ("lcty_align_tr_params_default", "lcty_align_haplotypes_transitive", "lcty_align_tr_out_free"):
        assert hasattr(L, s) and s in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "locityper_amd", "csrc", "lcty_api.hip")).read()
    assert '"align_cigar_store_mb"' in src[src.index("known[] = {"):src.index("nullptr};")]


def test_entry_point_fails_loudly_without_a_context():
    o, to = cdefs.AlignOut(), cdefs.AlignTrOut()
    p, tp = api.align_params(), api.align_tr_params()
    rc = _lib.lib().lcty_align_haplotypes_transitive(None, 0, None, None, 0, None, None, None, C.byref(p), C.byref(tp), C.byref(o), C.byref(to), None, None)
    assert rc == cdefs.ERR_INVALID_INPUT
