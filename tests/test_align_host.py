"""CPU tier of the pairwise haplotype alignments: hand-derived answers for the transliteration (tests/pyref_align.py), the host-side
PAF writer against the transliterated line byte for byte, the round trip through lcty_paf_read, and the fitness of the designed cases
(tests/align_cases.py) the GPU tests rest on."""
import numpy as np
import pytest

from locityper_amd import api, io
from tests import align_cases as AC
from tests import oracle_ffi as O
from tests import pyref_align as R


# ---- 1. hand-derived answers ---------------------------------------------------------------------------------------------------------
def test_matches_of_two_short_strings():
    # 5-mers of ACGTACGTA: ACGTA@0, CGTAC@1, GTACG@2, TACGT@3, ACGTA@4; of TACGTAC: TACGT@0, ACGTA@1, CGTAC@2
    assert R.kmer_matches(b"ACGTACGTA", b"TACGTAC", 5) == [(0, 1), (1, 2), (3, 0), (4, 1)]
    assert R.kmer_matches(b"ACGTNACGTA", b"ACGTA", 5) == [(5, 0)]           # a window with an N is no k-mer
    assert R.kmer_matches(b"ACG", b"ACGTACGT", 5) == []                      # shorter than k


@pytest.mark.parametrize("matches,k,score,path", [
    ([(0, 0), (1, 1), (2, 2)], 5, 7, [0, 1, 2]),                             # a diagonal run: 5, 6, 7
    ([(0, 0), (5, 5)], 5, 10, [0, 1]),                                       # a jump that clears k on both sides
    ([(0, 0), (10, 12)], 5, 10, [0, 1]),
    ([(0, 0), (3, 4)], 5, 5, [0]),                                           # overlapping and off the diagonal: must not chain
    ([(0, 0), (5, 4)], 5, 5, [0]),                                           # clears k in one coordinate only
    ([(0, 0), (1, 1), (6, 7)], 5, 11, [0, 1, 2]),                            # run of two (6), then a jump (+ 5)
    ([], 5, 0, []),
])
def test_chain_score_by_hand(matches, k, score, path):
    s, p = R.lcskpp(matches, k)
    assert s == score and p == path


def _plain(seed=5, n=80):
    return AC.rand_seq(np.random.default_rng(seed), n)


def _aln(ref, query, k=25):
    cig, score = R.align_from_backbone(ref, query, k, 10000)
    return "".join(f"{ln}{op}" for op, ln in R.normalize(cig)), score


def test_cigar_and_score_by_hand():
    ref = _plain()
    snp = lambda s, p: s[:p] + bytes([AC.B[(AC.B.index(s[p]) + 1) % 4]]) + s[p + 1:]
    assert _aln(ref, ref) == ("80=", 0)
    assert _aln(ref, snp(ref, 40)) == ("40=1X39=", -4)
    assert _aln(ref, snp(ref, 3)) == ("3=1X76=", -4)                         # inside the first k bases
    assert _aln(ref, snp(ref, 77)) == ("77=1X2=", -4)                        # inside the last k bases
    assert _aln(ref, ref[:60]) == ("60=20D", -26)                            # the query is a prefix: a gap of 20 costs 6 + 20
    assert _aln(ref[:60], ref) == ("60=20I", -26)
    p = next(p for p in range(30, 50) if ref[p + 2] != ref[p - 1] and ref[p] != ref[p + 3])    # three bases that cannot slide
    assert _aln(ref, ref[:p] + ref[p + 3:]) == (f"{p}=3D{80 - p - 3}=", -9)
    assert _aln(ref[:p] + ref[p + 3:], ref) == (f"{p}=3I{80 - p - 3}=", -9)


def test_full_dp_by_hand():
    assert R.full_dp_score(b"ACGTACGT", b"ACGTACGT") == 0
    assert R.full_dp_score(b"ACGTACGT", b"ACGAACGT") == -4
    assert R.full_dp_score(b"ACGTACGT", b"ACGACGT") == -7                    # one gap of one base: 6 + 1
    assert R.full_dp_score(b"ACGT", b"") == -10
    assert R.full_dp_score(b"AAAA", b"TTTT") == -16                          # four mismatches (two gaps of four would cost 20)
    assert R.full_dp_score(b"ANNA", b"ANNA") == 0                            # N equals N


def test_all_pairs_order():
    r, q = api.align_all_pairs(4)
    assert list(zip(r.tolist(), q.tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


# ---- 2. + 3. the PAF text ---------------------------------------------------------------------------------------------------------------
def _hand_result():
    """four pairs over three sequences: an alignment with errors, a skipped pair, an identical pair (dv = 0), a pair with a gap"""
    names = ["hapA", "hapB", "hapC"]
    lens = [100, 100, 97]
    off = np.zeros(4, dtype=np.uint64); np.cumsum(lens, out=off[1:])
    ref = np.array([0, 0, 1, 2], dtype=np.uint32); qry = np.array([1, 2, 0, 1], dtype=np.uint32)
    items = [[("=", 40), ("X", 1), ("=", 59)], None, [("=", 100)], [("=", 50), ("I", 3), ("=", 47)]]
    scores = [-4, 0, 0, -9]
    um, md = [3, 250, 0, 7], [3 / 41, 0.5, 0.0, 7 / 39]
    res = {k: np.zeros(4, dtype=dt) for k, dt in (("aligned", np.uint8), ("n_matches", np.uint32), ("aln_len", np.uint32), ("nerrs", np.uint32),
                                                  ("score", np.int32), ("best_k", np.uint32), ("um", np.uint32), ("md", np.float64))}
    coff, words = [0], []
    for x, it in enumerate(items):
        if it is not None:
            nm, ne = R.counts(it)
            res["aligned"][x] = 1; res["n_matches"][x] = nm; res["nerrs"][x] = ne; res["aln_len"][x] = nm + ne; res["score"][x] = scores[x]
            res["best_k"][x] = 25
            words += R.words(it).tolist()
        res["um"][x] = um[x]; res["md"][x] = md[x]
        coff.append(len(words))
    res["cigar_off"] = np.array(coff, dtype=np.uint64); res["cigar"] = np.array(words, dtype=np.uint32)
    return names, lens, off, ref, qry, items, scores, um, md, res


@pytest.mark.parametrize("skip_div", [0, 1])
def test_paf_text_equals_the_transliterated_lines(skip_div):
    names, lens, off, ref, qry, items, scores, um, md, res = _hand_result()
    p = api.align_params(skip_div=skip_div, thresh_div=0.25, max_gap=500, backbone_ks=[25, 51])
    text = io.paf_write(names, off, ref, qry, res, p)
    want = R.paf_header(15, 15, 0.25, (25, 51), 500)
    for x in range(4):
        r, q = int(ref[x]), int(qry[x])
        want += R.paf_line(names[q], lens[q], names[r], lens[r], None if items[x] is None else (items[x], scores[x]),
                           None if skip_div else (um[x], md[x]))
    assert text == want.encode()
    lines = text.decode().split("\n")
    assert lines[0] == "# minimizers=15,15; max_divergence=0.25000; backbone-ks=25,51; accuracy=9; max-gap=500"
    assert lines[1].startswith("hapB\t100\t0\t100\t+\thapA\t100\t0\t100\t99\t100\t255\tNM:i:1\tAS:i:-4\tdv:f:0.010000000\tqv:f:20.000000")
    assert "\t0\t0\t255" in lines[2] and "cg:Z:" not in lines[2]
    assert "dv:f:0.000000000\tqv:f:inf" in lines[3]
    assert lines[1].endswith("cg:Z:40=1X59=")
    assert ("um:i:3\tmd:f:0.073170732" in lines[1]) == (not skip_div)


def test_paf_header_of_never_align():
    names, lens, off, ref, qry, items, scores, um, md, res = _hand_result()
    text = io.paf_write(names, off, ref[:0], qry[:0], {k: (v[:1] if k == "cigar_off" else v[:0]) for k, v in res.items()}, api.align_params(thresh_div=0.0))
    assert text == R.paf_header(thresh_div=0.0).encode() == b"# minimizers=15,15; max_divergence=-1.00000; backbone-ks=; accuracy=9; max-gap=10000\n"


def test_paf_round_trip(tmp_path):
    names, lens, off, ref, qry, items, scores, um, md, res = _hand_result()
    path = tmp_path / "haplotypes.paf.gz"
    io.write_gz(path, io.paf_write(names, off, ref, qry, res))
    ents = io.paf_read(path, names)
    want = [(int(qry[x]), int(ref[x]), R.words(items[x]).tolist(), *R.counts(items[x])) for x in range(4) if items[x] is not None]
    got = [(e[0], e[1], e[2].tolist(), e[3], e[4] - e[3]) for e in ents]
    assert got == want


# ---- 4. the designed cases are fit for purpose --------------------------------------------------------------------------------------------
def _unique_pairs():
    return [(c.name, r, q) for c in AC.cases() if c.unique for r, q in c.pairs]


@pytest.mark.parametrize("name,ref,query", _unique_pairs())
def test_unique_chain_cases_are_solved_optimally(name, ref, query):
    items, score, _ = AC.reference_multik(name, ref, query)
    assert score == R.calculate_score(items)
    assert score == AC.optimum(name, ref, query), "the backbone route misses the full-DP optimum: no unique-chain case"
    c = AC.by_name(name)
    for k in c.ks:                                                          # every k alone reaches it too: best_k is the first one
        m, chain, path = AC.reference(name, ref, query, k)
        cig, s = R.align_from_path(c.seqs[ref], c.seqs[query], m, path, k, c.max_gap)
        assert s == score


def test_case_shapes():
    for c in AC.cases():
        assert 4 <= len(c.seqs) <= 12 and all(len(s) <= 3000 for s in c.seqs) and set(c.ks) <= {5, 25, 33, 51, 101}
    assert any(len(s) < 25 for s in AC.by_name("short").seqs)
    r, q = AC.by_name("unrelated").seqs[:2]
    assert R.kmer_matches(r, q, 25) == []
    assert len(AC.reference("tandem", 0, 1, 25)[0]) > 5000                   # quadratic matches


def _probe():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("align_probe", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "align_probe.py"))
    probe = importlib.util.module_from_spec(spec); spec.loader.exec_module(probe)
    return probe


# ---- 5. the host-thread form of the probe -----------------------------------------------------------------------------------------------
def test_probe_host_route_equals_the_transliteration():
    """scripts/align_probe_host.cpp (the comparison point of scripts/align_probe.py) on the unique-chain cases: score and best k of
    align_multik; on every case its score is that of its own CIGAR-free route and never above the full-DP optimum."""
    probe = _probe()
    for c in AC.cases():
        seqs, off = c.arrays()
        ref = [p[0] for p in c.pairs]; query = [p[1] for p in c.pairs]
        score, best, _, _ = probe.host_route(seqs, off, ref, query, c.ks, c.max_gap, threads=3)
        for x, (r, q) in enumerate(c.pairs):
            assert int(score[x]) <= AC.optimum(c.name, r, q)
            if c.unique:
                _, want, k = AC.reference_multik(c.name, r, q)
                assert (int(score[x]), int(best[x])) == (want, k)


# ---- 6. the aligner primitives of lcty_gotoh.hpp, compiled for the host, on stretches where a tie rule decides -----------------------------
def n_optimal_alignments(ref, query):
    """(optimum, number of distinct end-to-end alignments that reach it) under 4 / 6 / 1, by counting over the three matrices: an
    alignment is its sequence of operations, and that sequence fixes the path through (cell, matrix)."""
    n, m, INF = len(ref), len(query), 1 << 30
    best = {(0, 0, "M"): (0, 1)}

    def get(i, j, s):
        return best.get((i, j, s), (INF, 0))

    def merge(cands):
        v = min(c[0] for c in cands)
        return (v, sum(c[1] for c in cands if c[0] == v)) if v < INF else (INF, 0)
    for i in range(n + 1):
        for j in range(m + 1):
            if i and j:
                sub = 0 if ref[i - 1] == query[j - 1] else R.MISMATCH
                best[i, j, "M"] = merge([(get(i - 1, j - 1, s)[0] + sub, get(i - 1, j - 1, s)[1]) for s in "MDI"])
            if i:
                best[i, j, "D"] = merge([(get(i - 1, j, "D")[0] + R.GAP_EXTEND, get(i - 1, j, "D")[1])] +
                                        [(get(i - 1, j, s)[0] + R.GAP_OPEN + R.GAP_EXTEND, get(i - 1, j, s)[1]) for s in "MI"])
            if j:
                best[i, j, "I"] = merge([(get(i, j - 1, "I")[0] + R.GAP_EXTEND, get(i, j - 1, "I")[1])] +
                                        [(get(i, j - 1, s)[0] + R.GAP_OPEN + R.GAP_EXTEND, get(i, j - 1, s)[1]) for s in "MD"])
    pen, cnt = merge([get(n, m, s) for s in "MDI"])
    return -pen, cnt


def test_tie_cases_have_ties():
    """The last column of AC.TIE_CASES is what the enumeration says, its optimum is pyref_align's full-matrix optimum, and at least
    four of the stretches have more than one optimal alignment: homopolymer (7: the gap of three in front of any of the six bases of the
    query, or behind the last), dinucleotide, both substitutions next to an indel, and the stretch beyond max_gap."""
    tied = 0
    for name, r, q, _, co in AC.TIE_CASES:
        opt, cnt = n_optimal_alignments(r, q)
        assert opt == R.full_dp_score(r, q), name
        assert (cnt > 1) == co, (name, cnt)
        assert len(r) < 25 and len(q) < 25
        tied += cnt > 1
    assert tied >= 4
    assert n_optimal_alignments(b"A" * 9, b"A" * 6) == (-9, 7)


def test_header_host_instantiation_on_tie_cases():
    """scripts/align_probe_host.cpp::align_probe_stretch — routing, align_simple, the straight comparison, the cell, the end state and the
    walk back of locityper_amd/csrc/lcty_gotoh.hpp — against pyref_align.smart_align: the score, and the CIGAR as the recording
    sink saw it. The aligner and the straight comparison push base by base (push_checked joins them: compared joined); align_simple,
    DEL and INS push whole items (push_unchecked: compared push for push)."""
    probe = _probe()
    lib = probe.host_lib()
    routes = set()
    for name, r, q, mg in AC.tie_runs():
        cig = R.Cig()
        want = R.smart_align(R.norm(r), 0, len(r), R.norm(q), 0, len(q), mg, cig)
        score, pushes = probe.host_stretch(r, q, mg, lib)
        got = [[R.OPS[op], ln] for op, ln in pushes]
        assert score == want, name
        joined = R.Cig()
        for op, ln in got:
            joined.push_checked(op, ln)
        assert joined.t == [list(t) for t in R.normalize(cig)], name
        simple = bool(r) and bool(q) and (mg < len(r) or mg < len(q))
        exact = bool(r) and bool(q) and not simple and not (len(r) == len(q) and len(r) <= R.SAFE_MISMATCH)
        if simple or not (r and q):
            assert got == cig.t, name
        if exact:
            assert score == R.full_dp_score(r, q), name
            assert all(ln == 1 for _, ln in got)
        routes.add("simple" if simple else "exact" if exact else "gap" if not (r and q) else "straight")
    assert routes == {"simple", "exact", "gap", "straight"}


# ---- 7. the designed sets for the limits of the device aligner are fit for purpose (tests/test_gpu_align_limits.py runs them) -----------------
LEVEL_DIM, LEVEL_CELLS = (255, 2047, 16383), (1 << 16, 1 << 22, 1 << 26)     # kLevelDim, kLevelCells of lcty_align.hip


def _level(n, m):
    return next(l for l in range(3) if n <= LEVEL_DIM[l] and m <= LEVEL_DIM[l] and (n + 1) * (m + 1) <= LEVEL_CELLS[l])


def _plan(name, r, q, k=AC.K):
    c = AC.by_name(name)
    m, _, path = AC.reference(name, r, q, k)
    return m, path, AC.plan_bound(c.seqs[r], c.seqs[q], m, path, k, c.max_gap)


@pytest.mark.parametrize("shape", AC.LEVEL_SHAPES, ids=[s[0] for s in AC.LEVEL_SHAPES])
def test_level_cases_are_one_stretch_of_the_intended_shape(shape):
    name, n, m, pairs, max_gap, n_level, n_dropped = shape
    c = AC.by_name("lv_" + name)
    assert tuple(int(x) for x in name.split("x")) == c.stretch[pairs[0]]
    assert not any(c.middles[0][p:p + AC.K] in c.middles[1] for p in range(n - AC.K + 1))          # R and Q share no 25-mer
    for r, q in pairs:
        matches, path, (anchors, stretches) = _plan(c.name, r, q)
        a, b = c.stretch[(r, q)]
        # the flanks' windows on their two diagonals and nothing else: no unintended match
        want = [(p, p) for p in range(AC.FLANK - AC.K + 1)] + [(AC.FLANK + a + p, AC.FLANK + b + p) for p in range(AC.FLANK - AC.K + 1)]
        assert matches == want and path == list(range(len(want)))
        assert anchors == 2 and stretches == [("dropped" if n_dropped else "exact", a, b, min(a, b) + 1 if n_dropped else a + b)]
        if not n_dropped:
            assert [int(l == _level(a, b)) for l in range(3)] == n_level
        counters = {}
        if name in AC.BEYOND_ORACLE:
            with pytest.raises(R.UnfitCase):
                R.align_from_path(c.seqs[r], c.seqs[q], matches, path, AC.K, max_gap)
            continue
        cig, score = R.align_from_path(c.seqs[r], c.seqs[q], matches, path, AC.K, max_gap, counters=counters)     # no UnfitCase
        assert counters.get("dropped", 0) == n_dropped
        AC.check_cigar(R.normalize(cig), score, c.seqs[r], c.seqs[q])
        if n_dropped:                                                          # the oracle's aligner itself refuses this one too
            assert O.dp_align(c.seqs[r][AC.FLANK:-AC.FLANK], c.seqs[q][AC.FLANK:-AC.FLANK])[0] == R.DROPPED
    # the limits the shapes stand at
    assert _level(255, 255) == 0 and _level(255, 256) == 1 and _level(2047, 2047) == 1 and _level(2047, 2048) == 2 and _level(2048, 1) == 2


def test_reuse_cases_fill_their_level_beyond_its_lanes():
    c = AC.by_name("reuse1")
    widths = set()
    assert len(c.pairs) == 136 > 128
    for r, q in c.pairs:
        matches, path, (anchors, stretches) = _plan("reuse1", r, q)
        assert anchors == 2 and len(stretches) == 1 and stretches[0][0] == "exact"
        _, a, b, _ = stretches[0]
        assert _level(a, b) == 1, (r, q, a, b)
        assert len(matches) == len(path) == len(c.seqs[r]) - a - 2 * (AC.K - 1)           # the two flank diagonals only
        widths.add(b)
        R.align_from_path(c.seqs[r], c.seqs[q], matches, path, AC.K, c.max_gap)            # answers: no UnfitCase
    assert len(widths) > 8
    c = AC.by_name("reuse2")
    assert len(c.pairs) == 24
    for r, q in c.pairs:
        matches, path, (anchors, stretches) = _plan("reuse2", r, q)
        a, b = len(c.seqs[r]) - 2 * AC.FLANK, len(c.seqs[q]) - 2 * AC.FLANK
        assert anchors == 2 and stretches == [("exact", a, b, a + b)] and max(a, b) == 2048 and 8 <= min(a, b) <= 19 and _level(a, b) == 2
        assert len(matches) == 2 * (AC.FLANK - AC.K + 1)
        R.align_from_path(c.seqs[r], c.seqs[q], matches, path, AC.K, c.max_gap)


def test_tight_bound_case_fills_the_bound():
    c = AC.by_name("tight_bound")
    shape = {"X=X": ("straight", 3, 3, 3), "=X=": ("straight", 3, 3, 3), "9x12": ("simple", 9, 12, 10), "12x9": ("simple", 12, 9, 10),
             "D": ("gap", 5, 0, 1), "I": ("gap", 0, 7, 1)}
    for r, q in c.pairs:
        kinds = c.kinds[(r, q)]
        matches, path, (anchors, stretches) = _plan("tight_bound", r, q)
        assert len(matches) == len(path) == anchors == len(kinds) + 1            # anchors of exactly k bases: one 25-mer each, no other match
        want = [shape[kd] for kd in kinds]
        if r > q:
            want = [(t, m, n, b) for t, n, m, b in want]
        assert stretches == want and len(stretches) >= 6
        items, count = AC.tight_bound_items(r, q)
        assert len(items) == count
        if "=X=" not in kinds:
            assert count == anchors + sum(s[3] for s in stretches) and sum(s[0] != "gap" for s in stretches) >= 6
            assert min(sum(s[0] == t for s in stretches) for t in ("straight", "simple", "gap")) >= 3      # an undercount by one in any route outgrows the start of 2


def test_lowcomplexity_and_lengths_and_random_cases_answer():
    c = AC.by_name("lowcomplexity")
    assert max(len(AC.reference(c.name, r, q, 5)[0]) for r, q in c.pairs) > 10000
    for name in ["lowcomplexity", "lengths"] + [f"random_k{k}" for k in AC.RANDOM_KS]:
        c = AC.by_name(name)
        for r, q in c.pairs:
            for k in c.ks:
                m, chain, path = AC.reference(name, r, q, k)
                cig, score = R.align_from_path(c.seqs[r], c.seqs[q], m, path, k, c.max_gap)       # no UnfitCase
                AC.check_cigar(R.normalize(cig), score, c.seqs[r], c.seqs[q], AC.optimum(name, r, q))
    c = AC.by_name("lengths")
    assert [len(s) for s in c.seqs] == [1024] + AC.LENGTHS and len(c.pairs) == 24
    assert len(AC.reference("lengths", 0, 4, AC.K)[0]) == 0 and len(AC.reference("lengths", 0, 3, AC.K)[0]) == 0     # 25 bases with a substitution, 24 bases
    assert sum(len(c.pairs) for c in AC.limit_cases() if c.name.startswith("random")) == AC.N_RANDOM
    for k in AC.RANDOM_KS:
        c = AC.by_name(f"random_k{k}")
        assert all(60 <= len(c.seqs[r]) <= 400 for r, _ in c.pairs)
        assert any(b"N" in c.seqs[q] for _, q in c.pairs) and any(c.seqs[q] != c.seqs[q].upper() for _, q in c.pairs)


def test_header_host_instantiation_on_level_shapes():
    """the cell, the end state and the walk back of lcty_gotoh.hpp, compiled for the host, on the stretches of the level cases the
    oracle's aligner answers: score and CIGAR of pyref_align.smart_align at up to 2 047 x 2 048"""
    probe = _probe()
    lib = probe.host_lib()
    for name, _, _, pairs, max_gap, _, n_dropped in AC.LEVEL_SHAPES:
        if name in AC.BEYOND_ORACLE or n_dropped:
            continue
        c = AC.by_name("lv_" + name)
        for r, q in pairs:
            a, b = c.seqs[r][AC.FLANK:-AC.FLANK], c.seqs[q][AC.FLANK:-AC.FLANK]
            cig = R.Cig()
            want = R.smart_align(R.norm(a), 0, len(a), R.norm(b), 0, len(b), max_gap, cig)
            score, pushes = probe.host_stretch(a, b, max_gap, lib)
            joined = R.Cig()
            for op, ln in pushes:
                joined.push_checked(R.OPS[op], ln)
            assert score == want == R.full_dp_score(a, b) and joined.t == [list(t) for t in R.normalize(cig)], name
