"""Host side of pruning (`locityper prune`): the transliteration's clustering against SciPy where the dendrogram is unique, and the host
entry points — divergences from the PAF, multiplicities, Newick / discarded texts, the thinned files — against tests/pyref_prune.py.
No device."""
import ctypes as C
import math

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import prune_cases as PC
from tests import pyref_db as DB
from tests import pyref_prune as R


@pytest.mark.parametrize("name", [c.name for c in PC.LINKAGE if c.distinct and c.n > 1])
def test_pyref_linkage_equals_scipy_where_values_are_distinct(name):
    from scipy.cluster.hierarchy import linkage
    c = PC.by_name(name)
    Z = linkage(c.tri, "complete")
    steps = PC.expected_steps(name)
    assert len(steps) == c.n - 1 == len(Z)
    for (a, b, d, sz), z in zip(steps, Z):
        assert a < b and (a, b) == (int(min(z[0], z[1])), int(max(z[0], z[1]))) and d == z[2] and sz == int(z[3])


def test_pyref_linkage_tie_rule_on_a_hand_case():
    # all equal: (0, 1) first, then the smallest labels left: (2, 3), (4, 5) = new labels; complete linkage keeps every height equal
    steps = R.linkage([1.0] * 10, 5)
    assert [(a, b) for a, b, _, _ in steps] == [(0, 1), (2, 3), (4, 5), (6, 7)]
    assert [s[3] for s in steps] == [2, 2, 3, 5]


PAF_NAMES = ["hA", "hB", "hC", "hD"]


def _paf_line(q, t, tags, n_cols=12):
    cols = [q, "100", "0", "100", "+", t, "100", "0", "100", "90", "100", "60"][:n_cols]
    return "\t".join(cols + tags)


PAF_TEXT = "\n".join([
    "# a comment line",
    _paf_line("hA", "hB", ["NM:i:3", "dv:f:0.0125", "qv:f:19"]),
    _paf_line("hB", "hA", ["dv:f:0.0125"]),                   # the same value again: not a conflict
    _paf_line("hB", "hA", ["dv:f:0.5"]),                      # a different one: the first stays
    _paf_line("hA", "hA", ["dv:f:0.0"]),                      # self pair
    _paf_line("hA", "hX", ["dv:f:0.3"]),                      # unknown target
    _paf_line("hX", "hA", ["dv:f:0.3"]),                      # unknown query
    _paf_line("hC", "hA", ["NM:i:1"]),                        # no tag
    _paf_line("hC", "hB", ["dv:f:-0.25"]),                    # negative
    _paf_line("hD", "hA", ["dvx:f:9", "dv:f:1e-3", "dv:f:7"]) + "\t \r",   # the first tag that starts with dv: ; trailing blanks
    _paf_line("hD", "hB", ["dv:f:.5"]),
    _paf_line("hD", "hC", ["de:f:0.25", "dv:f:inf"]),
    "",
    "hX\tshort",                                               # an unknown name is skipped before the columns are counted
]) + "\n"


@pytest.mark.parametrize("field,repl", [("dv", 0.002), ("de", math.inf), ("NM", 7.5)])
def test_paf_divergences_equal_the_transliteration(field, repl):
    want, wstats = R.load_divergences(PAF_TEXT, PAF_NAMES, field, repl)
    tri, stats = api.paf_divergences(PAF_TEXT.encode(), PAF_NAMES, field, repl)
    assert np.array_equal(tri, np.array(want)) and stats == wstats
    if field == "dv":
        assert list(tri) == [0.0125, 0.002, 1e-3, 0.002, 0.5, math.inf]
        assert stats == {"n_missing": 2, "n_negative": 1, "n_conflicting": 1, "missing_i": 1, "missing_j": 2}
    if field == "NM":
        assert list(tri) == [3.0, 1.0, 7.5, 7.5, 7.5, 7.5] and stats["missing_i"] == 2 and stats["missing_j"] == 3


def _raises(code, fn):
    with pytest.raises(_lib.LocityperError) as e:
        fn()
    assert e.value.code == code and _lib.lib().lcty_last_error() != b""


def test_paf_divergences_errors():
    only_comments = "# nothing\n" + _paf_line("hA", "hX", ["dv:f:0.1"]) + "\n"
    with pytest.raises(R.InvalidInput):
        R.load_divergences(only_comments, PAF_NAMES)
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.paf_divergences(only_comments.encode(), PAF_NAMES))      # all pairs missing
    for bad in ("dv:f:abc", "dv:f:", "dv:f: 0.1", "dv:f:0x10", "dv:f:1e", "dv:f:1_0"):
        text = _paf_line("hA", "hB", [bad]) + "\n"
        with pytest.raises(R.ParsingError):
            R.load_divergences(text, PAF_NAMES)
        _raises(cdefs.ERR_INVALID_DATA, lambda: api.paf_divergences(text.encode(), PAF_NAMES))
    _raises(cdefs.ERR_INVALID_DATA, lambda: api.paf_divergences(b"hA\t1\t2\n", PAF_NAMES))                   # a known contig, fewer than 6 columns
    _raises(cdefs.ERR_INVALID_DATA, lambda: api.paf_divergences(_paf_line("hA", "hB", [], n_cols=8).encode(), PAF_NAMES))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.paf_divergences(PAF_TEXT.encode(), PAF_NAMES, "d:v"))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.paf_divergences(PAF_TEXT.encode(), ["hA"]))               # one haplotype: no pair at all
    # accepted spellings of str::parse::<f64>
    for good, val in (("+1.5E-3", 1.5e-3), ("Infinity", math.inf), ("5.", 5.0), ("-0", -0.0)):
        tri, _ = api.paf_divergences((_paf_line("hA", "hB", ["dv:f:" + good]) + "\n").encode(), ["hA", "hB"])
        assert tri[0] == val == R.load_divergences(_paf_line("hA", "hB", ["dv:f:" + good]) + "\n", ["hA", "hB"])[0][0]


OLD_DISCARDED = "hB = x1, x2\nhZ = y1\nhD ~ hZ, hA, z9\n"


def test_multiplicities_follow_the_old_discarded_file():
    want, all_id = R.load_discarded(OLD_DISCARDED, PAF_NAMES)
    assert want == {1: ["x1", "x2"], 3: ["hZ", "y1", "z9"]} and not all_id      # hA is in the FASTA: skipped; hZ brings what it had folded
    mult, got_id = api.prune_multiplicities(OLD_DISCARDED.encode(), PAF_NAMES)
    assert list(mult) == [1, 3, 1, 4] and got_id is False
    assert list(api.prune_multiplicities(None, PAF_NAMES)[0]) == [1, 1, 1, 1]
    assert api.prune_multiplicities(b"hB = x1\n", PAF_NAMES)[1] is True
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.prune_multiplicities(b"hB =\n", PAF_NAMES))


@pytest.mark.parametrize("name", ["n1", "n2", "n3", "two_level", "five_values40", "inf30", "cut_equal_to_step", "cut_zero", "cut_above_all",
                                  "n_clusters_11", "repr_power_2", "repr_tie"])
def test_texts_equal_the_transliteration(name):
    """lcty_prune_texts on the transliteration's own steps, clusters and representatives: Newick and discarded lines byte for byte"""
    c, want = PC.by_name(name), PC.expected(name)
    names = PC.names(c)
    old = None
    if c.mult is not None:
        old = "".join(f"h{i} = " + ", ".join(f"d{i}_{t}" for t in range(int(m) - 1)) + "\n" for i, m in enumerate(c.mult) if m > 1).encode()
        assert list(api.prune_multiplicities(old, names)[0]) == list(c.mult)
    steps = np.array([(a, b, d, sz, 0) for a, b, d, sz in want["steps"]], dtype=cdefs.PRUNE_STEP_DTYPE)
    nwk, disc = api.prune_texts(names, steps, want["clusters"], want["repr"], old)
    assert nwk == want["newick"].encode()
    assert disc == (old or b"") + want["new_lines"].encode()
    if name == "n1":
        assert nwk == b"h0;\n" and disc == b""
    if name == "n3":
        assert nwk == b"(h1:0.00015000,(h0:0.00005000,h2:0.00005000):0.00010000);\n"      # child 1 is the smaller label
    if name == "inf30":
        assert b":inf" in nwk


def test_texts_with_old_discarded_names_on_a_hand_case():
    names = ["a", "b", "c"]
    steps = np.array([(0, 2, 0.5, 2, 0), (1, 3, 1.0, 3, 0)], dtype=cdefs.PRUNE_STEP_DTYPE)
    nwk, disc = api.prune_texts(names, steps, [[0, 2], [1]], [2, 1], b"a = a2, a3\n")
    assert nwk == b"(b:0.50000000,((a:0,a2:0,a3:0):0.25000000,c:0.25000000):0.25000000);\n"
    assert disc == b"a = a2, a3\nc ~ a\n"


def _locus_files(n, rng, k=5):
    names = [f"s{i}" for i in range(n)]
    seqs = ["".join(rng.choice(list("ACGT"), int(rng.integers(k - 2, 40)))).encode() for _ in range(n)]
    seqs[1] = b"ACG"                                         # shorter than k: an empty block
    blocks = b"".join(DB.kmer_counts_save(k, 2, [rng.integers(0, 65536, max(len(s) + 1 - k, 0)).astype(np.uint16) for s in seqs]) for _ in range(2))
    uniq = rng.integers(0, 100000, n * (n - 1) // 2).astype(np.uint32)
    dists = DB.write_divergences(15, 15, n, uniq)
    lines = ["# header\tkept as it is"]
    for i in range(n):
        for j in range(n):
            if i != j and rng.random() < 0.7:
                lines.append(_paf_line(names[i], names[j], ["dv:f:%g" % rng.random()]))
    lines.append(_paf_line("other", names[0], ["dv:f:0.1"]))
    return names, seqs, blocks, uniq, dists, "\n".join(lines) + "\n"


@pytest.mark.parametrize("keep", [[0, 2, 3, 6], [1], [0, 1, 2, 3, 4, 5, 6]])
def test_thinned_files_equal_the_transliteration_and_parse_back(keep):
    rng = np.random.default_rng(11)
    n = 7
    names, seqs, blocks, uniq, dists, paf = _locus_files(n, rng)
    flat = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    got = api.prune_thin(names, flat, off, paf.encode(), keep, blocks, dists)
    assert got["fasta"] == R.write_fasta(names, seqs, keep)
    assert got["paf"] == R.prune_paf(paf, names, keep).encode()
    assert got["kmers"] == R.thin_kmers(blocks, keep) and got["distances"] == R.thin_distances(dists, n, keep)
    assert got["warn_bits"] == 0 and list(got["keep"]) == keep
    # parsed back by the readers of the library
    kk, coff, counts, used = api.parse_kmer_counts(got["kmers"])
    _, coff0, counts0, _ = api.parse_kmer_counts(blocks)
    assert kk == 5 and len(coff) == len(keep) + 1
    for t, a in enumerate(keep):
        assert np.array_equal(counts[int(coff[t]):int(coff[t + 1])], counts0[int(coff0[a]):int(coff0[a + 1])])
    assert len(api.parse_kmer_counts(got["kmers"][used:])[1]) == len(keep) + 1               # the second block
    if len(keep) > 1:
        k, w, dist = io.distances_parse(got["distances"], len(keep))
        full = io.distances_parse(dists, n)[2]
        assert (k, w) == (15, 15) and np.array_equal(dist, full[np.ix_(keep, keep)])


def test_thin_refuses_bad_input_and_flags_counts_that_do_not_match():
    rng = np.random.default_rng(12)
    n = 4
    names, seqs, blocks, uniq, dists, paf = _locus_files(n, rng)
    flat = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.prune_thin(names, flat, off, paf.encode(), [2, 1]))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.prune_thin(names, flat, off, paf.encode(), [4]))
    _raises(cdefs.ERR_INVALID_DATA, lambda: api.prune_thin(names, flat, off, b"s0\ts1\tx\n", [0, 1]))      # fewer than 7 columns
    with pytest.raises(R.ParsingError):
        R.prune_paf("s0\ts1\tx\n", names, [0, 1])
    other = DB.kmer_counts_save(5, 2, [[1, 2, 3]] * n) * 2                                                  # lengths that are not the haplotypes'
    got = api.prune_thin(names, flat, off, paf.encode(), [0, 1], other)
    assert got["kmers"] == b"" and got["warn_bits"] == cdefs.PRUNE_WARN_KMERS and got["distances"] == b""


def test_prune_params_default_and_checks():
    p = api.prune_params()
    assert (p.threshold, p.n_clusters, p.power, p.only_tree, p.skip_tree) == (0.0002, 0, 2, 0, 0)       # prune.rs:39-55
    assert api.prune_power("min") == cdefs.PRUNE_POWER_MIN and api.prune_power("Max") == cdefs.PRUNE_POWER_MAX and api.prune_power("-3") == -3
    assert C.sizeof(cdefs.PruneStep) == 24 == cdefs.PRUNE_STEP_DTYPE.itemsize and C.sizeof(cdefs.PruneParams) == 24
    L = _lib.lib()
    tri = np.zeros(1)
    o = cdefs.PruneOut()
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_prune_cluster(None, 2, tri.ctypes.data, None, C.byref(p), C.byref(o))))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_prune_linkage(None, 2, tri.ctypes.data, None, None)))


def test_cluster_case_properties():
    """what the designed cases are there for, asserted on the transliteration's own results"""
    e, b = PC.expected("cut_equal_to_step"), PC.expected("cut_just_below_step")
    assert len(b["clusters"]) == len(e["clusters"]) + 1                         # equal to a step's height: merged; just below: cut
    assert len(PC.expected("cut_zero")["clusters"]) == 12 == len(PC.expected("cut_below_min")["clusters"])
    assert len(PC.expected("cut_above_all")["clusters"]) == 1
    assert sorted(len(m) for m in PC.expected("repr_power_2")["clusters"]) == [2, 64, 65, 300]
    t = PC.expected("repr_tie")
    assert sorted(sorted(m) for m in t["clusters"]) == [[0, 2, 4, 6], [1, 3, 5]]
    assert any(m[0] != min(m) for m in t["clusters"])                           # the first member is not always the smallest id
    for acc, mem, rep in zip(t["acc"], t["clusters"], t["repr"]):
        assert len(set(acc)) < len(acc) and acc[0] == min(acc) and rep == mem[0]      # equal best sums: the first wins
    tn = PC.expected("repr_tie_neg")
    for acc, mem, rep in zip(tn["acc"], tn["clusters"], tn["repr"]):
        assert acc[0] == max(acc) and rep == mem[0]
