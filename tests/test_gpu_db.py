"""Locus-database build on the device (lcty_db.hip) against tests/pyref_db.py, the serial restatement of the reference: minimizer lists,
all-pairs divergences, off-target k-mer counts and the whole of process_alleles. Every comparison is array / byte equality."""
import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io, synth
from tests import oracle_ffi as O
from tests import pyref_db as R
from tests.helpers import compare_gpu_to_oracle, random_alleles
from tests.test_db_host import _concat, _seqs

pytestmark = pytest.mark.gpu

KW = [(15, 15), (1, 1), (32, 63), (5, 2), (15, 10)]
RNG = np.random.default_rng(2024)


def _rand(n, rng=RNG):
    return "".join(rng.choice(list("ACGT"), n))


HOMOPOLYMER = "A" * 5000
TANDEM = "AC" * 2500
_core = _rand(400)
HAND = {
    "shorter_than_k": "ACGTACG",                          # < k for k = 15, 32
    "shorter_than_window": _rand(20),                     # < k + w - 1 for (15, 15), (15, 10), (32, 63)
    "exactly_one_window": _rand(29),                      # k + w - 1 for (15, 15)
    "empty": "",
    "homopolymer": HOMOPOLYMER,
    "tandem": TANDEM,
    "n_start": "N" + _core,
    "n_inside": _core[:200] + "N" + _core[200:],
    "n_end": _core + "N",
    "n_run_longer_than_w": _core[:150] + "N" * 70 + _core[150:],
    "n_runs_close": _core[:100] + "N" + _core[100:117] + "NN" + _core[117:],
    "all_n": "N" * 100,
    "lower_case": _core[:120] + _core[120:180].lower() + _core[180:],
    "other_letters": _core[:90] + "R" + _core[90:300] + "-" + _core[300:],
    "tile_edges": _rand(1024 + 14 + 1024 + 3),            # two full tiles of the clean kernel and a little more at k = 15
}


def _lists(moff, hashes):
    return [hashes[int(moff[i]):int(moff[i + 1])] for i in range(len(moff) - 1)]


@pytest.mark.parametrize("k,w", KW)
def test_minimizer_lists_equal_the_serial_loop(gpu_ctx, k, w):
    L = synth.SynthLocus(4, 16, base_len=3000, seed=11)
    strs = [L.allele(a).decode() for a in range(4)] + list(HAND.values())
    seqs, off = _seqs(strs)
    moff, hashes, st = api.db_minimizers(gpu_ctx, seqs, off, k, w)
    for name, s, got in zip(["synth"] * 4 + list(HAND), strs, _lists(moff, hashes)):
        want = R.sorted_minimizers(s.encode(), k, w)
        assert np.array_equal(got, want), (name, k, w, len(got), len(want))
    n_dirty = sum(any(c not in "ACGT" for c in s) for s in strs)
    assert st["n_walk"] == n_dirty and st["n_fast"] == len(strs) - n_dirty       # which path ran
    assert st["n_minimizers"] == int(moff[-1])


def test_minimizer_ties_and_duplicates(gpu_ctx):
    """Long runs of equal hashes: the homopolymer pushes one minimizer per window step (leftmost on rescan), so its list is one hash many times."""
    seqs, off = _seqs([HOMOPOLYMER, TANDEM])
    moff, hashes, _ = api.db_minimizers(gpu_ctx, seqs, off, 15, 15)
    homo, tandem = _lists(moff, hashes)
    assert len(set(homo.tolist())) == 1 and len(homo) > 300
    assert len(set(tandem.tolist())) == 1 and len(tandem) > 300      # two k-mers alternate; the smaller hash wins every window
    assert np.array_equal(tandem, R.sorted_minimizers(TANDEM.encode(), 15, 15))
    assert np.array_equal(homo, R.sorted_minimizers(HOMOPOLYMER.encode(), 15, 15))


def test_long_lists_are_sorted_too(gpu_ctx):
    """w = 1 pushes every k-mer: 20 000 entries, past what one workgroup sorts in LDS."""
    s = _rand(20_000, np.random.default_rng(5))
    seqs, off = _seqs([s, s[:9000]])
    moff, hashes, st = api.db_minimizers(gpu_ctx, seqs, off, 11, 1)
    assert st["n_sorted_host"] == 2
    for got, t in zip(_lists(moff, hashes), [s, s[:9000]]):
        assert np.array_equal(got, R.sorted_minimizers(t.encode(), 11, 1))


def _check_divergences(ctx, strs, k, w):
    seqs, off = _seqs(strs)
    uniq, div, chk, st = api.db_divergences(ctx, seqs, off, k, w)
    runiq, rdiv = R.divergences([s.encode() for s in strs], k, w)
    assert np.array_equal(uniq, runiq)
    assert np.array_equal(div, rdiv, equal_nan=True)
    assert chk == R.check_divergencies(rdiv, len(strs))
    return uniq, div, st


@pytest.mark.parametrize("n", [2, 3, 65, 300])
def test_divergences_equal_the_merge(gpu_ctx, n):
    strs = [s.decode() for s in random_alleles(n, 1200, seed=n, snp_rate=0.02)]
    strs[-1] = strs[0]                                     # an identical pair: 0
    uniq, div, _ = _check_divergences(gpu_ctx, strs, 15, 15)
    assert uniq[n - 2] == 0 and div[n - 2] == 0.0         # pair (0, n - 1)


def test_divergences_with_empty_lists_are_nan(gpu_ctx):
    strs = ["ACGT", _rand(500), "", _rand(500), "N" * 40]
    uniq, div, _ = _check_divergences(gpu_ctx, strs, 15, 15)
    pairs = R.triangle_indices(5)
    assert np.isnan(div[pairs.index((0, 2))]) and np.isnan(div[pairs.index((2, 4))]) and uniq[pairs.index((0, 2))] == 0
    assert div[pairs.index((0, 1))] == 1.0


def test_divergences_of_multisets(gpu_ctx):
    """Tandem repeats of different lengths: the same hash with different multiplicities on the two sides, min(c_i, c_j) is what the merge counts."""
    strs = ["AC" * 2500, "AC" * 1800 + _rand(300), "A" * 5000, "A" * 3100 + "AC" * 900, _rand(700) + "AC" * 400]
    for (k, w) in [(15, 15), (5, 2)]:
        lists = [R.sorted_minimizers(s.encode(), k, w) for s in strs]
        cnt = [dict(zip(*np.unique(l, return_counts=True))) for l in lists]
        shared = [h for h in cnt[0] if h in cnt[1] and cnt[0][h] >= 3 and cnt[1][h] >= 3 and cnt[0][h] != cnt[1][h]]
        assert shared, "the case this test is about has vanished: no hash with multiplicity >= 3 and different counts on both sides"
        _check_divergences(gpu_ctx, strs, k, w)


def test_divergences_over_several_column_chunks(gpu_ctx):
    strs = [s.decode() for s in random_alleles(70, 3000, seed=4, snp_rate=0.03)] + ["AC" * 1500, "AC" * 900]
    seqs, off = _seqs(strs)
    one = api.db_divergences(gpu_ctx, seqs, off, 15, 15)
    gpu_ctx.set_knob("db_chunk_cols", 2048)
    try:
        uniq, div, _, st = api.db_divergences(gpu_ctx, seqs, off, 15, 15)
    finally:
        gpu_ctx.set_knob("db_chunk_cols", -1)
    assert one[3]["n_chunks"] == 1 and st["n_chunks"] >= 3 and st["n_columns"] == one[3]["n_columns"]
    assert np.array_equal(uniq, one[0]) and np.array_equal(div, one[1], equal_nan=True)
    assert np.array_equal(uniq, R.divergences([s.encode() for s in strs], 15, 15)[0])


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _off_target_case(k, counter_bytes, with_runs=True, seed=0):
    rng = np.random.default_rng(100 * k + counter_bytes + seed)
    maxv = R.max_value(counter_bytes)
    rep = _rand(60, rng)                                                       # every k-mer of it occurs three times in the reference
    poly = "A" * 50
    parts = [_rand(10, rng), "NNN" if with_runs else "ACG", _rand(80, rng), rep, _rand(70, rng), "N" * 50 if with_runs else _rand(50, rng),
             _rand(90, rng), rep, _rand(40, rng), poly, _rand(55, rng), rep, _rand(65, rng)]
    ref = "".join(parts)
    n_ref = len(ref) + 1 - k
    ref_counts = rng.integers(3, 60, n_ref).astype(np.uint16)
    p_rep = [ref.index(rep), ref.index(rep, ref.index(rep) + 1)]
    ref_counts[p_rep[0]:p_rep[0] + 61 - k] = 2                                 # first count 2, three occurrences: saturates, have_negatives
    ref_counts[p_rep[1]:p_rep[1] + 61 - k] = 40                                # a different count at a later occurrence: ignored by or_insert
    ref_counts[ref.index(poly):ref.index(poly) + 51 - k] = 9                   # A^k: its FIRST occurrence is the N run (count zeroed) when with_runs
    top = rng.choice(n_ref, 25, replace=False)
    ref_counts[top] = maxv                                                     # counts at the maximum stay
    ref_counts[p_rep[0] + 3] = maxv                                            # ... also for a repeated k-mer
    alleles = [
        ref.replace("N", "A")[20:400],
        _rand(100, rng) + _revcomp(ref[150:330].replace("N", "A")) + _rand(30, rng),      # reverse complements of reference k-mers
        ref.replace("N", "A")[300:420] + "N" + _rand(60, rng) + "n" + ref.replace("N", "A")[430:],       # holds N and a lower-case letter
        _rand(k - 1, rng), _rand(k, rng), "A" * 120,
    ]
    counts = [rng.integers(0, maxv + 1, max(len(a) + 1 - k, 0)).astype(np.uint16) for a in alleles]
    counts[0][:4] = maxv
    return ref, ref_counts, alleles, counts


@pytest.mark.parametrize("k", [25, 40])
@pytest.mark.parametrize("counter_bytes", [1, 2])
def test_off_target_counts_equal_the_hashmap_loop(gpu_ctx, k, counter_bytes):
    for with_runs in (True, False):
        ref, ref_counts, alleles, counts = _off_target_case(k, counter_bytes, with_runs)
        seqs, off = _seqs(alleles)
        flat, coff = _concat(counts, np.uint16)
        got, warn, st = api.db_off_target(gpu_ctx, seqs, off, flat, coff, k, counter_bytes, np.frombuffer(ref.encode(), dtype=np.uint8), ref_counts)
        want, neg, err = R.off_target([a.encode() for a in alleles], counts, k, counter_bytes, ref.encode(), ref_counts)
        assert np.array_equal(got, np.concatenate(want))
        assert neg and bool(warn & cdefs.DB_WARN_NEGATIVES_SEEN) and bool(warn & cdefs.DB_WARN_REF_MISMATCH) == err == (not with_runs)
        assert not np.array_equal(got, flat)                                   # the map was hit at all
    # a reference that agrees with its counts: no warning
    ref = _rand(300, np.random.default_rng(k))
    rc = np.full(len(ref) + 1 - k, 5, dtype=np.uint16)
    seqs, off = _seqs([ref[10:200]])
    old = np.full(191 - k, 7, dtype=np.uint16)
    got, warn, _ = api.db_off_target(gpu_ctx, seqs, off, old, [0, len(old)], k, counter_bytes, np.frombuffer(ref.encode(), dtype=np.uint8), rc)
    assert warn == 0 and np.all(got == 4)


def _table_for(names, strs, ref, k, counter_bytes, seed=1):
    rng = np.random.default_rng(seed)
    maxv = R.max_value(counter_bytes)
    counts = [rng.integers(0, min(maxv, 300) + 1, max(len(s) + 1 - k, 0)).astype(np.uint16) for s in strs + [ref]]
    return counts


@pytest.mark.parametrize("calc_div,k", [(1, 25), (0, 40)])
def test_build_locus_equals_its_parts_and_the_reference(gpu_ctx, tmp_path, calc_div, k):
    base = [s.decode() for s in random_alleles(6, 2500, seed=8, snp_rate=0.02)]
    strs = [base[0], base[1], base[0], base[2], base[3], base[1], base[4], base[0]]
    names = [f"hap{i}" for i in range(len(strs))]
    ref = base[5][:700] + "N" * 30 + base[5][730:]
    counts = _table_for(names, strs, ref, k, 2)
    seqs, off = _seqs(strs)
    flat, coff = _concat(counts, np.uint16)
    refb = np.frombuffer(ref.encode(), dtype=np.uint8)
    prm = api.db_params(calc_div=calc_div, div_k=15, div_w=10)
    res = api.db_build_locus(gpu_ctx, names, seqs, off, refb, flat, coff, k=k, counter_bytes=2, params=prm)
    want = R.build_locus(names, [s.encode() for s in strs], ref.encode(), counts, k, 2, 15, 10, bool(calc_div))
    assert list(res["kept"]) == want["kept"] == [0, 1, 3, 4, 6]
    for f in ("fasta", "kmers", "distances", "discarded"):
        assert res[f] == want[f], f
    assert (res["distances"] != b"") == bool(calc_div) and res["discarded"] == b"hap0 = hap2, hap7\nhap1 = hap5\n"
    # the composition of the single calls
    kept, _, text = api.db_discard_identical(names, seqs, off)
    kseqs, koff = _seqs([strs[i] for i in kept])
    kflat, kcoff = _concat([counts[i] for i in kept], np.uint16)
    offt, warn, _ = api.db_off_target(gpu_ctx, kseqs, koff, kflat, kcoff, k, 2, refb, counts[-1])
    assert res["kmers"] == io.kmer_counts_write(k, 2, kcoff, offt) + io.kmer_counts_write(k, 2, kcoff, kflat) and res["warn_bits"] == warn
    assert res["fasta"] == io.fasta_text([names[i] for i in kept], kseqs, koff) and res["discarded"] == text
    if calc_div:
        uniq, _, chk, _ = api.db_divergences(gpu_ctx, kseqs, koff, 15, 10)
        assert res["distances"] == io.distances_write(15, 10, len(kept), uniq) and res["check"] == chk
    # through the containers
    io.write_br(tmp_path / "kmers.bin.br", res["kmers"])
    assert io.read_file(tmp_path / "kmers.bin.br") == want["kmers"]
    io.write_gz(tmp_path / "haplotypes.fa.gz", res["fasta"])
    assert io.read_file(tmp_path / "haplotypes.fa.gz") == want["fasta"]
    # only_seqs: the FASTA alone, no counts needed
    only = api.db_build_locus(gpu_ctx, names, seqs, off, params=api.db_params(only_seqs=1))
    assert only["fasta"] == want["fasta"] and only["kmers"] == b"" and only["distances"] == b"" and only["discarded"] == want["discarded"]


def test_error_statuses_of_the_device_entries(gpu_ctx):
    def raises(code, fn):
        with pytest.raises(_lib.LocityperError) as e:
            fn()
        assert e.value.code == code and _lib.lib().lcty_last_error() != b""
    seqs, off = _seqs([_rand(100), _rand(100)])
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_minimizers(gpu_ctx, seqs, off, 15, 64))          # w = 64: the circular array holds 64 hashes
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_minimizers(gpu_ctx, seqs, off, 15, 0))
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_minimizers(gpu_ctx, seqs, off, 33, 15))
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_minimizers(gpu_ctx, seqs, off, 0, 15))
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_divergences(gpu_ctx, seqs, off, 15, 64))
    raises(cdefs.ERR_INVALID_DATA, lambda: api.db_divergences(gpu_ctx, seqs[:100], off[:2], 15, 15))          # fewer than two haplotypes
    cnt = [np.zeros(76, dtype=np.uint16), np.zeros(76, dtype=np.uint16)]
    flat, coff = _concat(cnt, np.uint16)
    ref = np.frombuffer(_rand(90).encode(), dtype=np.uint8)
    rc = np.zeros(66, dtype=np.uint16)
    api.db_off_target(gpu_ctx, seqs, off, flat, coff, 25, 2, ref, rc)
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_off_target(gpu_ctx, seqs, off, flat, coff, 1, 2, ref, rc))
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_off_target(gpu_ctx, seqs, off, flat, coff, 64, 2, ref, rc))
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_off_target(gpu_ctx, seqs, off, flat, coff, 25, 0, ref, rc))
    raises(cdefs.ERR_INVALID_DATA, lambda: api.db_off_target(gpu_ctx, seqs, off, flat[:151], [0, 76, 151], 25, 2, ref, rc))    # len + 1 - k
    raises(cdefs.ERR_INVALID_DATA, lambda: api.db_off_target(gpu_ctx, seqs, off, flat, coff, 25, 2, ref, rc[:65]))
    full, foff = _concat(cnt + [rc], np.uint16)
    raises(cdefs.ERR_INVALID_DATA, lambda: api.db_build_locus(gpu_ctx, ["a"], seqs[:100], off[:2], ref, full, foff[1:], 25, 2))
    raises(cdefs.ERR_INVALID_DATA, lambda: api.db_build_locus(gpu_ctx, ["a", "b"], seqs, off, ref, full[:-1], [0, 76, 152, 217], 25, 2))


def test_size_run_1024_haplotypes(gpu_ctx):
    """1 024 haplotypes x 50 kb. The Python merge of all 523 776 pairs is too slow for a test, so a seeded SAMPLE of 2 000 pairs is compared
    with it (a limit on cost, not a tolerance: every sampled value must be equal), and the whole u32 triangle must have the same sum — and
    the same values — in a second device pass with another chunk size."""
    L = synth.SynthLocus(1024, 16, base_len=50_000, seed=77)
    uniq, _, _, st = api.db_divergences(gpu_ctx, L.seqs, L.seq_off, 15, 15, with_f64=False)
    gpu_ctx.set_knob("db_chunk_cols", 2048)
    try:
        uniq2, _, _, st2 = api.db_divergences(gpu_ctx, L.seqs, L.seq_off, 15, 15, with_f64=False)
    finally:
        gpu_ctx.set_knob("db_chunk_cols", -1)
    assert st2["n_chunks"] > st["n_chunks"]
    assert int(uniq.astype(np.uint64).sum()) == int(uniq2.astype(np.uint64).sum()) and np.array_equal(uniq, uniq2)
    n_sample = 2000
    pairs = R.triangle_indices(1024)
    pick = np.random.default_rng(12345).choice(len(pairs), n_sample, replace=False)
    lists = {}
    for t in pick:
        for a in pairs[t]:
            if a not in lists:
                lists[a] = R.sorted_minimizers(L.allele(a), 15, 15)
    for t in pick:
        i, j = pairs[t]
        assert int(uniq[t]) == R.jaccard_distance(lists[i], lists[j])[0], (i, j)


def test_repeat_calls_and_a_resident_locus(gpu_ctx):
    """The build leaves nothing behind on the context: the same bytes again, and a locus resident beside it scores as before."""
    L = synth.SynthLocus(8, 2000, seed=31, base_len=10_000)
    p = api.resolve_params(api.default_params(), L.bg)
    loc = api.Locus(gpu_ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    ol = O.OracleLocus(L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    chunk = L.reads(0, 2000)
    names = [f"a{i}" for i in range(8)]
    ref = L.allele(0)
    counts = _table_for(names, [L.allele(a).decode() for a in range(8)], ref.decode(), 25, 2)
    flat, coff = _concat(counts, np.uint16)
    prm = api.db_params(calc_div=1)
    first = api.db_build_locus(gpu_ctx, names, L.seqs, L.seq_off, np.frombuffer(ref, dtype=np.uint8), flat, coff, 25, 2, prm)
    aa = api.AllAlignments.load(loc, chunk)
    second = api.db_build_locus(gpu_ctx, names, L.seqs, L.seq_off, np.frombuffer(ref, dtype=np.uint8), flat, coff, 25, 2, prm)
    for f in ("fasta", "kmers", "distances", "discarded"):
        assert first[f] == second[f] and (f == "discarded" or first[f])
    compare_gpu_to_oracle(aa, ol.load(chunk))
    aa2 = api.AllAlignments.load(loc, chunk)
    compare_gpu_to_oracle(aa2, ol.load(chunk))
