"""Genome k-mer counts on the device (lcty_genome.hip: pack, query table, scan, gather) against the serial restatement of
tests/pyref_kmer_count.py. Every comparison is integer or byte equality."""
import gzip

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from tests import pyref_kmer_count as R

pytestmark = pytest.mark.gpu
RUN = cdefs.GENOME_SCAN_RUN


def _concat(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), off


def _genome(ctx, contigs, piece=None):
    g = api.Genome(ctx)
    for name, seq in contigs:
        if piece is None or len(seq) <= piece:
            g.append(name, seq)
        else:
            for at in range(0, len(seq), piece):
                g.append(name if at == 0 else None, seq[at:at + piece], continues=at > 0)
    return g


def _counts(g, seqs, k, cb=2):
    sq, off = _concat(seqs)
    counts, cnt_off, st = g.kmer_counts(sq, off, k, cb)
    assert [int(x) for x in cnt_off] == [0] + list(np.cumsum([max(len(s) + 1 - k, 0) for s in seqs]))
    return [counts[int(cnt_off[i]):int(cnt_off[i + 1])] for i in range(len(seqs))], st


def _same(got, want):
    assert len(got) == len(want)
    for a, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == np.uint16 and np.array_equal(x, y), (a, np.flatnonzero(x != y)[:5] if len(x) == len(y) else (len(x), len(y)))


def _check(ctx, contigs, seqs, k, cb=2, piece=None):
    g = _genome(ctx, contigs, piece)
    got, st = _counts(g, seqs, k, cb)
    _same(got, R.kmer_counts(contigs, seqs, k, cb))
    g.close()
    return st


def _rand(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def _repetitive(rng, n, unit=37, rate=0.02):
    """n bases in which most k-mers occur several times: a random unit tiled, with point changes"""
    u = np.frombuffer(_rand(rng, unit), dtype=np.uint8)
    s = np.tile(u, n // unit + 1)[:n].copy()
    hit = rng.random(n) < rate
    s[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    return s.tobytes()


@pytest.mark.parametrize("k", [25, 31])
def test_every_length_across_the_word_edges_and_a_threads_run(gpu_ctx, k):
    """one contig of every length from 0 to k + 2 RUN + 70, queried with itself: the 16-, 32- and 64-base word edges of the packing and
    both ends of a scan thread's run. The hits are counted too: the floor of 1 cannot hide a k-mer the scan did not see."""
    rng = np.random.default_rng(100 + k)
    whole = _repetitive(rng, k + 2 * RUN + 70)
    for n in range(0, len(whole) + 1):
        seq = whole[:n]
        st = _check(gpu_ctx, [("c", seq)], [seq], k)
        assert st["n_hits"] == max(n + 1 - k, 0) == st["n_query_kmers"], n
        assert st["scan_run"] == RUN


def _five_contigs(rng, k):
    big1 = bytearray(_repetitive(rng, 120_000, unit=997, rate=0.01))
    big1[5_000:5_040] = b"N" * 40
    big1[60_000:62_000] = bytes(big1[60_000:62_000]).lower()
    big2 = _rand(rng, 60_000) + bytes(big1[10_000:30_000])
    return [("big1", bytes(big1)), ("short", _rand(rng, k - 1)), ("exact", bytes(big1[70_000:70_000 + k])), ("empty", b""), ("big2", big2)]


@pytest.mark.parametrize("k", [1, 3, 15, 25, 31])
def test_every_k_on_five_contigs(gpu_ctx, k):
    rng = np.random.default_rng(7)
    contigs = _five_contigs(rng, k)
    b1, b2 = contigs[0][1], contigs[4][1]
    seqs = [b1[9_000:14_000], b1[59_500:62_500].upper(), b2[58_000:63_000], contigs[2][1], contigs[1][1], _rand(rng, 1_000)]
    st = _check(gpu_ctx, contigs, seqs, k)
    assert st["n_scanned"] == sum(len(s) for _, s in contigs) + 4              # one separator in front of every contig but the first
    assert st["table_slots"] >= 2 * st["n_distinct"] and st["n_distinct"] <= st["n_query_kmers"]


M64 = (1 << 64) - 1


def _mix64(x):
    """mix64 of lcty_seq.hpp: the slot hash of the query table"""
    x ^= x >> 33; x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33; x = x * 0xc4ceb9fe1a85ec53 & M64
    return x ^ x >> 33


def _revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def _canonical(s):
    """the smaller of the k-mer and its reverse complement as 2-bit numbers, first base in the highest bits"""
    value = lambda t: int("".join(str(b"ACGT".index(c)) for c in t), 4)
    return min(value(s), value(_revcomp(s)))


def test_claim_compact_and_find_where_a_chain_wraps(gpu_ctx):
    """The key table of a call at its smallest (lcty_table.hpp): 18 distinct 15-mers, asked for 40 times each. The first table has
    2 048 slots and hundreds of threads claim equal keys at once; the compacted one has 64, four keys whose home is its last slot (their
    chain wraps to slot 0 and beyond) and two whose home is slot 0 (which the wrapped chain pushes on)."""
    rng = np.random.default_rng(41)
    k, last, first, others = 15, [], [], []
    seen = set()
    for _ in range(5_000):
        s = _rand(rng, k)
        c = _canonical(s)
        if c in seen:
            continue
        home = _mix64(c) & 63
        group = last if home == 63 and len(last) < 4 else first if home == 0 and len(first) < 2 else others if len(others) < 12 else None
        if group is not None:
            group.append(s); seen.add(c)
        if (len(last), len(first), len(others)) == (4, 2, 12):
            break
    chosen = last + first + others
    assert [_mix64(_canonical(s)) & 63 for s in chosen[:6]] == [63] * 4 + [0] * 2 and len(chosen) == len(seen) == 18
    # occurrence j of k-mer i is its reverse complement when j is odd; an N between any two
    times = [1 + i % 4 for i in range(len(chosen))]
    contigs = [("c", b"N".join(s if j % 2 == 0 else _revcomp(s) for i, s in enumerate(chosen) for j in range(times[i])))]
    seqs = chosen * 40
    g = _genome(gpu_ctx, contigs)
    got, st = _counts(g, seqs, k)
    assert st["n_query_kmers"] == 720 and st["n_distinct"] == 18 and st["table_slots"] == 64
    assert [int(x[0]) for x in got[:18]] == times
    _same(got, R.kmer_counts(contigs, seqs, k))
    g.close()


def test_non_bases_split_and_lower_case_counts(gpu_ctx):
    rng = np.random.default_rng(11)
    k = 9
    core = _repetitive(rng, 600, unit=23)
    contigs = [("n_start", b"N" + core[:100]), ("n_inside", core[:50] + b"N" + core[50:120]), ("n_end", core[:100] + b"N"),
               ("n_run", core[:40] + b"N" * (k + 3) + core[40:90]), ("n_close", core[:30] + b"N" + core[31:35] + b"N" + core[36:90]),
               ("all_n", b"N" * 50), ("iupac", core[:20] + b"R" + core[21:40] + b"y" + core[41:60] + b"KMSWBDHVkmswbdhvn" + core[60:100]),
               ("lower", core[:200] + core[200:400].lower() + core[400:])]
    seqs = [core, core[:100], _rand(rng, 200)]
    _check(gpu_ctx, contigs, seqs, k)
    upper = [(n, s.upper() if n == "lower" else s) for n, s in contigs]
    g1, g2 = _genome(gpu_ctx, contigs), _genome(gpu_ctx, upper)
    _same(_counts(g1, seqs, k)[0], _counts(g2, seqs, k)[0])
    for name, seq in contigs:
        assert g1.fetch(name, 0, len(seq)) == R.standardize(seq), name


@pytest.mark.parametrize("bad", [b"-", b"7", b"*", b"\n", b"U"])
def test_a_byte_that_is_no_nucleotide_names_contig_and_position(gpu_ctx, bad):
    g = api.Genome(gpu_ctx)
    g.append("chr1", b"ACGT" * 30)
    with pytest.raises(_lib.LocityperError) as e:
        g.append("chrBad", b"ACGTN" * 20 + bad + b"ACGT", continues=False)
    assert e.value.code == cdefs.ERR_INVALID_DATA
    assert "chrBad" in str(e.value) and "position 100" in str(e.value) and f"0x{bad[0]:02x}" in str(e.value)
    with pytest.raises(_lib.LocityperError) as e:                              # in a later piece of a contig: the position is the contig's
        g2 = api.Genome(gpu_ctx)
        g2.append("c", b"ACGT" * 10)
        g2.append(None, b"AC" + bad, continues=True)
    assert e.value.code == cdefs.ERR_INVALID_DATA and "position 42" in str(e.value)


def test_contig_junction_is_not_an_occurrence(gpu_ctx):
    rng = np.random.default_rng(13)
    k = 25
    c1, c2 = _rand(rng, 300), _rand(rng, 300)
    junction = c1[-(k - 1):] + c2[:1]
    contigs = [("c1", c1), ("c2", c2)]
    assert junction not in c1 and junction not in c2
    g = _genome(gpu_ctx, contigs)
    got, st = _counts(g, [junction, c1[-k:], c2[:k]], k)
    assert [list(x) for x in got] == [[1], [1], [1]] and st["n_hits"] == 2       # the junction's 1 is the floor, the others are seen
    _check(gpu_ctx, contigs, [c1[-40:] + c2[:40]], k)
    # as one contig the same k-mer is there
    got, st = _counts(_genome(gpu_ctx, [("c", c1 + c2)]), [junction], k)
    assert list(got[0]) == [1] and st["n_hits"] == 1


def test_pieces_of_any_length_give_the_same_genome(gpu_ctx):
    rng = np.random.default_rng(17)
    k = 25
    a = bytearray(_repetitive(rng, 1_700, unit=61))
    a[300:302] = b"NN"; a[700] = ord("R"); a[1_000:1_100] = bytes(a[1_000:1_100]).lower()
    contigs = [("a", bytes(a)), ("b", _rand(rng, k)), ("e", b""), ("c", b"N" + _repetitive(rng, 1_200, unit=61) + b"n")]
    seqs = [bytes(a[:300]), bytes(a[702:1_000]), contigs[3][1][1:-1], contigs[1][1]]
    want = R.kmer_counts(contigs, seqs, k)
    for piece in (1, k - 1, k, 1_000, None):
        g = _genome(gpu_ctx, contigs, piece)
        assert g.contigs() == [(n, len(s)) for n, s in contigs] and g.n_bases() == sum(len(s) for _, s in contigs)
        for name, seq in contigs:
            if seq:
                assert g.fetch(name, 0, len(seq)) == R.standardize(seq), (piece, name)
        _same(_counts(g, seqs, k)[0], want)
        g.close()


def test_clamp_and_seventy_thousand_adds_on_one_counter(gpu_ctx):
    k = 25
    contigs = [("a", b"A" * 70_000), ("t", b"T" * 300)]
    g = _genome(gpu_ctx, contigs)
    seqs = [b"A" * 40, b"T" * 40]
    for cb, want in ((2, 65_535), (1, 255), (4, 65_535)):
        got, st = _counts(g, seqs, k, cb)
        assert all(int(v) == want for x in got for v in x) and len(got[0]) == 16
        assert st["n_hits"] == 70_000 - 24 + 300 - 24 and st["n_distinct"] == 1
        _same(got, R.kmer_counts(contigs, seqs, k, cb))
    got, _ = _counts(_genome(gpu_ctx, [("t", b"T" * 300)]), seqs, k, 2)         # below the clamp: the exact number
    assert all(int(v) == 276 for x in got for v in x)


def test_query_side(gpu_ctx):
    rng = np.random.default_rng(19)
    k = 25
    long_q = _rand(rng, 300_000 + k - 1)
    contigs = [("c", _rand(rng, 30_000) + long_q[100_000:120_000] + long_q[5:3_000].lower())]
    g = _genome(gpu_ctx, contigs)
    table = R.genome_table(contigs, k)
    seqs = [b"", b"ACGT", long_q[100_000:100_500], long_q[100_000:100_500], _rand(rng, k), long_q]
    got, st = _counts(g, seqs, k)
    _same(got, R.query(table, seqs, k))
    assert len(got[0]) == 0 and len(got[1]) == 0 and np.array_equal(got[2], got[3]) and list(got[4]) == [1]
    assert st["n_distinct"] >= 300_000 and st["table_slots"] >= 1 << 20
    sq, off = _concat([b"ACGT" * 10, b"ACGTNACGT" * 5])
    with pytest.raises(_lib.LocityperError) as e:
        g.kmer_counts(sq, off, 5)
    assert e.value.code == cdefs.ERR_RUNTIME and "Cannot count k-mers for sequence with Ns" in str(e.value)
    for bad in (b"ACGTaCGT", b"ACGTRCGT", b"ACG-T"):
        sq, off = _concat([bad])
        with pytest.raises(_lib.LocityperError) as e:
            g.kmer_counts(sq, off, 3)
        assert e.value.code == cdefs.ERR_INVALID_INPUT
    got, _ = _counts(g, [], k)                                                  # no sequence at all
    assert got == []


def test_nothing_of_a_call_is_seen_by_the_next(gpu_ctx):
    rng = np.random.default_rng(23)
    contigs = [("x", _repetitive(rng, 20_000, unit=501)), ("y", _rand(rng, 5_000))]
    x = contigs[0][1]
    calls = [(25, [x[:2_000], x[7_000:7_100]]), (15, [x[1_000:1_500], _rand(rng, 300)]), (31, [x[100:900]]), (25, [x[:2_000], x[7_000:7_100]])]
    g = _genome(gpu_ctx, contigs)
    for k, seqs in calls:
        got, st = _counts(g, seqs, k)
        fresh, st2 = _counts(_genome(gpu_ctx, contigs), seqs, k)
        _same(got, fresh)
        _same(got, R.kmer_counts(contigs, seqs, k))
        assert st["n_hits"] == st2["n_hits"]


def test_fetch_windows_and_their_errors(gpu_ctx):
    rng = np.random.default_rng(29)
    a = bytearray(_rand(rng, 500))
    a[100:140] = bytes(a[100:140]).lower(); a[140:150] = b"NRYKMSWBDH"
    contigs = [("chrA", bytes(a)), ("chrB", _rand(rng, 77))]
    g = _genome(gpu_ctx, contigs)
    std = R.standardize(bytes(a))
    for s, e in ((0, 1), (0, 500), (499, 500), (90, 160), (139, 141), (31, 33), (0, 64)):
        assert g.fetch("chrA", s, e) == std[s:e], (s, e)
    assert g.fetch("chrB", 0, 77) == contigs[1][1] and g.fetch("chrB", 76, 77) == contigs[1][1][76:]
    for name, s, e in (("chrA", 5, 5), ("chrA", 6, 5), ("chrA", 0, 501), ("chrB", 77, 78), ("chrC", 0, 1)):
        with pytest.raises(_lib.LocityperError) as err:
            g.fetch(name, s, e)
        assert err.value.code == cdefs.ERR_INVALID_INPUT, (name, s, e)


def _fasta(contigs, width, eol):
    out = b""
    for name, seq in contigs:
        out += b">" + name.encode() + b" some description" + eol
        for at in range(0, len(seq), width):
            out += seq[at:at + width] + eol
    return out


def test_load_fasta_plain_gzip_and_crlf(gpu_ctx, tmp_path):
    rng = np.random.default_rng(31)
    k = 25
    a = bytearray(_repetitive(rng, 40_000, unit=777))
    a[1_000:1_050] = b"N" * 50; a[2_000:2_500] = bytes(a[2_000:2_500]).lower()
    contigs = [("chr1", bytes(a)), ("chr2", _rand(rng, 59)), ("chr3", _rand(rng, 60)), ("chr4", _rand(rng, 10_001))]
    seqs = [bytes(a[3_000:6_000]), contigs[3][1][:500]]
    want, _ = _counts(_genome(gpu_ctx, contigs), seqs, k)
    _same(want, R.kmer_counts(contigs, seqs, k))
    files = {"plain.fa": _fasta(contigs, 60, b"\n"), "crlf.fa": _fasta(contigs, 60, b"\r\n"), "one_line.fa": _fasta(contigs, 1 << 30, b"\n")}
    for name, text in files.items():
        (tmp_path / name).write_bytes(text)
    with gzip.open(tmp_path / "zipped.fa.gz", "wb") as f:
        f.write(files["crlf.fa"])
    for name in list(files) + ["zipped.fa.gz"]:
        g = api.Genome.from_fasta(gpu_ctx, tmp_path / name)
        assert g.contigs() == [(n, len(s)) for n, s in contigs], name
        _same(_counts(g, seqs, k)[0], want)
        assert g.fetch("chr1", 990, 1_060) == R.standardize(bytes(a[990:1_060]))
        g.close()
    (tmp_path / "headless.fa").write_bytes(b"ACGT\n>c\nACGT\n")
    with pytest.raises(_lib.LocityperError) as e:
        api.Genome.from_fasta(gpu_ctx, tmp_path / "headless.fa")
    assert e.value.code == cdefs.ERR_INVALID_DATA
    with pytest.raises(_lib.LocityperError) as e:
        api.Genome.from_fasta(gpu_ctx, tmp_path / "missing.fa")
    assert e.value.code == cdefs.ERR_INVALID_INPUT


def test_the_base_limit_refuses_before_anything_is_uploaded(gpu_ctx):
    """2^32 positions is the limit of the 32-bit counters; the knob lowers it to where a test can reach it"""
    rng = np.random.default_rng(37)
    gpu_ctx.set_knob("genome_max_bases", 1_000)
    try:
        g = api.Genome(gpu_ctx)
        first = _rand(rng, 600)
        g.append("a", first)
        for name, n, cont in (("b", 399, False), (None, 400, True), ("b", 5_000, False)):   # 600 + separator + 399 = 1 000: not below the limit
            with pytest.raises(_lib.LocityperError) as e:
                g.append(name, _rand(rng, n), continues=cont)
            assert e.value.code == cdefs.ERR_UNSUPPORTED and "genome_max_bases" in str(e.value)
        assert g.contigs() == [("a", 600)] and g.n_bases() == 600             # nothing of the refused pieces is there
        g.append("b", _rand(rng, 398))
        assert g.n_bases() == 998 and g.fetch("a", 0, 600) == first
        _same(_counts(g, [first], 25)[0], R.kmer_counts([("a", first), ("b", g.fetch("b", 0, 398))], [first], 25))
    finally:
        gpu_ctx.set_knob("genome_max_bases", -1)
