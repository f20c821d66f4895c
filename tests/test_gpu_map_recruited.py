"""lcty_reads_map_append_recruited: the in-locus mapper fed from a resident set of recruited reads leaves the batch as
lcty_reads_map_append of the host chunk of the same pairs (tests/pyref_recruited.py builds it) does — the records, the CIGAR words, and
after lcty_score_reads the status, the unique k-mer counts (read from the re-oriented bases), the pair alignments and the matrix —
over the whole range and in three uneven parts, on both routes."""
import numpy as np
import pytest

from locityper_amd import api, cdefs
from locityper_amd._lib import LocityperError
from tests import pyref_recruited as PR
from tests.helpers import locus_arrays, make_bg, random_alleles
from tests.test_gpu_recruited import chunk_of, make_targets
from tests.test_gpu_sample_bam import _two_loci
from tests.test_oracle_recruit import revcomp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    """the session's context: it outlives every batch and locus made on it here, whenever the collector gets to them"""
    return gpu_ctx


def host_chunk(E, l):
    mate_len, mate_off, b2, nm, _ = E.locus(l)
    z = np.zeros(len(mate_len) // 2 + 1, dtype=np.uint64)
    return cdefs.ReadsChunk(mate_len, mate_off, np.concatenate([b2, [0, 0]]).astype(np.uint32), np.concatenate([nm, [0]]).astype(np.uint32), z,
                            np.zeros(0, dtype=cdefs.ALN_REC_DTYPE), z, np.zeros(0, dtype=np.uint32))


def batches_equal(a, b, scored):
    for x, y in zip(a.records(), b.records()):
        assert np.array_equal(x, y)
    if scored:
        assert a.n_good() == b.n_good()
        for x, y in zip(a.status(), b.status()):
            assert np.array_equal(x, y)
        (o1, p1), (o2, p2) = a.pair_alns(), b.pair_alns()
        assert np.array_equal(o1, o2) and np.array_equal(p1, p2)
        assert np.array_equal(a.best_aln_matrix(), b.best_aln_matrix())


def three_routes(loc, rset, l, chunk, mp, parts):
    """the batch of locus l's reads: from the host chunk, from the set at once, from the set in parts"""
    sized = api.map_reads(loc, chunk, mp)
    make = lambda: api.AllAlignments(loc, chunk.n_pairs, chunk.n_bases, len(sized.recs), len(sized.cigar))
    via_host, whole, in_parts = make(), make(), make()
    api.map_append(via_host, chunk, mp)
    api.map_append_recruited(whole, rset, l, mp)
    at = 0
    for k in parts:
        api.map_append_recruited(in_parts, rset, l, mp, first_pair=at, n_pairs=k)
        at += k
    assert at == chunk.n_pairs and whole.n_pairs == in_parts.n_pairs == via_host.n_pairs == chunk.n_pairs
    for b in (whole, in_parts):
        batches_equal(b, via_host, scored=False)
    for b in (via_host, whole, in_parts):
        b.score()
    for b in (whole, in_parts):
        batches_equal(b, via_host, scored=True)
    return via_host, whole, in_parts


def test_short_route_from_the_set_equals_the_host_chunk(ctx):
    loci = _two_loci()
    rng = np.random.default_rng(4)
    pairs = []
    for i in range(400):
        if i % 4 == 3:                                                       # a foreign pair
            s1, s2 = (bytes(rng.choice(list(b"ACGT"), 150).astype(np.uint8).tolist()) for _ in range(2))
        else:
            al = loci[i % 2][int(rng.integers(0, 3))]
            p = int(rng.integers(0, len(al) - 500))
            s1, s2 = al[p:p + 150], revcomp(al[p + 300:p + 450])
        pairs.append((s1, s2))
    chunk = chunk_of(pairs)
    bg = make_bg()
    prm = api.resolve_params(api.default_params(), bg)
    targets = api.Targets(ctx, api.recruit_params(paired=True))
    locs = []
    for alleles in loci:
        seqs, seq_off, cflat, cnt_off, _ = locus_arrays(alleles, 25)
        targets.add_locus(seqs, seq_off, cflat, cnt_off, 25)
        locs.append(api.Locus(ctx, seqs, seq_off, cflat, cnt_off, 25, bg, prm))
    targets.finalize()
    rset, E = api.Recruited(targets), PR.Expected(2)
    for lo, hi in ((0, 130), (130, 400)):                                    # two adds
        part = chunk.slice(lo, hi)
        cnt, out_loci = targets.recruit(part)
        rset.add(part, cnt, out_loci)
        E.add(part, cnt, out_loci)
    mp = api.map_params()
    for l, loc in enumerate(locs):
        api.build_map_index(loc, [0, 1, 2], k=mp.k)
        hc = host_chunk(E, l)
        n = hc.n_pairs
        assert n == rset.sizes(l)[0] and n > 120
        via_host, whole, in_parts = three_routes(loc, rset, l, hc, mp, (7, n - 50, 43))
        assert via_host.n_good() > 50
        # edge ranges: nothing to do; past the end
        api.map_append_recruited(whole, rset, l, mp, first_pair=n, n_pairs=0)
        api.map_append_recruited(whole, rset, l, mp, first_pair=3, n_pairs=0)
        assert whole.n_pairs == n
        for first, k in ((0, n + 1), (n - 1, 2), (n + 1, 0)):
            with pytest.raises(LocityperError) as e:
                api.map_append_recruited(whole, rset, l, mp, first_pair=first, n_pairs=k)
            assert e.value.code == cdefs.ERR_INVALID_INPUT
        with pytest.raises(LocityperError) as e:
            api.map_append_recruited(whole, rset, 2, mp, first_pair=0, n_pairs=0)
        assert e.value.code == cdefs.ERR_INVALID_INPUT
    # a batch of another context
    other = api.Context(0)
    seqs, seq_off, cflat, cnt_off, _ = locus_arrays(loci[0], 25)
    far = api.Locus(other, seqs, seq_off, cflat, cnt_off, 25, bg, prm)
    api.build_map_index(far, [0], k=mp.k)
    batch = api.AllAlignments(far, 10, 10_240, 100, 1000)
    try:
        with pytest.raises(LocityperError) as e:
            api.map_append_recruited(batch, rset, 0, mp, first_pair=0, n_pairs=5)
        assert e.value.code == cdefs.ERR_INVALID_INPUT and "context" in str(e.value)
    finally:
        # a context outlives what was made on it: closed here, in that order, not left to the collector (the traceback of a caught
        # error keeps this frame in a cycle, whose objects are finalized in any order)
        batch.close(); far.close(); other.close()
    rset.close()


def test_long_route_from_the_set_equals_the_host_chunk(ctx):
    rng = np.random.default_rng(6)
    alleles = random_alleles(3, 8000, seed=12)
    bg = make_bg(technology=cdefs.TECH_NANOPORE, paired=False)
    prm = api.resolve_params(api.default_params(), bg)
    seqs, seq_off, cflat, cnt_off, _ = locus_arrays(alleles, 25)
    loc = api.Locus(ctx, seqs, seq_off, cflat, cnt_off, 25, bg, prm)
    reads = []
    for i in range(64):
        al = bytearray(alleles[int(rng.integers(0, 3))])
        ln = int(rng.integers(2800, 3200))
        at = int(rng.integers(0, len(al) - ln))
        s = al[at:at + ln]
        for q in rng.integers(0, ln, 12):                                    # a few substitutions, one base that is not ACGT
            s[q] = ord("ACGT"[int(rng.integers(0, 4))])
        s[int(rng.integers(0, ln))] = ord("N")
        reads.append((revcomp(bytes(s)) if i % 3 == 0 else bytes(s), None))
    chunk = chunk_of(reads)
    targets = make_targets(ctx, 2)                                           # the set needs loci, the answers are designed
    cnt = np.ones(64, dtype=np.uint32)
    out_loci = np.array([[0 if i % 4 else 1] for i in range(64)], dtype=np.uint32)
    rset, E = api.Recruited(targets), PR.Expected(2)
    for lo, hi in ((0, 20), (20, 64)):
        part = chunk.slice(lo, hi)
        rset.add(part, cnt[lo:hi], out_loci[lo:hi], paired=False)
        E.add(part, cnt[lo:hi], out_loci[lo:hi])
    mp = api.map_params(long_reads=True, route=cdefs.MAP_ROUTE_LONG)
    api.build_map_index(loc, [0, 1, 2], k=mp.k)
    hc = host_chunk(E, 0)
    assert hc.n_pairs == 48
    via_host, whole, in_parts = three_routes(loc, rset, 0, hc, mp, (5, 30, 13))
    recs = via_host.records()[1]
    assert int(((recs["flags"] & cdefs.FLAG_UNMAPPED) == 0).sum()) >= 40 and int(recs["n_cigar"].max()) > 1 and via_host.n_good() > 0
    rset.close()
