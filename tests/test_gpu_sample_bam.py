"""lcty_sample_bam_fetch on the device against the index-free restatement (tests/pyref_sample_bam.py): the fetched stream, the pairs in
the reference's order, the packed bases word for word, recruitment from the device-resident reads, the writer, every error status.
Files of at most a few thousand records in BGZF blocks of 512 - 4 096 bytes: records and chunk ends straddle blocks."""
import struct

import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from locityper_amd._lib import LocityperError
from tests import oracle_ffi as O
from tests import pyref_sample_bam as P
from tests import sample_bam_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _two_loci():
    """two loci of three alleles of 3 000 bases; locus 1 holds a stretch of locus 0 (reads from it belong to both)"""
    rng = np.random.default_rng(21)
    loci = []
    for _ in range(2):
        base = rng.choice(list(b"ACGT"), 3000).astype(np.uint8)
        alleles = []
        for _ in range(3):
            s = base.copy(); m = rng.random(3000) < 0.01
            s[m] = rng.choice(list(b"ACGT"), int(m.sum()))
            alleles.append(bytes(s))
        loci.append(alleles)
    loci[1] = [a[:1000] + loci[0][0][500:1500] + a[2000:] for a in loci[1]]
    return loci


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    """the seeded file (a third of its pairs drawn from two loci), its records, and the restatement's answer for all regions + the tail"""
    d = tmp_path_factory.mktemp("gpu_sample_bam")
    loci = _two_loci()
    recs = S.seeded_records(loci=loci)
    path = str(d / "seeded.bam")
    P.write_bam(path, S.SEEDED_REFS, recs, block_size=1500)
    return dict(path=path, recs=recs, loci=loci, exp=S.expected(recs, S.SEEDED_REGIONS, True, True), dir=d)


def _assert_equal(reads, exp, paired):
    src, mates, n_kept, n_discarded = exp
    chunk, got_src, got_paired = reads.view()
    assert got_paired == paired
    assert reads.stats["records_kept"] == n_kept and reads.stats["n_pairs"] == len(mates) and reads.stats["n_discarded"] == n_discarded
    assert got_src.tolist() == src.tolist()
    mate_len, mate_off, bases2, nmask = P.packed(mates)
    assert chunk.mate_len.tolist() == mate_len.tolist() and chunk.mate_off.tolist() == mate_off.tolist()
    assert np.array_equal(chunk.bases2[:len(bases2)], bases2) and np.array_equal(chunk.nmask[:len(nmask)], nmask)
    return chunk


def test_hand_made_file(ctx, tmp_path):
    recs = S.hand_records()
    path = str(tmp_path / "hand.bam")
    P.write_bam(path, S.HAND_REFS, recs, block_size=512)
    exp = S.expected(recs, S.HAND_REGIONS, True, True)
    assert exp[2] == len(S.HAND_STREAM) and exp[3] == S.HAND_DISCARDED and len(exp[1]) == len(S.HAND_PAIRS)
    bam = lio.SampleBam(path)
    reads = bam.fetch(ctx, S.HAND_REGIONS, with_unmapped=True)              # paired: asked of the file
    _assert_equal(reads, exp, True)
    assert reads.stats["records_primary"] <= reads.stats["records_walked"] <= len(recs)
    _assert_equal(bam.fetch(ctx, S.HAND_REGIONS, with_unmapped=False, paired=True), S.expected(recs, S.HAND_REGIONS, False, True), True)
    _assert_equal(bam.fetch(ctx, S.HAND_REGIONS, with_unmapped=True, paired=False), S.expected(recs, S.HAND_REGIONS, True, False), False)


def test_stream_and_pairs_of_the_seeded_file(ctx, seeded):
    recs, (src, mates, n_kept, n_discarded) = seeded["recs"], seeded["exp"]
    # what the file must cover
    stream = P.fetched_stream(recs, S.SEEDED_REGIONS, True)
    in_stream = set(stream)
    assert any(r["flag"] & 0x100 for r in recs) and any(r["flag"] & 0x800 for r in recs)
    assert any(r["tid"] == 0 and r["pos"] < 10_000 < P.endpos(r) for r in recs)                       # reaches into a region
    assert any(r["tid"] == 0 and 13_900 <= r["pos"] < 14_000 and P.endpos(r) > 14_000 for r in recs)   # pos < min_start of the adjacent region
    assert any((r["flag"] & 4) and r["tid"] >= 0 and j in in_stream for j, r in enumerate(recs))
    assert n_discarded > 10 and len(mates) > 300 and any(recs[j]["tid"] < 0 for j in stream)
    bam = lio.SampleBam(seeded["path"])
    reads = bam.fetch(ctx, S.SEEDED_REGIONS, with_unmapped=True)
    _assert_equal(reads, seeded["exp"], True)
    st = reads.stats
    assert st["n_regions"] == 5 and st["records_walked"] < len(recs) and st["bytes_read"] < st["file_bytes"]
    # a second call: bit-identical
    again = bam.fetch(ctx, S.SEEDED_REGIONS, with_unmapped=True)
    a, b = reads.view(), again.view()
    for x, y in zip((a[0].mate_len, a[0].mate_off, a[0].bases2, a[0].nmask, a[1]), (b[0].mate_len, b[0].mate_off, b[0].bases2, b[0].nmask, b[1])):
        assert np.array_equal(x, y)
    # single-end over the same regions, and every region on its own
    _assert_equal(bam.fetch(ctx, S.SEEDED_REGIONS, with_unmapped=True, paired=False), S.expected(recs, S.SEEDED_REGIONS, True, False), False)
    for region in S.SEEDED_REGIONS:
        _assert_equal(bam.fetch(ctx, [region], paired=True), S.expected(recs, [region], False, True), True)


@pytest.mark.parametrize("bits", [4, 0])
def test_pairing_under_hash_collisions(ctx, seeded, bits):
    ctx.set_knob("sample_bam_hash_bits", bits)
    try:
        _assert_equal(lio.SampleBam(seeded["path"]).fetch(ctx, S.SEEDED_REGIONS, with_unmapped=True), seeded["exp"], True)
    finally:
        ctx.set_knob("sample_bam_hash_bits", -1)


@pytest.mark.parametrize("bits", [-1, 0])
def test_names_that_differ_in_the_last_character_or_by_a_prefix(ctx, tmp_path, bits):
    rng = np.random.default_rng(4)
    names = ["read1", "read2", "read", "read11", "r", "read1x", "x" * 250 + "a", "x" * 250 + "b", "abcd", "abce", "abc"]
    recs = []
    for k, nm in enumerate(names):
        recs.append(P.rec(0, 100 + k, nm, 0x41, [("M", 50)], S._seq(rng, 50), None, 0, 400 + k))
    for k, nm in reversed(list(enumerate(names))):
        recs.append(P.rec(0, 400 + (len(names) - k), nm, 0x81, [("M", 50)], S._seq(rng, 50), None, 0, 100 + k))
    path = str(tmp_path / "names.bam")
    P.write_bam(path, S.HAND_REFS, recs, block_size=700)
    exp = S.expected(recs, [(0, 0, 1000)], False, True)
    assert len(exp[1]) == len(names) and exp[3] == 0
    ctx.set_knob("sample_bam_hash_bits", bits)
    try:
        _assert_equal(lio.SampleBam(path).fetch(ctx, [(0, 0, 1000)]), exp, True)
    finally:
        ctx.set_knob("sample_bam_hash_bits", -1)


LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 500, 501, 10_007]


def test_unpacking_at_the_edges(ctx, tmp_path):
    """single-end reads of the lengths at which the packing changes words, forward and reverse; every BAM code at the first, the last and a
    word-boundary position"""
    rng = np.random.default_rng(6)
    recs, pos = [], 100
    for ln in LENGTHS:
        for flag in (0, 0x10):
            recs.append(P.rec(0, pos, f"l{ln}_{flag}", flag, [("M", ln)], S._seq(rng, ln), bytes(rng.integers(0, 41, ln).tolist())))
            pos += 1
    for code in P.CODES:
        for flag in (0, 0x10):
            for ln in (33, 48, 70):
                s = list(S._seq(rng, ln))
                for at in (0, ln - 1, 15, 16, 31, 32):
                    s[at] = code
                recs.append(P.rec(0, pos, f"c{P.CODES.index(code)}_{flag}_{ln}", flag, [("M", ln)], "".join(s)))
                pos += 1
    path = str(tmp_path / "edges.bam")
    P.write_bam(path, S.HAND_REFS, recs, block_size=4096)
    regions = [(0, 0, 50_000)]
    reads = lio.SampleBam(path).fetch(ctx, regions)
    chunk = _assert_equal(reads, S.expected(recs, regions, False, False), False)
    assert chunk.n_pairs == len(recs) and int(chunk.mate_len.max()) == 10_007
    # the whole file as DirectBamReader reads it: the same reads
    _assert_equal(lio.SampleBam(path).fetch(ctx, whole_file=True), S.expected(recs, [], False, False, whole_file=True), False)


def test_whole_file_single_end(ctx, seeded):
    recs = seeded["recs"]
    exp = S.expected(recs, [], False, False, whole_file=True)
    assert exp[2] == sum((r["flag"] & 0x900) == 0 for r in recs)
    _assert_equal(lio.SampleBam(seeded["path"]).fetch(ctx, whole_file=True, paired=False), exp, False)


@pytest.mark.parametrize("reach", [0, 1])
def test_long_cigar_decides_the_overlap_by_one_base(ctx, tmp_path, reach):
    """a record of 3 000 CIGAR operations that ends exactly at the region's start (not fetched), or one base behind it (fetched)"""
    ops = []
    for k in range(1000):
        ops += [("M", 3), ("I", 1), ("D", 2)]
    ref_len = 5000
    ops[-1] = ("D", 2 + reach)
    seq = S._seq(np.random.default_rng(8), 4000)
    recs = [P.rec(0, 1000, "long", 0, ops, seq), P.rec(0, 7000, "after", 0, [("M", 10)], "ACGTACGTAC")]
    assert P.rlen(recs[0]) == ref_len + reach and len(ops) == 3000
    path = str(tmp_path / "long.bam")
    P.write_bam(path, S.HAND_REFS, recs, block_size=1024)
    regions = [(0, 6000, 8000)]
    exp = S.expected(recs, regions, False, False)
    assert exp[2] == 1 + reach
    _assert_equal(lio.SampleBam(path).fetch(ctx, regions), exp, False)


def _targets(ctx, loci, paired=True, base_k=25):
    prm = api.recruit_params(paired=paired)
    gt = api.Targets(ctx, prm)
    ot = O.OracleTargets(prm.minimizer_k, prm.minimizer_w, prm.match_frac, prm.match_length, prm.thresh_kmer_count)
    for alleles in loci:
        counts = [np.zeros(len(a) - base_k + 1, dtype=np.uint16) for a in alleles]
        seqs = np.frombuffer(b"".join(alleles), dtype=np.uint8)
        seq_off = np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64)
        cnt_off = np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64)
        gt.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, base_k)
        ot.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, base_k)
    gt.finalize(); ot.finalize()
    return gt, ot


def test_recruitment_and_writer(ctx, seeded):
    """recruitment from the device-resident reads = lcty_recruit on their view = the oracle on the restatement's sequences; the per-locus
    files = the restatement's bytes"""
    src, mates, _, _ = seeded["exp"]
    recs = seeded["recs"]
    gt, ot = _targets(ctx, seeded["loci"])
    reads = lio.SampleBam(seeded["path"]).fetch(ctx, S.SEEDED_REGIONS, with_unmapped=True)
    cnt, loci = reads.recruit(gt)
    chunk, _, _ = reads.view()
    cnt2, loci2 = gt.recruit(chunk, paired=True)
    answered = np.arange(loci.shape[1])[None, :] < cnt[:, None]              # the entries behind out_cnt are not written
    assert np.array_equal(cnt, cnt2) and np.array_equal(loci[answered], loci2[answered])
    for i, (m1, m2) in enumerate(mates):
        assert loci[i, :cnt[i]].tolist() == ot.recruit(m1.encode(), m2.encode()), i
    assert (cnt > 0).sum() > 50 and (cnt == 2).sum() > 0 and (cnt == 0).sum() > 50
    # the writer
    stream = P.fetched_stream(recs, S.SEEDED_REGIONS, True)
    paths = [str(seeded["dir"] / f"locus{k}.fq") for k in range(2)]
    w = lio.FastxWriters(paths)
    assert reads.write_recruited(w, cnt, loci) == int((cnt > 0).sum())
    w.close()
    want = [b"", b""]
    for i in range(len(mates)):
        text = P.record_text(recs[stream[src[2 * i]]]) + P.record_text(recs[stream[src[2 * i + 1]]])
        for k in loci[i, :cnt[i]].tolist():
            want[k] += text
    for k in range(2):
        assert open(paths[k], "rb").read() == want[k] and len(want[k]) > 1000
    # ... which lcty_fastx_open reads back to the same pairs
    fx = lio.Fastx(paths[0], interleaved=True)
    back = fx.next(1 << 20)
    sel = [i for i in range(len(mates)) if 0 in loci[i, :cnt[i]].tolist()]
    ml, mo, b2, nm = P.packed([mates[i] for i in sel])
    assert back.mate_len.tolist() == ml.tolist() and np.array_equal(back.bases2[:len(b2)], b2) and np.array_equal(back.nmask[:len(nm)], nm)
    gt.close()


def test_writer_formats(ctx, tmp_path):
    """FASTQ forward and reverse, FASTA when the qualities start with 255, a read of 700 bases (the reference writes qualities 512 at a time)"""
    rng = np.random.default_rng(12)
    q = lambda n: bytes(rng.integers(0, 60, n).tolist())
    recs = [P.rec(0, 10, "fwd", 0, [("M", 40)], S._seq(rng, 40), q(40)), P.rec(0, 11, "rev", 0x10, [("M", 40)], S._seq(rng, 39) + "R", q(40)),
            P.rec(0, 12, "noq", 0x10, [("M", 40)], S._seq(rng, 40), None), P.rec(0, 13, "q255", 0, [("M", 40)], S._seq(rng, 40), b"\xff" + q(39)),
            P.rec(0, 14, "long", 0x10, [("M", 700)], S._seq(rng, 700), q(700)), P.rec(0, 15, "longf", 0, [("M", 700)], S._seq(rng, 700), q(700))]
    path = str(tmp_path / "w.bam")
    P.write_bam(path, S.HAND_REFS, recs, block_size=600)
    reads = lio.SampleBam(path).fetch(ctx, [(0, 0, 1000)], paired=False)
    out = [str(tmp_path / "a.fq"), str(tmp_path / "b.fq")]
    w = lio.FastxWriters(out)
    cnt = np.array([1, 1, 2, 1, 1, 0], dtype=np.uint32)
    loci = np.array([[0, 0], [0, 0], [0, 1], [1, 0], [0, 0], [0, 0]], dtype=np.uint32)
    assert reads.write_recruited(w, cnt, loci) == 5
    w.close()
    assert open(out[0], "rb").read() == b"".join(P.record_text(recs[i]) for i in (0, 1, 2, 4))
    assert open(out[1], "rb").read() == b"".join(P.record_text(recs[i]) for i in (2, 3))


def _refused(ctx, path, status, name, regions=((0, 0, 90_000),), **kw):
    with pytest.raises(LocityperError) as err:
        lio.SampleBam(path).fetch(ctx, list(regions), **kw)
    assert err.value.code == status, str(err.value)
    assert name in str(err.value), str(err.value)


def test_every_error_status(ctx, tmp_path):
    R, M = P.rec, [("M", 4)]
    ok = [R(0, 10 + k, f"ok{k // 2}", 0x41 if k % 2 == 0 else 0x81, M, "ACGT", None, 0, 10 + (k ^ 1)) for k in range(6)]
    path = str(tmp_path / "e.bam")

    def write(records, **kw):
        P.write_bam(path, S.HAND_REFS, records, block_size=512, **kw)

    # a record without 0x40 / 0x80 in paired mode; the first of two offenders is named
    write(ok + [R(0, 50, "solo", 0x1, M, "ACGT"), R(0, 51, "solo2", 0x1, M, "ACGT")])
    _refused(ctx, path, cdefs.ERR_INVALID_DATA, "read solo is unpaired", paired=True)
    lio.SampleBam(path).fetch(ctx, [(0, 0, 90_000)], paired=False)                    # single-end: nothing wrong with it
    # two first mates
    write(ok + [R(0, 50, "twice", 0x41, M, "ACGT", None, 0, 60), R(0, 60, "twice", 0x41, M, "ACGT", None, 0, 50)])
    _refused(ctx, path, cdefs.ERR_INVALID_DATA, "alignments for twice for the same read end", paired=True)
    # a primary without sequence (a secondary without one is fine)
    write(ok + [R(0, 50, "sec", 0x141, M, ""), R(0, 51, "bare", 0x41, M, "", None, 0, 70)])
    _refused(ctx, path, cdefs.ERR_INVALID_DATA, "read bare has no sequence")
    # a record length that leaves the slice
    blobs = [P.record_bytes(r) for r in ok]
    blobs[-1] = struct.pack("<I", 1_000_000) + blobs[-1][4:]
    write(ok, raw_records=blobs)
    _refused(ctx, path, cdefs.ERR_INVALID_DATA, "leaves the slice")
    # ... and one that is shorter than its fields (l_seq says 4 000 bases)
    blobs = [P.record_bytes(r) for r in ok]
    blobs[2] = blobs[2][:20] + struct.pack("<I", 4000) + blobs[2][24:]
    write(ok, raw_records=blobs)
    _refused(ctx, path, cdefs.ERR_INVALID_DATA, "shorter than its fields")
    # the placeholder of a CIGAR kept in a CG tag: kSmN
    write(ok + [R(0, 50, "huge", 0x41, [("S", 4), ("N", 70_000)], "ACGT", None, 0, 70)])
    _refused(ctx, path, cdefs.ERR_UNSUPPORTED, "huge")
    # coordinates that run backwards
    write(ok + [R(0, 500, "late", 0x41, M, "ACGT", None, 0, 70), R(0, 400, "early", 0x81, M, "ACGT", None, 0, 70)])
    _refused(ctx, path, cdefs.ERR_INVALID_DATA, "early")
    # a slice over the cap
    write(ok)
    ctx.set_knob("sample_bam_max_slice_bytes", 100)
    try:
        _refused(ctx, path, cdefs.ERR_UNSUPPORTED, "sample_bam_max_slice_bytes")
    finally:
        ctx.set_knob("sample_bam_max_slice_bytes", -1)
    reads = lio.SampleBam(path).fetch(ctx, [(0, 0, 90_000)])
    assert reads.stats["n_pairs"] == 3
    # paired reads of a whole file; regions out of order; nothing asked for
    _refused(ctx, path, cdefs.ERR_UNSUPPORTED, "index", regions=(), whole_file=True)
    _refused(ctx, path, cdefs.ERR_INVALID_INPUT, "sorted", regions=((0, 50, 60), (0, 10, 20)))
    _refused(ctx, path, cdefs.ERR_INVALID_INPUT, "nothing to fetch", regions=())
    # a file without records
    write([])
    _refused(ctx, path, cdefs.ERR_INVALID_DATA, "empty")
    assert lio.SampleBam(path).fetch(ctx, [(0, 0, 90_000)], paired=True).stats["n_pairs"] == 0


def test_the_index_lcty_write_bam_writes(ctx, tmp_path):
    """the per-genotype BAM of read placements and its .bai, both written by the library: what a fetch through that index gives equals
    the restatement on a linear walk of the file"""
    from locityper_amd import synth
    n_alleles, n_pairs, attempts = 4, 600, 4
    L = synth.SynthLocus(n_alleles, n_pairs, base_len=12_000)
    p = api.resolve_params(api.default_params(), L.bg)
    loc = api.Locus(ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    ch = L.reads(0, n_pairs)
    aa = api.AllAlignments.load(loc, ch)
    gt = np.array(L.true_genotype, dtype=np.uint16)
    read_off, counts = api.assignment_counts(aa, gt, api.default_solver(cdefs.SOLVER_ANNEAL), attempts, api.chain_seeds(9, attempts))
    path = str(tmp_path / "00.bam")
    lio.write_bam(path, aa, ch, [f"read{r}" for r in range(n_pairs)], [f"hap{a}" for a in range(n_alleles)], gt, attempts, read_off, counts)
    refs, recs = P.read_bam(path)
    bam = lio.SampleBam(path)
    assert bam.contigs == [n for n, _ in refs] and len(recs) > 500
    for regions in ([(0, 2_000, 3_000)], [(0, 0, 500), (0, 500, 700), (len(refs) - 1, 6_000, 9_000)], [(t, 0, ln) for t, (_, ln) in enumerate(refs)]):
        chunks, n_blocks = bam.plan(regions, True)
        assert len(chunks) >= 1 and n_blocks >= 1
        for paired in (False, True):
            _assert_equal(bam.fetch(ctx, regions, with_unmapped=True, paired=paired), S.expected(recs, regions, True, paired), paired)
