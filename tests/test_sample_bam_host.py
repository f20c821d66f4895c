"""A sample's indexed BAM file, the host side (lcty_sample_bam_open / _contigs / _is_paired / _plan, lcty_recruit_fetch_regions): the
restatement of tests/pyref_sample_bam.py against answers derived by hand, the library's regions against it, and the chunks the library
plans from the index against a linear walk of the file. No device is needed."""
import struct

import numpy as np
import pytest

from locityper_amd import cdefs, io as lio
from locityper_amd._lib import LocityperError
from tests import pyref_sample_bam as P
from tests import sample_bam_cases as S


# ---- the restatement against hand-derived answers -----------------------------------------------------------------------------------

def test_restatement_on_the_hand_made_file():
    recs = S.hand_records()
    stream = P.fetched_stream(recs, S.HAND_REGIONS, with_unmapped=True)
    assert stream == S.HAND_STREAM
    pairs, discarded = P.pairs_of(recs, stream)
    assert pairs == S.HAND_PAIRS and discarded == S.HAND_DISCARDED
    assert P.fetched_stream(recs, S.HAND_REGIONS, with_unmapped=False) == [j for j in S.HAND_STREAM if j < 15]
    assert P.fetched_stream(recs, [], whole_file=True) == [j for j in range(19) if j not in (3, 18)]
    # strand restore and the writer: record 5 is reverse, record 8 has no qualities
    r = recs[5]
    assert P.restored(r) == r["seq"][::-1].translate(str.maketrans("ACGT", "TGCA"))
    text = P.record_text(r).split(b"\n")
    assert text[0] == b"@b" and text[1].decode() == P.restored(r) and text[3] == bytes(q + 33 for q in r["qual"][::-1])
    assert P.record_text(recs[8]) == f">d\n{recs[8]['seq']}\n".encode()
    assert P.restored(P.rec(0, 0, "n", 0x10, [], "ACGTNRY=")) == "NNNNACGT"


def test_restatement_refuses_what_the_reference_refuses():
    R = P.rec
    M = [("M", 4)]
    with pytest.raises(P.Refused, match="unpaired") as e:
        P.pairs_of([R(0, 5, "solo", 0x1, M, "ACGT")], [0])
    assert e.value.status == P.ERR_INVALID_DATA and e.value.name == "solo"
    two = [R(0, 5, "t", 0x41, M, "ACGT", None, 0, 9), R(0, 9, "t", 0x41, M, "ACGT", None, 0, 5)]
    with pytest.raises(P.Refused, match="same read end"):
        P.pairs_of(two, [0, 1])
    with pytest.raises(P.Refused, match="no sequence"):
        P.fetched_stream([R(0, 5, "empty", 0, M, "")], [(0, 0, 10)])
    with pytest.raises(P.Refused, match="sorted"):
        P.fetched_stream([], [(0, 10, 20), (0, 15, 30)])


# ---- postprocess_targets ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("intervals, lens, padding, alt, dist, exp", [
    ([(0, 500, 900)], [10_000], 1000, 0, 1000, [(0, 0, 1900)]),                                   # padding clamped at 0
    ([(0, 9_500, 9_900)], [10_000], 1000, 0, 1000, [(0, 8_500, 10_000)]),                         # ... and at the contig's end
    ([(0, 5_000, 6_000)], [100_000, 3_000, 4_000], 0, 4_000, 1000, [(0, 5_000, 6_000), (1, 0, 3_000)]),   # shorter than alt_contig_len: whole; equal: not
    ([(0, 1_000, 2_000), (0, 3_000, 4_000)], [100_000], 0, 0, 1000, [(0, 1_000, 4_000)]),         # exactly merge_distance apart: one
    ([(0, 1_000, 2_000), (0, 3_001, 4_000)], [100_000], 0, 0, 1000, [(0, 1_000, 2_000), (0, 3_001, 4_000)]),   # one base further: two
    ([(1, 100, 200)], [100_000, 3_000], 50, 10_000, 1000, [(1, 0, 3_000)]),                       # an interval inside a short contig
    ([(1, 10, 20), (0, 700, 800), (0, 100, 900)], [5_000, 5_000], 10, 0, 0, [(0, 90, 910), (1, 0, 30)]),      # unsorted input, one inside another
])
def test_fetch_regions(intervals, lens, padding, alt, dist, exp):
    assert P.postprocess_targets(intervals, lens, padding, alt, dist) == exp
    t, s, e = lio.fetch_regions([i[0] for i in intervals], [i[1] for i in intervals], [i[2] for i in intervals], lens, padding, alt, dist)
    assert list(zip(t.tolist(), s.tolist(), e.tolist())) == exp


def test_fetch_regions_seeded_and_misuse():
    rng = np.random.default_rng(2)
    lens = [int(x) for x in rng.integers(2_000, 300_000, 12)]
    iv = []
    for _ in range(300):
        t = int(rng.integers(0, 12)); s = int(rng.integers(0, lens[t] - 1)); e = int(rng.integers(s + 1, min(lens[t], s + 5_000) + 1))
        iv.append((t, s, e))
    for padding, alt, dist in [(0, 0, 0), (1100, 10_000, 1000), (137, 50_000, 1), (10_000, 300_000, 1000)]:
        t, s, e = lio.fetch_regions([i[0] for i in iv], [i[1] for i in iv], [i[2] for i in iv], lens, padding, alt, dist)
        assert list(zip(t.tolist(), s.tolist(), e.tolist())) == P.postprocess_targets(iv, lens, padding, alt, dist)
    for bad in [([3], [0], [10]), ([0], [10], [10])]:
        with pytest.raises(LocityperError) as err:
            lio.fetch_regions(*bad, [100, 100], 0, 0, 0)
        assert err.value.code == cdefs.ERR_INVALID_INPUT


# ---- the header, the index, the plan ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    d = tmp_path_factory.mktemp("sample_bam")
    recs = S.seeded_records()
    path = str(d / "seeded.bam")
    voffs = P.write_bam(path, S.SEEDED_REFS, recs, block_size=1500)
    return path, recs, voffs


def _records_of_chunks(path, chunks):
    """the records a reader of exactly these chunks sees: zlib on the blocks they touch, the chain of lengths inside them"""
    data, blocks = P.read_bgzf(path)
    ustart = {c: u for u, c, _ in blocks}
    out = []
    for beg, end in chunks.tolist():
        a = ustart[beg >> 16] + (beg & 0xFFFF)
        b = ustart[end >> 16] + (end & 0xFFFF) if (end >> 16) in ustart else len(data)
        out += P.parse_records(data, a, b)
    return out


def test_open_contigs_and_pairedness(seeded, tmp_path):
    path, recs, _ = seeded
    bam = lio.SampleBam(path)
    assert bam.contigs == [n for n, _ in S.SEEDED_REFS] and bam.lengths.tolist() == [ln for _, ln in S.SEEDED_REFS]
    assert bam.is_paired() == bool(recs[0]["flag"] & 1)
    single = str(tmp_path / "single.bam")
    P.write_bam(single, S.HAND_REFS, [P.rec(0, 10, "r", 0, [("M", 4)], "ACGT")])
    assert lio.SampleBam(single).is_paired() is False
    # the index under the file's name with .bam replaced, and one given by name
    other = str(tmp_path / "x.bam")
    P.write_bam(other, S.HAND_REFS, S.hand_records(), index=str(tmp_path / "x.bai"))
    assert lio.SampleBam(other).contigs == ["chrA", "chrB"]
    P.write_bam(other, S.HAND_REFS, S.hand_records(), index=str(tmp_path / "elsewhere.idx"))
    assert lio.SampleBam(other, str(tmp_path / "elsewhere.idx")).is_paired()
    empty = str(tmp_path / "empty.bam")
    P.write_bam(empty, S.HAND_REFS, [])
    with pytest.raises(LocityperError, match="empty") as err:
        lio.SampleBam(empty).is_paired()
    assert err.value.code == cdefs.ERR_INVALID_DATA


@pytest.mark.parametrize("block_size", [512, 1500, 4096, 0xff00])
def test_planned_chunks_hold_what_a_linear_walk_finds(tmp_path, block_size):
    recs = S.seeded_records(seed=block_size, n_pairs=400, n_tail=10)
    path = str(tmp_path / "b.bam")
    voffs = P.write_bam(path, S.SEEDED_REFS, recs, block_size=block_size)
    bam = lio.SampleBam(path)
    file_records = P.read_bam(path)[1]
    assert len(file_records) == len(recs)
    region_sets = [[r] for r in S.SEEDED_REGIONS] + [S.SEEDED_REGIONS, S.SEEDED_REGIONS[1:4], [(0, 0, 200_000)], [(1, 100_000, 150_000)], [(0, 16_383, 16_385)]]
    for regions in region_sets:
        for with_unmapped in (False, True):
            chunks, n_blocks = bam.plan(regions, with_unmapped)
            assert np.all(chunks[:, 0] < chunks[:, 1]) and np.all(chunks[1:, 0] >> 16 > chunks[:-1, 1] >> 16)      # sorted, merged
            seen = _records_of_chunks(path, chunks)
            want = [file_records[j]["at"] for j in P.fetched_stream(file_records, regions, with_unmapped)]
            got = [seen[j]["at"] for j in P.fetched_stream(seen, regions, with_unmapped)]
            assert got == want, (regions, with_unmapped)
            assert n_blocks >= len(chunks) or len(chunks) == 0
    # the tail starts where the placed records end
    chunks, _ = bam.plan([], True)
    n_placed = sum(r["tid"] >= 0 for r in recs)
    assert len(chunks) == 1 and int(chunks[0, 0]) == voffs[n_placed]


def test_one_region_reads_fewer_blocks_than_the_file_has(seeded):
    path, recs, _ = seeded
    _, blocks = P.read_bgzf(path)
    assert len(blocks) >= 200
    chunks, n_blocks = lio.SampleBam(path).plan([S.SEEDED_REGIONS[2]])
    assert 0 < n_blocks < len(blocks) // 4


def test_errors(tmp_path, seeded):
    path, recs, _ = seeded
    lone = str(tmp_path / "lone.bam")
    P.write_bam(lone, S.HAND_REFS, S.hand_records(), index=False)
    with pytest.raises(LocityperError, match="no index") as err:
        lio.SampleBam(lone)
    assert err.value.code == cdefs.ERR_INVALID_INPUT
    with pytest.raises(LocityperError) as err:
        lio.SampleBam(lone, str(tmp_path / "missing.bai"))
    assert err.value.code == cdefs.ERR_INVALID_INPUT
    csi = str(tmp_path / "lone.bam.csi")
    open(csi, "wb").write(b"CSI\1" + struct.pack("<iii", 14, 5, 0))
    with pytest.raises(LocityperError, match="CSI") as err:
        lio.SampleBam(lone)
    assert err.value.code == cdefs.ERR_UNSUPPORTED
    with pytest.raises(LocityperError, match="CSI") as err:
        lio.SampleBam(lone, csi)
    assert err.value.code == cdefs.ERR_UNSUPPORTED
    cram = str(tmp_path / "s.cram")
    open(cram, "wb").write(b"CRAM\3\0" + bytes(40))
    with pytest.raises(LocityperError, match="CRAM") as err:
        lio.SampleBam(cram)
    assert err.value.code == cdefs.ERR_UNSUPPORTED
    bam = lio.SampleBam(path)
    for regions in ([(0, 500, 900), (0, 100, 200)], [(0, 100, 300), (0, 200, 400)], [(1, 5, 9), (0, 5, 9)], [(0, 9, 9)], [(7, 0, 10)]):
        with pytest.raises(LocityperError) as err:
            bam.plan(regions)
        assert err.value.code == cdefs.ERR_INVALID_INPUT, regions
