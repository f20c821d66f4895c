"""`locityper paf-vcf` without a device: the serial restatement (tests/pyref_pafvcf.py) pinned to answers worked out by hand, the host entry
point lcty_pafvcf_samples against it, and the BGZF writer."""
import re
import struct
import zlib

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import pafvcf_cases as PC
from tests import pyref_pafvcf as R


def cg(text):
    return [(op.encode(), int(n)) for n, op in re.findall(r"(\d+)([=XIDMHS])", text)]


EX_NAMES = [b"ref", b"S1.1", b"S1.2", b"S2.1", b"S2.2", b"S3"]
EX_SEQS = [b"ACGTTTTGCA", b"ACGTTTGCA", b"ACGTTTTGAA", b"ACCTTTTGCA", b"GGACGTTTTGCA", b"ACGTTTTCCA"]
EX_CIGARS = ["6=1D3=", "8=1X1=", "2=1X7=", "2I10=", "7=1X2="]
EX_ENTRIES = [(i + 1, 0, cg(c)) for i, c in enumerate(EX_CIGARS)]
EX_HEADER = (b"##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
             b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\tS3\n")
EX_MERGED = (b"ref\t1\t.\tA\tGGA\t60\t.\t.\tGT\t0|0\t0|1\t0\n"
             b"ref\t3\t.\tGT\tG,CT\t60\t.\t.\tGT\t1|0\t2|0\t0\n"
             b"ref\t8\t.\tG\tC\t60\t.\t.\tGT\t0|0\t0|0\t1\n"
             b"ref\t9\t.\tC\tA\t60\t.\t.\tGT\t0|1\t0|0\t0\n")
EX_SEPARATE = EX_MERGED.replace(b"ref\t3\t.\tGT", b"ref\t3\t.\tG\tC\t60\t.\t.\tGT\t.|0\t1|0\t0\nref\t3\t.\tGT")


def test_the_pinned_example_both_files_byte_for_byte():
    vars_ = R.process_paf(EX_SEQS, 0, EX_ENTRIES)
    assert vars_ == [[], [[2, 4, 2, 3]], [[8, 9, 8, 9]], [[2, 3, 2, 3]], [[0, 1, 0, 3]], [[7, 8, 7, 8]]]      # S1.1: (5,7,5,6) shifted to (2,4,2,3)
    unique, merged = R.combine_ranges(vars_)
    assert unique == [(0, 1), (2, 3), (2, 4), (7, 8), (8, 9)] and merged == [(0, 1), (2, 4), (7, 8), (8, 9)]
    m, s, stats = R.paf_to_vcf(EX_NAMES, EX_SEQS, EX_ENTRIES, b"ref")
    assert m == EX_HEADER + EX_MERGED and s == EX_HEADER + EX_SEPARATE
    assert stats["n_shifted"] == 1 and stats["n_missing"] == 0 and stats["n_bad_len"] == 0


def test_a_shift_stops_at_the_previous_variant():
    # GC A [A->C] A A A [A deleted] T: the deleted A could travel to position 2; the substitution ends at 4, so the gap stops at 4 + prefix
    ref, hap = b"GCAAAAAAT", b"GCACAAAT"
    assert R.process_haplotype(ref, hap, cg("3=1X3=1D1=")) == [[3, 4, 3, 4], [4, 6, 4, 5]]
    # without the substitution it goes all the way to the first A (padded by the C in front of it)
    assert R.process_haplotype(ref, b"GCAAAAAT", cg("7=1D1=")) == [[1, 3, 1, 2]]
    # a tandem repeat: one copy of CA inserted behind three copies moves left by whole rotations and part of one
    assert R.process_haplotype(b"TTCACACAGG", b"TTCACACACAGG", cg("8=2I2=")) == [[1, 2, 1, 4]]


def test_the_right_padded_first_variant_and_its_quirk():
    assert R.process_haplotype(b"ACGTTTTGCA", b"GGACGTTTTGCA", cg("2I10=")) == [[0, 1, 0, 3]]
    assert R.process_haplotype(b"ACGT", b"CGT", cg("1D3=")) == [[0, 2, 0, 1]]
    # the padding base lets an edit one base further on join the first variant (rpos <= ref_end)
    assert R.process_haplotype(b"ACGT", b"GGATGT", cg("2I1=1X2=")) == [[0, 2, 0, 4]]
    # as written upstream: a gap of the other kind directly behind a gap at position 0 — the variant does not describe the haplotype
    assert R.process_haplotype(b"GG", b"AAAAAG", cg("5I1D1=")) == [[0, 1, 0, 6]]
    with pytest.raises(R.RuntimeErr):
        R.process_haplotype(b"ACGT", b"ACGT", cg("2=1M1="))
    with pytest.raises(R.RuntimeErr):                     # the padded end reaches past the reference
        R.process_haplotype(b"", b"AAAAA", cg("5I"))


def test_touching_ranges_are_not_merged_and_overlapping_ones_are():
    v = lambda *r: [[a, b, a, b] for a, b in r]
    assert R.combine_ranges([v((2, 4)), v((4, 6))]) == ([(2, 4), (4, 6)], [(2, 4), (4, 6)])
    assert R.combine_ranges([v((2, 5)), v((4, 6)), None, v((2, 5), (9, 10))]) == ([(2, 5), (4, 6), (9, 10)], [(2, 6), (9, 10)])
    # a long range keeps absorbing: (1,9) (2,3) (8,10)
    assert R.combine_ranges([v((1, 9)), v((2, 3), (8, 10))])[1] == [(1, 10)]


def test_an_allele_with_n_is_a_dot_and_a_range_with_one_allele_is_skipped():
    names, seqs = [b"ref", b"A.1", b"A.2"], [b"ACGTACGT", b"ACNTACGT", b"ACGTACCT"]
    entries = [(1, 0, cg("2=1X5=")), (2, 0, cg("6=1X1="))]
    m, _, _ = R.paf_to_vcf(names, seqs, entries, b"ref")
    body = m.split(b"\n", 3)[3]
    assert body == b"ref\t7\t.\tG\tC\t60\t.\t.\tGT\t0|1\n"            # position 3 has the reference's allele alone: no line; A.1 is 0 at 7
    m, _, _ = R.paf_to_vcf(names[:2], seqs[:2], entries[:1], b"ref")
    assert m.split(b"\n", 3)[3] == b""
    # a missing haplotype and an empty slot are dots, a haploid sample has one column
    names, seqs = [b"ref", b"A.2", b"B", b"C_1"], [b"ACGT", b"AGGT", b"ACGT", b"ACGA"]
    m, _, stats = R.paf_to_vcf(names, seqs, [(1, 0, cg("1=1X2=")), (0, 2, cg("4="))], b"ref")
    assert m.split(b"\n", 3)[3] == b"ref\t2\t.\tC\tG\t60\t.\t.\tGT\t.|1\t0\t.|.\n" and stats["n_missing"] == 1


def test_region_and_shift():
    m, _, _ = R.paf_to_vcf(EX_NAMES, EX_SEQS, EX_ENTRIES, b"ref", region=(b"chr7", 1000, 1010))
    assert m == EX_HEADER + EX_MERGED.replace(b"ref\t1\t", b"chr7\t1001\t").replace(b"ref\t3\t", b"chr7\t1003\t").replace(b"ref\t8\t", b"chr7\t1008\t") \
        .replace(b"ref\t9\t", b"chr7\t1009\t")
    with pytest.raises(R.InvalidData):
        R.paf_to_vcf(EX_NAMES, EX_SEQS, EX_ENTRIES, b"ref", region=(b"chr7", 1000, 1011))


def test_process_paf_rules():
    seqs = [b"ACGT", b"AGT", b"ACGTT", b"ACGT"]
    stats = {}
    vars_ = R.process_paf(seqs, 0, [(1, 0, cg("4=")),                 # wrong lengths: skipped and counted
                                    (1, 2, cg("3=")),                 # the reference on neither side
                                    (0, 1, cg("1=1I2=")),             # the reference as the query: the insertion is a deletion of the haplotype
                                    (2, 0, cg("4=1X")),               # wrong lengths again
                                    (2, 0, cg("4=1I")), (2, 0, cg("3=1I1="))], stats)     # the later entry replaces the earlier one
    assert vars_ == [[], [[0, 2, 0, 1]], [[2, 3, 2, 4]], None] and stats["n_bad_len"] == 2 and stats["n_missing"] == 1


# ---- lcty_pafvcf_samples against the restatement --------------------------------------------------------------------------------------

def _samples_agree(names, ref_hap, discarded=None):
    want = R.group_haplotypes(names, ref_hap, discarded)
    got = api.pafvcf_samples(names, ref_hap, discarded)
    assert got == want
    return got


def test_samples_suffixes_and_partial_samples():
    groups, ref_id, warn = _samples_agree([b"ref", b"S1.1", b"S1.2", b"T_2", b"U", b"a-b.c.9", b"Z.3", b"Z.1", b"0x", b"S1.10"], b"ref")
    assert ref_id == 0 and warn == 0
    assert dict(groups)[b"T"] == [None, 3] and dict(groups)[b"U"] == [4] and dict(groups)[b"a-b.c"] == [None] * 8 + [5] and dict(groups)[b"Z"] == [7, None, 6]
    assert dict(groups)[b"S1.10"] == [9]                               # ".10" is no suffix: the digit must be 1-9 and the last character
    assert [g[0] for g in groups] == sorted(g[0] for g in groups)      # bytewise: "0x" < "S1" < "a-b.c"
    # a later writer of a slot replaces an earlier one
    assert dict(_samples_agree([b"r", b"A.1", b"A_1"], b"r")[0])[b"A"] == [2, None]
    for names in PC.make_case(3, 11, 1000, [1])[:1] + PC.make_case(4, 64, 1000, [1], round_trip=True)[:1]:
        _samples_agree(names, b"ref")


def test_samples_discarded_names_and_the_reference():
    names = [b"ref.1", b"A.1", b"B.1"]
    disc = b"A.1 = A.2, C.1\nX.1 = Y.1\nB.1 = X.1 B.2\nA.1 ~ ignored.1\nA.1 = A.2\n"
    groups, ref_id, warn = _samples_agree(names, b"ref.1", disc)
    # the last line of A.1 wins (IntMap::insert); X.1 is not in the FASTA, so Y.1 chains to B.1; '~' anywhere: "previously pruned"
    assert dict(groups) == {b"A": [1, 1], b"B": [2, 2], b"X": [2, None], b"Y": [2, None], b"ref": [0, None]}
    assert ref_id == 0 and warn == cdefs.PAFVCF_WARN_REF_SUFFIX | cdefs.PAFVCF_WARN_PRUNED
    # a reference found only among the discarded names: it is the contig it was identical to, and that contig stays a sample
    groups, ref_id, warn = _samples_agree([b"A.1", b"B.1"], b"GRCh38", b"B.1 = GRCh38\n")
    assert ref_id == 1 and warn == 0 and dict(groups) == {b"A": [0, None], b"B": [1, None]}
    # a name of the FASTA on the right-hand side is passed over; no final newline; commas are stripped
    assert _samples_agree([b"r", b"A.1", b"A.2"], b"r", b"A.1 = A.2, A.3,")[0] == [(b"A", [1, 2, 1])]


def test_samples_errors():
    def code(names, ref, disc=None):
        with pytest.raises(_lib.LocityperError) as e:
            api.pafvcf_samples(names, ref, disc)
        return e.value.code
    for bad in (b"-x", b"a b", b"a/b", b"x\n", b".1"):
        with pytest.raises(R.ParsingError):
            R.group_haplotypes([b"ref", bad], b"ref")
        assert code([b"ref", bad], b"ref") == cdefs.ERR_INVALID_DATA
    with pytest.raises(R.InvalidInput):
        R.group_haplotypes([b"a", b"b"], b"ref")
    assert code([b"a", b"b"], b"ref") == cdefs.ERR_INVALID_INPUT
    with pytest.raises(R.InvalidInput):
        R.group_haplotypes([b"a", b"b"], b"a", b"a =\n")
    assert code([b"a", b"b"], b"a", b"a =\n") == cdefs.ERR_INVALID_INPUT
    assert code([b"a", b"b"], b"a", b"a = c\n\nb = d\n") == cdefs.ERR_INVALID_INPUT       # an empty line has fewer than 3 columns
    with pytest.raises(R.ParsingError):                                                   # a discarded name is parsed like any other
        R.group_haplotypes([b"a"], b"a", b"a = b/c\n")
    assert code([b"a"], b"a", b"a = b/c\n") == cdefs.ERR_INVALID_DATA


# ---- lcty_io_write_bgzf ----------------------------------------------------------------------------------------------------------------

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.mark.parametrize("size", [0, 1, 0xff00 - 1, 0xff00, 0xff00 + 1, 200_000])
def test_write_bgzf_blocks_eof_and_content(tmp_path, size):
    rng = np.random.default_rng(size)
    data = PC.random_seq(rng, size)
    path = tmp_path / "x.vcf.gz"
    io.write_bgzf(path, data)
    raw = path.read_bytes()
    assert raw.endswith(EOF_BLOCK)
    at, out, sizes = 0, b"", []
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 10:at + 16] == b"\x06\x00BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        block = raw[at:at + bsize]
        payload = zlib.decompress(block[18:-8], -15)
        crc, isize = struct.unpack("<II", block[-8:])
        assert isize == len(payload) <= 0xff00 and crc == zlib.crc32(payload)
        out += payload
        sizes.append(len(payload))
        at += bsize
    assert at == len(raw) and out == data and sizes[-1] == 0 and all(sizes[:-1])
    assert len(sizes) == 1 + (size + 0xff00 - 1) // 0xff00
    if size:
        assert io.read_file(path) == data                                # and through the library's own reader
