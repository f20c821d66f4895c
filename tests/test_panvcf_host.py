"""A locus from a pangenome VCF, without a device: the restatement (tests/pyref_panvcf.py) pinned to hand-derived answers, and the
host entry points — the VCF reader, the haplotype names — against it."""
import gzip

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import panvcf_cases as PC
from tests import pyref_panvcf as R

REF = b"ACGTACGTAC"          # [100, 110)
S, E = 100, 110


def _rec(records, gt, names=None, frac=1.0, overlaps=False):
    names = names or [f"h{i}" for i in range(len(gt[0]) if gt else 1)]
    return R.reconstruct("chr1", S, E, REF, records, gt, names, frac, overlaps)


# ---------------------------------------------------------------- boundary search, known answers
def test_boundary_without_records_keeps_the_locus_side():
    # all k-mers unique, no records: every window scores 1, the penalty makes the innermost position the maximum
    n, k, mw = 51, 5, 10
    counts = [1] * (n + mw - k)
    at, w = R.find_best_boundary(100, 151, [], k, counts, 50, mw, True)
    assert at == 150 and w[50] == 1.0 and w[0] == 1.0 - (1.0 * (0.2 / 50.0)) * 50.0
    at, w = R.find_best_boundary(100, 151, [], k, counts, 50, mw, False)
    assert at == 100 and w[0] == 1.0 and w[50] == 1.0 - (1.0 * (0.2 / 50.0)) * 50.0


def test_boundary_moves_ten_bases_clear_of_a_record_over_it():
    n, k, mw, d = 51, 5, 10, 0.2 / 50.0
    counts = [0] * (n + mw - k)
    # left side, locus side at 150, a record over [148, 153): 148.. are 0, 147 scores 0.9, 139 scores 0.1, 138 is clear
    at, w = R.find_best_boundary(100, 151, [(148, 5)], k, counts, 50, mw, True)
    assert at == 138
    assert w[48] == 0.0 and w[50] == 0.0
    assert w[47] == 0.9 - (0.9 * d) * 3.0 and w[39] == 0.1 - (0.1 * d) * 11.0 and w[38] == 1.0 - (1.0 * d) * 12.0
    # right side, locus side at 100, a record over [98, 103): 103 scores 0.1, 111 scores 0.9, 112 is clear
    at, w = R.find_best_boundary(100, 151, [(98, 5)], k, counts, 50, mw, False)
    assert at == 112
    assert w[0] == 0.0 and w[2] == 0.0 and w[3] == 0.1 - (0.1 * d) * 3.0 and w[11] == 0.9 - (0.9 * d) * 11.0 and w[12] == 1.0 - (1.0 * d) * 12.0


def test_boundary_margins_of_two_records_multiply_in_record_order():
    n, k, mw, d = 40, 5, 10, 0.2 / 1000.0
    counts = [1, 0, 7, 1, 1, 3] * 8
    counts = counts[:n + mw - k]
    recs = [(120, 1), (130, 1)]
    _, w = R.find_best_boundary(100, 140, recs, k, counts, 1000, mw, False)
    # position 122: two bases right of the first record (i = 1 -> 2 / 10), eight left of the second (i = 7 -> 2 / 10)
    uniq = sum(1 for c in counts[22:28] if c <= 1)
    x = float(uniq) / 6.0
    x *= 2.0 / 10.0
    x *= float(9 - 7) / 10.0
    x -= (x * d) * 22.0
    assert w[22] == x and x != 0.0
    # position 126: i = 5 -> 6 / 10, then i = 3 -> 6 / 10
    y = float(sum(1 for c in counts[26:32] if c <= 1)) / 6.0
    y *= 6.0 / 10.0
    y *= 6.0 / 10.0
    y -= (y * d) * 26.0
    assert w[26] == y
    assert w[20] == 0.0 and w[30] == 0.0


def test_boundary_all_zero_weights_is_none_and_the_degenerate_interval():
    assert R.find_best_boundary(100, 151, [], 5, [2] * 56, 50, 10, True)[0] is None
    assert R.find_best_boundary(100, 151, [], 5, [9] * 56, 50, 10, False)[0] is None
    # start == end (add.rs:381-387): a record over the point -> none, else the point itself
    assert R.find_best_boundary(100, 100, [(90, 5)], 5, [], 50, 10, True) == (100, None)
    assert R.find_best_boundary(100, 100, [(90, 10)], 5, [], 50, 10, True) == (None, None)
    assert R.find_best_boundary(100, 100, [(100, 0)], 5, [], 50, 10, False) == (None, None)
    assert R.find_best_boundary(100, 100, [(101, 3)], 5, [], 50, 10, False) == (100, None)


TIE_LEFT = dict(counts=[1] * 8 + [5] + [1] * 4, n=6)       # weights 1, 7/8 x 5; allowed expansion 8: 1 - (0.2 / 8) 5 == 7 / 8
TIE_RIGHT = dict(counts=[1] * 4 + [5] + [1] * 8, n=6)


def test_boundary_tie_rule():
    at, w = R.find_best_boundary(10, 16, [], 3, TIE_LEFT["counts"], 8, 10, True)
    assert w[0] == w[5] == 0.875 and max(w) == 0.875 and at == 15              # the last maximum on the left
    at, w = R.find_best_boundary(10, 16, [], 3, TIE_RIGHT["counts"], 8, 10, False)
    assert w[0] == w[5] == 0.875 and max(w) == 0.875 and at == 10              # the first on the right


# ---------------------------------------------------------------- reconstruction, known answers
def test_reconstruct_single_variants():
    cases = [
        ((102, [b"G", b"T"]), b"ACTTACGTAC"),                  # SNP
        ((104, [b"AC", b"GG"]), b"ACGTGGGTAC"),                # MNP
        ((103, [b"T", b"TAAA"]), b"ACGTAAAACGTAC"),            # insertion
        ((105, [b"CGT", b"C"]), b"ACGTACAC"),                  # deletion
        ((107, [b"TAC", b"T"]), b"ACGTACGT"),                  # deletion that ends exactly at ref_end
        ((100, [b"A", b"G"]), b"GCGTACGTAC"),                  # record at ref_start
    ]
    for rec, want in cases:
        out = _rec([rec], [[0, 1]])
        assert out["seqs"] == [REF, want] and out["reason"] == [0, 0] and out["n_kept_records"] == 1
    # a record nobody carries is not kept; one before the interval is skipped; one behind ends the walk; a straddling one is refused
    assert _rec([(102, [b"G", b"T"])], [[0, 0]])["n_kept_records"] == 0
    assert _rec([(98, [b"AA", b"T"]), (102, [b"G", b"T"]), (110, [b"A", b"T"]), (109, [b"CA", b"C"])], [[1], [1], [1], [1]])["seqs"] == [b"ACTTACGTAC"]
    for rec in ((99, [b"GA", b"G"]), (109, [b"CA", b"C"])):
        with pytest.raises(R.PanvcfError) as e:
            _rec([rec], [[1]])
        assert e.value.kind == "Boundary" and e.value.record == 0


def test_reconstruct_overlaps_missing_and_n():
    recs = [(102, [b"GTA", b"G"]), (103, [b"T", b"C"])]
    out = _rec(recs, [[1, 1, 0], [1, 0, 1]], overlaps=True)
    assert out["seqs"] == [b"ACGCGTAC", b"ACGCGTAC", b"ACGCACGTAC"] and out["total_overlaps"] == 1
    with pytest.raises(R.PanvcfError) as e:
        _rec(recs, [[1, 1, 0], [0, 1, 1]], names=["a", "b", "c"])
    assert (e.value.kind, e.value.record, e.value.column) == ("Overlap", 1, 1) and "chr1:104 for b" in str(e.value)
    # a missing allele: the reference, ref_len unknown bases; dropped when f64(unknown) > unknown_frac * f64(len)
    recs = [(102, [b"G", b"T"]), (105, [b"CG", b"C"])]
    out = _rec(recs, [[-1, 1, -1], [0, 1, -1]], frac=0.1)
    assert out["seqs"][0] == REF and out["unknown"] == [1, 0, 3]
    assert out["reason"] == [0, 0, 1] and out["kept"] == [0, 1]            # 1.0 > 0.1 * 10.0 is false: equality keeps
    # N in an ALT allele: the sequence is removed afterwards; a column with too many unknown bases is counted there first
    out = _rec([(102, [b"G", b"N"])], [[1, 0, -1]], frac=0.0)
    assert out["seqs"][0] == b"ACNTACGTAC" and out["reason"] == [2, 0, 1]


# ---------------------------------------------------------------- the reader
SAMPLES, PLOIDY = ["HG1", "HG2", "chm"], [2, 2, 1]


def _vcf_case(n=40, seed=5):
    s, e, ref, records, gt = PC.make_case(seed, 600, n, 5, 0.3, missing_rate=0.05, ref_start=1000)
    return ref, records, gt


def _check_region(got, records, gt, idx):
    want = PC.flat([records[i] for i in idx])
    for key in ("pos", "ref_len", "rec_allele", "allele_off", "allele_bytes"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["gt"], gt[idx]) and got["phased"].shape == (len(idx), 3) and got["phased"].all()


def test_reader_plain_gzip_bgzf_and_the_fetch_rule(tmp_path):
    ref, records, gt = _vcf_case()
    text = PC.vcf_text("chr7", records, SAMPLES, PLOIDY, gt)
    (tmp_path / "a.vcf").write_bytes(text)
    (tmp_path / "b.vcf.gz").write_bytes(gzip.compress(text))
    (tmp_path / "c.vcf.gz").write_bytes(PC.bgzf(text, block=700))
    (tmp_path / "d.vcf").write_bytes(PC.vcf_text("chr7", records, SAMPLES, PLOIDY, gt, extra_format=True))                  # GT:DP
    (tmp_path / "e.vcf").write_bytes(PC.vcf_text("chr7", records, SAMPLES, PLOIDY, gt, extra_format=True, gt_first=False))  # DP:GT
    for name in ("a.vcf", "b.vcf.gz", "c.vcf.gz", "d.vcf", "e.vcf"):
        v = io.Vcf(tmp_path / name)
        assert v.samples == SAMPLES and v.ploidy.tolist() == PLOIDY and v.hap_off.tolist() == [0, 2, 4, 5] and v.n_records == len(records)
        _check_region(v.region("chr7", 0, 1 << 30), records, gt, list(range(len(records))))
        # both edges: a record is in when pos < end and pos + len(REF) > start
        long_ = max(range(len(records)), key=lambda i: len(records[i][1][0]))
        p, rl = records[long_][0], len(records[long_][1][0])
        assert rl > 1
        for start, end in ((p + rl - 1, p + rl), (p + rl, p + rl + 50), (p, p + 1), (p - 3, p), (1100, 1300)):
            idx = R.fetch(records, start, end)
            _check_region(v.region("chr7", start, end), records, gt, idx)
            assert (long_ in idx) == (p < end and p + rl > start)
        assert v.region("chrX", 0, 1 << 30)["pos"].size == 0
        v.close()
    info, recs = io.vcf_region(tmp_path / "a.vcf", "chr7", 1100, 1300)
    assert info["samples"] == SAMPLES and len(recs["pos"]) == len(R.fetch(records, 1100, 1300))
    with pytest.raises(_lib.LocityperError) as e:
        io.Vcf(tmp_path / "x.bcf")
    assert e.value.code == cdefs.ERR_UNSUPPORTED


def test_reader_refuses_ploidy_changes_and_unphased_calls(tmp_path):
    ref, records, gt = _vcf_case(6)
    lines = PC.vcf_text("chr7", records, SAMPLES, PLOIDY, gt).decode().split("\n")
    hdr = [l for l in lines if l.startswith("#")]
    body = [l for l in lines if l and not l.startswith("#")]

    def region(rows, used=None):
        (tmp_path / "t.vcf").write_text("\n".join(hdr + rows) + "\n")
        v = io.Vcf(tmp_path / "t.vcf")
        try:
            return v, v.region("chr7", 0, 1 << 30, used)
        finally:
            v.close()

    f = body[2].split("\t")
    for bad, msg in (("0", "has ploidy 1 (expected 2)"), ("0|1|1", "has ploidy 3 (expected 2)"), ("0/1", "is unphased in sample HG2"), (".", "has ploidy 1 (expected 2)")):
        rows = body[:2] + ["\t".join(f[:10] + [bad] + f[11:])] + body[3:]
        with pytest.raises(_lib.LocityperError) as e:
            region(rows)
        assert e.value.code == cdefs.ERR_INVALID_DATA and msg in str(e.value) and f"chr7:{f[1]}" in str(e.value)
        region(rows, used=[1, 0, 1])                                     # a sample that was left out is not looked at
    # haploid calls: an allele, a missing one; the first record defines the ploidy
    rows = body[:2] + ["\t".join(f[:11] + ["."])] + body[3:]
    assert region(rows)[1]["gt"][2, 4] == -1
    rows = ["\t".join(body[0].split("\t")[:11] + ["0|1"])] + body[1:]
    with pytest.raises(_lib.LocityperError) as e:
        region(rows)
    assert "in sample chm has ploidy 1 (expected 2)" in str(e.value)
    # a header without samples; a file without records
    (tmp_path / "n.vcf").write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nchr7\t5\t.\tAC\tA,ACC\t.\t.\t.\n")
    v = io.Vcf(tmp_path / "n.vcf")
    r = v.region("chr7", 0, 100)
    assert v.samples == [] and v.n_haps == 0 and r["pos"].tolist() == [4] and r["ref_len"].tolist() == [2] and r["allele_bytes"].tobytes() == b"ACAACC"
    assert r["rec_allele"].tolist() == [0, 3] and r["gt"].shape == (1, 0)
    (tmp_path / "e.vcf").write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\n")
    with pytest.raises(_lib.LocityperError) as e:
        io.Vcf(tmp_path / "e.vcf")
    assert e.value.code == cdefs.ERR_INVALID_DATA and "does not contain any records" in str(e.value)


# ---------------------------------------------------------------- names
def _names(samples, ploidy, ref, leave=()):
    names, cs, ch, left = api.panvcf_names(samples, ploidy, ref, leave)
    cols = [(None if int(s) == cdefs.NONE_U32 else int(s), int(h)) for s, h in zip(cs, ch)]
    want = R.haplotype_names(samples, ploidy, ref, leave)
    assert (names, cols, left) == want
    return names, cols, left


def test_names_follow_ploidy_and_leave_out():
    assert _names(SAMPLES, PLOIDY, "GRCh38")[0] == ["GRCh38", "HG1.1", "HG1.2", "HG2.1", "HG2.2", "chm"]
    assert _names(SAMPLES, PLOIDY, "GRCh38", ["HG1"]) == (["GRCh38", "HG2.1", "HG2.2", "chm"], [(None, 0), (1, 0), (1, 1), (2, 0)], 2)
    assert _names(SAMPLES, PLOIDY, "GRCh38", ["HG2.1", "GRCh38", "nobody"]) == (["HG1.1", "HG1.2", "HG2.2", "chm"], [(0, 0), (0, 1), (1, 1), (2, 0)], 2)
    assert _names(SAMPLES, PLOIDY, "GRCh38", ["HG1.1", "HG1.2"])[0] == ["GRCh38", "HG2.1", "HG2.2", "chm"]      # the sample stays, without haplotypes
    assert _names(["a", "b"], [0, 1], "ref", ["a"])[0] == ["ref", "b"]                                            # left out before its ploidy is looked at
    for samples, ploidy, ref, leave, msg in ((["a", "a"], [1, 1], "r", [], "Duplicate haplotype name (a)"), (["a.1", "a"], [1, 2], "r", [], "Duplicate haplotype name (a.1)"),
                                             (["a"], [1], "a", [], "Duplicate haplotype name (a)"), (["a"], [0], "r", [], "zero ploidy"),
                                             (["a"], [256], "r", [], "extremely high ploidy"), (["a", "b"], [2, 1], "r", ["a", "b"], "Loaded zero haplotypes"),
                                             ([], [], "r", [], "Loaded zero haplotypes")):
        with pytest.raises(_lib.LocityperError) as e:
            api.panvcf_names(samples, ploidy, ref, leave)
        assert e.value.code == cdefs.ERR_INVALID_DATA and msg in str(e.value)
        with pytest.raises(R.PanvcfError) as e2:
            R.haplotype_names(samples, ploidy, ref, leave)
        assert msg in str(e2.value)


def test_a_haploid_sample_beside_diploid_ones(tmp_path):
    """reader -> names -> columns -> the restatement: the matrix the device entry takes, for a VCF with ploidies 2, 2, 1"""
    recs = [(102, [b"G", b"T"]), (105, [b"CGT", b"C", b"CGTT"])]
    gt = np.array([[0, 1, 1, 0, 1], [2, 0, 0, 1, -1]], dtype=np.int16)
    (tmp_path / "h.vcf").write_bytes(PC.vcf_text("chr1", recs, SAMPLES, PLOIDY, gt))
    info, r = io.vcf_region(tmp_path / "h.vcf", "chr1", S, E)
    names, cs, ch, _ = api.panvcf_names(info["samples"], info["ploidy"], "ref", ["HG2.1"])
    m = api.panvcf_columns(r["gt"], info["hap_off"], cs, ch)
    assert names == ["ref", "HG1.1", "HG1.2", "HG2.2", "chm"] and m.tolist() == [[0, 0, 1, 0, 1], [0, 2, 0, 1, -1]]
    out = R.reconstruct("chr1", S, E, REF, recs, m.tolist(), names, 1.0, False)
    assert out["seqs"] == [REF, b"ACGTACGTTAC", b"ACTTACGTAC", b"ACGTACAC", b"ACTTACGTAC"] and out["unknown"] == [0, 0, 0, 0, 3]


def test_device_entry_points_fail_loudly_without_a_device():
    L = _lib.lib()
    import ctypes as C
    o, f, at = cdefs.PanvcfOut(), C.c_int32(), C.c_uint32()
    assert L.lcty_panvcf_reconstruct(None, b"c", 0, 10, None, 0, None, None, None, None, None, 1, None, b"a\0", 0.0, 0, C.byref(o)) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_db_find_boundary(None, 0, 10, 0, None, None, 5, None, 0, 10, 10, 1, C.byref(f), C.byref(at), None) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_panvcf_filter(None, 0, 1, None, None, None) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_db_locus_from_vcf(None, None, None, None) == cdefs.ERR_INVALID_INPUT
    if api.device_count() == 0:
        with pytest.raises(_lib.LocityperError) as e:
            api.Context(0)
        assert e.value.code == cdefs.ERR_RUNTIME and "no CPU fallback" in str(e.value)
