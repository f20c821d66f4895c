"""A locus from a pangenome VCF on the device (lcty_panvcf.hip) against the serial restatement (tests/pyref_panvcf.py): every comparison
is byte / array / f64-bit equality."""
import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import panvcf_cases as PC
from tests import pyref_db as RD
from tests import pyref_panvcf as R

pytestmark = pytest.mark.gpu

GATHER_TILE = 2048      # output bytes of one gather workgroup (lcty_panvcf.hip)


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _check(ctx, s, e, ref, records, gt, frac=1.0, overlaps=True, names=None):
    gt = np.asarray(gt, dtype=np.int16)
    names = names or [f"hap{c}" for c in range(gt.shape[1])]
    want = R.reconstruct("chr1", s, e, ref, records, gt.tolist(), names, frac, overlaps)
    got = api.panvcf_reconstruct(ctx, "chr1", s, e, _u8(ref), PC.flat(records), gt, names, frac, overlaps)
    assert got["col_unknown"].tolist() == want["unknown"]
    assert got["col_len"].tolist() == [len(x) for x in want["seqs"]]
    assert got["col_reason"].tolist() == want["reason"]
    assert got["kept_cols"].tolist() == want["kept"] and got["names"] == [names[c] for c in want["kept"]]
    assert got["total_overlaps"] == want["total_overlaps"] and got["n_kept_records"] == want["n_kept_records"]
    off = got["seq_off"]
    assert len(off) == len(want["kept"]) + 1 and off[0] == 0
    for i, c in enumerate(want["kept"]):
        assert got["seqs"][int(off[i]):int(off[i + 1])].tobytes() == want["seqs"][c], (i, c)
    return want, got


# columns x records x reference length x non-reference rate: every class of both, 0.6 makes overlaps dense in every batch
SHAPES = [(1, 0, 1000, 0.0), (2, 1, 1000, 0.6), (63, 63, 2000, 0.02), (64, 64, 3000, 0.6), (65, 65, 5000, 0.02), (130, 3000, 20000, 0.02),
          (130, 3000, 20000, 0.6), (1, 3000, 20000, 0.6), (64, 3000, 10000, 0.0), (2, 65, 1000, 0.6), (65, 64, 1500, 0.6), (63, 1, 1000, 0.6),
          (130, 63, 4000, 0.02), (1, 64, 1000, 0.02), (2, 3000, 12000, 0.02)]


@pytest.mark.parametrize("cols,recs,ref_len,rate", SHAPES)
def test_reconstruction_equals_the_serial_walk(gpu_ctx, cols, recs, ref_len, rate):
    s, e, ref, records, gt = PC.make_case(cols * 7919 + recs, ref_len, recs, cols, rate, missing_rate=0.002)
    want, _ = _check(gpu_ctx, s, e, ref, records, gt, frac=0.0005)
    if rate == 0.6 and recs >= 63:
        assert want["total_overlaps"] > 0
    # everything kept: no compaction
    _check(gpu_ctx, s, e, ref, records, gt, frac=1.0)


def test_an_insertion_longer_than_a_gather_tile(gpu_ctx):
    rng = np.random.default_rng(3)
    ref = PC.random_seq(rng, 1001)
    recs = [(1300, [ref[300:301], ref[300:301] + PC.random_seq(rng, 5000)]), (1500, [ref[500:503], ref[500:501]])]
    want, got = _check(gpu_ctx, 1000, 2001, ref, recs, [[0, 1, 1, 0], [0, 0, 1, 1]])
    assert got["col_len"].tolist() == [1001, 6001, 5999, 999] and want["seqs"][0] == ref      # a column that is all reference equals the reference


def test_segment_ends_on_tile_edges(gpu_ctx):
    rng = np.random.default_rng(4)
    ref = PC.random_seq(rng, 6001)                                         # the second column begins inside an 8-byte word
    for at in (GATHER_TILE - 1, GATHER_TILE, GATHER_TILE + 1):             # the allele begins at a tile edge and one byte either side
        for end in (2 * GATHER_TILE - 1, 2 * GATHER_TILE, 2 * GATHER_TILE + 1):      # ... and ends at one
            recs = [(1000 + at, [ref[at:at + 1], PC.random_seq(rng, end - at)]), (1000 + at + 40, [ref[at + 40:at + 41], b"T"])]
            _check(gpu_ctx, 1000, 7001, ref, recs, [[1, 0, 1], [0, 1, 1]])
    # in a later column the edges are relative to the word the column begins in: sweep the allele's length over a whole word
    for extra in range(9):
        recs = [(1000 + 7, [ref[7:8], PC.random_seq(rng, GATHER_TILE - 7 - 4 + extra)])]
        _check(gpu_ctx, 1000, 7001, ref, recs, [[0, 1, 1]])


def test_missing_columns_unknown_threshold_and_n(gpu_ctx):
    rng = np.random.default_rng(5)
    ref = PC.random_seq(rng, 1000)
    s, e = 5000, 6000
    recs = [(5000 + 10 * i, [ref[10 * i:10 * i + 1], b"T" if ref[10 * i:10 * i + 1] != b"T" else b"G"]) for i in range(90)]
    gt = np.zeros((90, 5), dtype=np.int16)
    gt[:, 0] = 1
    gt[:, 1] = -1                                                           # every record missing: the reference, 90 unknown bases
    gt[7, 2] = -1                                                           # one unknown base of 1 000: equality at 0.001 keeps the column
    gt[7, 3] = gt[8, 3] = -1                                                # two: dropped
    want, got = _check(gpu_ctx, s, e, ref, recs, gt, frac=0.001)
    assert want["unknown"] == [0, 90, 1, 2, 0] and want["reason"] == [0, 1, 0, 1, 0] and want["seqs"][1] == ref == want["seqs"][4]
    # N only in the last byte of a sequence; a column over the unknown threshold is counted there, not under N
    recs = [(5999, [ref[999:], b"N"])]
    want, got = _check(gpu_ctx, s, e, ref, recs, [[1, 0, -1, 1]], frac=0.0)
    assert want["reason"] == [2, 0, 1, 2] and want["seqs"][0][-1:] == b"N" and got["names"] == ["hap1"]


def test_prev_end_crosses_a_wavefront_batch(gpu_ctx):
    rng = np.random.default_rng(6)
    ref = PC.random_seq(rng, 3000)
    s = 100
    recs = [(s + 10 * i, [ref[10 * i:10 * i + 1], b"A" if ref[10 * i:10 * i + 1] != b"A" else b"C"]) for i in range(260)]
    for first in (0, 100):                                                  # a deletion that reaches over the next 64 records, not the 65th
        recs[first] = (s + 10 * first, [ref[10 * first:10 * first + 645], ref[10 * first:10 * first + 1]])
    gt = np.zeros((260, 4), dtype=np.int16)
    gt[[0, 64, 65, 100, 164, 165], 0] = 1                                   # 64 and 164 fall into the deletions 64 entries earlier; 65 and 165 do not
    gt[[64, 65, 164, 165], 1] = 1                                           # without the deletions all four are taken
    gt[[0, 63, 64, 65, 66, 100, 128, 129, 165], 2] = 1
    gt[:, 3] = 1                                                            # everything: 64 ignored after each deletion
    want, _ = _check(gpu_ctx, s, s + 3000, ref, recs, gt)
    assert want["total_overlaps"] == 2 + 0 + 4 + 128
    with pytest.raises(_lib.LocityperError) as e:
        api.panvcf_reconstruct(gpu_ctx, "chr1", s, s + 3000, _u8(ref), PC.flat(recs), gt, ["a", "b", "c", "d"], 1.0, False)
    with pytest.raises(R.PanvcfError) as w:
        R.reconstruct("chr1", s, s + 3000, ref, recs, gt.tolist(), ["a", "b", "c", "d"], 1.0, False)
    assert e.value.code == cdefs.ERR_INVALID_DATA and str(w.value) in str(e.value) and (w.value.record, w.value.column) == (1, 3)


def test_forbidden_overlap_names_the_first_in_record_major_order(gpu_ctx):
    s, e, ref, records, gt = PC.make_case(77, 4000, 500, 70, 0.3)
    names = [f"S{c // 2}.{c % 2 + 1}" for c in range(70)]
    with pytest.raises(R.PanvcfError) as w:
        R.reconstruct("chr1", s, e, ref, records, gt.tolist(), names, 1.0, False)
    with pytest.raises(_lib.LocityperError) as g:
        api.panvcf_reconstruct(gpu_ctx, "chr1", s, e, _u8(ref), PC.flat(records), gt, names, 1.0, False)
    assert w.value.kind == "Overlap" and g.value.code == cdefs.ERR_INVALID_DATA and str(w.value) in str(g.value)


def test_a_record_over_an_end_of_the_interval_is_refused(gpu_ctx):
    rng = np.random.default_rng(8)
    ref = PC.random_seq(rng, 500)
    inner = [(1200, [ref[200:201], b"T"]), (1300, [ref[300:304], ref[300:301]])]
    for bad in ((998, [b"ACG", b"A"]), (1498, [b"ACG", b"A"])):
        recs = sorted(inner + [bad])
        gt = [[1, 0], [0, 1], [1, 1]]
        with pytest.raises(R.PanvcfError) as w:
            R.reconstruct("chr1", 1000, 1500, ref, recs, gt, ["a", "b"], 1.0, True)
        with pytest.raises(_lib.LocityperError) as g:
            api.panvcf_reconstruct(gpu_ctx, "chr1", 1000, 1500, _u8(ref), PC.flat(recs), np.array(gt), ["a", "b"], 1.0, True)
        assert w.value.kind == "Boundary" and g.value.code == cdefs.ERR_INVALID_INPUT and str(w.value) in str(g.value)
        # nobody carries it: it is not a kept record, the rest goes through; before / behind the interval it is skipped / ends the walk
        gt = [[1, 0], [0, 1], [1, 1]]
        gt[recs.index(bad)] = [0, -1]
        _check(gpu_ctx, 1000, 1500, ref, recs, gt)
    recs = [(990, [b"ACG", b"A"])] + inner + [(1500, [b"A", b"C"]), (1499, [b"AC", b"A"])]
    _check(gpu_ctx, 1000, 1500, ref, recs, [[1, 1]] * 5)
    # an allele index the record does not have
    with pytest.raises(_lib.LocityperError) as g:
        api.panvcf_reconstruct(gpu_ctx, "chr1", 1000, 1500, _u8(ref), PC.flat(inner), np.array([[1, 0], [0, 2]]), ["a", "b"], 1.0, True)
    assert g.value.code == cdefs.ERR_INVALID_DATA and "chr1:1301" in str(g.value)


def test_filter_marks_the_records_with_variation(gpu_ctx):
    _, _, _, records, gt = PC.make_case(9, 2000, 300, 67, 0.01, missing_rate=0.05)
    assert api.panvcf_filter(gpu_ctx, gt).tolist() == [R.has_variation(row) for row in gt.tolist()]


# ---------------------------------------------------------------- boundary search
def _boundary_case(seed, n, k, mw, start=50_000, rate=0.03, high=4):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, high, n + mw - k).astype(np.uint16)
    m = max(int(n * rate), 3)
    anchors = rng.integers(start - 15, start + n + 15, m)
    pos = np.sort(np.concatenate([anchors, anchors[: m // 2] + rng.integers(0, 9, m // 2), [start - 9, start - 1, start, start + n - 1, start + n, start + n + 8]]))
    rlen = rng.integers(1, 12, len(pos))
    return counts, [(int(p), int(l)) for p, l in zip(pos, rlen)]


def _check_boundary(ctx, start, end, variants, k, counts, allowed, mw, left):
    want_at, want_w = R.find_best_boundary(start, end, variants, k, [int(c) for c in counts], allowed, mw, left)
    at, w = api.db_find_boundary(ctx, start, end, [v[0] for v in variants], [v[1] for v in variants], k, counts, allowed, mw, left)
    assert at == want_at
    if want_w is not None:
        assert w.view(np.uint64).tolist() == R.bits(want_w)
    return at


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 20001])
@pytest.mark.parametrize("left", [True, False])
def test_boundary_equals_the_serial_loops_to_the_bit(gpu_ctx, n, left):
    for k, mw in ((25, 500), (11, 11)):                                     # k == moving_window: one k-mer per window
        counts, variants = _boundary_case(n * 2 + left, n, k, mw)
        _check_boundary(gpu_ctx, 50_000, 50_000 + n, variants, k, counts, max(n - 1, 1), mw, left)
        _check_boundary(gpu_ctx, 50_000, 50_000 + n, [], k, counts, 20_000, mw, left)
    # a deletion longer than the flank; counts all above 1
    counts, variants = _boundary_case(n + 7, n, 25, 500)
    assert _check_boundary(gpu_ctx, 50_000, 50_000 + n, sorted(variants + [(49_990, n + 30)]), 25, counts, 20_000, 500, left) is None
    assert _check_boundary(gpu_ctx, 50_000, 50_000 + n, [], 25, np.full(n + 475, 2, dtype=np.uint16), 20_000, 500, left) is None


def test_boundary_known_answers_and_the_tie_rule(gpu_ctx):
    from tests.test_panvcf_host import TIE_LEFT, TIE_RIGHT
    assert _check_boundary(gpu_ctx, 10, 16, [], 3, np.array(TIE_LEFT["counts"], dtype=np.uint16), 8, 10, True) == 15
    assert _check_boundary(gpu_ctx, 10, 16, [], 3, np.array(TIE_RIGHT["counts"], dtype=np.uint16), 8, 10, False) == 10
    ones = np.ones(56, dtype=np.uint16)
    assert _check_boundary(gpu_ctx, 100, 151, [], 5, ones, 50, 10, True) == 150 and _check_boundary(gpu_ctx, 100, 151, [], 5, ones, 50, 10, False) == 100
    assert _check_boundary(gpu_ctx, 100, 151, [(148, 5)], 5, ones, 50, 10, True) == 138 and _check_boundary(gpu_ctx, 100, 151, [(98, 5)], 5, ones, 50, 10, False) == 112
    for variants in ([(90, 5)], [(90, 10)], [(100, 0)], [(101, 3)]):
        for left in (True, False):
            _check_boundary(gpu_ctx, 100, 100, variants, 5, np.zeros(0, dtype=np.uint16), 50, 10, left)
    with pytest.raises(_lib.LocityperError) as e:
        api.db_find_boundary(gpu_ctx, 100, 151, [120, 110], [1, 1], 5, ones, 50, 10, True)
    assert e.value.code == cdefs.ERR_INVALID_DATA
    with pytest.raises(_lib.LocityperError) as e:
        api.db_find_boundary(gpu_ctx, 100, 151, [], [], 5, ones[:-1], 50, 10, True)
    assert e.value.code == cdefs.ERR_INVALID_INPUT


# ---------------------------------------------------------------- expansion
K, MW, EXP = 15, 100, (200, 1000, 5000)


class _Contig:
    def __init__(self, seed, length=40_000):
        rng = np.random.default_rng(seed)
        self.seq = bytearray(PC.random_seq(rng, length))
        self.counts = rng.choice(np.array([0, 1, 1, 2, 9], dtype=np.uint16), length + 1 - K)
        self.len = length

    def count_of(self, start, end):
        return [int(c) for c in self.counts[start:end + 1 - K]]

    def window(self, inner_start, inner_end):
        ws, we = max(inner_start - EXP[-1], 0), min(inner_end + EXP[-1], self.len)
        return ws, _u8(self.seq[ws:we]), self.counts[ws:we + 1 - K]


def _expand(ctx, c, inner_start, inner_end, variants, expansions=EXP):
    ws, wseq, wcnt = c.window(inner_start, inner_end)
    return api.db_expand_locus(ctx, "L1", inner_start, inner_end, c.len, ws, wseq, K, wcnt, [v[0] for v in variants], [v[1] for v in variants], expansions, MW)


def _expand_case(ctx, c, inner_start, inner_end, variants, expansions=EXP):
    want = R.expand("L1", inner_start, inner_end, c.len, bytes(c.seq), c.count_of, K, variants, expansions, MW)
    got = _expand(ctx, c, inner_start, inner_end, variants, expansions)
    assert (got["start"], got["end"], got["attempt"]) == want
    return got


def test_expansion_follows_the_retry_loop(gpu_ctx):
    c = _Contig(11)
    rng = np.random.default_rng(12)
    small = sorted((int(p), int(l)) for p, l in zip(rng.integers(14_000, 27_000, 150), rng.integers(1, 8, 150)))
    got = _expand_case(gpu_ctx, c, 20_000, 21_000, small)
    assert got["attempt"] == 0 and got["allowed_expansion"] == 200 and got["crop_bits"] == 0
    # a deletion over the whole first left flank: the first attempt fails, the second succeeds
    got = _expand_case(gpu_ctx, c, 20_000, 21_000, sorted(small + [(19_700, 310)]))
    assert got["attempt"] == 1 and got["start"] < 19_700 and got["n_attempts"] == 2
    # ... and over every flank: all attempts fail
    with pytest.raises(_lib.LocityperError) as e:
        _expand(gpu_ctx, c, 20_000, 21_000, sorted(small + [(14_000, 6_010)]))
    assert e.value.code == cdefs.ERR_RUNTIME and "Cannot expand locus L1" in str(e.value)
    with pytest.raises(R.PanvcfError):
        R.expand("L1", 20_000, 21_000, c.len, bytes(c.seq), c.count_of, K, sorted(small + [(14_000, 6_010)]), EXP, MW)
    # the contig's end clips the right flank
    got = _expand_case(gpu_ctx, c, 39_000, 39_950, [(39_960, 3)])
    assert got["end"] <= 40_000
    got = _expand_case(gpu_ctx, c, 39_000, 40_000, [])
    assert got["end"] == 40_000
    # an allowed expansion of 0 alone: the locus as it is
    assert _expand_case(gpu_ctx, c, 20_000, 21_000, small, (0,))["start"] == 20_000
    # a locus shorter than the moving window
    with pytest.raises(_lib.LocityperError) as e:
        _expand(gpu_ctx, c, 20_000, 20_050, [])
    assert e.value.code == cdefs.ERR_INVALID_INPUT and "shorter (50) than the moving window (100)" in str(e.value)


def test_expansion_crops_at_unknown_bases(gpu_ctx):
    c = _Contig(13)
    c.seq[19_900] = ord("N")
    c.seq[21_150] = ord("N")
    got = _expand_case(gpu_ctx, c, 20_000, 21_000, [])
    assert got["crop_bits"] == 3 and got["start"] > 19_900 and got["end"] <= 21_150
    c.seq[19_999] = ord("N")                                                # the base before the locus: the left flank is the locus side alone
    assert _expand_case(gpu_ctx, c, 20_000, 21_000, [])["start"] == 20_000
    for at in (20_000, 20_099, 20_999, 20_900):                             # inside the locus side of a flank
        d = _Contig(13)
        d.seq[at] = ord("N")
        with pytest.raises(_lib.LocityperError) as e:
            _expand(gpu_ctx, d, 20_000, 21_000, [])
        assert e.value.code == cdefs.ERR_INVALID_INPUT and "Unknown sequence at the locus L1" in str(e.value)
        with pytest.raises(R.PanvcfError):
            R.expand("L1", 20_000, 21_000, d.len, bytes(d.seq), d.count_of, K, [], EXP, MW)


# ---------------------------------------------------------------- the whole step
def test_locus_from_vcf_equals_build_locus_on_the_restatement(gpu_ctx, tmp_path):
    c = _Contig(21, 30_000)
    rng = np.random.default_rng(22)
    samples, ploidy = ["HG1", "HG2", "HG3", "chm13"], [2, 2, 2, 1]
    _, _, _, records, gt = PC.make_case(23, 12_000, 400, 7, 0.08, missing_rate=0.0, ref_start=9_000, max_indel=12)
    records = [(p, [bytes(c.seq[p:p + len(a[0])])] + a[1:]) for p, a in records]
    gt[:, 3] = gt[:, 0]                                                     # HG2.2 equals HG1.1: discarded_haplotypes.txt
    (tmp_path / "p.vcf.gz").write_bytes(PC.bgzf(PC.vcf_text("chr5", records, samples, ploidy, gt)))
    inner_start, inner_end, expansions = 14_000, 16_000, (300, 2_000)
    ws, we = inner_start - expansions[-1], inner_end + expansions[-1]
    info, recs = io.vcf_region(tmp_path / "p.vcf.gz", "chr5", ws, we)
    names, cs, ch, left = api.panvcf_names(info["samples"], info["ploidy"], "GRCh38", ["HG3.2"])
    assert left == 1 and names == ["GRCh38", "HG1.1", "HG1.2", "HG2.1", "HG2.2", "HG3.1", "chm13"]
    m = api.panvcf_columns(recs["gt"], info["hap_off"], cs, ch)
    # the restatement: kept records of the window, expansion, reconstruction, check_sequences, process_alleles
    idx = R.fetch(records, ws, we)
    wrecs = [records[i] for i in idx]
    kept = [(p, len(a[0])) for (p, a), row in zip(wrecs, m.tolist()) if R.has_variation(row)]
    start, end, attempt = R.expand("L1", inner_start, inner_end, c.len, bytes(c.seq), c.count_of, K, kept, expansions, 500)
    sub = R.fetch(wrecs, start, end)
    want = R.reconstruct("chr5", start, end, bytes(c.seq[start:end]), [wrecs[i] for i in sub], [m[i].tolist() for i in sub], names, 0.0001, True)
    seqs = [want["seqs"][col] for col in want["kept"]]
    knames = [names[col] for col in want["kept"]]
    assert len(seqs) == 7 and R.check_sequences(seqs) & 3 == 2
    counts = [rng.integers(0, 300, len(x) + 1 - K).astype(np.uint16) for x in seqs + [bytes(c.seq[start:end])]]
    files = RD.build_locus(knames, seqs, bytes(c.seq[start:end]), counts, K, 2)
    flat = np.concatenate(counts)
    coff = np.concatenate([[0], np.cumsum([len(x) for x in counts])]).astype(np.uint64)
    args = dict(k=K, win_counts=c.counts[ws:we + 1 - K], expansions=expansions, overlaps_allowed=True)
    first = api.db_locus_from_vcf(gpu_ctx, "L1", "chr5", inner_start, inner_end, c.len, ws, _u8(c.seq[ws:we]), recs, m, names, **args)
    assert first["fasta"] == files["fasta"] and first["kmers"] == b""      # only_seqs: the sequences to count
    got = api.db_locus_from_vcf(gpu_ctx, "L1", "chr5", inner_start, inner_end, c.len, ws, _u8(c.seq[ws:we]), recs, m, names, hap_counts=flat, hap_cnt_off=coff, **args)
    for f in ("fasta", "kmers", "discarded"):
        assert got[f] == files[f], f
    assert got["discarded"] == b"HG1.1 = HG2.2\n" and got["kept"].tolist() == files["kept"] and got["hap_cols"].tolist() == want["kept"]
    assert got["ref_bed"] == f"chr5\t{start}\t{end}\tL1\n".encode()
    st = got["locus_stats"]
    assert (st["start"], st["end"], st["attempt"]) == (start, end, attempt) and (start, end) != (inner_start, inner_end)
    assert st["warn_bits"] == R.check_sequences(seqs) and st["n_identical"] == 1 and st["n_haplotypes"] == 7 and st["n_unknown"] == 0 and st["n_with_n"] == 0
    # fewer than two haplotypes
    with pytest.raises(_lib.LocityperError) as e:
        api.db_locus_from_vcf(gpu_ctx, "L1", "chr5", inner_start, inner_end, c.len, ws, _u8(c.seq[ws:we]), recs, m[:, :1], names[:1], **args)
    assert e.value.code == cdefs.ERR_INVALID_DATA and "Less than two haplotypes" in str(e.value)


def test_locus_from_vcf_refuses_sequences_shorter_than_the_affix(gpu_ctx):
    ref = b"ACGTACGTAC" * 3
    recs = [(1001, [ref[1:29], ref[1:2]])]
    with pytest.raises(_lib.LocityperError) as e:
        api.db_locus_from_vcf(gpu_ctx, "L1", "chr5", 1000, 1030, 5000, 1000, _u8(ref), PC.flat(recs), np.array([[0, 1]]), ["a", "b"], k=K, expansions=(0,))
    assert e.value.code == cdefs.ERR_INVALID_INPUT and "fewer than the 5" in str(e.value)
