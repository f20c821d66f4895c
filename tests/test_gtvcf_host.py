"""The host half of the lcty_gtvcf_* section (extra/into_vcf.py, extra/into_csv.py) and its restatement (tests/pyref_gtvcf.py): the
restatement is pinned to answers written out by hand, the library's host entries to the restatement and to the same answers. No GPU."""
import gzip
import struct

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import gtvcf_cases as GC
from tests import pyref_gtvcf as R
from tests import pyref_sample_bam as P
from tests import vcf_index_cases as VC

# ---- one small locus, its complete file written out ------------------------------------------------------------------------------------
# variants file: V0 haploid, V1 diploid, V2 triploid -> columns V0: 0, V1: 1 2, V2: 3 4 5
SMALL = dict(
    chrom=b"chr7", contig_len=159345973, samples=[b"HG001", b"HG002", b"HG003", b"HG004"],
    recs=[dict(pos=99, alleles=[b"A", b"C"], ref_len=1), dict(pos=99, alleles=[b"AT", b"A", b"ATT"], ref_len=2), dict(pos=250, alleles=[b"G"], ref_len=1)],
    ids=[b"rs1", b"", b"."],
    gt=[[1, 0, 1, -1, 0, 1], [2, 1, 0, 2, 2, -1], [0, 0, 0, 0, 0, 0]],
    #      V1.2, GRCh38    nothing   V0      V2_1, V2.3, V1_1
    preds=[[2, R.REF], [], [0], [3, 5, 1]],
    feats=dict(qual10=[273, None, 270, None], reads=[1500, None, 0, 12], unexpl=[7, None, None, 3], wdist5=[123, None, 0, 1000000]),
    warns=[b"*", b"ignored", b"", b"GtQual;FewReads"])
SMALL_HEADER = (
    b'##fileformat=VCFv4.2\n'
    b'##FILTER=<ID=PASS,Description="All filters passed">\n'
    b'##contig=<ID=chr7,length=159345973>\n'
    b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    b'##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Converted genotype quality">\n'
    b'##FORMAT=<ID=qual,Number=1,Type=Float,Description="Raw genotype quality">\n'
    b'##FORMAT=<ID=reads,Number=1,Type=Integer,Description="Total number of reads used to predict locus genotype">\n'
    b'##FORMAT=<ID=unexpl,Number=1,Type=Integer,Description="Number of unexplained reads within the locus">\n'
    b'##FORMAT=<ID=wdist,Number=1,Type=Float,Description="Weighted distance between primary and non-primary genotype predictions">\n'
    b'##FORMAT=<ID=warn,Number=1,Type=String,Description="Genotype warnings">\n'
    b'#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tHG001\tHG002\tHG003\tHG004\n')
SMALL_LINES_ALL = (
    b'chr7\t100\trs1\tA\tC\t.\t.\t.\tGT:qual:reads:unexpl:wdist:warn\t1|0:27.3:1500:7:0.00123:*\t.\t1:27:0:.:0:.\t.|1|0:.:12:3:10:GtQual;FewReads\n'
    b'chr7\t100\t.\tAT\tA,ATT\t.\t.\t.\tGT:qual:reads:unexpl:wdist:warn\t0|0:27.3:1500:7:0.00123:*\t.\t2:27:0:.:0:.\t2|.|1:.:12:3:10:GtQual;FewReads\n'
    b'chr7\t251\t.\tG\t.\t.\t.\t.\tGT:qual:reads:unexpl:wdist:warn\t0|0:27.3:1500:7:0.00123:*\t.\t0:27:0:.:0:.\t0|0|0:.:12:3:10:GtQual;FewReads\n')
SMALL_LINES_UPSTREAM = (
    b'chr7\t100\trs1\tA\tC\t.\t.\t.\tGT:reads:unexpl:wdist\t1|0:1500:7:0.00123\t.\t1:0:.:0\t.|1|0:12:3:10\n'
    b'chr7\t100\t.\tAT\tA,ATT\t.\t.\t.\tGT:reads:unexpl:wdist\t0|0:1500:7:0.00123\t.\t2:0:.:0\t2|.|1:12:3:10\n'
    b'chr7\t251\t.\tG\t.\t.\t.\t.\tGT:reads:unexpl:wdist\t0|0:1500:7:0.00123\t.\t0:0:.:0\t0|0|0:12:3:10\n')
SMALL_CALLS = [[1, 0, 1, -1, 1, 0], [0, 0, 2, 2, -1, 1], [0, 0, 0, 0, 0, 0]]


def test_restatement_writes_the_small_locus_as_written_out_here():
    text, line_off, calls = R.locus_text(SMALL)
    assert text == SMALL_HEADER + SMALL_LINES_ALL and calls == SMALL_CALLS
    assert line_off[0] == len(SMALL_HEADER) and line_off[-1] == len(text) and all(text[o - 1:o] == b"\n" for o in line_off)
    assert R.locus_text(SMALL, R.UPSTREAM)[0] == SMALL_HEADER + SMALL_LINES_UPSTREAM
    assert R.locus_text(SMALL, 0)[0].splitlines()[-1] == b"chr7\t251\t.\tG\t.\t.\t.\t.\tGT\t0|0\t.\t0\t0|0|0"
    with pytest.raises(R.Refused):
        R.locus_text(dict(SMALL, warns=[b"*", b"", b"a b", b"*"]))
    R.locus_text(dict(SMALL, warns=[b"*", b"a b", b"", b"*"]))           # the text of a sample without a prediction is not read
    with pytest.raises(R.Refused):
        R.locus_text(dict(SMALL, gt=[[1, 0, 2, -1, 0, 1]] + SMALL["gt"][1:]))      # allele 2 of a record with two


# ---- lcty_gtvcf_columns -------------------------------------------------------------------------------------------------------------------
VS, PL = [b"V0", b"V1", b"V2", b"a.b", b"GRCh38"], [1, 2, 3, 2, 1]
COLUMN_ANSWERS = [(b"V0", 0), (b"V1.1", 1), (b"V1_2", 2), (b"V2.3", 5), (b"V2_1", 3), (b"GRCh38", R.REF), (b"a.b.1", 6), (b"a.b_2", 7), (b"V0.1", 0),
                  (b"V0_1", 0)]
# an unknown sample, with and without suffix; a last byte that is no digit; the digit 0; a digit above the ploidy; no suffix and ploidy 2, 3;
# `a.b` has a suffix by the rule of line 102 and names the sample `a`; a two-byte name is never split
COLUMN_ERRORS = [b"V9.1", b"V9", b"V1.x", b"V1.0", b"V1.3", b"V0.2", b"V1", b"V2", b"a.b", b"_1", b".1", b""]


def test_columns_every_branch_and_every_error():
    names = [a for a, _ in COLUMN_ANSWERS]
    want = [c for _, c in COLUMN_ANSWERS]
    assert [R.column(VS, PL, b"GRCh38", a) for a in names] == want
    assert api.gtvcf_columns(VS, PL, b"GRCh38", names).tolist() == want
    assert api.gtvcf_columns(VS, PL, b"GRCh38", []).tolist() == []
    # a genome name that looks suffixed is a sample first (102 before 107); one that is also a haploid sample is the genome (107 before 110)
    assert api.gtvcf_columns(VS, PL, b"V1.1", [b"V1.1"]).tolist() == [1] == [R.column(VS, PL, b"V1.1", b"V1.1")]
    assert api.gtvcf_columns(VS, PL, b"V0", [b"V0"]).tolist() == [R.REF] == [R.column(VS, PL, b"V0", b"V0")]
    for bad in COLUMN_ERRORS:
        with pytest.raises(R.Refused):
            R.column(VS, PL, b"GRCh38", bad)
        with pytest.raises(_lib.LocityperError) as e:
            api.gtvcf_columns(VS, PL, b"GRCh38", [b"V0", bad, b"V1.1"])
        assert e.value.code == cdefs.ERR_INVALID_DATA and f"`{bad.decode()}`" in str(e.value)


# ---- fixed point ------------------------------------------------------------------------------------------------------------------------
PRINT_ANSWERS = [((273, 1), b"27.3", b"27.3"), ((270, 1), b"27", b"27.0"), ((0, 1), b"0", b"0.0"), ((5, 1), b"0.5", b"0.5"), ((123, 5), b"0.00123", b"0.00123"),
                 ((1, 5), b"0.00001", b"0.00001"), ((100000, 5), b"1", b"1.00000"), ((120000, 5), b"1.2", b"1.20000"), ((10 ** 10, 1), b"1000000000", b"1000000000.0"),
                 ((-15, 1), b"-1.5", b"-1.5"), ((-20, 1), b"-2", b"-2.0"), ((42, 0), b"42", b"42"), ((R.ABSENT, 1), b".", b"nan"), ((R.ABSENT, 5), b".", b"nan"),
                 (((1 << 62) - 1, 18), b"4.611686018427387903", b"4.611686018427387903")]
PARSE_ANSWERS = [(("1000000000.0", 1), 10 ** 10), (("0.00001", 5), 1), (("nan", 1), R.ABSENT), (("NaN", 5), R.ABSENT), (("NA", 1), R.ABSENT), (("27.3", 1), 273),
                 (("27", 1), 270), (("27.", 1), 270), ((".5", 1), 5), (("27.39", 1), 273), (("-27.39", 1), -274), (("-27.30", 1), -273), (("+3", 0), 3),
                 (("0.1", 5), 10000), (("12345.678901", 5), 1234567890), (("007", 0), 7)]
PARSE_ERRORS = ["", ".", "-", "1e5", "inf", "-inf", "1.2.3", "1,5", " 1", "1 ", "0x10", "na", "99999999999999999999"]


def test_fixed_point_prints_parses_and_round_trips():
    for (v, d), plain, padded in PRINT_ANSWERS:
        assert R.fixed_print(v, d) == plain and R.fixed_print(v, d, True) == padded
        assert api.gtvcf_fixed_print(v, d) == plain and api.gtvcf_fixed_print(v, d, True) == padded
    for (text, d), want in PARSE_ANSWERS:
        assert R.fixed_parse(text, d) == want and api.gtvcf_fixed_parse(text, d) == want, text
    for bad in PARSE_ERRORS:
        if bad != "99999999999999999999":
            with pytest.raises(R.Refused):
                R.fixed_parse(bad, 1)
        with pytest.raises(_lib.LocityperError) as e:
            api.gtvcf_fixed_parse(bad, 1)
        assert e.value.code == cdefs.ERR_INVALID_DATA
    rng = np.random.default_rng(11)
    values = [0, 1, 9, 10, 99, 100, 99999, 100000, 100001, 10 ** 10, -1, -100000, R.ABSENT] + [int(x) for x in rng.integers(-10 ** 12, 10 ** 12, 300)]
    for d in (0, 1, 5):
        for v in values:
            for pad in (False, True):
                text = api.gtvcf_fixed_print(v, d, pad)
                assert text == R.fixed_print(v, d, pad)
                if text != b".":                                         # `.` is the VCF's absent value, not a number of the table
                    assert api.gtvcf_fixed_parse(text, d) == v == R.fixed_parse(text.decode(), d)
    # quality as into_csv.py:91, 96 writes it and into_vcf.py:32 reads it: floor(10 q) tenths
    for q in (0.0, 27.349, 27.35, 1234.96, 0.04):
        tenths = int(np.floor(10 * q))
        assert api.gtvcf_fixed_parse("%.1f" % (tenths * 0.1), 1) == tenths
    with pytest.raises(_lib.LocityperError):
        api.gtvcf_fixed_print(1, 19)


# ---- header -----------------------------------------------------------------------------------------------------------------------------
def test_header_text():
    assert R.header([(b"chr7", 159345973)], SMALL["samples"]) == SMALL_HEADER
    assert api.gtvcf_header([(b"chr7", 159345973)], SMALL["samples"]) == SMALL_HEADER
    got = api.gtvcf_header([(b"chr1", 248956422), (b"chrUn", None), (b"chrX", 156040895)], [b"s"])
    assert got == R.header([(b"chr1", 248956422), (b"chrUn", None), (b"chrX", 156040895)], [b"s"])
    lines = got.split(b"\n")
    assert lines[2:5] == [b"##contig=<ID=chr1,length=248956422>", b"##contig=<ID=chrUn>", b"##contig=<ID=chrX,length=156040895>"]
    assert [l[:16] for l in lines[5:12]] == [b"##FORMAT=<ID=" + k for k in (b"GT,", b"GQ,", b"qua", b"rea", b"une", b"wdi", b"war")]
    assert api.gtvcf_header([], []).endswith(b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\n")


# ---- lcty_tbi_write -----------------------------------------------------------------------------------------------------------------------
def expected_index(n_contigs, records, voffs):
    """bins, chunks, linear index and pseudo-bin of a tabix index, from reg2bin: per reference (bins {bin: [[beg, end]]}, linear, meta)"""
    refs = [dict(bins={}, lin={}, first=None, last=None, n=0) for _ in range(n_contigs)]
    for i, (t, pos, rl) in enumerate(records):
        ref, end = refs[t], pos + max(rl, 1)
        chunks = ref["bins"].setdefault(P.reg2bin(pos, end), [])
        if chunks and chunks[-1][1] == voffs[i]:
            chunks[-1][1] = voffs[i + 1]
        else:
            chunks.append([voffs[i], voffs[i + 1]])
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            ref["lin"].setdefault(w, voffs[i])
        ref["first"] = voffs[i] if ref["first"] is None else ref["first"]
        ref["last"], ref["n"] = voffs[i + 1], ref["n"] + 1
    return refs


def parse_index(plain):
    assert plain[:4] == b"TBI\1"
    n_ref, fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<8i", plain, 4)
    assert (fmt, cs, cb, ce, meta, skip) == (2, 1, 2, 0, ord("#"), 0)
    names = plain[36:36 + l_nm].split(b"\0")
    assert names[-1] == b"" and len(names) == n_ref + 1
    at, refs = 36 + l_nm, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", plain, at)
        at += 4
        bins, order, pseudo = {}, [], None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", plain, at)
            cs = [list(struct.unpack_from("<QQ", plain, at + 8 + 16 * c)) for c in range(n_chunk)]
            at += 8 + 16 * n_chunk
            order.append(b)
            if b == 37450:
                pseudo = cs
            else:
                assert b not in bins
                bins[b] = cs
        (n_intv,) = struct.unpack_from("<i", plain, at)
        lin = list(struct.unpack_from(f"<{n_intv}Q", plain, at + 4))
        at += 4 + 8 * n_intv
        refs.append((bins, lin, pseudo, order))
    assert plain[at:] == struct.pack("<Q", 0)
    return names[:-1], refs


def tbi_case(tmp_path):
    """a BGZF VCF of three contigs (one without records) whose records cross 16-kb windows, bin levels and 0xff00-byte blocks"""
    rng = np.random.default_rng(5)
    samples = [b"A", b"B"]
    head = R.header([(b"chr1", 10 ** 8), (b"chr2", None), (b"chr3", 5 * 10 ** 8)], samples)
    recs = []
    for t, positions in ((0, [0, 5, 5, 16383, 16383, 16384, 40000, 131071, 131072, 1 << 20, (1 << 26) - 3, 99999990]), (2, [7, (1 << 29) - 60])):
        for p in positions:
            recs.append((t, p, int(rng.choice([1, 1, 2, 50, 70000 if p < 10 ** 6 else 3]))))
    lines, line_off, text = [], [], bytearray(head)
    for t, p, rl in recs:
        line_off.append(len(text))
        pad = b"N" * int(rng.integers(0, 9000))                          # long lines: the text spans several blocks
        text += b"\t".join([(b"chr1", b"chr2", b"chr3")[t], b"%d" % (p + 1), b".", b"A" * rl, b"C" + pad, b".", b".", b".", b"GT", b"0|1", b"1|0"]) + b"\n"
    line_off.append(len(text))
    data, starts = P.bgzf_blocks(bytes(text), 0xff00)
    block_off = [c for _, c in starts]                                   # every data block and the end of the last
    path = tmp_path / "calls.vcf.gz"
    path.write_bytes(data)
    return path, recs, line_off, block_off, bytes(text)


def test_tbi_write_against_reg2bin_and_accepted_by_the_indexed_reader(tmp_path):
    path, recs, line_off, block_off, text = tbi_case(tmp_path)
    assert len(block_off) == (len(text) + 0xff00 - 1) // 0xff00 + 1 and len(block_off) > 3
    api.tbi_write(str(path) + ".tbi", [b"chr1", b"chr2", b"chr3"], [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], line_off, block_off)
    raw = open(str(path) + ".tbi", "rb").read()
    assert raw[:4] == b"\x1f\x8b\x08\x04" and raw[12:14] == b"BC"             # the index is BGZF itself
    plain = gzip.decompress(raw)
    voffs = [(block_off[u // 0xff00] << 16) | (u % 0xff00) for u in line_off]
    names, refs = parse_index(plain)
    assert names == [b"chr1", b"chr2", b"chr3"]
    want = expected_index(3, recs, voffs)
    for (bins, lin, pseudo, order), w in zip(refs, want):
        assert bins == w["bins"]
        assert order == sorted(order)
        if w["n"]:
            assert pseudo == [[w["first"], w["last"]], [w["n"], 0]]
            filled, prev = [], 0
            for k in range(max(w["lin"]) + 1):
                prev = w["lin"].get(k, prev)
                filled.append(prev)
            assert lin == filled
        else:
            assert pseudo is None and bins == {} and lin == []
    assert len(refs[0][0]) >= 6 and any(len(c) > 1 for c in refs[0][0].values())      # several levels, a bin with two chunks
    assert plain == VC.tbi_plain(["chr1", "chr2", "chr3"], recs, voffs)               # the writer the reader's tests were built on
    # the reader takes it, and plans every record's window to a chunk that holds the record's line
    v = io.VcfIndexed(path)
    assert v.samples == ["A", "B"] and v.ploidy.tolist() == [2, 2]
    for i, (t, p, rl) in enumerate(recs):
        chunks, _ = v.plan(("chr1", "chr2", "chr3")[t], p, p + 1)
        assert any(int(b) <= voffs[i] < int(e) for b, e in chunks), (i, t, p)
    assert len(v.plan("chr2", 0, 1 << 29)[0]) == 0
    v.close()


def test_tbi_write_refuses_what_a_tabix_index_cannot_hold(tmp_path):
    out = str(tmp_path / "x.tbi")
    ok = dict(contigs=[b"c"], contig_ix=[0, 0], pos=[5, 9], ref_len=[1, 1], line_off=[10, 20, 30], block_off=[0, 100])
    api.tbi_write(out, **ok)
    for change, code in ((dict(pos=[9, 5]), cdefs.ERR_INVALID_INPUT), (dict(contig_ix=[0, 1]), cdefs.ERR_INVALID_INPUT),
                         (dict(contigs=[b"c", b"d"], contig_ix=[1, 0]), cdefs.ERR_INVALID_INPUT), (dict(line_off=[10, 10, 30]), cdefs.ERR_INVALID_INPUT),
                         (dict(line_off=[10, 20, 0xff00 * 2]), cdefs.ERR_INVALID_INPUT), (dict(pos=[5, (1 << 29) - 1], ref_len=[1, 2]), cdefs.ERR_UNSUPPORTED)):
        with pytest.raises(_lib.LocityperError) as e:
            api.tbi_write(out, **dict(ok, **change))
        assert e.value.code == code, change
    api.tbi_write(out, **dict(ok, pos=[5, (1 << 29) - 1]))              # the last base a tabix index reaches
    api.tbi_write(out, [b"c"], [], [], [], [10], [0, 100])               # no record
    names, refs = parse_index(gzip.decompress(open(out, "rb").read()))
    assert names == [b"c"] and refs[0][:3] == ({}, [], None)


def test_set_and_locus_arguments_are_checked_before_a_device_is_needed():
    L = _lib.lib()
    assert L.lcty_gtvcf_create(None, b"a\0", 1, cdefs.GTVCF_ALL, None) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_gtvcf_add_locus(None, None, None) == cdefs.ERR_INVALID_INPUT
    L.lcty_gtvcf_destroy(None)
    L.lcty_gtvcf_out_free(None)
    assert (cdefs.GTVCF_REF, cdefs.GTVCF_ABSENT, cdefs.GTVCF_ALL, cdefs.GTVCF_UPSTREAM) == (R.REF, R.ABSENT, R.ALL, R.UPSTREAM)
    assert cdefs.GTVCF_UPSTREAM == cdefs.GTVCF_READS | cdefs.GTVCF_UNEXPL | cdefs.GTVCF_WDIST


# ---- the table between into_csv.py and into_vcf.py --------------------------------------------------------------------------------------

def into_csv_row(res):
    """process_sample's row (into_csv.py:85-96), restated with Python's own float formatting"""
    import math
    if "genotype" not in res:
        return "*"
    nan = float("nan")
    qual = math.floor(10 * float(res["quality"])) * 0.1
    get = lambda k: nan if res.get(k) is None else res[k]
    return f"{res['genotype']}\t{qual:.1f}\t{get('total_reads')}\t{get('unexpl_reads')}\t{get('weight_dist'):.5f}\t{';'.join(res.get('warnings', '*'))}"


def library_res_json(quality, n_good, unexpl, warnings, weighted_dist):
    """a res.json.gz text by the library's own writer (lcty_res_to_json)"""
    import math
    call = cdefs.Call()
    call.n_out = 1
    call.ixs[0] = 0; call.ln_probs[0] = math.log(0.9)
    call.quality = quality; call.unexpl_reads = unexpl; call.n_good = n_good; call.warnings = warnings
    return io.res_to_json(call, np.array([[1, 3]], dtype=np.uint16), ["HG001.1", "HG002.2", "NA12878", "chm13"], [-1000.0], [4.0], distances=[0],
                          weighted_dist=weighted_dist)


def test_res_summary_reads_what_the_library_writes_and_what_into_csv_reads(tmp_path):
    import json
    p = tmp_path / "res.json.gz"
    # the quality floors to tenths (27.39 -> 273), weight_dist rounds as :.5f (0.001234567 -> 123), warnings are joined by `;`
    for quality, wd, warn in ((27.39, 0.001234567, cdefs.WARN_FEW_READS | cdefs.WARN_NO_PROBABLE_GENOTYPE), (10.0, 1.25, 0), (0.05, 2.000005, 0),
                              (1e9, float("nan"), cdefs.WARN_FEW_READS)):
        text = library_res_json(quality, 9000, 17, warn, wd)
        io.write_gz(p, text.encode())
        res = json.loads(text)
        s = api.res_summary_read(p)
        cells = into_csv_row(res).split("\t")
        assert s["state"] == cdefs.RES_CALLED and s["genotype"] == b"HG002.2,chm13" == cells[0].encode()
        assert api.gtvcf_fixed_print(s["qual10"], 1, pad=True).decode() == cells[1]
        assert (s["reads"], s["unexpl"]) == (9000, 17) == (int(cells[2]), int(cells[3]))
        assert api.gtvcf_fixed_print(cdefs.GTVCF_ABSENT if s["wdist5"] is None else s["wdist5"], 5, pad=True).decode() == cells[4]
        assert s["warnings"].decode() == cells[5]
    assert (s["qual10"], s["wdist5"], s["warnings"]) == (10 ** 10, None, b"FewReads(9000)")
    # hand-written files: no genotype key is `*`, null and absent numbers are absent, a missing file is the `?` row
    for text, want in (('{"total_reads": 5, "quality": 1}', dict(state=cdefs.RES_NO_GENOTYPE, genotype=None, warnings=None, qual10=None, reads=None, unexpl=None, wdist5=None)),
                       ('{"genotype": "a.1,b_2", "quality": -0.01, "total_reads": null, "weight_dist": 0.000005, "warnings": []}',
                        dict(state=cdefs.RES_CALLED, genotype=b"a.1,b_2", warnings=b"", qual10=-1, reads=None, unexpl=None, wdist5=1 if f"{0.000005:.5f}" == "0.00001" else 0)),
                       ('{"genotype": "x", "quality": 3.999, "unexpl_reads": 0, "total_reads": 12}',
                        dict(state=cdefs.RES_CALLED, genotype=b"x", warnings=b"*", qual10=39, reads=12, unexpl=0, wdist5=None))):
        io.write_gz(p, text.encode())
        assert api.res_summary_read(p) == want, text
    assert api.res_summary_read(tmp_path / "absent" / "res.json.gz")["state"] == cdefs.RES_MISSING
    for text in ('{"genotype": "x"}', '{"genotype": "x", "quality": null}', '{"genotype": 3, "quality": 1}', '{"genotype": "x", "quality": 1, "total_reads": 1.5}',
                 '{"genotype": "x", "quality": 1, "warnings": "w"}', '[1]', '{"genotype": '):
        io.write_gz(p, text.encode())
        with pytest.raises(_lib.LocityperError) as e:
            api.res_summary_read(p)
        assert e.value.code == cdefs.ERR_INVALID_DATA, text
    p.write_bytes(b'{"genotype": "x", "quality": 1}')
    with pytest.raises(_lib.LocityperError) as e:
        api.res_summary_read(p)
    assert e.value.code == cdefs.ERR_INVALID_DATA


def test_predictions_csv_writer_and_reader_against_each_other_and_a_written_out_table(tmp_path):
    import json
    p = tmp_path / "res.json.gz"
    io.write_gz(p, library_res_json(27.39, 9000, 17, cdefs.WARN_FEW_READS, 0.001234567).encode())
    from_file = api.res_summary_read(p)
    called = dict(state=cdefs.RES_CALLED, genotype=b"NA12878,chm13", warnings=b"*", qual10=10 ** 10, reads=0, unexpl=None, wdist5=1)
    rows = [("s2", "locA", from_file), ("s10", "locA", dict(state=cdefs.RES_NO_GENOTYPE)), ("s1", "locB", dict(state=cdefs.RES_MISSING)), ("s1", "locA", called),
            ("S9", "locB", dict(called, qual10=None, wdist5=None, warnings=b""))]
    want = ("sample\tlocus\tgenotype\tquality\ttotal_reads\tunexpl_reads\tweight_dist\twarnings\n"
            "s2\tlocA\tHG002.2,chm13\t27.3\t9000\t17\t0.00123\tFewReads(9000)\n"
            "s10\tlocA\t*\n"
            "s1\tlocB\t?\n"
            "s1\tlocA\tNA12878,chm13\t1000000000.0\t0\tnan\t0.00001\t*\n"
            "S9\tlocB\tNA12878,chm13\tnan\t0\tnan\tnan\t\n")
    # the first row is what into_csv.py writes for the library's file
    assert want.split("\n")[1] == "s2\tlocA\t" + into_csv_row(json.loads(gzip.open(p, "rt").read()))
    for name in ("pred.csv", "pred.csv.gz"):
        out = tmp_path / name
        api.predictions_csv_write(out, rows)
        assert (gzip.open(out, "rb").read() if name.endswith(".gz") else out.read_bytes()) == want.encode()
        back = api.predictions_csv_read(out)
        assert back["samples"] == [b"S9", b"s1", b"s10", b"s2"]                      # bytewise (into_vcf.py:44)
        assert len(back["rows"]) == len(rows)
        for got, (sample, locus, s) in zip(back["rows"], rows):
            assert (got["sample"], got["locus"]) == (sample.encode(), locus.encode())
            if s["state"] != cdefs.RES_CALLED:
                assert got["genotype"] == (b"*" if s["state"] == cdefs.RES_NO_GENOTYPE else b"?") and got["warnings"] == b""
                assert [got[k] for k in ("qual10", "reads", "unexpl", "wdist5")] == [None] * 4
            else:
                assert {k: got[k] for k in ("genotype", "warnings", "qual10", "reads", "unexpl", "wdist5")} == {k: s[k] for k in ("genotype", "warnings", "qual10", "reads", "unexpl", "wdist5")}
    # read_csv: comment lines before the column line, columns by name in any order, NA, a table without the optional columns, \r\n
    out = tmp_path / "other.csv"
    out.write_bytes(b"# made by hand\n#\nlocus\tweight_dist\tgenotype\textra\tsample\tquality\r\nL\tNA\ta.1,a.2\tx\tb\t12.349999999999999999\r\n\nL\t0.5\t*\ty\ta\t-0.05\n")
    back = api.predictions_csv_read(out)
    assert back["samples"] == [b"a", b"b"]
    assert back["rows"][0] == dict(sample=b"b", locus=b"L", genotype=b"a.1,a.2", warnings=b"", qual10=123, reads=None, unexpl=None, wdist5=None)
    assert back["rows"][1] == dict(sample=b"a", locus=b"L", genotype=b"*", warnings=b"", qual10=-1, reads=None, unexpl=None, wdist5=50000)
    for text in (b"", b"# only\n", b"sample\tlocus\nq\tw\n", b"sample\tlocus\tgenotype\na\tb\n", b"sample\tlocus\tgenotype\tquality\na\tb\tc\t1e3\n"):
        out.write_bytes(text)
        with pytest.raises(_lib.LocityperError) as e:
            api.predictions_csv_read(out)
        assert e.value.code == cdefs.ERR_INVALID_DATA, text
    for bad in (("s\t1", "l", called), ("s", "", called), ("s", "l", dict(called, genotype=b"a\nb")), ("s", "l", dict(called, state=7))):
        with pytest.raises(_lib.LocityperError) as e:
            api.predictions_csv_write(out, [bad])
        assert e.value.code == cdefs.ERR_INVALID_INPUT


def test_indexed_reader_lists_the_contigs_of_the_head_in_index_order(tmp_path):
    """lcty_vcf_indexed_contigs: the ##contig lines in file order with their lengths, then what only the tabix index names"""
    rng = np.random.default_rng(3)
    recs = [VC.rec(c, 10 + 5 * i, b"A", [b"C"], VC.random_calls(rng, [2], 1)) for c in ("chrB", "chrOnlyInIndex") for i in range(3)]
    head = [b"##fileformat=VCFv4.2", b"##contig=<ID=chrZ,length=999>", b"##contig=<length=50000,ID=chrA,assembly=x>", b"##contig=<ID=chrB>",
            b"##contig=<ID=chrZ,length=5>", b"##contig=<assembly=y>", b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">']
    VC.write_indexed(tmp_path / "v.vcf.gz", ["S"], recs, header=head)
    v = io.VcfIndexed(tmp_path / "v.vcf.gz")
    assert v.contigs() == [("chrZ", 999), ("chrA", 50000), ("chrB", 0), ("chrOnlyInIndex", 0)]
    v.close()
    VC.write_indexed(tmp_path / "w.vcf.gz", ["S"], recs[:3], header=head[:1])
    v = io.VcfIndexed(tmp_path / "w.vcf.gz")
    assert v.contigs() == [("chrB", 0)]
    v.close()
