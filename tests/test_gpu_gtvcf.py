"""A cohort's genotypes as a VCF on the device (lcty_gtvcf.hip) against the serial restatement (tests/pyref_gtvcf.py), byte for byte, at the
smallest shapes where the kernels can go wrong; and the round trip through the library's own deflate, tabix writer and indexed reader,
which trusts neither."""
import functools

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import gtvcf_cases as GC
from tests import pyref_gtvcf as R
from tests import test_gtvcf_host as H

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(seed, n_samples, n_recs, no_pred=(), allele_counts=None, **kw):
    c = GC.make_case(seed, n_samples, n_recs, no_pred=no_pred, allele_counts=allele_counts, **kw)
    c["want"] = {}
    return c


def want(c, mask):
    if mask not in c["want"]:
        c["want"][mask] = R.locus_text(c, mask)
    return c["want"][mask]


def run(ctx, c, mask=cdefs.GTVCF_ALL, vcf=None, **over):
    own = vcf is None
    vcf = api.GenotypeVcf(ctx, c["samples"], mask) if own else vcf
    try:
        a = dict(chrom=c["chrom"], contig_len=c.get("contig_len"), recs=GC.arrays(c), gt=GC.gt_matrix(c),
                 preds=c["preds"], ids=c.get("ids"), feats=c.get("feats"), warns=c.get("warns"), want_calls=True, locus=c.get("locus"),
                 contig_ix=c.get("contig_ix", 0), start=c.get("start", 0), end=c.get("end", 0))
        a.update(over)
        return vcf.add_locus(**a)
    finally:
        if own:
            vcf.close()


def check(ctx, c, mask=cdefs.GTVCF_ALL, vcf=None):
    got = run(ctx, c, mask, vcf)
    text, line_off, calls = want(c, mask)
    assert got["text"] == text
    assert got["line_off"].tolist() == line_off
    n_slots = sum(len(p) for p in c["preds"])
    assert got["calls"].shape == (len(c["recs"]), n_slots) and got["calls"].tolist() == [list(r) for r in calls]
    st = got["stats"]
    assert (st["n_records"], st["n_samples"], st["n_slots"], st["text_bytes"]) == (len(c["recs"]), len(c["samples"]), n_slots, len(text))
    assert st["n_predicted"] == sum(1 for p in c["preds"] if p) and st["header_bytes"] == line_off[0]
    return got


def small_case():
    c = dict(H.SMALL, n_haps=6)
    c["want"] = {}
    return c


def test_small_locus_is_the_text_written_out_by_hand(gpu_ctx):
    c = small_case()
    assert check(gpu_ctx, c)["text"] == H.SMALL_HEADER + H.SMALL_LINES_ALL
    assert check(gpu_ctx, c, cdefs.GTVCF_UPSTREAM)["text"] == H.SMALL_HEADER + H.SMALL_LINES_UPSTREAM


@pytest.mark.parametrize("n_samples", [1, 3, 64, 65, 257])
def test_sample_counts_at_the_wavefront_and_the_scan_chunk_edges(gpu_ctx, n_samples):
    # 70 records: more than one wavefront of records; ploidy 1, 2, 3 mixed, missing alleles, the genome's name, haploid samples without suffix
    c = case(100 + n_samples, n_samples, 70)
    names = [a for p in c["pred_names"] if p for a in p]
    if n_samples >= 64:
        assert GC.GENOME in names and any(a in c["vsamples"] for a in names) and any(a[-2:-1] == b"." for a in names) and any(a[-2:-1] == b"_" for a in names)
        assert {len(p) for p in c["preds"]} == {1, 2, 3} and any(v < 0 for row in want(c, cdefs.GTVCF_ALL)[2] for v in row)
    check(gpu_ctx, c)


@pytest.mark.parametrize("n_recs", [0, 1])
def test_no_record_and_one_record(gpu_ctx, n_recs):
    c = case(7, 5, n_recs)
    got = check(gpu_ctx, c)
    assert got["text"].count(b"\n") == 11 + n_recs
    check(gpu_ctx, case(8, 0, n_recs))                                   # and no sample at all


def test_allele_numbers_of_every_digit_count_and_300_alt_alleles(gpu_ctx):
    # the designed columns 0 .. 5 hold the last allele and alleles 9, 10, 99, 100: records with 10, 11, 100, 101 and 32 768 alleles
    c = case(3, 9, 8, allele_counts=(10, 11, 100, 101, 32768, 301), missing_rate=0.05)
    text, _, calls = want(c, cdefs.GTVCF_ALL)
    seen = {v for row in calls for v in row}
    assert {9, 10, 99, 100, 32767} <= seen
    assert any(len(a) == 0 for a in c["recs"][5]["alleles"]) and max(len(a) for a in c["recs"][5]["alleles"]) == 300
    check(gpu_ctx, c)


@pytest.mark.parametrize("where", ["first", "last", "every", "inner"])
def test_samples_without_a_prediction(gpu_ctx, where):
    n = 66
    none = dict(first=(0,), last=(n - 1,), every=tuple(range(n)), inner=(1, 63, 64))[where]
    c = case(21, n, 5, no_pred=none)
    got = check(gpu_ctx, c)
    if where == "every":
        assert got["calls"].shape == (5, 0) and got["text"].endswith(b"\t." * n + b"\n")


def test_every_field_mask_absent_features_and_warning_texts(gpu_ctx):
    long_text = bytes(np.random.default_rng(1).choice(list(b"abc;_-*"), 65535).astype(np.uint8))
    c = case(31, 9, 3, warn_texts=(b"", long_text, b"*", b"A;B"), absent_rate=0.4)
    assert any(len(w) == 65535 for w in c["warns"]) and any(len(w) == 0 for w in c["warns"])
    assert any(v is None for v in c["feats"]["qual10"]) and any(v is not None for v in c["feats"]["wdist5"])
    for mask in range(32):
        got = check(gpu_ctx, c, mask)
        assert got["text"].splitlines()[-1].split(b"\t")[8] == R.format_key(mask)
    # arrays that are not given at all are absent for everyone
    bare = dict(c, feats=None, warns=None, want={})
    line = check(gpu_ctx, bare)["text"].splitlines()[-1].split(b"\t")
    assert all(f == b"." or f.endswith(b":.:.:.:.:.") for f in line[9:])
    check(gpu_ctx, dict(c, ids=None, want={}))


def test_two_calls_give_identical_bytes_and_a_set_serves_many_loci(gpu_ctx):
    a, b = case(41, 65, 30), dict(case(42, 65, 3, no_pred=(2,)), contig_ix=1)      # another contig: another contig index
    vcf = api.GenotypeVcf(gpu_ctx, a["samples"])
    first = check(gpu_ctx, a, vcf=vcf)
    check(gpu_ctx, b, vcf=vcf)                                           # a smaller locus in the scratch of a larger one
    again = check(gpu_ctx, a, vcf=vcf)
    assert first["text"] == again["text"] and np.array_equal(first["line_off"], again["line_off"]) and np.array_equal(first["calls"], again["calls"])
    vcf.close()


def test_every_error_status_leaves_the_set_usable(gpu_ctx):
    c = case(51, 6, 4)
    vcf = api.GenotypeVcf(gpu_ctx, c["samples"])
    check(gpu_ctx, c, vcf=vcf)
    arrays, gt = GC.arrays(c), GC.gt_matrix(c)
    bad_gt = gt.copy(); bad_gt[2, 0] = len(c["recs"][2]["alleles"])      # column 0 is V0, which sample 0 reads
    bad_ra = arrays["rec_allele"].copy(); bad_ra[1] = bad_ra[2]
    bad_ao = arrays["allele_off"].copy(); bad_ao[1] = bad_ao[-1] + 5
    cases = [(dict(warns=[b"a b"] + c["warns"][1:]), cdefs.ERR_INVALID_DATA, "S0000"), (dict(warns=[b"*", b"x:y"] + c["warns"][2:]), cdefs.ERR_INVALID_DATA, "S0001"),
             (dict(warns=c["warns"][:-1] + [b"a\tb"]), cdefs.ERR_INVALID_DATA, "S0005"), (dict(warns=[b"a\nb"] + c["warns"][1:]), cdefs.ERR_INVALID_DATA, "S0000"),
             (dict(gt=bad_gt), cdefs.ERR_INVALID_DATA, "record 2"), (dict(preds=[[c["n_haps"]]] + c["preds"][1:]), cdefs.ERR_INVALID_INPUT, "column"),
             (dict(preds=[[0] * 256] + c["preds"][1:]), cdefs.ERR_UNSUPPORTED, "256"), (dict(warns=[b"x" * 65536] + c["warns"][1:]), cdefs.ERR_UNSUPPORTED, "65536"),
             (dict(recs=dict(arrays, rec_allele=bad_ra)), cdefs.ERR_INVALID_INPUT, "record 1 has no allele"),
             (dict(recs=dict(arrays, allele_off=bad_ao)), cdefs.ERR_INVALID_INPUT, "allele_off"), (dict(chrom=b""), cdefs.ERR_INVALID_INPUT, "contig")]
    for over, code, word in cases:
        with pytest.raises(_lib.LocityperError) as e:
            run(gpu_ctx, c, vcf=vcf, **over)
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
        check(gpu_ctx, c, vcf=vcf)
    vcf.close()
    for samples, mask in (([b"a", b""], 31), ([b"a\tb"], 31), ([b"a"], 32)):
        with pytest.raises(_lib.LocityperError) as e:
            api.GenotypeVcf(gpu_ctx, samples, mask)
        assert e.value.code == cdefs.ERR_INVALID_INPUT


# ---- the merge ---------------------------------------------------------------------------------------------------------------------------

def check_merge(ctx, loci, mask=cdefs.GTVCF_ALL, vcf=None):
    """add the loci in the order given, merge, compare with the restatement"""
    own = vcf is None
    vcf = api.GenotypeVcf(ctx, loci[0]["samples"], mask) if own else vcf
    try:
        for c in loci:
            c.setdefault("want", {})
            if own:
                check(ctx, c, mask, vcf)
        got = vcf.merge()
        text, line_off, info, joined = R.merge_text(loci, mask)
        assert got["text"] == text
        assert got["line_off"].tolist() == line_off and got["n_joined"] == joined
        # line_contig is the place among the header's contigs (what tbi_write takes), contig_ix the variants file's index of each
        assert got["contig_ix"].tolist() == sorted(set(c["contig_ix"] for c in loci)) and len(got["contigs"]) == len(got["contig_ix"])
        assert all(0 <= k < len(got["contigs"]) for k in got["line_contig"].tolist())
        assert list(zip(got["contig_ix"][got["line_contig"]].tolist(), got["line_pos"].tolist(), got["line_ref_len"].tolist())) == info
        assert got["stats"]["n_records"] == sum(len(c["recs"]) for c in loci)
        return got
    finally:
        if own:
            vcf.close()


def overlapping(n_samples=70, designed=True):
    """three loci over one window of 30 records: A [0, 20), B [10, 30), C [15, 25), each with its own predictions and features"""
    base = case(71, n_samples, 30)
    others = [GC.make_case(72 + k, n_samples, 0, no_pred=(4,) if designed and k == 1 else (5,) if designed and k == 0 else ()) for k in range(3)]
    if designed:                                                         # tenths in A, B: larger, equal in whole units, smaller, absent first, absent later
        for s, (qa, qb) in enumerate([(100, 205), (200, 209), (300, 100), (None, 5), (50, 60), (50, 60), (70, None)]):
            others[0]["feats"]["qual10"][s], others[1]["feats"]["qual10"][s] = qa, qb
        for s in (0, 1, 2, 3, 6):                                        # other columns in B than in A: the GTs differ in most records
            others[0]["preds"][s], others[1]["preds"][s] = [0, 1 + s], [6 + s, 2]
    return [GC.window(base, others[0], 0, 20, b"A"), GC.window(base, others[1], 10, 30, b"B"), GC.window(base, others[2], 15, 25, b"C")]


def test_merge_of_two_and_three_overlapping_loci(gpu_ctx):
    a, b, c = overlapping()
    got = check_merge(gpu_ctx, [a, b])
    assert got["n_joined"] == 10 and len(got["line_pos"]) == 30
    # the designed samples in the joined records (10 .. 19 of the window): a larger quality replaces a differing GT, an equal and a smaller
    # one do not, an absent quality loses, a sample predicted in one locus only shows that prediction
    keys = sorted((r["pos"], tuple(r["alleles"])) for r in a["recs"] + b["recs"][10:])
    assert len(set(keys)) == 30

    def field(cell):
        return b"|".join(b"." if v < 0 else b"%d" % v for v in cell[0]) + cell[1]
    replaced = 0
    for k in range(10, 20):
        ra, rb = R.locus_records(a)[k][4], R.locus_records(b)[k - 10][4]
        at = keys.index((a["recs"][k]["pos"], tuple(a["recs"][k]["alleles"])))
        line = got["text"][int(got["line_off"][at]):int(got["line_off"][at + 1])].rstrip(b"\n").split(b"\t")[9:]
        for s in (0, 3):
            assert line[s] == field(rb[s] if ra[s][0] != rb[s][0] else ra[s])
            replaced += ra[s][0] != rb[s][0]
        assert line[1] == field(ra[1]) and line[2] == field(ra[2]) and line[6] == field(ra[6])
        assert rb[4][0] is None and line[4] == field(ra[4]) and ra[5][0] is None and line[5] == field(rb[5])
    assert replaced >= 5
    got3 = check_merge(gpu_ctx, [a, b, c])
    assert got3["n_joined"] == 20 and len(got3["line_pos"]) == 30
    for mask in (0, cdefs.GTVCF_UPSTREAM):                               # the join reads the quality whatever the FORMAT shows
        check_merge(gpu_ctx, [dict(x, want={}) for x in (a, b, c)], mask)


def test_merge_takes_the_loci_in_sorted_order_whatever_the_order_of_the_adds(gpu_ctx):
    a, b, c = overlapping(9)
    far = GC.window(case(73, 9, 6), GC.make_case(74, 9, 0), 0, 6, b"far", contig_ix=0, chrom=a["chrom"], contig_len=a["contig_len"])
    for r in far["recs"]:
        r["pos"] += 10 ** 6
    far["start"], far["end"] = far["start"] + 10 ** 6, far["end"] + 10 ** 6
    other = GC.window(case(75, 9, 5), GC.make_case(76, 9, 0), 0, 5, b"other", contig_ix=3, chrom=b"chrOther", contig_len=None)
    early = GC.window(case(77, 9, 4), GC.make_case(78, 9, 0), 0, 4, b"early", contig_ix=1, chrom=b"chrEarly", contig_len=12345)
    empty = GC.window(case(79, 9, 0), GC.make_case(80, 9, 0), 0, 0, b"empty", contig_ix=1, chrom=b"chrEarly", contig_len=12345)
    texts = set()
    for order in ([far, c, other, b, empty, a, early], [a, b, c, far, early, empty, other], [other, early, far, empty, c, b, a]):
        got = check_merge(gpu_ctx, [dict(x, want={}) for x in order])
        texts.add(got["text"])
        assert got["contigs"] == [a["chrom"], b"chrEarly", b"chrOther"] and sorted(set(got["line_contig"].tolist())) == [0, 1, 2] and got["contig_ix"].tolist() == [0, 1, 3]
    assert len(texts) == 1                                               # a, b, c differ in (start, end): the order of the adds never decides
    # two loci with the same interval: the one added first is the first
    twin = dict(b, locus=b"B2", feats=dict(b["feats"], qual10=[None] * 9), want={})
    t1 = check_merge(gpu_ctx, [dict(b, want={}), twin])["text"]
    t2 = check_merge(gpu_ctx, [twin, dict(b, want={})])["text"]
    assert t1 != t2


TUPLES = [(b"A", b"C"), (b"A", b"C", b"G"), (b"A",), (b"A", b"CC"), (b"AT", b"C"), (b"A", b"C", b"G", b"T"), (b"A", b""), (b"", b"C"), (b"A", b"C", b""),
          (b"AC", b"C"), (b"A", b"D"), (b"a", b"C"), (b"A", b"C\xff"), (b"A", b"C", b"G")]


def test_merge_one_position_with_several_allele_tuples(gpu_ctx):
    n = 5
    p1, p2 = GC.make_case(81, n, 0), GC.make_case(82, n, 0)
    n_haps = p1["n_haps"]
    r1, g1 = GC.records_at(500, TUPLES[:9], n_haps, 1)
    r2, g2 = GC.records_at(500, TUPLES[5:][::-1], n_haps, 2)             # shares four tuples with the first, one of them twice in itself
    low, glow = GC.records_at(499, [(b"T", b"TT")], n_haps, 3)
    a = dict(p1, recs=low + r1, gt=glow + g1, ids=None, locus=b"a", contig_ix=0, start=499, end=501, want={})
    b = dict(p2, recs=r2, gt=g2, ids=None, locus=b"b", contig_ix=0, start=500, end=501, chrom=p1["chrom"], contig_len=p1["contig_len"], want={})
    got = check_merge(gpu_ctx, [a, b])
    keys = [tuple(l.split(b"\t")[3:5]) for l in got["text"].splitlines() if not l.startswith(b"#")]
    assert len(keys) == 1 + len(set(TUPLES)) and got["n_joined"] == 1 + len(r1) + len(r2) - len(keys) == 5
    assert keys[1][0] == b"" and keys.index((b"A", b".")) < keys.index((b"A", b"")) < keys.index((b"A", b"C")) < keys.index((b"A", b"C,")) < keys.index((b"A", b"C,G"))


def run_of(n_records, n_samples=3):
    """n_records records at one position with different alleles, over two loci that share eight of them"""
    p1, p2 = GC.make_case(91, n_samples, 0), GC.make_case(92, n_samples, 0)
    tuples = [(b"G", b"G" + b"%d" % k) for k in range(n_records)]
    r1, g1 = GC.records_at(77, tuples[:40][::-1], p1["n_haps"], 4)
    r2, g2 = GC.records_at(77, tuples[32:], p1["n_haps"], 5)
    a = dict(p1, recs=r1, gt=g1, ids=None, locus=b"a", contig_ix=2, start=77, end=78, want={})
    b = dict(p2, recs=r2, gt=g2, ids=None, locus=b"b", contig_ix=2, start=77, end=79, chrom=p1["chrom"], contig_len=p1["contig_len"], want={})
    return a, b


def test_merge_run_of_64_records_and_65_refused(gpu_ctx):
    a, b = run_of(56)                                                    # 40 + 24 = 64 records at the position, 56 keys
    got = check_merge(gpu_ctx, [a, b])
    assert got["stats"]["n_records"] == 64 and got["n_joined"] == 8 and len(got["line_pos"]) == 56
    a, b = run_of(57)                                                    # 65
    vcf = api.GenotypeVcf(gpu_ctx, a["samples"])
    check(gpu_ctx, a, vcf=vcf)
    check(gpu_ctx, b, vcf=vcf)
    with pytest.raises(_lib.LocityperError) as e:
        vcf.merge()
    assert e.value.code == cdefs.ERR_UNSUPPORTED and "position 78" in str(e.value)
    check(gpu_ctx, a | dict(locus=b"again", want={}), vcf=vcf)           # the set is usable: an add, and the same refusal
    with pytest.raises(_lib.LocityperError):
        vcf.merge()
    with pytest.raises(_lib.LocityperError) as e:
        run(gpu_ctx, a, vcf=vcf)                                         # a locus of this name is in the set
    assert e.value.code == cdefs.ERR_INVALID_INPUT
    vcf.close()
    empty = api.GenotypeVcf(gpu_ctx, a["samples"])
    got = empty.merge()                                                  # no locus: the header without contigs
    assert got["text"] == R.header([], a["samples"]) and got["line_off"].tolist() == [len(got["text"])]
    empty.close()


def test_merge_twice_gives_identical_bytes_and_round_trips_through_the_index(gpu_ctx, tmp_path):
    """merged.vcf.gz + .tbi, deflated on the device, reopened: every locus's interval gives back the positions and alleles that went in"""
    a, b, c = overlapping(20, designed=False)
    # sparse contig indices, as a cohort on chromosomes 3 and 22 of a variants file has them: the index lists the header's two contigs
    other = GC.window(case(75, 20, 5), GC.make_case(76, 20, 0), 0, 5, b"other", contig_ix=21, chrom=b"chrOther", contig_len=None)
    a, b, c = (dict(x, contig_ix=2) for x in (a, b, c))
    loci = [other, c, a, b]
    vcf = api.GenotypeVcf(gpu_ctx, a["samples"])
    for x in loci:
        x["want"] = {}
        check(gpu_ctx, x, vcf=vcf)
    got = check_merge(gpu_ctx, loci, vcf=vcf)
    assert vcf.merge()["text"] == got["text"]
    vcf.close()
    data, block_off, _ = io.bgzf_deflate(gpu_ctx, got["text"])
    path = tmp_path / "merged.vcf.gz"
    path.write_bytes(data.tobytes())
    api.tbi_write(str(path) + ".tbi", got["contigs"], got["line_contig"], got["line_pos"], got["line_ref_len"], got["line_off"], block_off)
    v = io.VcfIndexed(path, ctx=gpu_ctx)
    for x in loci:
        back = v.region(x["chrom"].decode(), x["start"], x["end"])
        arrays = GC.arrays(x)
        keep = [r for r in range(len(x["recs"])) if arrays["pos"][r] < x["end"] and arrays["pos"][r] + arrays["ref_len"][r] > x["start"]]
        mine = sorted((x["recs"][r]["pos"], tuple(x["recs"][r]["alleles"])) for r in keep)
        theirs = []
        for r in range(len(back["pos"])):
            al = [back["allele_bytes"][int(back["allele_off"][k]):int(back["allele_off"][k + 1])].tobytes() for k in range(back["rec_allele"][r], back["rec_allele"][r + 1])]
            theirs.append((int(back["pos"][r]), tuple(al)))
        # the window of the merged file holds every record of the locus, in order, and nothing the loci did not give
        assert theirs == sorted(theirs) and len(set(theirs)) == len(theirs) and set(mine) <= set(theirs)
        assert all(p < x["end"] for p, _ in theirs)
    v.close()


def test_round_trip_through_deflate_tabix_writer_and_indexed_reader(gpu_ctx, tmp_path):
    """the written file, deflated on the device and indexed by lcty_tbi_write, read back by lcty_vcf_indexed_fetch: the GT matrix is the
    gathered calls, positions and alleles are the inputs"""
    c = case(61, 70, 40, no_pred=(5, 69), allele_counts=(120, 12, 1), all_predicted=True)
    got = run(gpu_ctx, c)
    arrays = GC.arrays(c)
    data, block_off, _ = io.bgzf_deflate(gpu_ctx, got["text"])
    path = tmp_path / "locus.vcf.gz"
    path.write_bytes(data.tobytes())
    api.tbi_write(str(path) + ".tbi", [c["chrom"]], np.zeros(len(arrays["pos"]), np.uint32), arrays["pos"], arrays["ref_len"], got["line_off"], block_off)
    v = io.VcfIndexed(path, ctx=gpu_ctx)
    assert [s.encode() for s in v.samples] == c["samples"]
    assert v.ploidy.tolist() == [max(len(p), 1) for p in c["preds"]]
    # a sample without a prediction reads back as one missing allele
    cols, k = [], 0
    for p in c["preds"]:
        cols.append(list(range(k, k + len(p))) if p else [None])
        k += len(p)
    want_gt = np.array([[-1 if j is None else row[j] for p in cols for j in p] for row in got["calls"].tolist()], dtype=np.int16)
    last = int(arrays["pos"][-1])
    back = v.region(c["chrom"].decode(), 0, last + 1)
    assert np.array_equal(back["gt"], want_gt)
    for key in ("pos", "ref_len", "rec_allele", "allele_off", "allele_bytes"):
        assert np.array_equal(back[key], arrays[key]), key
    # windows inside the locus come through the index: the records fetch(start, end) returns
    for start, end in ((int(arrays["pos"][7]), int(arrays["pos"][20]) + 1), (last, last + 1), (0, 1)):
        keep = [r for r in range(len(arrays["pos"])) if arrays["pos"][r] < end and arrays["pos"][r] + arrays["ref_len"][r] > start]
        part = v.region(c["chrom"].decode(), start, end)
        assert part["pos"].tolist() == arrays["pos"][keep].tolist() and np.array_equal(part["gt"], want_gt[keep])
    v.close()
