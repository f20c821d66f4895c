"""The indexed VCF reader on the device (lcty_vcf_indexed_fetch, io.VcfIndexed.region) against the whole-file host reader (io.Vcf.region)
on the same BGZF file: every array equal, every error the same status and text, with the host and the device inflate. The files are
small and designed (tests/vcf_index_cases.py): BGZF blocks of 700 bytes, so lines straddle blocks and chunks start inside one."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, io
from locityper_amd._lib import LocityperError
from tests import pyref_panvcf as R
from tests import vcf_index_cases as VC

pytestmark = pytest.mark.gpu
KEYS = ("pos", "ref_len", "rec_allele", "allele_off", "allele_bytes", "gt", "phased")
ALL = (0, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def outcome(reader, *args, **kw):
    """('ok', arrays) or ('error', status, text) of a region call"""
    try:
        return ("ok", reader.region(*args, **kw))
    except LocityperError as e:
        return ("error", e.code, str(e))


def same(got, want, what):
    assert got[0] == want[0], (what, got, want)
    if want[0] == "error":
        assert got[1:] == want[1:], what
        return
    for key in KEYS:
        assert got[1][key].dtype == want[1][key].dtype and got[1][key].shape == want[1][key].shape and np.array_equal(got[1][key], want[1][key]), (what, key)


def compare(ctx, path, regions, used=None):
    """Every region with both inflates against the host reader; -> the host reader's outcomes and the stats of the last fetches."""
    v, w = io.Vcf(path), io.VcfIndexed(path, ctx=ctx)
    assert w.samples == v.samples and w.ploidy.tolist() == v.ploidy.tolist()
    wants, stats = [], []
    try:
        for contig, start, end in regions:
            want = outcome(v, contig, start, end, used)
            for inflate in (0, 1):
                ctx.set_knob("sample_bam_inflate", inflate)
                same(outcome(w, contig, start, end, used), want, (contig, start, end, inflate))
            wants.append(want)
            stats.append(w.stats)
    finally:
        ctx.set_knob("sample_bam_inflate", -1)
        v.close(); w.close()
    return wants, stats


@pytest.mark.parametrize("n_samples", [1, 3, 65, 130])
def test_line_shapes_and_format_variants(ctx, tmp_path, n_samples):
    pl, recs = VC.shaped_records(100 + n_samples, n_samples, n=70)
    assert 1 in pl[:n_samples] or n_samples == 1
    path = str(tmp_path / "a.vcf.gz")
    info = VC.write_indexed(path, VC.names_of(n_samples), recs)
    lens = [len(VC.line_of(r)) for r in recs]
    assert max(lens) > 256 and (min(lens) < 64 or n_samples > 3) and {r["fmt"] for r in recs} == {"GT", "GT:DP", "DP:GT"}
    text = info["text"].decode()
    assert "\t.|" in text or "|.\t" in text or "\t.\t" in text
    p = [r["pos"] for r in recs]
    wants, _ = compare(ctx, path, [("chr1",) + ALL, ("chr1", p[10], p[40]), ("chr1", p[69], p[69] + 1), ("chr1", 0, p[0])])
    assert len(wants[0][1]["pos"]) == 70 and 25 <= len(wants[1][1]["pos"]) <= 45 and len(wants[3][1]["pos"]) == 0
    big = wants[0][1]["gt"]
    assert (big >= 100).any() and (big >= 10).any() and (big == -1).any()
    # a subset of the samples: nothing changes for a clean file
    used = np.arange(n_samples) % 2
    compare(ctx, path, [("chr1",) + ALL], used)


def test_a_head_longer_than_four_steps(ctx, tmp_path):
    rng = np.random.default_rng(3)
    pl = [2, 1, 2]
    recs = [VC.rec("chr1", 500 + 10 * i, b"A", [b"C"], VC.random_calls(rng, pl, 1)) for i in range(5)]
    long_ = VC.rec("chr1", 600, VC.seq(rng, 300), [b"G", VC.seq(rng, 400)], VC.random_calls(rng, pl, 2), vid="x" * 80)
    recs += [long_] + [VC.rec("chr1", 1000 + 10 * i, b"AT", [b"A"], VC.random_calls(rng, pl, 1)) for i in range(5)]
    line = VC.line_of(long_)
    ninth = [i for i, c in enumerate(line) if c == 9][8]
    assert ninth > 4 * 64 and ninth > 256 + 256
    path = str(tmp_path / "a.vcf.gz")
    VC.write_indexed(path, ["A", "B", "C"], recs)
    wants, _ = compare(ctx, path, [("chr1",) + ALL, ("chr1", 899, 900), ("chr1", 900, 901), ("chr1", 600, 601)])
    got = wants[0][1]
    assert got["ref_len"].tolist()[5] == 300 and got["allele_bytes"].size == 5 * 2 + 701 + 5 * 3 and len(wants[1][1]["pos"]) == 1 and len(wants[2][1]["pos"]) == 0


def test_contigs_are_compared_in_full(ctx, tmp_path):
    rng = np.random.default_rng(4)
    pl = [2, 2]
    recs = [VC.rec(c, 100 + 50 * i, VC.seq(rng, 1 + i % 3), [VC.seq(rng, 2)], VC.random_calls(rng, pl, 1)) for c in ("chr1", "chr10", "chr2") for i in range(40)]
    path = str(tmp_path / "a.vcf.gz")
    VC.write_indexed(path, ["A", "B"], recs)
    wants, _ = compare(ctx, path, [("chr1",) + ALL, ("chr10",) + ALL, ("chr2", 300, 900), ("chrX",) + ALL, ("chr", 0, 1 << 20), ("chr100", 0, 1 << 20)])
    assert [len(w[1]["pos"]) for w in wants] == [40, 40, 12, 0, 0, 0]
    a, b = wants[0][1], wants[1][1]
    assert not np.array_equal(a["allele_bytes"], b["allele_bytes"])            # chr1 did not take the records of chr10
    # an index that files the lines of chr10 under chr1: the device compares the names, not the index
    plain = VC.tbi_plain(["chr1", "chr1x", "chr2"], [(0 if i < 80 else 2, r["pos"], len(r["ref"])) for i, r in enumerate(recs)], VC.write_indexed(path, ["A", "B"], recs)["voffs"])
    open(path + ".tbi", "wb").write(VC.P.bgzf_blocks(plain, 0xff00)[0])
    wants, _ = compare(ctx, path, [("chr1",) + ALL])
    assert np.array_equal(wants[0][1]["allele_bytes"], a["allele_bytes"])


def test_the_edges_of_the_fetch_rule(ctx, tmp_path):
    from tests import panvcf_cases as PC
    s, e, ref, records, gt = PC.make_case(5, 600, 40, 5, 0.3, missing_rate=0.05, ref_start=1000)
    samples, ploidy = ["HG1", "HG2", "chm"], [2, 2, 1]
    lines = PC.vcf_text("chr7", records, samples, ploidy, gt).split(b"\n")
    recs = [VC.rec("chr7", p, a[0], a[1:], []) for p, a in records]
    body = [l for l in lines if l and not l.startswith(b"#")]
    path = str(tmp_path / "a.vcf.gz")
    VC.write_indexed(path, samples, recs, raw_lines=dict(enumerate(body)))
    long_ = max(range(len(records)), key=lambda i: len(records[i][1][0]))
    p, rl = records[long_][0], len(records[long_][1][0])
    assert rl > 1
    gap = next(i for i in range(len(records) - 1) if records[i + 1][0] > max(q + len(a[0]) for q, a in records[:i + 1]) + 1)
    lo = max(q + len(a[0]) for q, a in records[:gap + 1])
    regions = [(p + rl - 1, p + rl), (p + rl, p + rl + 50), (p, p + 1), (p - 3, p), (1100, 1300), (lo, records[gap + 1][0])]
    wants, _ = compare(ctx, path, [("chr7", a, b) for a, b in regions])
    for (a, b), w in zip(regions, wants):
        idx = R.fetch(records, a, b)
        assert w[1]["pos"].tolist() == [records[i][0] for i in idx] and np.array_equal(w[1]["gt"], gt[idx])
    assert len(wants[5][1]["pos"]) == 0 and wants[5][1]["rec_allele"].tolist() == [0] and wants[5][1]["allele_off"].tolist() == [0]


def test_several_chunks(ctx, tmp_path):
    pl, recs = VC.two_boundaries()
    path = str(tmp_path / "a.vcf.gz")
    info = VC.write_indexed(path, ["A", "B", "C"], recs)
    regions = [("chrA", 16384, 16584), ("chrA", 131072, 131272), ("chrA", 16380, 16385), ("chrA", 131000, 131080), ("chrA", 16000, 132000), ("chrA",) + ALL]
    for contig, a, b in regions[:2]:
        chunks = VC.plan(info["tbi"], contig, a, b)
        assert len(chunks) >= 2 and all(y[0] >> 16 > x[1] >> 16 for x, y in zip(chunks, chunks[1:]))      # disjoint: a BGZF block apart
    wants, stats = compare(ctx, path, regions)
    for (contig, a, b), w, st in zip(regions, wants, stats):
        assert st["n_chunks"] == len(VC.plan(info["tbi"], contig, a, b)) and st["records_kept"] == len(w[1]["pos"]) and st["lines_walked"] >= st["records_kept"]
        assert w[1]["pos"].tolist() == [r["pos"] for r in recs if r["pos"] < b and r["pos"] + len(r["ref"]) > a]          # file order
    assert stats[0]["n_chunks"] >= 2 and stats[1]["n_chunks"] >= 2
    assert len(wants[0][1]["pos"]) == 13 and len(wants[1][1]["pos"]) == 13             # the record across the boundary and the twelve behind it


@pytest.mark.parametrize("eol,last_eol", [(b"\r\n", True), (b"\n", False), (b"\r\n", False)])
def test_line_ends(ctx, tmp_path, eol, last_eol):
    pl, recs = VC.shaped_records(8, 3, n=30)
    path = str(tmp_path / "a.vcf.gz")
    VC.write_indexed(path, VC.names_of(3), recs, eol=eol, last_eol=last_eol)
    p = [r["pos"] for r in recs]
    wants, _ = compare(ctx, path, [("chr1",) + ALL, ("chr1", p[29], p[29] + 1), ("chr1", p[5], p[20])])
    assert len(wants[0][1]["pos"]) == 30 and len(wants[1][1]["pos"]) >= 1


@pytest.fixture(scope="module")
def three_contigs(tmp_path_factory):
    """A window in the middle of a 3-contig file of more than 200 blocks whose chunks are under a tenth of it (checked here, on the CPU)."""
    path = str(tmp_path_factory.mktemp("three") / "a.vcf.gz")
    recs, info, window = VC.three_contig_file(path)
    return path, recs, info, window


def test_bytes_read_follow_the_window(ctx, three_contigs):
    path, recs, info, window = three_contigs
    wants, stats = compare(ctx, path, [window])
    assert 5 <= len(wants[0][1]["pos"]) <= 30
    st = stats[0]
    assert 0 < st["bytes_inflated"] < len(info["text"]) / 5 and 0 < st["bytes_read"] < info["file_bytes"] / 5 and st["file_bytes"] == info["file_bytes"]


SAMPLES, PLOIDY = ["HG1", "HG2", "chm"], [2, 2, 1]


def _error_file(tmp_path, row, first_ploidy=None):
    """Twelve clean records; record 3 is an unphased call of HG1 (the first offending line), record 7 is `row` (a function of its clean
    line's columns). first_ploidy: the call of chm in the first record."""
    rng = np.random.default_rng(12)
    recs = [VC.rec("chr7", 1000 + 100 * i, b"AC", [b"A", b"ACC"], VC.random_calls(rng, PLOIDY, 2, missing=0.0)) for i in range(12)]
    raw = {}
    if first_ploidy is not None:
        raw[0] = b"\t".join(VC.line_of(recs[0]).split(b"\t")[:11] + [first_ploidy])
    f = VC.line_of(recs[3]).split(b"\t")
    raw[3] = b"\t".join(f[:9] + [b"1/0"] + f[10:])
    if row is not None:
        raw[7] = row(VC.line_of(recs[7]).split(b"\t"))
    path = str(tmp_path / "a.vcf.gz")
    VC.write_indexed(path, SAMPLES, recs, raw_lines=raw)
    return path


ROWS = {
    "ploidy 1": (lambda f: b"\t".join(f[:10] + [b"0"] + f[11:]), "in sample HG2 has ploidy 1 (expected 2)", cdefs.ERR_INVALID_DATA, [1, 0, 1]),
    "ploidy 3": (lambda f: b"\t".join(f[:10] + [b"0|1|1"] + f[11:]), "in sample HG2 has ploidy 3 (expected 2)", cdefs.ERR_INVALID_DATA, [1, 0, 1]),
    "unphased": (lambda f: b"\t".join(f[:10] + [b"0/1"] + f[11:]), "is unphased in sample HG2", cdefs.ERR_INVALID_DATA, [1, 0, 1]),
    "missing": (lambda f: b"\t".join(f[:10] + [b"."] + f[11:]), "in sample HG2 has ploidy 1 (expected 2)", cdefs.ERR_INVALID_DATA, [1, 0, 1]),
    "column missing": (lambda f: b"\t".join(f[:11]), "has 11 columns (expected 12)", cdefs.ERR_INVALID_DATA, None),
    "no GT": (lambda f: b"\t".join(f[:8] + [b"DP:GQ"] + f[9:]), "has no GT field", cdefs.ERR_INVALID_DATA, None),
    "0|x": (lambda f: b"\t".join(f[:10] + [b"0|x"] + f[11:]), "cannot parse the genotype '0|x'", cdefs.ERR_INVALID_DATA, None),
    "40000": (lambda f: b"\t".join(f[:10] + [b"0|40000"] + f[11:]), "allele index above 32767", cdefs.ERR_UNSUPPORTED, None),
}


@pytest.mark.parametrize("name", list(ROWS))
def test_errors_are_those_of_the_host_reader_first_in_file_order(ctx, tmp_path, name):
    row, text, status, mask = ROWS[name]
    path = _error_file(tmp_path, row)
    whole, second, clean = ("chr7",) + ALL, ("chr7", 1500, 3000), ("chr7", 1800, 3000)
    wants, _ = compare(ctx, path, [whole, second, clean])
    assert wants[0][0] == "error" and wants[0][1] == cdefs.ERR_INVALID_DATA and "chr7:1301 is unphased in sample HG1" in wants[0][2]      # the first of the two
    assert wants[1][0] == "error" and wants[1][1] == status and text in wants[1][2] and "chr7:1701" in wants[1][2]
    assert wants[2][0] == "ok" and len(wants[2][1]["pos"]) == 4                       # both offending lines are outside the window
    # the offending samples masked: HG1 alone leaves the second line's error, both give the arrays — unless the line itself is broken
    wants, _ = compare(ctx, path, [whole], used=[0, 1, 1])
    assert wants[0][0] == "error" and text in wants[0][2]
    if mask is not None:
        wants, _ = compare(ctx, path, [whole], used=[0, 0, 1])
        assert wants[0][0] == "ok" and len(wants[0][1]["pos"]) == 12
    else:
        wants, _ = compare(ctx, path, [whole], used=[0, 0, 0])
        assert wants[0][0] == "error" and wants[0][1] == status and text in wants[0][2]


def test_the_first_record_defines_the_ploidy(ctx, tmp_path):
    path = _error_file(tmp_path, None, first_ploidy=b"0|1")
    wants, _ = compare(ctx, path, [("chr7",) + ALL, ("chr7", 0, 1001)])
    assert wants[0][0] == "error" and "chr7:1101 in sample chm has ploidy 1 (expected 2)" in wants[0][2]
    assert wants[1][0] == "ok" and wants[1][1]["gt"].shape == (1, 6)
    wants, _ = compare(ctx, path, [("chr7",) + ALL], used=[0, 1, 0])
    assert wants[0][0] == "ok" and wants[0][1]["gt"].shape == (12, 6)                  # unused samples keep their entries, -1 where the call is short


def test_a_bad_position_in_the_chunks_is_the_open_error_of_the_host_reader(ctx, tmp_path):
    rng = np.random.default_rng(14)
    recs = [VC.rec("chr7", 1000 + 100 * i, b"A", [b"C"], VC.random_calls(rng, PLOIDY, 1, missing=0.0)) for i in range(12)]
    f = VC.line_of(recs[5]).split(b"\t")
    path = str(tmp_path / "a.vcf.gz")
    VC.write_indexed(path, SAMPLES, recs, raw_lines={5: b"\t".join(f[:1] + [b"15x1"] + f[2:])})
    with pytest.raises(LocityperError) as want:
        io.Vcf(path)
    w = io.VcfIndexed(path, ctx=ctx)
    for inflate in (0, 1):
        ctx.set_knob("sample_bam_inflate", inflate)
        got = outcome(w, "chr7", 0, 1 << 20)
        assert got == ("error", want.value.code, str(want.value)) and "bad position" in got[2]
    ctx.set_knob("sample_bam_inflate", -1)


def test_the_slice_limit_names_its_knob(ctx, three_contigs):
    path, recs, info, window = three_contigs
    w = io.VcfIndexed(path, ctx=ctx)
    ctx.set_knob("vcf_max_slice_bytes", 1024)
    try:
        with pytest.raises(LocityperError) as e:
            w.region(*window)
        assert e.value.code == cdefs.ERR_UNSUPPORTED and "vcf_max_slice_bytes" in str(e.value)
    finally:
        ctx.set_knob("vcf_max_slice_bytes", -1)
    assert len(w.region(*window)["pos"]) >= 5
