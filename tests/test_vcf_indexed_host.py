"""The indexed VCF reader, the host side (lcty_vcf_indexed_open / _view_get / _plan, the tabix parser, the shared chunk rule): against
io.Vcf on the same file and the Python restatement of tests/vcf_index_cases.py. No device is needed."""
import os
import shutil
import subprocess

import pytest

from locityper_amd import api, cdefs, io
from locityper_amd._lib import LocityperError
from tests import pyref_sample_bam as P
from tests import sample_bam_cases as S
from tests import vcf_index_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _file(tmp_path, n_samples=3, name="a.vcf.gz", **kw):
    pl, recs = VC.shaped_records(11, n_samples)
    recs += VC.shaped_records(12, n_samples, contig="chr10")[1] + VC.shaped_records(13, n_samples, contig="chr2", start=16000, step=90)[1]
    path = str(tmp_path / name)
    return path, pl, recs, VC.write_indexed(path, VC.names_of(n_samples), recs, **kw)


def test_open_gives_the_view_of_the_whole_file_reader(tmp_path):
    for n_samples in (0, 1, 3, 65):
        path, pl, recs, _ = _file(tmp_path, n_samples, name=f"s{n_samples}.vcf.gz")
        v, w = io.Vcf(path), io.VcfIndexed(path)
        assert w.samples == v.samples == VC.names_of(n_samples) and w.ploidy.tolist() == v.ploidy.tolist() == pl
        assert w.hap_off.tolist() == v.hap_off.tolist() and w.n_haps == v.n_haps and w.n_records == 0          # the file is not walked
        w.close(); v.close()
    # a header longer than the first read: thousands of ##contig lines over many BGZF blocks, CRLF line ends, an explicit index path
    header = VC.HEADER + [f"##contig=<ID=scaffold_{i},length={1000 + i}>".encode() for i in range(5000)]
    path, pl, recs, info = _file(tmp_path, 3, name="long.vcf.gz", header=header, eol=b"\r\n", block=0xff00)
    assert len(info["text"]) > 3 * 0xff00
    shutil.move(path + ".tbi", str(tmp_path / "elsewhere.tbi"))
    v, w = io.Vcf(path), io.VcfIndexed(path, str(tmp_path / "elsewhere.tbi"))
    assert w.samples == v.samples and w.ploidy.tolist() == v.ploidy.tolist() == pl and w.hap_off.tolist() == v.hap_off.tolist()
    # a file whose only record has no newline behind it
    one = str(tmp_path / "one.vcf.gz")
    VC.write_indexed(one, ["A", "B"], [VC.rec("c", 4, b"A", [b"C"], ["0|1", "1"])], last_eol=False)
    assert io.VcfIndexed(one).ploidy.tolist() == [2, 1]


def test_open_raises_the_errors_of_the_whole_file_reader(tmp_path):
    head = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA"
    line = b"c\t5\t.\tA\tC\t.\t.\t.\tGT\t0|1"
    for k, lines in enumerate(([b"##fileformat=VCFv4.2", line], [b"##fileformat=VCFv4.2"], [head], [line, head], [head, b"c\t5\t.\tA\tC\t.\t.\t.\tGT"],
                               [head, b"c\tx\t.\tA\tC\t.\t.\t.\tGT\t0"], [head, b"c\t5\t.\tA\tC\t.\t.\t.\tDP\t0"], [head, b"c\t5\t.\tA\tC\t.\t.\t.\tGT\t0|x"])):
        path = str(tmp_path / f"e{k}.vcf.gz")
        data, voffs, _ = VC.bgzf_lines(lines, 700)
        open(path, "wb").write(data)
        open(path + ".tbi", "wb").write(VC.tbi_bytes(["c"], [(0, 4, 1)], [voffs[-2], voffs[-1]]))
        with pytest.raises(LocityperError) as want:
            io.Vcf(path)
        with pytest.raises(LocityperError) as got:
            io.VcfIndexed(path)
        assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)), lines


def test_plan_follows_the_chunk_rule(tmp_path):
    path, pl, recs, info = _file(tmp_path, 3, block=700)
    w = io.VcfIndexed(path)
    text_blocks = info["n_blocks"]
    assert text_blocks > 20
    regions = [("chr1", 0, 1 << 29), ("chr1", 1000, 1001), ("chr1", 1500, 1900), ("chr10", 1200, 1300), ("chr2", 16000, 16400), ("chr2", 16384, 16385),
               ("chr2", 0, 100), ("chr2", 20000, 1 << 31), ("chr2", 17000, 17000), ("chr2", 17000, 16500), ("chr1", 5, 0), ("chrX", 0, 1 << 29)]
    some = 0
    for contig, start, end in regions:
        chunks, n_blocks = w.plan(contig, start, end)
        want = VC.plan(info["tbi"], contig, start, end)
        assert chunks.tolist() == want, (contig, start, end)
        assert (n_blocks >= len(want)) and (n_blocks > 0) == (len(want) > 0)
        some += len(want)
    assert some >= 8
    # the designed files of tests/test_gpu_vcf_indexed.py: two disjoint chunks across 16 384 and 131 072; a window of a 3-contig file
    pl2, recs2 = VC.two_boundaries()
    p2 = str(tmp_path / "two.vcf.gz")
    info2 = VC.write_indexed(p2, ["A", "B", "C"], recs2)
    w2 = io.VcfIndexed(p2)
    for contig, start, end in (("chrA", 16384, 16584), ("chrA", 131072, 131272), ("chrA", 16380, 16385), ("chrA", 131000, 131080), ("chrA", 0, 0xFFFFFFFF)):
        chunks, _ = w2.plan(contig, start, end)
        assert chunks.tolist() == VC.plan(info2["tbi"], contig, start, end) and (len(chunks) >= 2 or start not in (16384, 131072))
    p3 = str(tmp_path / "three.vcf.gz")
    recs3, info3, window = VC.three_contig_file(p3)
    chunks, n_blocks = io.VcfIndexed(p3).plan(*window)
    assert chunks.tolist() == VC.plan(info3["tbi"], *window) and 0 < n_blocks < info3["n_blocks"] / 10
    # the chunks of a region hold every line the whole-file reader returns for it: their lines are inside the chunks' offsets
    v = io.Vcf(path)
    for contig, start, end in regions:
        got = v.region(contig, start, end)["pos"]
        chunks = VC.plan(info["tbi"], contig, start, end)
        for i, r in enumerate(recs):
            if r["contig"] == contig and r["pos"] < end and r["pos"] + len(r["ref"]) > start:
                assert any(c[0] <= info["voffs"][i] and info["voffs"][i + 1] <= c[1] for c in chunks), (contig, start, end, i)
        assert len(got) == sum(r["contig"] == contig and r["pos"] < end and r["pos"] + len(r["ref"]) > start for r in recs)


def test_sample_bam_plan_is_what_it_was(tmp_path):
    """lcty_sample_bam_plan goes through the same definition now: its chunks are those of the rule on the tables of the .bai."""
    recs = S.seeded_records(seed=1500, n_pairs=400, n_tail=10)
    path = str(tmp_path / "b.bam")
    voffs = P.write_bam(path, S.SEEDED_REFS, recs, block_size=1500)
    _, refs = VC.index_tables(open(path + ".bai", "rb").read(), bai=True)
    bam = io.SampleBam(path)
    n = 0
    for regions in [[r] for r in S.SEEDED_REGIONS] + [S.SEEDED_REGIONS, [(0, 16_383, 16_385)]]:
        cs = [c for tid, start, end in regions for c in VC.plan_ref(*refs[tid], start, end)]
        want = VC.plan_ref({0: cs}, [], 0, 1)                        # the chunks of all regions, sorted and merged together
        chunks, _ = bam.plan(regions)
        assert chunks.tolist() == want, regions
        n += len(want)
    assert n >= 8
    n_placed = sum(r["tid"] >= 0 for r in recs)
    chunks, _ = bam.plan([], True)
    assert chunks.tolist() == [[voffs[n_placed], os.path.getsize(path) << 16]]


def test_every_index_of_the_corpus_returns_its_status(tmp_path):
    path, pl, recs, info = _file(tmp_path, 1)
    cases = VC.index_cases()
    assert len(cases) > 300 and {st for _, st in cases} == {VC.OK, VC.ERR_INVALID_DATA, VC.ERR_UNSUPPORTED}
    ip = str(tmp_path / "case.tbi")
    for k, (plain, status) in enumerate(cases):
        open(ip, "wb").write(P.bgzf_blocks(plain, 0xff00)[0])
        if status == VC.OK:
            io.VcfIndexed(path, ip).close()
            continue
        with pytest.raises(LocityperError) as e:
            io.VcfIndexed(path, ip)
        assert e.value.code == status, k
        assert "case.tbi" in str(e.value), k                          # the index file is named


def test_csi_bcf_missing_index_and_plain_files(tmp_path):
    path, pl, recs, info = _file(tmp_path, 2)
    tbi = open(path + ".tbi", "rb").read()
    for p, ip, status, word in ((str(tmp_path / "x.bcf"), None, cdefs.ERR_UNSUPPORTED, "BCF"), (path, str(tmp_path / "a.vcf.gz.csi"), cdefs.ERR_UNSUPPORTED, "CSI"),
                                (path, str(tmp_path / "nowhere.tbi"), cdefs.ERR_INVALID_INPUT, "no index")):
        with pytest.raises(LocityperError) as e:
            io.VcfIndexed(p, ip)
        assert e.value.code == status and word in str(e.value)
    os.remove(path + ".tbi")
    with pytest.raises(LocityperError) as e:
        io.VcfIndexed(path)
    assert e.value.code == cdefs.ERR_INVALID_INPUT and "no index" in str(e.value)
    open(path + ".csi", "wb").write(tbi)
    with pytest.raises(LocityperError) as e:
        io.VcfIndexed(path)
    assert e.value.code == cdefs.ERR_UNSUPPORTED and "CSI" in str(e.value)
    # an index that is not compressed, and files that are not BGZF: plain text, plain gzip
    open(str(tmp_path / "raw.tbi"), "wb").write(info["tbi"])
    with pytest.raises(LocityperError) as e:
        io.VcfIndexed(path, str(tmp_path / "raw.tbi"))
    assert e.value.code == cdefs.ERR_INVALID_DATA and "raw.tbi" in str(e.value)
    import gzip
    for name, data in (("p.vcf", info["text"]), ("g.vcf.gz", gzip.compress(info["text"]))):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        open(p + ".tbi", "wb").write(tbi)
        io.Vcf(p).close()                                             # the whole-file reader takes both
        with pytest.raises(LocityperError) as e:
            io.VcfIndexed(p)
        assert e.value.code == cdefs.ERR_INVALID_INPUT and "must be BGZF" in str(e.value)


def test_fetch_fails_loudly_without_a_device(tmp_path):
    path, pl, recs, info = _file(tmp_path, 2)
    w = io.VcfIndexed(path)
    if api.device_count() == 0:
        with pytest.raises(LocityperError) as e:
            w.region("chr1", 0, 1 << 29)
        assert e.value.code == cdefs.ERR_RUNTIME and "no CPU fallback" in str(e.value)
    else:
        with pytest.raises(LocityperError) as e:                     # no context: a null argument, not a host parse
            w.region("chr1", 0, 1 << 29)
        assert e.value.code == cdefs.ERR_INVALID_INPUT


def test_the_host_passes_are_clean_under_the_sanitizers(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    exe, corpus = str(tmp_path / "vcf_index_probe_host"), str(tmp_path / "corpus.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "locityper_amd", "csrc"), os.path.join(ROOT, "scripts", "vcf_index_probe_host.cpp"), "-o", exe], check=True)
    n = VC.write_corpus(corpus)
    assert n > 300
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"{n} cases, ") and r.stdout.rstrip().endswith(" 0 wrong"), r.stdout
