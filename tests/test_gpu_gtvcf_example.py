"""examples/genotypes_to_vcf.cpp from compiled code: a database directory, a BGZF variants file with its index and
res.json.gz files written by the library in; per-locus and merged .vcf.gz + .tbi out. The files must inflate to the bytes the Python API
gives for the same inputs, their indices must fetch the right records, and --fields upstream must give the three-field form."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from locityper_amd import api, cdefs, io
from tests import vcf_index_cases as VC
from tests.test_gpu_example import build_example

GENOME = "GRCh"
VCF_SAMPLES, PLOIDY = ["HG1", "HG2", "NA3"], [2, 2, 1]
ALLELES = ["HG1.1", "HG1.2", "HG2_1", "HG2_2", "NA3", GENOME]
# contig indices 1 and 2 of the variants file: chrZ is declared first and has no locus
HEADER = [b"##fileformat=VCFv4.2", b"##contig=<ID=chrZ,length=999>", b"##contig=<ID=chrA,length=50000,assembly=x>", b"##contig=<ID=chrB>",
          b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">']
LOCI = {"L1": ("chrA", 90, 400), "L2": ("chrA", 300, 700), "L3": ("chrB", 0, 100), "Lnone": ("chrA", 10, 20)}
# sample -> locus -> (genotype as allele indices or None for a file without a genotype, quality, weight_dist, warnings); no entry: no file
COHORT = {"s2": {"L1": ((0, 3), 27.39, 0.001234567, cdefs.WARN_FEW_READS), "L2": ((4, 5), 31.0, 2.5, 0), "L3": ((1, 1), 5.55, float("nan"), 0)},
          "s10": {"L1": (None, 0.0, float("nan"), 0), "L2": ((2, 0), 12.0, 0.5, 0), "L3": ((5, 5), 99.99, 0.25, cdefs.WARN_NO_PROBABLE_GENOTYPE)},
          "S1": {"L1": ((3, 2), 8.0, 1.0, 0), "L3": ((4, 4), 1.0, 0.0, 0)}}


def variants(path):
    rng = np.random.default_rng(5)
    recs = []
    for contig, n, step in (("chrA", 40, 17), ("chrB", 6, 13)):
        for i in range(n):
            n_alt = 1 + i % 3
            recs.append(VC.rec(contig, 95 + i * step if contig == "chrA" else 3 + i * step, VC.seq(rng, 1 + i % 4), [VC.seq(rng, 1 + (i + a) % 5) for a in range(n_alt)],
                               VC.random_calls(rng, PLOIDY, n_alt), vid="."))
    VC.write_indexed(path, VCF_SAMPLES, recs, header=HEADER)
    return recs


def write_inputs(root):
    os.makedirs(root / "DB" / "loci")
    for name, (chrom, start, end) in LOCI.items():
        os.makedirs(root / "DB" / "loci" / name)
        (root / "DB" / "loci" / name / "ref.bed").write_text(f"{chrom}\t{start}\t{end}\t{name}\n")
    lines = ["# path sample"]
    for sample, by_locus in COHORT.items():
        for locus in ("L1", "L2", "L3"):
            os.makedirs(root / "out" / sample / "loci" / locus)     # a directory without a file is the `?` row
            if locus not in by_locus:
                continue
            gt, quality, wd, warn = by_locus[locus]
            call = cdefs.Call()
            call.quality, call.unexpl_reads, call.n_good, call.warnings = quality, 17, 9000, warn
            if gt is not None:
                call.n_out = 1
                call.ixs[0] = 0; call.ln_probs[0] = math.log(0.9)
            text = io.res_to_json(call, np.array([gt or (0, 0)], dtype=np.uint16)[:int(call.n_out)].reshape(int(call.n_out), 2), ALLELES, [-10.0][:int(call.n_out)],
                                  [1.0][:int(call.n_out)], weighted_dist=wd)
            io.write_gz(root / "out" / sample / "loci" / locus / "res.json.gz", text.encode())
        lines.append(f"{root / 'out' / sample} {sample}")
    (root / "list.txt").write_text("\n".join(lines) + "\n")


def api_files(ctx, table, vcf_path, mask, loci):
    """the same cohort through the Python API: {locus: text}, the merged text and the records of every locus"""
    samples = table["samples"]
    last = {(r["locus"], r["sample"]): r for r in table["rows"]}
    v = io.VcfIndexed(vcf_path, ctx=ctx)
    contigs = v.contigs()
    assert contigs == [("chrZ", 999), ("chrA", 50000), ("chrB", 0)]
    tid = {name: i for i, (name, _) in enumerate(contigs)}
    out, fetched = {}, {}
    gv = api.GenotypeVcf(ctx, samples, mask)
    for name in sorted(loci):
        chrom, start, end = LOCI[name]
        if not any(r["locus"] == name.encode() for r in table["rows"]):
            continue
        recs = v.region(chrom, start, end)
        preds, feats, warns = [], {k: [] for k in ("qual10", "reads", "unexpl", "wdist5")}, []
        for s in samples:
            r = last.get((name.encode(), s))
            called = r is not None and r["genotype"] not in (b"*", b"?")
            preds.append(list(api.gtvcf_columns(VCF_SAMPLES, PLOIDY, GENOME, r["genotype"].decode().split(","))) if called else [])
            for k in feats:
                feats[k].append(r[k] if called else None)
            warns.append(r["warnings"] if called else b"")
        got = gv.add_locus(chrom, contigs[tid[chrom]][1], recs, recs["gt"], preds, feats=feats, warns=warns, locus=name, contig_ix=tid[chrom], start=start, end=end)
        out[name], fetched[name] = got["text"], recs
    merged = gv.merge()
    gv.close(); v.close()
    return out, merged, fetched


def run(cmd):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_genotypes_to_vcf_example_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "genotypes_to_vcf"), "genotypes_to_vcf.cpp")


@pytest.mark.gpu
def test_cohort_from_res_json_files_to_indexed_vcf_files(gpu_ctx, tmp_path):
    exe = tmp_path / "genotypes_to_vcf"
    build_example(str(exe), "genotypes_to_vcf.cpp")
    write_inputs(tmp_path)
    vcf_path = tmp_path / "variants.vcf.gz"
    variants(vcf_path)
    # 1. -I: the res.json.gz files, the table written on the way, all five fields, the device's deflate
    out1 = tmp_path / "vcf1"
    js = run([exe, "-I", tmp_path / "list.txt", "-d", tmp_path / "DB", "-v", vcf_path, "-g", GENOME, "-o", out1, "--csv", tmp_path / "pred.csv"])
    table = api.predictions_csv_read(tmp_path / "pred.csv")
    assert table["samples"] == [b"S1", b"s10", b"s2"] and len(table["rows"]) == 9
    cells = {(r["sample"], r["locus"]): r for r in table["rows"]}
    assert cells[(b"S1", b"L2")]["genotype"] == b"?" and cells[(b"s10", b"L1")]["genotype"] == b"*"
    assert cells[(b"s2", b"L1")] == dict(sample=b"s2", locus=b"L1", genotype=b"HG1.1,HG2_2", warnings=b"FewReads(9000)", qual10=273, reads=9000, unexpl=17, wdist5=123)
    texts, merged, fetched = api_files(gpu_ctx, table, vcf_path, cdefs.GTVCF_ALL, ["L1", "L2", "L3", "Lnone"])
    assert sorted(texts) == ["L1", "L2", "L3"] and all(len(fetched[k]["pos"]) for k in texts)
    assert (js["samples"], js["loci"], js["loci_without_predictions"], js["merged_records"], js["joined"]) == (3, 3, 1, len(merged["line_pos"]), merged["n_joined"])
    assert js["joined"] > 0 and js["records"] == sum(len(f["pos"]) for f in fetched.values())
    for name, text in list(texts.items()) + [("merged", merged["text"])]:
        assert io.read_file(out1 / (name + ".vcf.gz")) == text, name
        assert text.split(b"\n")[-2].split(b"\t")[8] == b"GT:qual:reads:unexpl:wdist:warn"
    assert b"##contig=<ID=chrA,length=50000>\n##contig=<ID=chrB>\n" in merged["text"] and b"chrZ" not in merged["text"]
    # the written indices fetch the records of every locus's interval, from the locus's file and from the merged one. The reader wants one
    # ploidy per used sample, and a sample without a prediction in one locus is `.` there: s2, called in every locus, is the sample read.
    used = [0, 0, 1]
    for name in texts:
        chrom, start, end = LOCI[name]
        for path in (out1 / (name + ".vcf.gz"), out1 / "merged.vcf.gz"):
            v = io.VcfIndexed(path, ctx=gpu_ctx)
            back = v.region(chrom, start, end, sample_used=used)
            v.close()
            assert back["pos"].tolist() == fetched[name]["pos"].tolist() and back["allele_bytes"].tobytes() == fetched[name]["allele_bytes"].tobytes()
            if path.name != "merged.vcf.gz":                             # s2's calls in the locus's own file: the GT of its two predicted columns
                cols = api.gtvcf_columns(VCF_SAMPLES, PLOIDY, GENOME, cells[(b"s2", name.encode())]["genotype"].decode().split(","))
                want = np.stack([np.zeros(len(back["pos"]), np.int16) if c == cdefs.GTVCF_REF else fetched[name]["gt"][:, c] for c in cols], axis=1)
                assert np.array_equal(back["gt"][:, -2:], np.where(want < 0, -1, want))
    # a sample's call is the GT of its predicted haplotypes: s2 in L1 is HG1.1 | HG2_2, columns 0 and 3 of the variants file
    line = texts["L1"].split(b"\n")[-2].split(b"\t")
    gt = fetched["L1"]["gt"][-1]
    assert line[9 + 2].split(b":")[0] == b"|".join(b"." if x < 0 else b"%d" % x for x in (gt[0], gt[3]))
    assert line[9 + 2].split(b":")[1:] == [b"27.3", b"9000", b"17", b"0.00123", b"FewReads(9000)"] and line[9 + 1] == b"."
    # 2. -i: the table, upstream's three fields, a subset of the loci, the host's deflate
    out2 = tmp_path / "vcf2"
    js2 = run([exe, "-i", tmp_path / "pred.csv", "-d", tmp_path / "DB", "-v", vcf_path, "-x", str(vcf_path) + ".tbi", "-g", GENOME, "-o", out2, "--fields", "upstream",
               "--deflate", "host", "--subset-loci", "L3", "L1"])
    texts2, merged2, _ = api_files(gpu_ctx, table, vcf_path, cdefs.GTVCF_UPSTREAM, ["L1", "L3"])
    assert (js2["loci"], js2["joined"], js2["fields"]) == (2, 0, "upstream") and not os.path.exists(out2 / "L2.vcf.gz")
    for name, text in list(texts2.items()) + [("merged", merged2["text"])]:
        assert io.read_file(out2 / (name + ".vcf.gz")) == text, name
        fields = text.split(b"\n")[-2].split(b"\t")
        assert fields[8] == b"GT:reads:unexpl:wdist" and all(f == b"." or f.count(b":") == 3 for f in fields[9:])
    v = io.VcfIndexed(out2 / "merged.vcf.gz", ctx=gpu_ctx)
    assert v.region("chrB", 0, 100, sample_used=used)["pos"].tolist() == fetched["L3"]["pos"].tolist()
    v.close()
