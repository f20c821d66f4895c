"""A locus's haplotypes as a VCF on the device (lcty_pafvcf.hip) against the serial restatement (tests/pyref_pafvcf.py): every comparison is
array or byte equality, for each part and for the whole step; and the round trip through lcty_panvcf_reconstruct, which needs no restatement."""
import functools

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import pafvcf_cases as PC
from tests import pyref_pafvcf as R

pytestmark = pytest.mark.gpu

MIX = [0, 1, 63, 64, 65, 2, 5, 9, 30, 12, 7, 100, 17]
# haplotypes x reference length x CIGAR items x rate of runs of adjacent edits: every class of haplotypes (1, 2, 63, 64, 65, 130) and of items
# (0, 1, 63, 64, 65, ~3 000), sparse (a few items on a long reference, isolated edits) and dense (an item every 3-7 bases, long runs)
SHAPES = [(1, 1000, (1,), 0.2), (2, 1000, (0, 63), 0.5), (63, 2000, (63, 64, 65, 1, 0), 0.05), (64, 3000, (64,), 0.5), (65, 5000, (65, 1), 0.05),
          (130, 20000, tuple(MIX), 0.3), (2, 20000, (3000,), 0.05), (5, 12000, (3000, 1, 2999), 0.6), (1, 12000, (3001,), 0.3), (64, 1000, (65, 200), 0.7)]


@functools.lru_cache(maxsize=None)
def case(n_haps, ref_len, items, run_rate, round_trip=False):
    """the inputs and everything the restatement says about them, computed once"""
    names, seqs, entries, ref_hap = PC.make_case(n_haps * 7919 + ref_len + len(items), n_haps, ref_len, list(items), run_rate=run_rate, indel_at_0_rate=0.3,
                                                 n_rate=0.03, missing_rate=0.05, ref_n=2, round_trip=round_trip)
    groups, ref_id, warn = R.group_haplotypes(names, ref_hap)
    stats = {}
    vars_ = R.process_paf(seqs, ref_id, entries, stats)
    unique, merged = R.combine_ranges(vars_)
    tables = {k: R.allele_table(r, vars_, seqs, ref_id) for k, r in (("unique", unique), ("merged", merged))}
    flat, off = PC.flat(seqs)
    return dict(names=names, seqs=seqs, entries=entries, api_entries=PC.api_entries(entries), ref_hap=ref_hap, groups=groups, ref_id=ref_id, stats=stats,
                vars=vars_, unique=unique, merged=merged, tables=tables, flat=flat, off=off)


def want_variant_arrays(c):
    off = np.zeros(len(c["seqs"]) + 1, dtype=np.uint64)
    np.cumsum([len(v or []) for v in c["vars"]], out=off[1:])
    rows = np.array([v for hv in c["vars"] for v in (hv or [])], dtype=np.uint32).reshape(-1, 4)
    return off, rows, np.array([v is not None for v in c["vars"]], dtype=np.uint8)


def check_table(c, got, ranges, want):
    ix, alleles = want
    assert got["allele_ix"].shape == (len(ranges), len(c["seqs"]))
    assert np.array_equal(got["allele_ix"], np.array(ix, dtype=np.int32).reshape(len(ranges), len(c["seqs"])))
    assert got["n_alleles"].tolist() == [len(a) for a in alleles]
    assert got["allele_off"].tolist() == np.concatenate([[0], np.cumsum([len(a) - 1 for a in alleles])]).astype(np.uint64).tolist()
    k = 0
    for r, al in enumerate(alleles):
        for a in al[1:]:
            h, s, n = int(got["allele_hap"][k]), int(got["allele_start"][k]), int(got["allele_len"][k])
            assert c["seqs"][h][s:s + n] == a and ix[r][h] == al.index(a) and all(x != al.index(a) for x in ix[r][:h])      # the first carrier
            k += 1


def check_all_parts(ctx, c):
    v = api.pafvcf_variants(ctx, c["flat"], c["off"], c["ref_id"], c["api_entries"])
    off, rows, has = want_variant_arrays(c)
    assert np.array_equal(v["var_off"], off) and np.array_equal(v["has_aln"], has)
    got_rows = np.stack([v["ref_start"], v["ref_end"], v["hap_start"], v["hap_end"]], axis=1)
    assert np.array_equal(got_rows, rows)
    assert (v["n_missing"], v["n_bad_len"], v["n_shifted"]) == (c["stats"]["n_missing"], c["stats"]["n_bad_len"], c["stats"]["n_shifted"])
    unique, merged = api.pafvcf_ranges(ctx, v["ref_start"], v["ref_end"])
    assert unique.tolist() == [list(r) for r in c["unique"]] and merged.tolist() == [list(r) for r in c["merged"]]
    for kind, ranges in (("merged", c["merged"]), ("unique", c["unique"])):
        t = api.pafvcf_table(ctx, c["flat"], c["off"], c["ref_id"], v, np.array(ranges, dtype=np.uint32).reshape(-1, 2))
        check_table(c, t, ranges, c["tables"][kind])
        text = api.pafvcf_text(ctx, c["flat"], c["off"], c["ref_id"], np.array(ranges, dtype=np.uint32).reshape(-1, 2), t, c["groups"], b"chr9", 123456)
        assert text == R.vcf_body(b"chr9", 123456, ranges, *c["tables"][kind], c["groups"])
    return v


def check_whole(ctx, c, **kw):
    m, s, stats = api.paf_to_vcf(ctx, c["names"], c["flat"], c["off"], c["api_entries"], c["ref_hap"], **kw)
    wm, ws, wstats = R.paf_to_vcf(c["names"], c["seqs"], c["entries"], c["ref_hap"], region=kw.get("region"))
    assert m == wm and s == ws
    for k in ("n_missing", "n_bad_len", "n_shifted", "warn_bits"):
        assert stats[k] == wstats[k], k
    assert (stats["n_unique"], stats["n_merged"], stats["n_samples"]) == (len(c["unique"]), len(c["merged"]), len(c["groups"]))
    assert stats["n_lines_merged"] == wm.count(b"\n") - 3 and stats["n_lines_separate"] == ws.count(b"\n") - 3
    return m, s


@pytest.mark.parametrize("n_haps,ref_len,items,run_rate", SHAPES)
def test_every_part_equals_the_restatement(gpu_ctx, n_haps, ref_len, items, run_rate):
    c = case(n_haps, ref_len, items, run_rate)
    v = check_all_parts(gpu_ctx, c)
    # what the inputs are meant to exercise: shifts, ranges that overlap, and — where the edits are dense — a shift that stopped at the
    # variant in front of it (the moved variant starts where that one ends)
    if max(items) >= 63:
        assert c["stats"]["n_shifted"] > 0
    if n_haps >= 63:
        assert len(c["unique"]) > len(c["merged"]) and c["stats"]["n_missing"] > 0 and c["stats"]["n_bad_len"] > 0
    if run_rate >= 0.5 and n_haps >= 5:
        assert any(a[1] == b[0] for hv in c["vars"] if hv for a, b in zip(hv, hv[1:]))
    assert len(v["ref_start"]) == sum(len(hv or []) for hv in c["vars"])


@pytest.mark.parametrize("n_haps,ref_len,items,run_rate", SHAPES)
def test_the_whole_step_equals_the_restatement(gpu_ctx, n_haps, ref_len, items, run_rate):
    c = case(n_haps, ref_len, items, run_rate)
    check_whole(gpu_ctx, c)
    if n_haps == 65:
        check_whole(gpu_ctx, c, region=(b"chr2", 5_000_000, 5_000_000 + ref_len))
        m, s, _ = api.paf_to_vcf(gpu_ctx, c["names"], c["flat"], c["off"], c["api_entries"], c["ref_hap"], with_separate=False)
        assert s is None and m == R.paf_to_vcf(c["names"], c["seqs"], c["entries"], c["ref_hap"])[0]
        with pytest.raises(_lib.LocityperError) as e:
            api.paf_to_vcf(gpu_ctx, c["names"], c["flat"], c["off"], c["api_entries"], c["ref_hap"], region=(b"chr2", 10, 10 + ref_len + 1))
        assert e.value.code == cdefs.ERR_INVALID_DATA


def test_the_pinned_example(gpu_ctx):
    from tests.test_pafvcf_host import EX_ENTRIES, EX_HEADER, EX_MERGED, EX_NAMES, EX_SEPARATE, EX_SEQS
    flat, off = PC.flat(EX_SEQS)
    m, s, stats = api.paf_to_vcf(gpu_ctx, EX_NAMES, flat, off, PC.api_entries(EX_ENTRIES), b"ref")
    assert m == EX_HEADER + EX_MERGED and s == EX_HEADER + EX_SEPARATE and stats["n_shifted"] == 1 and stats["n_variants"] == 5


def test_haplotypes_identical_to_the_reference_give_an_empty_body(gpu_ctx):
    c = case(7, 1000, (1,), 0.0, True)
    m, s = check_whole(gpu_ctx, c)
    assert m == s == R.vcf_header(c["groups"]) and not c["unique"]
    check_all_parts(gpu_ctx, c)
    # no entry at all: every haplotype is missing, no range, the header alone
    m, s, stats = api.paf_to_vcf(gpu_ctx, c["names"], c["flat"], c["off"], [], c["ref_hap"])
    assert m == s == R.vcf_header(c["groups"]) and stats["n_missing"] == 7


def test_an_allele_longer_than_a_workgroup_of_the_text_kernel(gpu_ctx):
    names, seqs, entries, ref_hap = PC.make_case(11, 3, 2000, [5, 9, 1], long_edit=5000, n_rate=0.0, missing_rate=0.0, dup_rate=0.0)
    flat, off = PC.flat(seqs)
    m, s, _ = api.paf_to_vcf(gpu_ctx, names, flat, off, PC.api_entries(entries), ref_hap)
    wm, ws, _ = R.paf_to_vcf(names, seqs, entries, ref_hap)
    assert m == wm and s == ws and max(len(f) for line in wm.split(b"\n") for f in line.split(b"\t")) >= 5000


@functools.lru_cache(maxsize=None)
def many_alleles_case():
    """120 haplotypes with an insertion behind the same base: 110 different ones (three-digit allele numbers), ten of them carried twice.
    The inserted bases end in no A and the base in front of them is an A, so none of them moves."""
    rng = np.random.default_rng(5)
    ref = bytearray(PC.random_seq(rng, 300))
    ref[99] = ord("A")
    ref = bytes(ref)
    names, seqs, entries = [b"ref"], [ref], []
    for i in range(120):
        k = i % 110
        ins = bytes(b"CGT"[(k // 3 ** d) % 3] for d in range(5))
        names.append(b"S%d.%d" % (i // 2, i % 2 + 1))
        seqs.append(ref[:100] + ins + ref[100:])
        entries.append((i + 1, 0, [(b"=", 100), (b"I", 5), (b"=", 200)]))
    return names, seqs, entries


def test_a_hundred_alleles_in_one_range_and_every_hash_colliding(gpu_ctx):
    names, seqs, entries = many_alleles_case()
    flat, off = PC.flat(seqs)
    wm, ws, _ = R.paf_to_vcf(names, seqs, entries, b"ref")
    line = wm.split(b"\n")[3]
    assert line.split(b"\t")[4].count(b",") == 109 and b"|110\t" in line and b"|10\t" in line       # >= 10 and >= 100 alleles: multi-digit GT
    m, s, _ = api.paf_to_vcf(gpu_ctx, names, flat, off, PC.api_entries(entries), b"ref")
    assert m == wm and s == ws
    c = case(64, 1000, (65, 200), 0.7)
    try:
        gpu_ctx.set_knob("pafvcf_hash_bits", 2)                         # four hash values: the bytes decide
        m2, s2, _ = api.paf_to_vcf(gpu_ctx, names, flat, off, PC.api_entries(entries), b"ref")
        assert m2 == wm and s2 == ws
        check_whole(gpu_ctx, c)
        gpu_ctx.set_knob("pafvcf_hash_bits", 0)                         # one hash value
        check_whole(gpu_ctx, c)
    finally:
        gpu_ctx.set_knob("pafvcf_hash_bits", -1)


def test_a_lying_equal_run_and_an_m_item_are_errors(gpu_ctx):
    c = case(5, 12000, (3000, 1, 2999), 0.6)
    h = next(q for q, t, cig in c["entries"] if t == 0 and len(cig) > 100)
    cig = next(cig for q, t, cig in c["entries"] if q == h and t == 0 and len(cig) > 100)
    k = max(i for i, (op, n) in enumerate(cig) if op == b"=" and n >= 2)       # the last long '=' run of the haplotype: behind the first 64 items
    qpos = sum(n for op, n in cig[:k] if op in (b"=", b"X", b"I")) + 1
    flat = c["flat"].copy()
    at = int(c["off"][h]) + qpos
    flat[at] = ord("A") if flat[at] != ord("A") else ord("C")
    with pytest.raises(_lib.LocityperError) as e:
        api.pafvcf_variants(gpu_ctx, flat, c["off"], c["ref_id"], c["api_entries"])
    assert e.value.code == cdefs.ERR_INVALID_DATA
    with pytest.raises(_lib.LocityperError) as e:
        api.paf_to_vcf(gpu_ctx, c["names"], flat, c["off"], c["api_entries"], c["ref_hap"])
    assert e.value.code == cdefs.ERR_INVALID_DATA
    # an M item in place of an X (the lengths stay right, else the entry is skipped before it is walked): in the first 64 items and behind them
    xs = [i for i, (op, n) in enumerate(cig) if op == b"X"]
    assert xs[0] < 64 < xs[-1]
    for where in (xs[0], xs[-1]):
        with_m = cig[:where] + [(b"M", cig[where][1])] + cig[where + 1:]
        entries = [(q, t, with_m if cg is cig else cg) for q, t, cg in c["entries"]]
        with pytest.raises(_lib.LocityperError) as e:
            api.pafvcf_variants(gpu_ctx, c["flat"], c["off"], c["ref_id"], PC.api_entries(entries))
        assert e.value.code == cdefs.ERR_RUNTIME
    entries = [(1, 0, [(b"=", 2), (b"M", 1), (b"=", 1)])]
    flat4, off4 = PC.flat([b"ACGT", b"ACGT"])
    with pytest.raises(_lib.LocityperError) as e:
        api.pafvcf_variants(gpu_ctx, flat4, off4, 0, PC.api_entries(entries))
    assert e.value.code == cdefs.ERR_RUNTIME
    # the quirk of the right-padded form is reproduced, and the slice it sends outside the haplotype is an error where the reference panics
    flatq, offq = PC.flat([b"GG", b"AAAAAG", b"GC"])
    v = api.pafvcf_variants(gpu_ctx, flatq, offq, 0, PC.api_entries([(1, 0, [(b"I", 5), (b"D", 1), (b"=", 1)]), (2, 0, [(b"=", 1), (b"X", 1)])]))
    assert [v[k].tolist() for k in ("ref_start", "ref_end", "hap_start", "hap_end")] == [[0, 1], [1, 2], [0, 1], [6, 2]]
    with pytest.raises(_lib.LocityperError) as e:
        api.pafvcf_table(gpu_ctx, flatq, offq, 0, v, [[0, 1], [1, 2]])
    assert e.value.code == cdefs.ERR_RUNTIME


@pytest.mark.parametrize("n_haps,ref_len,items,run_rate", [(1, 1000, (63,), 0.3), (2, 1000, (2, 65), 0.6), (64, 3000, (64, 9, 1), 0.5), (65, 5000, (65, 300), 0.2),
                                                           (130, 20000, tuple(MIX), 0.4), (5, 20000, (3000,), 0.5)])
def test_round_trip_through_the_vcf_reader_and_the_reconstruction(gpu_ctx, tmp_path, n_haps, ref_len, items, run_rate):
    """sequences -> true alignments -> VCF -> lcty_panvcf_reconstruct gives the sequences back: no restatement is trusted here"""
    names, seqs, entries, ref_hap = PC.make_case(n_haps * 31 + ref_len, n_haps, ref_len, list(items), run_rate=run_rate, indel_at_0_rate=0.5, round_trip=True)
    flat, off = PC.flat(seqs)
    merged, separate, stats = api.paf_to_vcf(gpu_ctx, names, flat, off, PC.api_entries(entries), ref_hap)
    assert stats["n_missing"] == 0 and stats["n_bad_len"] == 0 and stats["n_lines_merged"] > 0
    cells = b"".join(line.split(b"\t.\t.\tGT\t")[1] for line in merged.split(b"\n") if line and not line.startswith(b"#"))
    assert b"." not in cells
    path = tmp_path / "haplotypes.vcf.gz"
    io.write_bgzf(path, merged)
    info, recs = io.vcf_region(path, "ref", 0, ref_len)
    cols, cs, ch, left = api.panvcf_names(info["samples"], info["ploidy"], "ref", [])
    assert left == 0 and cols[0] == "ref" and sorted(cols[1:]) == sorted(n.decode() for n in names[1:])
    gt = api.panvcf_columns(recs["gt"], info["hap_off"], cs, ch)
    out = api.panvcf_reconstruct(gpu_ctx, "ref", 0, ref_len, np.frombuffer(seqs[0], dtype=np.uint8), recs, gt, cols, 0.0, False)
    assert out["total_overlaps"] == 0 and out["names"] == cols and not out["col_unknown"].any()
    by_name = {n.decode(): s for n, s in zip(names, seqs)}
    for i, n in enumerate(out["names"]):
        assert out["seqs"][int(out["seq_off"][i]):int(out["seq_off"][i + 1])].tobytes() == by_name[n], n
    # the separate file has cells that start or end inside a variant of their haplotype: dots are expected there, the identity is not
    assert separate.count(b"\n") >= merged.count(b"\n")
