"""The failure contract of the locus-file stages (include/locityper_hip.h, next to the status codes): on any non-zero status the out struct
is all zero, every out pointer is NULL with its length 0, and the matching free takes it; and the one contract of a haplotype set
(seq_off[0] = 0, the offsets checked against the stage's limits before a base is read).

Every call goes to the library itself (_lib.lib(), the cdefs structs). The arguments come from a valid call of the api wrapper: while
the wrapper runs, its library call is held back (`spied`), the failing variants are sent first with the wrapper's own arrays and outs
pre-filled with 0xAA, then one valid call into fresh outs, whose arrays must equal what the wrapper returns from its own call afterwards.
Status-code failures only: three haplotypes of 50 bases that differ in two positions, names a, b, c."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import pafvcf_cases as PC

pytestmark = pytest.mark.gpu

INPUT, DATA, RUNTIME, UNSUPPORTED = cdefs.ERR_INVALID_INPUT, cdefs.ERR_INVALID_DATA, cdefs.ERR_RUNTIME, cdefs.ERR_UNSUPPORTED


def _sub(s, p):
    return s[:p] + bytes([b"ACGT"[(b"ACGT".index(s[p]) + 1) % 4]]) + s[p + 1:]


A = bytes(np.random.default_rng(7).choice(list(b"ACGT"), 50).astype(np.uint8))
B, CC = _sub(A, 10), _sub(A, 30)
NAMES = ["a", "b", "c"]
FLAT, OFF = PC.flat([A, B, CC])
SAME, _ = PC.flat([A, A, A])
REF = np.frombuffer(A, dtype=np.uint8).copy()
ENTRIES = PC.api_entries([(1, 0, [(b"=", 10), (b"X", 1), (b"=", 39)]), (2, 0, [(b"=", 30), (b"X", 1), (b"=", 19)])])
LYING = PC.api_entries([(1, 0, [(b"=", 50)]), (2, 0, [(b"=", 30), (b"X", 1), (b"=", 19)])])      # b differs from a at 10
# haplotype sets that must be refused from their offsets alone: a start at 1, a descent, a length at the stage's limit over 64 bytes
OFF1 = np.array([1, 50, 100, 150], dtype=np.uint64)
DESC = np.array([0, 50, 40, 150], dtype=np.uint64)
BUF64 = np.full(64, ord("A"), dtype=np.uint8)
LIMIT = {"db": 1 << 31, "align": 1 << 28, "pafvcf": 0x7FFFFFF0}
AT_LIMIT = {k: np.array([0, v, v + 1, v + 2], dtype=np.uint64) for k, v in LIMIT.items()}

FREE = {cdefs.DbFiles: "lcty_db_files_free", cdefs.AlignOut: "lcty_align_out_free", cdefs.AlignBackboneOut: "lcty_align_backbone_out_free",
        cdefs.AlignTrOut: "lcty_align_tr_out_free", cdefs.PruneOut: "lcty_prune_out_free", cdefs.PruneFiles: "lcty_prune_files_free",
        cdefs.VcfRecords: "lcty_vcf_records_free", cdefs.PanvcfOut: "lcty_panvcf_out_free", cdefs.LocusVcfOut: "lcty_locus_vcf_out_free",
        cdefs.PafvcfOut: "lcty_pafvcf_out_free", C.c_void_p: "lcty_io_free"}


def _release(L, obj):
    name = FREE.get(type(obj))
    if name is not None:                                                # a length has nothing to release
        getattr(L, name)(obj if isinstance(obj, C.c_void_p) else C.byref(obj))


def _is_zero(obj):
    return bytes(obj) == bytes(C.sizeof(obj))


def _must_fail(L, real, args, outs, want):
    objs = [args[i]._obj for i in outs]
    for o in objs:
        C.memset(C.addressof(o), 0xAA, C.sizeof(o))
    rc = real(*args)
    assert rc == want, (rc, want, L.lcty_last_error())
    assert all(_is_zero(o) for o in objs), "an out is not all zero after status %d" % rc
    for o in objs:
        _release(L, o)
    assert all(_is_zero(o) for o in objs)


@contextlib.contextmanager
def spied(name, outs, bad=(), read=None, fails_with=None):
    """outs: the positions of the byref'd outs. bad: (arguments -> arguments, status) variants that must fail. read(arguments, outs) ->
    dict of what a valid call left. fails_with: the wrapper's own inputs are the failing ones (a late failure) and give this status."""
    L = _lib.lib()
    real = getattr(L, name)
    seen = {}

    def spy(*args):
        for change, want in bad:
            _must_fail(L, real, change(list(args)), outs, want)
        if fails_with is not None:
            _must_fail(L, real, list(args), outs, fails_with)
            seen["failed"] = True
            return real(*args)                                          # once more for the wrapper, which raises
        fresh, objs = list(args), [type(args[i]._obj)() for i in outs]
        for i, o in zip(outs, objs):
            fresh[i] = C.byref(o)
        assert real(*fresh) == 0, L.lcty_last_error()
        try:
            seen["direct"] = read(fresh, objs) if read else {}
        finally:
            for o in objs:
                _release(L, o)
        return real(*args)

    setattr(L, name, spy)
    try:
        yield seen
    finally:
        setattr(L, name, real)
    assert "direct" in seen or "failed" in seen, name + " was not called"


def late(name, outs, status, call):
    with spied(name, outs, fails_with=status) as seen:
        with pytest.raises(_lib.LocityperError) as e:
            call()
    assert e.value.code == status and seen["failed"]


def put(i, v):
    return lambda a: a[:i] + [v] + a[i + 1:]


def haps(i_seqs, i_off, stage=None):
    """the variants of a haplotype set at these argument positions: (a start at 1, a descent) and, with a stage, a length at its limit"""
    def at_limit(a):
        a[i_seqs], a[i_off] = BUF64.ctypes.data, AT_LIMIT[stage].ctypes.data
        return a
    return [(put(i_off, OFF1.ctypes.data), INPUT), (put(i_off, DESC.ctypes.data), INPUT)] + ([(at_limit, UNSUPPORTED)] if stage else [])


def take(p, n, dt):
    return np.frombuffer(C.string_at(p, int(n) * np.dtype(dt).itemsize), dtype=dt).copy() if n else np.zeros(0, dtype=dt)


def text(p, n):
    return C.string_at(p, n) if p and n else b""


def u64_at(address, i):
    return C.c_uint64.from_address(address + 8 * i).value


def same(direct, got):
    assert direct, "nothing was read from the direct call"
    for k, v in direct.items():
        w = got[k]
        assert (v == w) if isinstance(v, (bytes, int)) else np.array_equal(v, np.asarray(w).reshape(-1)), k


# ---- the database files (lcty_db.hip) ----------------------------------------------------------------------------------------------------------
COUNTS = np.zeros(4 * 26, dtype=np.uint16)                              # k = 25: 26 k-mers per sequence, the reference's block last
CNT_OFF = np.arange(5, dtype=np.uint64) * 26


def test_db(gpu_ctx):
    with spied("lcty_db_minimizers", [7], haps(2, 3, "db") + [(put(1, 0), INPUT)], lambda a, o: {"hashes": take(o[0], u64_at(a[6], 3), np.uint64)}) as s:
        moff, hashes, _ = api.db_minimizers(gpu_ctx, FLAT, OFF)
    same(s["direct"], {"hashes": hashes})
    with spied("lcty_db_divergences", [], haps(2, 3, "db")):
        api.db_divergences(gpu_ctx, FLAT, OFF)
    with spied("lcty_db_off_target", [], haps(2, 3, "db")):
        api.db_off_target(gpu_ctx, FLAT, OFF, COUNTS[:78], CNT_OFF[:4], 25, 2, REF, COUNTS[:26])
    with spied("lcty_db_discard_identical", [], haps(1, 2, "db")):
        api.db_discard_identical(NAMES, FLAT, OFF)

    def files(a, o):
        f = o[0]
        return {"fasta": text(f.fasta, f.fasta_len), "kmers": text(f.kmers, f.kmers_len), "distances": text(f.distances, f.distances_len),
                "discarded": text(f.discarded, f.discarded_len), "kept": take(f.kept, f.n_kept, np.uint32)}
    build = lambda seqs: api.db_build_locus(gpu_ctx, NAMES, seqs, OFF, REF, COUNTS, CNT_OFF, 25, 2, api.db_params(calc_div=1))
    with spied("lcty_db_build_locus", [12], haps(3, 4, "db") + [(put(2, None), INPUT), (put(1, 1), DATA)], files) as s:
        got = build(FLAT)
    same(s["direct"], got)
    assert got["fasta"] == b">a\n" + A + b"\n>b\n" + B + b"\n>c\n" + CC + b"\n" and got["distances"] and got["kmers"]
    late("lcty_db_build_locus", [12], DATA, lambda: build(SAME))        # calc_div with one distinct haplotype left: after the FASTA text is made


# ---- the basis haplotypes (lcty_basis.hip) --------------------------------------------------------------------------------------------------------
def test_basis(gpu_ctx):
    entries = [(q, t, w, 49, 50) for q, t, w in ENTRIES]
    p = api.basis_params(divergence=0.1, window=10, step=5)
    no_such = np.array([3, 3], dtype=np.uint32)
    with spied("lcty_basis_windows", [13], [(put(5, no_such.ctypes.data), INPUT), (put(12, None), INPUT)],
               lambda a, o: {"rows": take(o[0], u64_at(a[12], 3), np.uint32)}) as s:
        win_off, rows, _ = api.basis_windows(gpu_ctx, [50, 50, 50], entries, p)
    same(s["direct"], {"rows": rows})
    assert len(rows)
    with spied("lcty_basis_constraints", [5, 6], [(put(1, 0), INPUT), (put(3, None), INPUT)],
               lambda a, o: {"n": int(o[0].value), "rows": take(o[1], o[0].value, np.uint32)}) as s:
        out, _ = api.basis_constraints(gpu_ctx, 3, rows, minimal=True)
    same(s["direct"], {"n": len(out), "rows": out})


# ---- the pairwise alignments (lcty_align.hip, lcty_align_transitive.hip) -------------------------------------------------------------------------
def _align_out(o):
    n = int(o.n_pairs)
    d = {k: take(getattr(o, k), n, dt) for k, dt in (("aligned", np.uint8), ("n_matches", np.uint32), ("aln_len", np.uint32), ("nerrs", np.uint32),
                                                    ("score", np.int32), ("best_k", np.uint32), ("um", np.uint32), ("md", np.float64))}
    d["cigar_off"] = take(o.cigar_off, n + 1, np.uint64)
    d["cigar"] = take(o.cigar, d["cigar_off"][-1], np.uint32)
    return d


def test_align(gpu_ctx):
    r, q = [0, 0, 1], [1, 2, 2]
    p = api.align_params(backbone_ks=[11])
    never = api.align_params(backbone_ks=[11], thresh_div=0.0, skip_div=1)     # every pair passes and no k is left: "No alignment found"
    third = np.array([3, 0, 1], dtype=np.uint32)                               # pair 0 names sequence 3 of 3
    with spied("lcty_align_haplotypes", [9], haps(2, 3, "align") + [(put(5, third.ctypes.data), INPUT), (put(1, 1), INPUT)],
               lambda a, o: _align_out(o[0])) as s:
        got, _ = api.align_haplotypes(gpu_ctx, FLAT, OFF, r, q, p)
    same(s["direct"], got)
    assert got["aligned"].tolist() == [1, 1, 1] and got["nerrs"].tolist() == [1, 1, 2]
    late("lcty_align_haplotypes", [9], RUNTIME, lambda: api.align_haplotypes(gpu_ctx, FLAT, OFF, r, q, never))

    def backbone(a, o):
        o = o[0]
        return {"matches": take(o.matches, 2 * o.n_matches, np.uint32), "path": take(o.path, o.path_len, np.uint32), "cigar": take(o.cigar, o.n_cigar, np.uint32),
                "score": int(o.score), "chain_score": int(o.chain_score)}
    with spied("lcty_align_backbone", [8], haps(2, 3, "align") + [(put(4, 3), INPUT), (put(6, 4), INPUT)], backbone) as s:
        got, _ = api.align_backbone(gpu_ctx, FLAT, OFF, 0, 1, 11, p)
    same(s["direct"], got)

    def both(a, o):
        return dict(_align_out(o[0]), route=take(o[1].route, o[0].n_pairs, np.uint8), via=take(o[1].via, o[0].n_pairs, np.uint32))
    nan_div = api.align_tr_params(transitive_div=float("nan"))
    with spied("lcty_align_haplotypes_transitive", [10, 11], haps(2, 3, "align") + [(put(5, third.ctypes.data), INPUT), (put(9, C.byref(nan_div)), INPUT)], both) as s:
        got, _ = api.align_haplotypes_transitive(gpu_ctx, FLAT, OFF, r, q, p)
    same(s["direct"], got)
    assert got["route"].tolist() == [1, 1, 1]
    late("lcty_align_haplotypes_transitive", [10, 11], RUNTIME, lambda: api.align_haplotypes_transitive(gpu_ctx, FLAT, OFF, r, q, never))


# ---- prune (lcty_prune.hip) ---------------------------------------------------------------------------------------------------------------------
def _paf(dv):
    return "".join("%s\t50\t0\t50\t+\t%s\t50\t0\t50\t49\t50\t255\tdv:f:%s\n" % (q, t, d) for (q, t), d in zip((("b", "a"), ("c", "a"), ("c", "b")), dv)).encode()


def _files(a, o):
    f = o[0]
    return {"newick": text(f.newick, f.newick_len), "discarded": text(f.discarded, f.discarded_len), "fasta": text(f.fasta, f.fasta_len),
            "paf": text(f.paf, f.paf_len), "keep": take(f.keep, f.n_keep, np.uint32)}


def test_prune(gpu_ctx):
    tri = np.array([0.00001, 0.01, 0.01])                               # a and b fall into one cluster
    nan = np.array([0.00001, np.nan, 0.01])
    with spied("lcty_prune_cluster", [5], [(put(2, nan.ctypes.data), INPUT), (put(1, 0), INPUT)],
               lambda a, o: {"keep_ids": take(o[0].keep_ids, o[0].n_clusters, np.uint32), "repr": take(o[0].repr, o[0].n_clusters, np.uint32),
                             "members": take(o[0].members, o[0].n, np.uint32)}) as s:
        got = api.prune_cluster(gpu_ctx, 3, tri)
    same(s["direct"], dict(got, members=np.concatenate(got["clusters"])))
    assert len(got["keep_ids"]) == 2
    with spied("lcty_prune_texts", [5, 6, 7, 8], [(put(1, None), INPUT), (put(0, 0), INPUT)],
               lambda a, o: {"newick": text(o[0], o[1].value), "discarded": text(o[2], o[3].value)}) as s:
        got = api.prune_cluster(gpu_ctx, 3, tri, names=NAMES)
    same(s["direct"], got)
    assert got["newick"] and got["discarded"]
    paf = _paf(("0.00001", "0.01", "0.01"))
    with spied("lcty_prune_thin", [12], haps(2, 3) + [(put(1, None), INPUT), (put(11, 0), INPUT)], _files) as s:
        got = api.prune_thin(NAMES, FLAT, OFF, paf, [0, 2])
    same(s["direct"], got)
    assert got["fasta"] == b">a\n" + A + b"\n>c\n" + CC + b"\n" and got["paf"].count(b"\n") == 1
    with spied("lcty_db_prune_locus", [15], haps(3, 4) + [(put(2, None), INPUT), (put(1, 0), DATA)], _files) as s:
        got = api.db_prune_locus(gpu_ctx, NAMES, FLAT, OFF, paf)
    same(s["direct"], got)
    assert len(got["keep"]) == 2 and got["newick"]
    # a NaN divergence counts as missing (load_divergences); with every pair missing the call ends
    late("lcty_db_prune_locus", [15], INPUT, lambda: api.db_prune_locus(gpu_ctx, NAMES, FLAT, OFF, _paf(("NaN", "NaN", "NaN"))))
    # after the clustering on the device, with the tree, the kept ids and the discarded text made: a k-mer file that ends in its header
    late("lcty_db_prune_locus", [15], DATA, lambda: api.db_prune_locus(gpu_ctx, NAMES, FLAT, OFF, paf, kmers=b"\x01"))


# ---- a locus from a pangenome VCF (lcty_panvcf.hip, the reader in lcty_io.hip) -------------------------------------------------------------------
def _vcf(tmp_path, name, samples, lines):
    path = tmp_path / name
    path.write_text("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=1000>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(samples) + "\n" +
                    "".join("chr1\t%d\t.\t%s\t%s\t.\t.\t.\tGT\t%s\n" % (pos, ref, alt, "\t".join(gts)) for pos, ref, alt, gts in lines))
    return path


def test_panvcf(gpu_ctx, tmp_path):
    ch = lambda s, p: chr(s[p])
    # the window is chr1:101-150 = a; b and c carry one substitution each
    good = io.Vcf(_vcf(tmp_path, "good.vcf", ["b", "c"], [(111, ch(A, 10), ch(B, 10), ("1", "0")), (131, ch(A, 30), ch(CC, 30), ("0", "1"))]))
    # b carries a deletion of 111-113 and a substitution at 112
    ovl = io.Vcf(_vcf(tmp_path, "ovl.vcf", ["b", "c"], [(111, A[10:13].decode(), ch(A, 10), ("1", "0")), (112, ch(A, 11), ch(_sub(A, 11), 11), ("1", "0"))]))
    unphased = io.Vcf(_vcf(tmp_path, "unphased.vcf", ["b"], [(111, ch(A, 10), ch(B, 10), ("0|1",)), (131, ch(A, 30), ch(CC, 30), ("0/1",))]))

    def records(a, o):
        r = o[0]
        return {"pos": take(r.pos, r.n_recs, np.uint32), "ref_len": take(r.ref_len, r.n_recs, np.uint32), "rec_allele": take(r.rec_allele, r.n_recs + 1, np.uint32),
                "allele_off": take(r.allele_off, r.n_alleles + 1, np.uint64), "allele_bytes": take(r.allele_bytes, r.pool_len, np.uint8),
                "gt": take(r.gt, r.n_recs * r.n_haps, np.int16), "phased": take(r.phased, r.n_recs * r.n_samples, np.uint8)}
    with spied("lcty_vcf_region", [5], [(put(1, None), INPUT), (put(0, None), INPUT)], records) as s:
        recs = good.region("chr1", 100, 150)
    same(s["direct"], recs)
    assert recs["pos"].tolist() == [110, 130]
    late("lcty_vcf_region", [5], DATA, lambda: unphased.region("chr1", 100, 150))      # the second record, with the first one gathered
    names, cs, chs, _ = api.panvcf_names(good.samples, good.ploidy, "a")
    assert names == NAMES
    gt = api.panvcf_columns(recs["gt"], good.hap_off, cs, chs)
    bad_recs = ovl.region("chr1", 100, 150)
    bad_gt = api.panvcf_columns(bad_recs["gt"], ovl.hap_off, cs, chs)

    def rebuilt(a, o):
        o = o[0]
        off = take(o.seq_off, o.n_seqs + 1, np.uint64)
        return {"seq_off": off, "seqs": take(o.seqs, off[-1], np.uint8), "kept_cols": take(o.kept_cols, o.n_seqs, np.uint32),
                "col_unknown": take(o.col_unknown, o.n_cols, np.uint32), "col_len": take(o.col_len, o.n_cols, np.uint32),
                "col_reason": take(o.col_reason, o.n_cols, np.uint8)}
    with spied("lcty_panvcf_reconstruct", [16], [(put(13, None), INPUT), (put(3, 100), INPUT), (put(0, None), INPUT)], rebuilt) as s:
        got = api.panvcf_reconstruct(gpu_ctx, "chr1", 100, 150, REF, recs, gt, names)
    same(s["direct"], got)
    assert got["seqs"].tobytes() == A + B + CC and got["names"] == NAMES
    late("lcty_panvcf_reconstruct", [16], DATA, lambda: api.panvcf_reconstruct(gpu_ctx, "chr1", 100, 150, REF, bad_recs, bad_gt, names))   # overlaps forbidden

    def without_names(a):
        i = cdefs.LocusVcfIn.from_buffer_copy(a[1]._obj)
        i.names = None
        held.append(i)
        a[1] = C.byref(i)
        return a
    held = []

    def locus(a, o):
        o = o[0]
        return {"fasta": text(o.files.fasta, o.files.fasta_len), "kept": take(o.files.kept, o.files.n_kept, np.uint32), "ref_bed": text(o.ref_bed, o.ref_bed_len),
                "hap_cols": take(o.hap_cols, o.n_hap_cols, np.uint32)}
    from_vcf = lambda rc, g: api.db_locus_from_vcf(gpu_ctx, "L1", "chr1", 100, 150, 1000, 100, REF, rc, g, names, expansions=(0,))
    with spied("lcty_db_locus_from_vcf", [3], [(without_names, INPUT), (put(2, None), INPUT)], locus) as s:
        got = from_vcf(recs, gt)
    same(s["direct"], got)
    assert got["ref_bed"] == b"chr1\t100\t150\tL1\n" and got["fasta"] == b">a\n" + A + b"\n>b\n" + B + b"\n>c\n" + CC + b"\n"
    late("lcty_db_locus_from_vcf", [3], DATA, lambda: from_vcf(bad_recs, bad_gt))       # inside the reconstruction, after the device work
    for v in (good, ovl, unphased):
        v.close()


# ---- a locus's haplotypes as a VCF (lcty_pafvcf.hip) ------------------------------------------------------------------------------------------------
def test_pafvcf(gpu_ctx):
    def variants(a, o):
        o = o[0]
        d = {k: take(getattr(o, k), o.n_variants, np.uint32) for k in ("ref_start", "ref_end", "hap_start", "hap_end")}
        return dict(d, var_off=take(o.var_off, o.n_seqs + 1, np.uint64), has_aln=take(o.has_aln, o.n_seqs, np.uint8))
    with spied("lcty_pafvcf_variants", [10], haps(2, 3, "pafvcf") + [(put(4, 3), INPUT), (put(8, None), INPUT)], variants) as s:
        v = api.pafvcf_variants(gpu_ctx, FLAT, OFF, 0, ENTRIES)
    same(s["direct"], v)
    assert len(v["ref_start"]) == 2 and v["has_aln"][1:].tolist() == [1, 1]
    late("lcty_pafvcf_variants", [10], DATA, lambda: api.pafvcf_variants(gpu_ctx, FLAT, OFF, 0, LYING))

    def ranges(a, o):
        o = o[0]
        return {"unique": np.stack([take(o.unique_start, o.n_unique, np.uint32), take(o.unique_end, o.n_unique, np.uint32)], axis=1).reshape(-1),
                "merged": np.stack([take(o.merged_start, o.n_merged, np.uint32), take(o.merged_end, o.n_merged, np.uint32)], axis=1).reshape(-1)}
    with spied("lcty_pafvcf_ranges", [4], [(put(2, None), INPUT), (put(1, 0x7FFFFFF0), UNSUPPORTED)], ranges) as s:
        unique, merged = api.pafvcf_ranges(gpu_ctx, v["ref_start"], v["ref_end"])
    same(s["direct"], {"unique": unique, "merged": merged})
    assert len(merged) == 2

    def table(a, o):
        o = o[0]
        off = take(o.allele_off, o.n_ranges + 1, np.uint64)
        return {"allele_ix": take(o.allele_ix, o.n_ranges * o.n_seqs, np.int32), "n_alleles": take(o.n_alleles, o.n_ranges, np.uint32), "allele_off": off,
                "allele_hap": take(o.allele_hap, off[-1], np.uint32), "allele_start": take(o.allele_start, off[-1], np.uint32),
                "allele_len": take(o.allele_len, off[-1], np.uint32)}
    with spied("lcty_pafvcf_table", [14], haps(2, 3, "pafvcf") + [(put(5, None), INPUT), (put(4, 3), INPUT)], table) as s:
        t = api.pafvcf_table(gpu_ctx, FLAT, OFF, 0, v, merged)
    same(s["direct"], t)
    assert t["allele_ix"].shape == (2, 3) and t["n_alleles"].tolist() == [2, 2]
    groups, ref_id, _ = api.pafvcf_samples(NAMES, "a")
    assert ref_id == 0
    with spied("lcty_pafvcf_text", [19], haps(2, 3, "pafvcf") + [(put(17, None), INPUT), (put(8, None), INPUT)], lambda a, o: {"text": text(o[0].merged, o[0].merged_len)}) as s:
        body = api.pafvcf_text(gpu_ctx, FLAT, OFF, 0, merged, t, groups, b"chr9", 100)
    same(s["direct"], {"text": body})
    assert body.count(b"\n") == 2 and body.startswith(b"chr9\t")
    with spied("lcty_paf_to_vcf", [17], haps(3, 4, "pafvcf") + [(put(2, None), INPUT), (put(7, b"z"), INPUT)],
               lambda a, o: {"merged": text(o[0].merged, o[0].merged_len), "separate": text(o[0].separate, o[0].separate_len)}) as s:
        m, sep, _ = api.paf_to_vcf(gpu_ctx, NAMES, FLAT, OFF, ENTRIES, "a")
    same(s["direct"], {"merged": m, "separate": sep})
    assert m.startswith(b"##fileformat") and m.count(b"\n") == 3 + 2
    late("lcty_paf_to_vcf", [17], DATA, lambda: api.paf_to_vcf(gpu_ctx, NAMES, FLAT, OFF, LYING, "a"))
