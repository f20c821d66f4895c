"""Designed aln.bam files for the two readers of a locus's alignments (lcty_bam_read on the host, lcty_bam_read_device): record lists, the
files written from them, and — independently of both readers, from the record list and not from the bytes — the table AllAlignments::load
(src/model/locs.rs:405-461, 502-567, 1116-1150) makes of them, or the error it ends in. The shapes are the smallest at which the device
stage can go wrong: names, sequences and CIGARs of every length class, groups around a wavefront (64) and a workgroup (256), BGZF blocks
of 700 bytes so that every field straddles a block border, and every error at the first, a middle and the last record.

A design: name, refs (the header's (name, length)), alleles (the locus's names), data (the inflated bytes), block (BGZF block size),
recs (the record dicts of pyref_sample_bam.rec, None when the bytes are damaged by hand), err ({paired: (status, text with {path})} or
None). expected(design, paired) -> the table as a dict of arrays, or raises Refused."""
import struct

import numpy as np

from tests import pyref_sample_bam as SB

ERR_INVALID_DATA = 2
CODES = SB.CODES
UNMAPPED, REVERSE, MATE2, SECONDARY, SUPPL = 0x4, 0x10, 0x80, 0x100, 0x800
KEPT_FLAGS = UNMAPPED | REVERSE | MATE2 | SECONDARY | SUPPL

T_TRUNC = "{path}: truncated BAM"
T_NOT_BAM = "{path}: not a BAM file"
T_CORRUPT = "{path}: corrupt BAM record"
T_FIRST = "First record in the BAM file is secondary/supplementary"
T_NO_REF = "{path}: mapped record without a reference"


def t_second(name):
    return f"Read {name} does not have a second read end"


class Refused(Exception):
    def __init__(self, status, text):
        super().__init__(text)
        self.status, self.text = status, text


def _seq(n, seed, codes=CODES):
    x = (np.arange(n, dtype=np.int64) * 7 + seed * 13 + (np.arange(n, dtype=np.int64) // 5)) % len(codes)
    return "".join(codes[int(i)] for i in x)


def _cigar(n, seed=0):
    ops = "MIDNSHP=X"
    return [(ops[(k + seed) % 9], 1 + (k * 5 + seed) % 11) for k in range(n)]


def mk(name, flag=0, tid=0, pos=10, ncig=1, lseq=20, qual=True, mapq=60, seed=0, codes=CODES):
    q = bytes((seed + 3 * k) % 94 for k in range(lseq)) if qual else None
    return SB.rec(tid, pos, name, flag, _cigar(ncig, seed), _seq(lseq, seed, codes), q, mapq=mapq)


def group(name, flag, n_more, seed=0, lseq=20, ncig=1, tid=0, qual=True):
    """a primary and n_more non-primary records behind it (secondary and supplementary in turn, without SEQ)"""
    out = [mk(name, flag, tid=tid, pos=5 + seed, ncig=ncig, lseq=lseq, qual=qual, seed=seed, mapq=(seed * 7) % 61)]
    for k in range(n_more):
        out.append(mk(name, flag | (SECONDARY if k % 2 == 0 else SUPPL) | (REVERSE if k % 3 == 0 else 0), tid=(tid + k + 1) % 3, pos=100 + k,
                      ncig=(k % 4), lseq=0, seed=seed + k, mapq=k % 50))
    return out


def pair(name, n1=0, n2=0, seed=0, **kw):
    return group(name, 0, n1, seed, **kw) + group(name, MATE2, n2, seed + 1, **kw)


REFS3 = [("a0", 5000), ("a1", 6000), ("a2", 7000)]
ALLELES3 = ["a0", "a1", "a2"]


def design(name, recs, refs=REFS3, alleles=ALLELES3, block=0xff00, err=None, blobs=None, head=None, cut=None):
    blobs = [SB.record_bytes(r) for r in recs] if blobs is None else blobs
    data = (SB.header_bytes(refs) if head is None else head) + b"".join(blobs)
    if cut is not None:
        data = data[:len(data) - cut]
    return dict(name=name, refs=refs, alleles=alleles, data=data, block=block, recs=recs, err=err,
                head_len=len(SB.header_bytes(refs) if head is None else head), blob_lens=[len(b) for b in blobs])


def file_bytes(d, block=None):
    return SB.bgzf_blocks(d["data"], block or d["block"])[0]


def write(d, path, block=None):
    with open(path, "wb") as f:
        f.write(file_bytes(d, block))
    return path


# ---- the table from the record list --------------------------------------------------------------------------------------------------

def expected(d, paired):
    """The table of a design whose records are well-formed bytes: from the record dicts alone. Raises Refused for the semantic errors."""
    if d["err"] is not None and d["recs"] is None:
        st, text = d["err"][int(bool(paired))]
        raise Refused(st, text)
    recs, refs, alleles = d["recs"], d["refs"], d["alleles"]
    tid2contig = []
    for nm, _ in refs:
        if nm not in alleles:
            raise Refused(ERR_INVALID_DATA, f"Intermediate BAM file contains unexpected contigs (e.g. {nm})")
        tid2contig.append(alleles.index(nm))
    pairs = []                       # [name, [mate records...], [records]]
    expect_second, cur = False, None
    for i, r in enumerate(recs):
        primary = (r["flag"] & 0x900) == 0
        if i == 0 and not primary:
            raise Refused(ERR_INVALID_DATA, T_FIRST)
        if primary:
            if expect_second and paired:
                if r["name"] != cur["name"]:
                    raise Refused(ERR_INVALID_DATA, t_second(cur["name"]))
                cur["mates"].append(r); cur["n_recs_mate"].append(0)
                expect_second = False
            else:
                cur = dict(name=r["name"], mates=[r], recs=[], n_recs_mate=[0])
                pairs.append(cur)
                expect_second = bool(paired)
        if not (r["flag"] & UNMAPPED) and not (0 <= r["tid"] < len(refs)):
            raise Refused(ERR_INVALID_DATA, T_NO_REF)
        cur["recs"].append(r)
        cur["n_recs_mate"][-1] += 1
    if pairs and expect_second and paired:
        raise Refused(ERR_INVALID_DATA, t_second(cur["name"]))
    mate_len, mate_off, aln_off, cigar_off, name_off, qual_off = [], [0], [0], [0], [0], [0]
    rows, cigar, mapq, names, quals, n_recs_mate = [], [], [], b"", b"", []
    bases = []                       # (offset, sequence) per mate that is there
    at = 0
    for p in pairs:
        for m in range(2):
            if m < len(p["mates"]):
                s = p["mates"][m]["seq"]
                mate_len.append(len(s)); bases.append((at, s))
                q = p["mates"][m]["qual"]
                quals += b"\xff" * len(s) if q is None else bytes(q)
                at = (at + len(s) + 31) // 32 * 32
                n_recs_mate.append(p["n_recs_mate"][m])
            else:
                mate_len.append(0); n_recs_mate.append(0)
            mate_off.append(at); qual_off.append(len(quals))
        rel = 0
        for r in p["recs"]:
            unm = bool(r["flag"] & UNMAPPED)
            contig = 0 if unm or r["tid"] < 0 else tid2contig[r["tid"]]
            n = len(r["cigar"]) & 0xFFFF
            rows.append((max(r["pos"], 0), contig, r["flag"] & KEPT_FLAGS, n, rel))
            rel += n
            cigar += [(ln << 4) | SB.OPS.index(op) for op, ln in r["cigar"][:n]]
            mapq.append(r["mapq"])
        aln_off.append(len(rows)); cigar_off.append(len(cigar))
        names += p["name"].encode(); name_off.append(len(names))
    n_units = at // 32
    bases2 = np.zeros(max(2 * n_units, 2), dtype=np.uint32); nmask = np.zeros(max(n_units, 1), dtype=np.uint32)
    for off, s in bases:
        for k, c in enumerate(s):
            i = off + k
            if c in "ACGT":
                bases2[i >> 4] |= np.uint32("ACGT".index(c) << (2 * (i & 15)))
            else:
                nmask[i >> 5] |= np.uint32(1 << (i & 31))
    rec_dt = np.dtype([("pos", "<u4"), ("contig", "<u2"), ("flags", "<u2"), ("n_cigar", "<u4"), ("cigar_rel", "<u4")])
    return dict(n_pairs=len(pairs), n_refs=len(refs), mate_len=np.array(mate_len, dtype=np.uint32), mate_off=np.array(mate_off, dtype=np.uint64),
                aln_off=np.array(aln_off, dtype=np.uint64), cigar_off=np.array(cigar_off, dtype=np.uint64),
                recs=np.array(rows, dtype=rec_dt), cigar=np.array(cigar, dtype=np.uint32), names=[p["name"] for p in pairs],
                bases2=bases2, nmask=nmask, qual_off=np.array(qual_off, dtype=np.uint64), quals=np.frombuffer(quals, dtype=np.uint8),
                mapq=np.array(mapq, dtype=np.uint8), n_recs_mate=np.array(n_recs_mate, dtype=np.uint32))


# ---- designs -------------------------------------------------------------------------------------------------------------------------

NAME_LENS = (1, 2, 3, 4, 5, 254)
SEQ_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 255, 2017)
CIGAR_LENS = (0, 1, 63, 64, 65, 300)
GROUP_SIZES = (254, 0, 0, 0, 0, 1, 63, 64, 65, 255, 256, 257, 300, 0, 0, 0)     # non-primary records behind primary j: primaries at records 0, 255, 256, 257, 258, 259, ...


def _name(n, k):
    return ("q%d_" % k + "x" * n)[:n] if n > 3 else "abcd"[k % 2:][:n]


def shapes():
    """names, sequences, CIGARs, flags, references: every length class, in both ends of pairs"""
    recs = []
    k = 0
    for nl in NAME_LENS:
        recs += pair(_name(nl, k), 0, 0, seed=k, lseq=SEQ_LENS[k % len(SEQ_LENS)], ncig=CIGAR_LENS[k % len(CIGAR_LENS)]); k += 1
    recs += pair("pre", 1, 0, seed=k); k += 1                 # a name that is a prefix of its neighbour's
    recs += pair("prefix", 0, 2, seed=k); k += 1
    for i, ls in enumerate(SEQ_LENS):                         # odd and even, each length in the first and in the second end
        a = mk(f"s{i}", REVERSE if i % 2 else 0, tid=i % 3, lseq=ls, qual=i % 3 != 0, ncig=CIGAR_LENS[i % len(CIGAR_LENS)], seed=k)
        b = mk(f"s{i}", MATE2 | (0 if i % 2 else REVERSE), tid=(i + 1) % 3, lseq=SEQ_LENS[-1 - i], qual=i % 3 != 1, ncig=CIGAR_LENS[(i + 3) % len(CIGAR_LENS)], seed=k + 1)
        recs += [a, b]; k += 2
    for c in range(0, 16, 4):                                 # all 16 base codes, also in runs of one code
        recs += [mk(f"c{c}", 0, lseq=40, seed=k, codes=CODES[c:c + 4]), mk(f"c{c}", MATE2, lseq=33, seed=k, codes=CODES[c] * 2)]; k += 1
    # unmapped primaries: tid = -1 / pos = -1, and a tid beyond n_ref; a supplementary record behind an unmapped primary
    recs += [mk("u0", UNMAPPED, tid=-1, pos=-1, ncig=0, lseq=50, seed=k), mk("u0", UNMAPPED | MATE2, tid=7, pos=3, ncig=0, lseq=51, seed=k + 1),
             mk("u0", MATE2 | SUPPL, tid=2, pos=77, ncig=2, lseq=0, seed=k + 2)]
    recs += [mk("u1", UNMAPPED | REVERSE, tid=-1, pos=-1, ncig=0, lseq=0, seed=k), mk("u1", MATE2, tid=1, pos=0, ncig=1, lseq=1, seed=k)]
    return recs


def groups():
    recs = []
    for j, g in enumerate(GROUP_SIZES):
        recs += group(f"g{j // 2}", MATE2 if j % 2 else 0, g, seed=j, lseq=30 + j, ncig=1 + j % 3, tid=j % 3)
    return recs


def n_pairs_design(n):
    recs = []
    for p in range(n):
        recs += pair(f"p{p}", p % 2, (p + 1) % 3 % 2, seed=p, lseq=10 + p % 40, ncig=1 + p % 2)
    return recs


def _patch(blob, at, fmt, v):
    return blob[:at] + struct.pack(fmt, v) + blob[at + struct.calcsize(fmt):]


# offsets in a record's bytes (its block_size word included)
AT_BLOCK, AT_TID, AT_LNAME, AT_NCIGAR, AT_FLAG, AT_LSEQ = 0, 4, 12, 16, 18, 20


def good():
    big = [f"allele_{a:03d}_" + "n" * 60 for a in range(40)]
    sub = [(big[a], 1000 + a) for a in [(t * 7 + 3) % 40 for t in range(36)]]
    out = [design("shapes", shapes()), design("shapes_700", shapes(), block=700),
           design("groups", groups()), design("groups_700", groups(), block=700),
           design("cigar_65535", pair("big", 1, 0, seed=3, ncig=65535, lseq=64) + pair("small", 0, 1, seed=5)),
           design("empty", []),
           # the header spans several blocks of 700 bytes and lists a subset of the alleles in another order
           design("header_spans", [mk("h", 0, tid=t, lseq=35 + t, seed=t) for t in (0, 5)] + [mk("h2", 0, tid=2), mk("h2", MATE2 | SECONDARY, tid=3, lseq=0),
                                                                                             mk("h2", MATE2, tid=1)],
                  refs=sub, alleles=big, block=700)]
    for n in (1, 2, 63, 64, 65):
        out.append(design(f"pairs_{n}", n_pairs_design(n), block=700 if n % 2 else 0xff00))
    return out


def bad():
    out = []
    base = n_pairs_design(40)                                 # 40 pairs; records of 1 or 2 per end
    blobs = [SB.record_bytes(r) for r in base]
    n = len(base)
    prim = [i for i, r in enumerate(base) if not r["flag"] & 0x900]
    where = {"first": 0, "middle": n // 2, "last": n - 1}
    for w, i in where.items():
        # ---- damaged fields of one record
        for what, at, fmt, vals in (("block_size", AT_BLOCK, "<I", (0xFFFFFFFF, 0x7FFFFFFF, None, 31, 0)),
                                    ("l_read_name", AT_LNAME, "<B", (255, None)), ("n_cigar", AT_NCIGAR, "<H", (0xFFFF, None)),
                                    ("l_seq", AT_LSEQ, "<I", (0xFFFFFFFF, 0x7FFFFFFF, None))):
            for v in vals:
                b = blobs[i]
                block = len(b) - 4
                if what == "block_size":
                    val = v if v is not None else (sum(len(x) for x in blobs[i:]) - 4 + 1)           # one past the end of the file
                    text = T_CORRUPT if val < 32 else T_TRUNC
                else:
                    r = base[i]
                    fixed = 32 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (len(r["seq"]) + 1) // 2 + len(r["seq"])
                    assert fixed == block                     # records without tags: fixed fields == block is the border of rec_fits
                    if v is None:                             # one past the block
                        val = {"l_read_name": len(r["name"]) + 2, "n_cigar": len(r["cigar"]) + 1, "l_seq": len(r["seq"]) + 1}[what]
                    else:
                        val = v
                    text = T_CORRUPT
                bl = list(blobs); bl[i] = _patch(b, at, fmt, val)
                out.append(design(f"{what}_{val:x}_{w}", None, blobs=bl, err={0: (ERR_INVALID_DATA, text), 1: (ERR_INVALID_DATA, text)}, block=700 if i % 2 else 0xff00))
        # ---- the file ends inside this record, and inside its block_size word
        for cut_to in (2, 4 + 10, len(blobs[i]) - 1):
            out.append(design(f"cut_{cut_to}_{w}", None, blobs=blobs[:i + 1], cut=len(blobs[i]) - cut_to,
                              err={0: (ERR_INVALID_DATA, T_TRUNC), 1: (ERR_INVALID_DATA, T_TRUNC)}))
        # ---- a mapped record without a reference: tid -1, tid = n_ref
        for tid in (-1, 3):
            rs = [dict(r) for r in base]; rs[i]["tid"] = tid
            out.append(design(f"no_ref_{tid}_{w}", rs))
    # ---- a second primary of another name: in the first, a middle and the last pair; the file ends behind a first end
    for w, j in (("first", 1), ("middle", len(prim) // 2 | 1), ("last", len(prim) - 1)):
        rs = [dict(r) for r in base]
        for i in range(prim[j], prim[j + 1] if j + 1 < len(prim) else n):
            rs[i]["name"] = rs[i]["name"] + "x"               # its name has the first end's as a prefix
        out.append(design(f"other_name_{w}", rs))
    out.append(design("ends_after_first_end", base[:prim[-1]]))
    out.append(design("one_first_end", base[:prim[1]]))
    rs = [dict(r) for r in base]; rs[0]["flag"] |= SECONDARY
    out.append(design("first_is_secondary", rs))
    rs = [dict(r) for r in base]; rs[0]["flag"] |= SUPPL; rs[0]["tid"] = -1
    out.append(design("first_is_supplementary_without_reference", rs))
    # ---- two errors in one file: the earlier one in file order decides
    long = n_pairs_design(120)
    lb = [SB.record_bytes(r) for r in long]
    lp = [i for i, r in enumerate(long) if not r["flag"] & 0x900]

    def two(name, first, second, text0, text1=None):
        """first / second: (record, kind); kind 'ref' | 'name' | 'corrupt' | 'trunc'"""
        rs = [dict(r) for r in long]; bl = None
        for i, kind in (first, second):
            if kind == "ref":
                rs[i]["tid"] = 9
            elif kind == "name":
                j = lp.index(i)
                assert j % 2 == 1
                for t in range(i, lp[j + 1] if j + 1 < len(lp) else len(long)):
                    rs[t]["name"] = "z" + rs[t]["name"]
        bl = [SB.record_bytes(r) for r in rs]
        for i, kind in (first, second):
            if kind == "corrupt":
                bl[i] = _patch(bl[i], AT_LSEQ, "<I", len(rs[i]["seq"]) + 2)
            elif kind == "trunc":
                bl[i] = _patch(bl[i], AT_BLOCK, "<I", 0x7FFFFFF0)
        e = {0: (ERR_INVALID_DATA, text0), 1: (ERR_INVALID_DATA, text1 or text0)}
        out.append(design(name, None, blobs=bl, err=e, block=700))
    odd = [i for j, i in enumerate(lp) if j % 2 == 1]
    two("ref_then_corrupt_lower_lane", (70, "ref"), (130, "corrupt"), T_NO_REF)                       # lane 6 before lane 2 of a later wavefront
    two("ref_then_corrupt", (5, "ref"), (9, "corrupt"), T_NO_REF)                                      # class 4 before class 1
    two("corrupt_then_ref", (5, "corrupt"), (9, "ref"), T_CORRUPT)
    i_name = next(i for i in odd if i > 20)
    nm = long[lp[lp.index(i_name) - 1]]["name"]
    two("name_then_truncated", (i_name, "name"), (i_name + 40, "trunc"), T_TRUNC, t_second(nm))
    two("name_then_corrupt", (i_name, "name"), (i_name + 3, "corrupt"), T_CORRUPT, t_second(nm))
    two("ref_then_name", (i_name - 2, "ref"), (i_name, "name"), T_NO_REF)
    two("name_and_ref_at_one_record", (i_name, "name"), (i_name, "ref"), T_NO_REF, t_second(nm))        # set_name comes before the reference check
    two("corrupt_then_name", (i_name - 3, "corrupt"), (i_name, "name"), T_CORRUPT)
    # ---- the header: the damaged variants of the host reader's test, another magic, contigs the locus does not have
    head = SB.header_bytes(REFS3)
    l_text = struct.unpack_from("<I", head, 4)[0]
    at_nref = 8 + l_text
    whole = head + blobs[0] + blobs[1]
    hv = []
    for v in (0xFFFFFFFF, 0xFFFFFFFC, 0x7FFFFFFF, len(whole)):
        hv.append((f"l_text_{v:x}", whole[:4] + struct.pack("<I", v) + whole[8:], T_TRUNC))
        hv.append((f"l_name_{v:x}", whole[:at_nref + 4] + struct.pack("<I", v) + whole[at_nref + 8:], T_TRUNC))
        hv.append((f"n_ref_{v:x}", whole[:at_nref] + struct.pack("<I", v) + whole[at_nref + 4:], None))
    hv.append(("cut_in_n_ref", whole[:at_nref + 2], T_TRUNC))
    hv.append(("cut_at_10", whole[:10], T_TRUNC))
    hv.append(("magic", b"BAM\2" + whole[4:], T_NOT_BAM))
    for nm_, data, text in hv:
        if text is None:
            v = struct.unpack_from("<I", data, at_nref)[0]
            text = "{path}: truncated BAM (%u references in %u bytes)" % (v, len(data) - at_nref - 4)
        out.append(dict(name="header_" + nm_, refs=REFS3, alleles=ALLELES3, data=data, block=0xff00, recs=None,
                        err={0: (ERR_INVALID_DATA, text), 1: (ERR_INVALID_DATA, text)}, head_len=0, blob_lens=[]))
    out.append(design("unexpected_contig", base, alleles=["a0", "a2"]))
    return out


def all_designs():
    return good() + bad()


# ---- comparison ----------------------------------------------------------------------------------------------------------------------

FIELDS = ("mate_len", "mate_off", "aln_off", "cigar_off", "cigar", "bases2", "nmask", "qual_off", "quals", "mapq")


def table_of(T):
    """an io.BamTable (host reader, or device reader with host_copy) as the dict expected() returns, without n_recs_mate"""
    ch = T.chunk
    qual_off, quals, mapq = T.quals()
    return dict(n_pairs=T.n_pairs, n_refs=T.n_refs, mate_len=ch.mate_len, mate_off=ch.mate_off, aln_off=ch.aln_off, cigar_off=ch.cigar_off,
                recs=ch.recs, cigar=ch.cigar, names=T.names, bases2=ch.bases2, nmask=ch.nmask, qual_off=qual_off, quals=quals, mapq=mapq)


def assert_same_table(got, want, what):
    assert got["n_pairs"] == want["n_pairs"] and got["n_refs"] == want["n_refs"], what
    assert got["names"] == want["names"], what
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f"{what}: {f}"
    assert got["recs"].tobytes() == np.ascontiguousarray(want["recs"]).tobytes(), f"{what}: recs"


# ---- the corpus of scripts/aln_bam_probe_host.cpp ------------------------------------------------------------------------------------

def parse_py(data, alleles):
    """(status, n_ref, records walked, how the walk stopped: 0 end / 1 truncated / 2 block < 32, the last record's offset), from the
    SAM specification's layout, for the host passes of the device reader"""
    n = len(data)
    if n < 12 or data[:4] != b"BAM\1":
        return ERR_INVALID_DATA, 0, 0, 0, 0
    l_text = struct.unpack_from("<I", data, 4)[0]
    if 8 + l_text + 4 > n:
        return ERR_INVALID_DATA, 0, 0, 0, 0
    i = 8 + l_text
    n_ref = struct.unpack_from("<I", data, i)[0]; i += 4
    if n_ref > (n - i) // 8:
        return ERR_INVALID_DATA, 0, 0, 0, 0
    for _ in range(n_ref):
        if i + 4 > n:
            return ERR_INVALID_DATA, 0, 0, 0, 0
        l_name = struct.unpack_from("<I", data, i)[0]; i += 4
        if i + l_name + 4 > n:
            return ERR_INVALID_DATA, 0, 0, 0, 0
        nm = data[i:i + max(l_name, 1) - 1]
        if nm not in [a.encode() for a in alleles]:
            return ERR_INVALID_DATA, 0, 0, 0, 0
        i += l_name + 4
    n_rec = stop = last = 0
    while i < n:
        if i + 4 > n:
            stop = 1; break
        block = struct.unpack_from("<I", data, i)[0]
        if i + 4 + block > n:
            stop = 1; break
        if block < 32:
            stop = 2; break
        last = i; n_rec += 1; i += 4 + block
    return 0, n_ref, n_rec, stop, last


def corpus_cases():
    """every design, every prefix of two small ones, and byte mutations of the header and of the first records"""
    out = [(d["data"], d["alleles"]) for d in all_designs()]
    small = next(d for d in good() if d["name"] == "pairs_2")
    for k in range(len(small["data"])):
        out.append((small["data"][:k], small["alleles"]))
    rng = np.random.default_rng(5)
    base = bytearray(next(d for d in good() if d["name"] == "pairs_63")["data"])
    for t in range(1500):
        b = bytearray(base)
        for _ in range(1 + t % 3):
            at = int(rng.integers(0, 400 if t % 2 else len(b)))
            b[at] = int(rng.integers(0, 256))
        out.append((bytes(b), ALLELES3))
    return out


def write_corpus(path):
    n = 0
    with open(path, "wb") as f:
        for data, alleles in corpus_cases():
            blob = b"".join(a.encode() + b"\0" for a in alleles)
            f.write(struct.pack("<8I", len(data), len(alleles), len(blob), *parse_py(data, alleles)) + blob + data)
            n += 1
    return n
