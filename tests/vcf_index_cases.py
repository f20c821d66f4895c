"""Cases of the indexed VCF reader (lcty_vcf_indexed_*): a BGZF writer that cuts at a chosen block size and knows every line's virtual
offset, a tabix (.tbi) writer, a reader of .tbi / .bai tables and the chunk rule restated on them (plan), the designed files of
tests/test_gpu_vcf_indexed.py, and the corpus of scripts/vcf_index_probe_host.cpp (write_corpus). Not a test."""
import struct

import numpy as np

from tests import pyref_sample_bam as P

OK, ERR_INVALID_INPUT, ERR_INVALID_DATA, ERR_UNSUPPORTED = 0, 1, 2, 5
HEADER = [b"##fileformat=VCFv4.2", b'##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">']


# ---- BGZF with the offsets of the lines ------------------------------------------------------------------------------------------------

def bgzf_lines(lines, block_size, eol=b"\n", last_eol=True):
    """lines (bytes, without their ends) as one BGZF file cut every block_size bytes -> (file bytes, the virtual offset of every line
    and of the end of the text, the text)."""
    text, at = bytearray(), []
    for i, l in enumerate(lines):
        at.append(len(text))
        text += l
        if i + 1 < len(lines) or last_eol:
            text += eol
    at.append(len(text))
    data, starts = P.bgzf_blocks(bytes(text), block_size)
    ustarts = [u for u, _ in starts]

    def voff(u):
        k = int(np.searchsorted(ustarts, u, side="right")) - 1
        return (starts[k][1] << 16) | (u - starts[k][0])
    return data, [voff(u) for u in at], bytes(text)


# ---- the tabix index -------------------------------------------------------------------------------------------------------------------

def tbi_plain(contigs, records, voffs, fmt=2):
    """The inflated bytes of a .tbi (the tabix format; the binning scheme is BAI's): records [(contig index, 0-based pos, len(REF))] in
    file order, voffs[i] / voffs[i + 1] the virtual offsets of record i's line and of what follows it. A record is binned by
    [pos, pos + len(REF)); a chunk grows while the records of a bin follow each other."""
    n_ref = len(contigs)
    bins = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    span = [None] * n_ref
    count = [0] * n_ref
    last = (None, None)
    for i, (t, beg, rl) in enumerate(records):
        end = beg + max(rl, 1)
        b = P.reg2bin(beg, end)
        cs = bins[t].setdefault(b, [])
        if last == (t, b) and cs and cs[-1][1] == voffs[i]:
            cs[-1][1] = voffs[i + 1]
        else:
            cs.append([voffs[i], voffs[i + 1]])
        last = (t, b)
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[t].setdefault(w, voffs[i])
        span[t] = [voffs[i] if span[t] is None else span[t][0], voffs[i + 1]]
        count[t] += 1
    names = b"".join(c.encode() + b"\0" for c in contigs)
    out = b"TBI\1" + struct.pack("<8i", n_ref, fmt, 1, 2, 0, ord("#"), 0, len(names)) + names
    for t in range(n_ref):
        out += struct.pack("<i", len(bins[t]) + (1 if span[t] else 0))
        for b in sorted(bins[t]):
            out += struct.pack("<Ii", b, len(bins[t][b]))
            for c in bins[t][b]:
                out += struct.pack("<QQ", c[0], c[1])
        if span[t]:
            out += struct.pack("<IiQQQQ", 37450, 2, span[t][0], span[t][1], count[t], 0)
        n_intv = max(lin[t]) + 1 if lin[t] else 0
        out += struct.pack("<i", n_intv)
        prev = 0
        for w in range(n_intv):
            prev = lin[t].get(w, prev)
            out += struct.pack("<Q", prev)
    return out + struct.pack("<Q", 0)


def tbi_bytes(contigs, records, voffs):
    """tbi_plain, BGZF-compressed: the bytes of the .tbi file."""
    return P.bgzf_blocks(tbi_plain(contigs, records, voffs), 0xff00)[0]


def index_tables(plain, bai=False):
    """The tables of inflated .tbi bytes (or of a .bai file) -> (names or None, [(bins {bin: [(beg, end)]}, linear [offsets])] per reference)."""
    names = None
    if bai:
        assert plain[:4] == b"BAI\1"
        (n_ref,) = struct.unpack_from("<i", plain, 4)
        at = 8
    else:
        assert plain[:4] == b"TBI\1"
        n_ref, _fmt, _cs, _cb, _ce, _meta, _skip, l_nm = struct.unpack_from("<8i", plain, 4)
        at = 36
        names = [x.decode() for x in plain[at:at + l_nm].split(b"\0")[:n_ref]]
        at += l_nm
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", plain, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", plain, at)
            at += 8
            cs = [struct.unpack_from("<QQ", plain, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
            if b != 37450:
                bins.setdefault(b, []).extend(cs)
        (n_intv,) = struct.unpack_from("<i", plain, at)
        at += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", plain, at))
        at += 8 * n_intv
        refs.append((bins, lin))
    return names, refs


def plan_ref(bins, lin, start, end):
    """The chunk rule lcty_sample_bam_plan documents, on one reference's tables: the bins of [start, end), without the chunks that end at
    or before the linear index's offset of the region's first window; sorted; merged where they touch, overlap or meet in one BGZF block."""
    beg, e = min(start, (1 << 29) - 1), min(end, 1 << 29)
    min_off = lin[min(beg >> 14, len(lin) - 1)] if lin else 0
    cs = [c for b in P.reg2bins(beg, e) for c in bins.get(b, []) if c[1] > min_off and c[0] < c[1]]
    merged = []
    for c in sorted(cs):
        if merged and (c[0] >> 16) <= (merged[-1][1] >> 16):
            merged[-1][1] = max(merged[-1][1], c[1])
        else:
            merged.append([c[0], c[1]])
    return merged


def plan(plain, contig, start, end):
    """The merged chunks lcty_vcf_indexed_plan returns, from the inflated bytes of the .tbi. A record is fetched iff pos < end and
    pos + len(REF) > start, so a region with end <= start stands for the bases [end - 1, start]."""
    names, refs = index_tables(plain)
    if end == 0 or contig not in names:
        return []
    bins, lin = refs[names.index(contig)]
    return plan_ref(bins, lin, min(start, end - 1), max(end, start + 1))


# ---- files -----------------------------------------------------------------------------------------------------------------------------

def rec(contig, pos, ref, alts, calls, fmt="GT", vid=".", info="."):
    """One record: 0-based pos, REF and ALT alleles as bytes, calls = the sample fields as they stand in the file (str)."""
    return dict(contig=contig, pos=pos, ref=ref, alts=list(alts), calls=list(calls), fmt=fmt, id=vid, info=info)


def line_of(r):
    alt = b",".join(r["alts"]) or b"."
    cols = [r["contig"].encode(), str(r["pos"] + 1).encode(), r["id"].encode(), r["ref"], alt, b".", b".", r["info"].encode()]
    if r["fmt"] is not None:
        cols += [r["fmt"].encode()] + [c.encode() for c in r["calls"]]
    return b"\t".join(cols)


def write_indexed(path, samples, records, block=700, eol=b"\n", last_eol=True, header=None, raw_lines=None):
    """path (BGZF, cut every `block` bytes) and path + '.tbi' for the records (sorted by contig in order of appearance, then position).
    raw_lines {record ordinal: bytes}: that record's line as given (the index still files it under the record's coordinates).
    -> dict(voffs of the record lines + the end, contigs, tbi = the inflated index, text, n_blocks)"""
    head = list(HEADER if header is None else header)
    head.append(b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO"] + ([b"FORMAT"] + [s.encode() for s in samples] if samples else [])))
    lines = [raw_lines[i] if raw_lines and i in raw_lines else line_of(r) for i, r in enumerate(records)]
    data, voffs, text = bgzf_lines(head + lines, block, eol, last_eol)
    contigs = []
    for r in records:
        if r["contig"] not in contigs:
            contigs.append(r["contig"])
    rv = voffs[len(head):]
    plain = tbi_plain(contigs, [(contigs.index(r["contig"]), r["pos"], len(r["ref"])) for r in records], rv)
    with open(path, "wb") as f:
        f.write(data)
    with open(str(path) + ".tbi", "wb") as f:
        f.write(P.bgzf_blocks(plain, 0xff00)[0])
    return dict(voffs=rv, contigs=contigs, tbi=plain, text=text, n_blocks=(len(text) + block - 1) // block, file_bytes=len(data))


def random_calls(rng, ploidy, n_alt, missing=0.1, big=0.0, fmt="GT"):
    """A phased call per sample: allele indices up to n_alt, '.' at rate `missing`, an index of 2 or 3 digits at rate `big` (the reader
    does not compare an index with the record's alleles)."""
    out = []
    for pl in ploidy:
        al = []
        for _ in range(pl):
            u = rng.random()
            al.append("." if u < missing else str(int(rng.integers(10, 1000))) if u < missing + big else str(int(rng.integers(0, n_alt + 1))))
        call = "|".join(al)
        out.append(call if fmt == "GT" else call + ":" + str(int(rng.integers(0, 99))) if fmt == "GT:DP" else str(int(rng.integers(0, 99))) + ":" + call)
    return out


def mixed_ploidy(n):
    """Ploidies 1 and 2 in no regular order: hap_off is irregular."""
    return [1 if (i * 7 + i // 3) % 3 == 0 else 2 for i in range(n)]


def seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def shaped_records(seed, n_samples, n=60, contig="chr1", start=1000, step=37):
    """Records whose lines run from under 64 bytes (few samples) to over 256: short and long IDs and INFO, REF and ALT of 1 to 40 bases,
    no ALT, several ALT alleles, the three FORMAT variants, '.' calls and indices of 2 and 3 digits."""
    rng = np.random.default_rng(seed)
    pl = mixed_ploidy(n_samples)
    out = []
    for i in range(n):
        ref = seq(rng, int(rng.choice([1, 1, 2, 7, 40])))
        n_alt = int(rng.integers(0, 4))
        alts = [seq(rng, int(rng.choice([1, 1, 3, 33]))) for _ in range(n_alt)]
        fmt = ("GT", "GT:DP", "DP:GT")[i % 3]
        long_ = i % 5 == 4
        out.append(rec(contig, start + i * step + int(rng.integers(0, step // 2)), ref, alts, random_calls(rng, pl, max(n_alt, 1), 0.1, 0.15, fmt), fmt,
                       vid=("rs" + "9" * 70) if long_ else ".", info=("AC=1;" * 50) if long_ and i % 2 else "."))
    return pl, out


def names_of(n):
    return [f"S{i}" for i in range(n)]


def two_boundaries():
    """Records around 16 384 and 131 072; at each boundary one record with a 10-base REF across it, which lands in a higher-level bin, and
    behind it a run of records in front of the boundary — another smallest bin — that is longer than a BGZF block."""
    rng = np.random.default_rng(6)
    pl = [2, 1, 2]
    recs = []
    for edge in (16384, 131072):
        recs += [rec("chrA", edge - 300 + 20 * i, b"A", [b"C"], random_calls(rng, pl, 1)) for i in range(10)]
        recs.append(rec("chrA", edge - 4, seq(rng, 10), [b"G"], random_calls(rng, pl, 1)))
        recs += [rec("chrA", edge - 3 + i % 3, b"C", [seq(rng, 30)], random_calls(rng, pl, 1), info="RUN=" + "z" * 60) for i in range(24)]
        recs[-24:] = sorted(recs[-24:], key=lambda r: r["pos"])
        recs += [rec("chrA", edge + 15 * i, b"G", [b"T", b"TT"], random_calls(rng, pl, 2)) for i in range(12)]
    return pl, recs


def three_contig_file(path):
    """A 3-contig file of more than 200 BGZF blocks and a window in the middle of it whose chunks touch under a tenth of the blocks
    (checked here, with plan). -> (records, the dict of write_indexed, the window)"""
    rng = np.random.default_rng(9)
    pl = [2, 2, 1]
    recs = [rec(c, 4000 * i + int(rng.integers(0, 2000)), seq(rng, 1 + i % 4), [seq(rng, 1 + i % 7)], random_calls(rng, pl, 1), info="AF=0.25;NS=3;DP=14")
            for c in ("chr1", "chr2", "chr3") for i in range(900)]
    info = write_indexed(path, names_of(3), recs)
    window = ("chr2", 1_400_000, 1_450_000)
    chunks = plan(info["tbi"], *window)
    blocks = sorted({v >> 16 for v in info["voffs"]})
    touched = [b for b in blocks if any(c[0] >> 16 <= b <= c[1] >> 16 for c in chunks)]
    assert info["n_blocks"] >= 200 and 0 < len(touched) < len(blocks) / 10
    return recs, info, window


# ---- the corpus of scripts/vcf_index_probe_host.cpp --------------------------------------------------------------------------------------

def small_index():
    """A valid index of two contigs: several bins, a bin with two chunks, the pseudo-bin, a linear index."""
    recs = [(0, 100, 1), (0, 120, 3), (0, 16380, 10), (0, 16390, 1), (0, 40000, 2), (0, 150, 1), (1, 5, 1), (1, 70000, 5)]
    voffs = [(i * 300) << 16 | (i * 11) for i in range(len(recs) + 1)]
    return tbi_plain(["chr1", "chr2"], recs, voffs)


def index_cases():
    """[(inflated index bytes, expected status)]: the valid index, every truncation of it, and the designed errors."""
    good = small_index()
    cases = [(good, OK), (good[:-8], OK)]                         # n_no_coor is optional
    cases += [(good[:n], ERR_INVALID_DATA) for n in range(len(good) - 8)]
    cases += [(good[:n], ERR_INVALID_DATA) for n in range(len(good) - 7, len(good))]

    def put(at, fmt, v):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, v)
        return bytes(b)
    l_nm = struct.unpack_from("<i", good, 32)[0]
    ref0 = 36 + l_nm                                               # n_bin of the first reference
    n_chunk0 = ref0 + 8                                            # n_chunk of its first bin
    n_bin0 = struct.unpack_from("<i", good, ref0)[0]
    at = ref0 + 4
    for _ in range(n_bin0):
        at += 8 + 16 * struct.unpack_from("<i", good, at + 4)[0]
    n_intv0 = at
    cases += [(put(ref0, "<i", -1), ERR_INVALID_DATA), (put(n_chunk0, "<i", -3), ERR_INVALID_DATA), (put(n_intv0, "<i", -2), ERR_INVALID_DATA),
              (put(4, "<i", -1), ERR_INVALID_DATA), (put(32, "<i", -5), ERR_INVALID_DATA),
              (put(ref0, "<i", 1 << 30), ERR_INVALID_DATA), (put(n_chunk0, "<i", 1 << 27), ERR_INVALID_DATA), (put(n_intv0, "<i", 1 << 28), ERR_INVALID_DATA),
              (put(32, "<i", len(good)), ERR_INVALID_DATA),                              # l_nm beyond the file
              (good[:36] + good[36:36 + l_nm].replace(b"\0", b"x") + good[36 + l_nm:], ERR_INVALID_DATA),      # names without terminator
              (put(8, "<i", 0), ERR_INVALID_DATA), (put(8, "<i", 1), ERR_INVALID_DATA),  # format != 2
              (put(n_chunk0 + 4, "<Q", 1 << 60), ERR_INVALID_DATA),                      # beg > end
              (b"CSI\1" + good[4:], ERR_UNSUPPORTED), (b"BAI\1" + good[4:], ERR_INVALID_DATA), (b"", ERR_INVALID_DATA)]
    return cases


def line_cases():
    """[(line, samples, ploidy, expected status)] for the line functions: parse_line_head, then parse_record_line with all samples used."""
    s2, p2 = 2, [2, 1]
    return [(b"chr1\t5\t.\tA\tC,CT\t.\t.\t.\tGT\t0|1\t2", s2, p2, OK), (b"chr1\t5\t.\tA\t.\t.\t.\t.\tGT:DP\t.|1:3\t.:4", s2, p2, OK),
            (b"chr1\t5\t.\tA\tC\t.\t.\t.\tDP:GT\t3:0|1\t4", s2, p2, OK), (b"chr1\t5\t.\tA\tC\t.\t.\t.\tDP:GT\t3\t4:1", s2, p2, ERR_INVALID_DATA),
            (b"chr1\t5\t.\tA\tC\t.\t.\t.", 0, [], OK), (b"chr1\t5\t.\tA\tC\t.\t.", 0, [], ERR_INVALID_DATA),
            (b"chr1\t5\t.\tA", 0, [], ERR_INVALID_DATA), (b"chr1", 0, [], ERR_INVALID_DATA), (b"", 0, [], ERR_INVALID_DATA),
            (b"chr1\t\t.\tA\tC\t.\t.\t.", 0, [], ERR_INVALID_DATA), (b"chr1\t0\t.\tA\tC\t.\t.\t.", 0, [], ERR_INVALID_DATA),
            (b"chr1\t4294967295\t.\tA\tC\t.\t.\t.", 0, [], OK), (b"chr1\t4294967296\t.\tA\tC\t.\t.\t.", 0, [], ERR_INVALID_DATA),
            (b"chr1\t99999999999999999999999\t.\tA\tC\t.\t.\t.", 0, [], ERR_INVALID_DATA), (b"chr1\t5x\t.\tA\tC\t.\t.\t.", 0, [], ERR_INVALID_DATA),
            (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0|1", s2, p2, ERR_INVALID_DATA), (b"chr1\t5\t.\tA\tC\t.\t.\t.\tDP\t0|1\t1", s2, p2, ERR_INVALID_DATA),
            (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0/1\t1", s2, p2, ERR_INVALID_DATA), (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0|x\t1", s2, p2, ERR_INVALID_DATA),
            (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0|\t1", s2, p2, ERR_INVALID_DATA), (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0|1\t40000", s2, p2, ERR_UNSUPPORTED),
            (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0|1\t32767", s2, p2, OK), (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t0|1|1\t1", s2, p2, ERR_INVALID_DATA),
            (b"chr1\t5\t.\tA\tC\t.\t.\t.\tGT\t\t", s2, p2, ERR_INVALID_DATA)]


def write_corpus(path):
    """The corpus file: u32 n_index_cases, then per case u32 n, u32 status, n bytes; u32 n_line_cases, then per case u32 n, u32 status,
    u32 n_samples, n_samples x u32 ploidy, n bytes. Returns the number of cases."""
    ic, lc = index_cases(), line_cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(ic)))
        for b, st in ic:
            f.write(struct.pack("<II", len(b), st) + b)
        f.write(struct.pack("<I", len(lc)))
        for b, s, pl, st in lc:
            f.write(struct.pack("<III", len(b), st, s) + struct.pack(f"<{s}I", *pl) + b)
    return len(ic) + len(lc)
