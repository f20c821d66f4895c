"""The reads a sample's indexed BAM file gives to recruitment (`locityper genotype -a`), restated index-free on plain Python: a linear
walk of the whole file. The reference's route is recruit_to_targets (src/command/genotype.rs:872-907) -> postprocess_targets (776-797)
-> IndexedBamReader + PairedBamReader (src/seq/fastx.rs:577-874); rust-htslib cannot run here, so its fetch rule is stated from the SAM
specification and htslib's documented behaviour (bam_endpos: a reference length of 0 counts as 1).

Next to the restatement: a BAM writer (mate fields, qualities, any flags, a chosen BGZF block size) and a BAI writer (bins, linear
index, pseudo-bin, n_no_coor) for the tests, and a reader of BAM files by linear inflation."""
import struct
import zlib

import numpy as np

ERR_INVALID_INPUT, ERR_INVALID_DATA, ERR_UNSUPPORTED = 1, 2, 5
CODES = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
REF_OPS = set("MDN=X")


class Refused(Exception):
    """what the reference answers with an error: (status, the read's name)"""

    def __init__(self, status, name, what):
        super().__init__(f"{what} ({name})")
        self.status, self.name, self.what = status, name, what


# ---- records ----------------------------------------------------------------------------------------------------------------------

def rec(tid, pos, name, flag, cigar, seq, qual=None, mtid=-1, mpos=-1, mapq=60):
    """cigar: [(op char, len)]; seq: str of BAM code letters (=ACMGRSVTWYHKDBN); qual: bytes of phred values, None = absent (0xff)."""
    return dict(tid=tid, pos=pos, name=name, flag=flag, cigar=list(cigar), seq=seq, qual=qual, mtid=mtid, mpos=mpos, mapq=mapq)


def rlen(r):
    return 0 if r["flag"] & 4 else sum(n for o, n in r["cigar"] if o in REF_OPS)


def endpos(r):
    return r["pos"] + (rlen(r) or 1)


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += list(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def record_bytes(r):
    nm = r["name"].encode() + b"\0"
    cig = b"".join(struct.pack("<I", (n << 4) | OPS.index(o)) for o, n in r["cigar"])
    codes = [CODES.index(c) for c in r["seq"]]
    if len(codes) % 2:
        codes.append(0)
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    ls = len(r["seq"])
    qual = b"\xff" * ls if r["qual"] is None else bytes(r["qual"])
    assert len(qual) == ls
    b = reg2bin(r["pos"], endpos(r)) if r["tid"] >= 0 and r["pos"] >= 0 else 4680
    body = struct.pack("<iiBBHHHIiii", r["tid"], r["pos"], len(nm), r["mapq"], b, len(r["cigar"]) & 0xFFFF, r["flag"], ls, r["mtid"], r["mpos"], 0)
    body += nm + cig + packed + qual + r.get("tags", b"")
    return struct.pack("<I", len(body)) + body


def header_bytes(refs):
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    head = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for nm, ln in refs:
        head += struct.pack("<I", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<I", ln)
    return head


EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_blocks(data, block_size):
    """-> (file bytes, [(uncompressed start, compressed start)] of the blocks, the end-of-file block's included)"""
    out, starts = bytearray(), []
    for i in range(0, len(data), block_size):
        chunk = data[i:i + block_size]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        starts.append((i, len(out)))
        out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25)
        out += comp + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))
    starts.append((len(data), len(out)))
    out += EOF_BLOCK
    return bytes(out), starts


def write_bam(path, refs, records, block_size=0xff00, index=True, raw_records=None):
    """A BAM file of `records` in this order, in BGZF blocks of block_size uncompressed bytes, and path + '.bai' (index=True; a str: that
    path). raw_records: the records' bytes when a test wants them malformed. Returns the virtual offset of every record + the end."""
    head = header_bytes(refs)
    blobs = raw_records if raw_records is not None else [record_bytes(r) for r in records]
    offs, at = [], len(head)
    for b in blobs:
        offs.append(at)
        at += len(b)
    offs.append(at)
    data = head + b"".join(blobs)
    file_bytes, starts = bgzf_blocks(data, block_size)
    ustarts = [u for u, _ in starts]

    def voff(u):
        k = int(np.searchsorted(ustarts, u, side="right")) - 1
        return (starts[k][1] << 16) | (u - starts[k][0])
    with open(path, "wb") as f:
        f.write(file_bytes)
    voffs = [voff(u) for u in offs]
    if index:
        ipath = index if isinstance(index, str) else str(path) + ".bai"
        with open(ipath, "wb") as f:
            f.write(bai_bytes(refs, records, voffs))
    return voffs


def bai_bytes(refs, records, voffs):
    """The BAI index of a sorted file (SAM specification 5.2): per reference its bins with their chunks (a chunk grows while the records
    of a bin follow each other), the pseudo-bin 37450, the 16 kb linear index; then the number of records without coordinate."""
    n_ref = len(refs)
    bins = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    span = [None] * n_ref
    counts = [[0, 0] for _ in range(n_ref)]
    no_coor = 0
    last = (None, None)
    for i, r in enumerate(records):
        if r["tid"] < 0:
            no_coor += 1
            last = (None, None)
            continue
        t, beg, end = r["tid"], r["pos"], endpos(r)
        b = reg2bin(beg, end)
        cs = bins[t].setdefault(b, [])
        if last == (t, b) and cs and cs[-1][1] == voffs[i]:
            cs[-1][1] = voffs[i + 1]
        else:
            cs.append([voffs[i], voffs[i + 1]])
        last = (t, b)
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[t].setdefault(w, voffs[i])
        span[t] = [voffs[i] if span[t] is None else span[t][0], voffs[i + 1]]
        counts[t][1 if r["flag"] & 4 else 0] += 1
    out = b"BAI\1" + struct.pack("<I", n_ref)
    for t in range(n_ref):
        n_bin = len(bins[t]) + (1 if span[t] else 0)
        out += struct.pack("<I", n_bin)
        for b in sorted(bins[t]):
            out += struct.pack("<Ii", b, len(bins[t][b]))
            for c in bins[t][b]:
                out += struct.pack("<QQ", c[0], c[1])
        if span[t]:
            out += struct.pack("<IiQQQQ", 37450, 2, span[t][0], span[t][1], counts[t][0], counts[t][1])
        n_intv = max(lin[t]) + 1 if lin[t] else 0
        out += struct.pack("<I", n_intv)
        prev = 0
        for w in range(n_intv):
            prev = lin[t].get(w, prev)
            out += struct.pack("<Q", prev)
    return out + struct.pack("<Q", no_coor)


def read_bgzf(path):
    """-> (uncompressed bytes, [(uncompressed start, compressed start, compressed size)] per block)"""
    raw = open(path, "rb").read()
    out, blocks, at = bytearray(), [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        bsize, x = None, at + 12
        while x < at + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", raw, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", raw, x + 4)[0] + 1
            x += 4 + slen
        blocks.append((len(out), at, bsize))
        out += zlib.decompress(raw[at + 12 + xlen:at + bsize - 8], -15)
        at += bsize
    return bytes(out), blocks


def parse_records(data, at, end=None):
    """Records from byte `at` of an uncompressed BAM stream -> list of rec() dicts with 'at' (their offset)."""
    out = []
    end = len(data) if end is None else end
    while at < end:
        (bs,) = struct.unpack_from("<I", data, at)
        tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, mtid, mpos, _tlen = struct.unpack_from("<iiBBHHHIiii", data, at + 4)
        p = at + 36
        name = data[p:p + l_name - 1].decode()
        p += l_name
        cigar = [(OPS[w & 15], w >> 4) for w in struct.unpack_from(f"<{n_cig}I", data, p)]
        p += 4 * n_cig
        packed = data[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(CODES[(packed[j >> 1] >> (0 if j & 1 else 4)) & 15] for j in range(l_seq))
        q = data[p:p + l_seq]
        r = rec(tid, pos, name, flag, cigar, seq, None if (l_seq == 0 or q[0] == 255) else q, mtid, mpos, mapq)
        r["at"] = at
        out.append(r)
        at += 4 + bs
    return out


def read_bam(path):
    """-> (refs [(name, length)], records in file order) by inflating the whole file."""
    data, _ = read_bgzf(path)
    assert data[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<I", data, 4)
    at = 8 + l_text
    (n_ref,) = struct.unpack_from("<I", data, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<I", data, at)
        nm = data[at + 4:at + 4 + l_name - 1].decode()
        (ln,) = struct.unpack_from("<I", data, at + 4 + l_name)
        refs.append((nm, ln))
        at += 8 + l_name
    return refs, parse_records(data, at)


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def check_regions(regions):
    for i, (t, s, e) in enumerate(regions):
        if s >= e:
            raise Refused(ERR_INVALID_INPUT, "", "empty region")
        if i and (t, s) < (regions[i - 1][0], regions[i - 1][2]):
            raise Refused(ERR_INVALID_INPUT, "", "regions must be sorted")


def fetched_stream(records, regions, with_unmapped=True, whole_file=False):
    """IndexedBamReader (fastx.rs:732-803) / DirectBamReader (692-729): indices into `records` (file order) of the fetched stream."""
    def keep(r, min_start):
        if (r["flag"] & 0x900) == 0 and (min_start is None or r["pos"] >= min_start):       # BamRecord::read_from (587-611)
            if len(r["seq"]) == 0:
                raise Refused(ERR_INVALID_DATA, r["name"], "Primary alignment has no sequence")
            return True
        return False
    out = []
    if whole_file:
        return [i for i, r in enumerate(records) if keep(r, None)]
    check_regions(regions)
    for i, (t, s, e) in enumerate(regions):
        min_start = regions[i - 1][2] if i and regions[i - 1][0] == t else None                # fetch_next (762-783)
        for j, r in enumerate(records):
            if r["tid"] == t and r["pos"] < e and endpos(r) > s and keep(r, min_start):
                out.append(j)
    if with_unmapped:
        out += [j for j, r in enumerate(records) if r["tid"] < 0 and keep(r, None)]
    return out


def pairs_of(records, stream):
    """PairedBamReader::read_next (829-869) -> ([(mate 1, mate 2)] as indices into records, in the order of the completing records, discarded)."""
    waiting, pairs, discarded = {}, [], 0
    for j in stream:
        r = records[j]
        if (r["flag"] & 0xC0) == 0:
            raise Refused(ERR_INVALID_DATA, r["name"], "Expected paired-end reads, but read is unpaired")
        if r["name"] in waiting:
            m = waiting.pop(r["name"])
            first = bool(r["flag"] & 0x40)
            if first == bool(records[m]["flag"] & 0x40):
                raise Refused(ERR_INVALID_DATA, r["name"], "Found two primary alignments for the same read end")
            pairs.append((j, m) if first else (m, j))
        else:
            curr = (r["tid"] & 0xFFFFFFFF, r["pos"] & 0xFFFFFFFFFFFFFFFF)
            mate = (r["mtid"] & 0xFFFFFFFF, r["mpos"] & 0xFFFFFFFFFFFFFFFF)
            if curr <= mate:
                waiting[r["name"]] = j
            else:
                discarded += 1
    return pairs, discarded + len(waiting)


def complement_nt(c):
    """seq::complement_nt (src/seq/mod.rs:125-135); '=' is not a nucleotide there (it panics) and counts as N here"""
    return {"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N")


def restored(r):
    """the sequence as the sequencer gave it (fastx.rs:603-607)"""
    return "".join(complement_nt(c) for c in reversed(r["seq"])) if r["flag"] & 0x10 else r["seq"]


def packed(mates):
    """[[seq or None] x 2 per unit] -> mate_len, mate_off, bases2, nmask as lcty_reads_host lays them out"""
    n = len(mates)
    mate_len = np.zeros(2 * n, dtype=np.uint32)
    mate_off = np.zeros(2 * n + 1, dtype=np.uint64)
    off = 0
    for i, pair in enumerate(mates):
        for e in range(2):
            mate_off[2 * i + e] = off
            if pair[e] is not None:
                mate_len[2 * i + e] = len(pair[e])
                off += (len(pair[e]) + 31) // 32 * 32
    mate_off[2 * n] = off
    bases2 = np.zeros(max(off // 16, 2), dtype=np.uint32)
    nmask = np.zeros(max(off // 32, 1), dtype=np.uint32)
    for i, pair in enumerate(mates):
        for e in range(2):
            if pair[e] is None:
                continue
            o = int(mate_off[2 * i + e])
            for k, c in enumerate(pair[e]):
                at = o + k
                v = "ACGT".find(c)
                if v >= 0:
                    bases2[at >> 4] |= np.uint32(v << (2 * (at & 15)))
                else:
                    nmask[at >> 5] |= np.uint32(1 << (at & 31))
    return mate_len, mate_off, bases2, nmask


def record_text(r):
    """BamRecord::write_to (fastx.rs:633-668)"""
    seq = restored(r)
    if r["qual"] is None or len(r["qual"]) == 0 or r["qual"][0] == 255:
        return f">{r['name']}\n{seq}\n".encode()
    q = bytes(r["qual"])[::-1] if r["flag"] & 0x10 else bytes(r["qual"])
    return f"@{r['name']}\n{seq}\n+\n".encode() + bytes(x + 33 for x in q) + b"\n"


def postprocess_targets(intervals, contig_len, padding, alt_contig_len=10_000_000, merge_distance=1000):
    """genotype.rs:776-797 with Interval::add_padding (interv.rs:74-77) and Interval::merge (232-247); intervals: [(tid, start, end)]"""
    v = [(t, max(s - padding, 0), min(e + padding, contig_len[t])) for t, s, e in intervals]
    v += [(t, 0, ln) for t, ln in enumerate(contig_len) if ln < alt_contig_len]
    v.sort()
    merged = []
    for t, s, e in v:
        if merged and merged[-1][0] == t and merged[-1][2] + merge_distance >= s:
            merged[-1][2] = max(merged[-1][2], e)
        else:
            merged.append([t, s, e])
    return [tuple(m) for m in merged]
