"""A seeded synthetic sample for the background estimate (lcty_bg_estimate): a padded reference region, its k-mer counts and a BAM file
of the sample's alignments there, written by hand (BGZF through zlib, records through struct; no pysam).

Illumina: pairs at ~30x with NB(mean 400, sd 50) inserts, known substitution / indel rates and a GC-dependent depth; next to them the
record kinds the reference filters or treats specially: MAPQ < 30, secondary / supplementary / duplicate / QC-fail records, clipping
over 2 %, mates outside the interval, =/X CIGARs, a leading insertion, alignments that leave the padded sequence (dropped: no extended
CIGAR), one that ends a base before its end (kept) and records on another contig. ONT: single-end 10 kb reads."""
import struct
import zlib

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
OPS = "MIDNSHP=X"
PAD = 50_000


def bgzf(data):
    """BGZF blocks of <= 64 KB + the empty end block."""
    out = bytearray()
    for i in range(0, max(len(data), 1), 0xff00):
        chunk = data[i:i + 0xff00]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25)
        out += comp + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return bytes(out)


def bam_record(tid, pos, name, mapq, flag, cigar, seq):
    """cigar: [(op char, len)], seq: bytes of ACGTN."""
    nm = name.encode() + b"\0"
    cig = b"".join(struct.pack("<I", (n << 4) | OPS.index(o)) for o, n in cigar)
    codes = [("=ACMGRSVTWYHKDBN").index(chr(c)) for c in seq]
    if len(codes) % 2:
        codes.append(0)
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(nm), mapq, 4680, len(cigar), flag, len(seq), -1, -1, 0)
    body += nm + cig + packed + b"\xff" * len(seq)
    return struct.pack("<I", len(body)) + body


def write_bam(path, refs, records):
    """refs: [(name, length)]; records: [(tid, pos, name, mapq, flag, cigar, seq)] written in this order."""
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    head = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for nm, ln in refs:
        head += struct.pack("<I", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<I", ln)
    body = b"".join(bam_record(*r) for r in records)
    with open(path, "wb") as f:
        f.write(bgzf(head + body))


def rle(codes):
    out = []
    for c in codes:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [(o, n) for o, n in out]


class Sample:
    """padded_seq (bytes), padded_start, region [start, end), kmer counts (u16, k = 25), records, truth."""

    def __init__(self, seed=7, region_len=400_000, tech="illumina", depth=30.0, k=25, sub=0.005, ins=0.0003, dele=0.0003):
        rng = np.random.default_rng(seed)
        self.k, self.contig = k, "chrS"
        self.padded_start = 1_000_000
        self.start, self.end = self.padded_start + PAD, self.padded_start + PAD + region_len
        n = region_len + 2 * PAD
        # GC in 1.5 kb blocks, between 15 and 80 %
        nblk = n // 1500 + 1
        gc_blk = rng.uniform(0.15, 0.8, nblk)
        self.blk_noise = rng.gamma(5.0, 0.2, nblk)                    # depth varies from block to block beyond GC: var > mean
        gc = np.repeat(gc_blk, 1500)[:n]
        u = rng.random(n)
        at = rng.random(n) < 0.5
        gcb = rng.random(n) < 0.5
        seq = np.where(u < gc, np.where(gcb, ord("G"), ord("C")), np.where(at, ord("A"), ord("T"))).astype(np.uint8)
        self.padded_seq = seq.tobytes()
        # k-mer counts: mostly unique, some noise, planted repeats (windows there fail the 90 % filter)
        nk = n + 1 - k
        cnt = np.ones(nk, dtype=np.uint16)
        cnt[rng.random(nk) < 0.03] = 2
        self.repeats = []
        for s in rng.choice(np.arange(PAD, n - PAD - 6000, 6000), 12, replace=False):
            cnt[s:s + 4000] = rng.integers(2, 40, 4000)
            self.repeats.append((self.padded_start + int(s), self.padded_start + int(s) + 4000))
        self.kmer_counts = cnt
        self.tech, self.sub, self.ins, self.dele = tech, sub, ins, dele
        self.rng = rng
        self.records = []
        self.gc_blk = gc_blk
        if tech == "illumina":
            self._illumina(depth)
        else:
            self._ont(depth)

    # ---- read construction ----------------------------------------------------------------------------------------------------
    def _read(self, ref_pos, qlen, eqx=False):
        """ops over the reference from ref_pos (padded coordinates) -> (cigar, seq, ref_len)."""
        rng = self.rng
        m = int(qlen * 1.3) + 20
        r = rng.random(m)
        f = rng.gamma(4.0, 0.25)                                      # per-read error rate factor (mean 1): overdispersed edits
        sub, ins, dele = f * self.sub, f * self.ins, f * self.dele
        op = np.zeros(m, dtype=np.int8)                               # 0 match, 1 sub, 2 ins, 3 del
        op[r < sub + ins + dele] = 3
        op[r < sub + ins] = 2
        op[r < sub] = 1
        op[:3] = 0
        q_inc = (op != 3).astype(np.int64)
        qcum = np.cumsum(q_inc)
        last = int(np.searchsorted(qcum, qlen))                       # op index where the query reaches qlen
        op = op[:last + 1]
        op[-3:] = 0
        q_inc = (op != 3)
        r_inc = (op != 2)
        rp = ref_pos + np.cumsum(r_inc) - r_inc
        ref = np.frombuffer(self.padded_seq, dtype=np.uint8)
        rp_c = np.clip(rp, 0, len(ref) - 1)
        base = ref[rp_c].copy()
        subs = op == 1
        alt = rng.integers(1, 4, subs.sum())
        idx = (np.searchsorted(ACGT, base[subs]) + alt) % 4
        base[subs] = ACGT[idx]
        insm = op == 2
        base[insm] = ACGT[rng.integers(0, 4, insm.sum())]
        seq = base[q_inc].tobytes()
        if eqx:
            codes = np.array(["=", "X", "I", "D"])[op]
        else:
            codes = np.array(["M", "M", "I", "D"])[op]
        cigar = rle(codes.tolist())
        return cigar, seq, int(r_inc.sum())

    def _depth_weight(self, pos):
        b = np.minimum(pos // 1500, len(self.gc_blk) - 1)
        g = self.gc_blk[b]
        return np.clip(1.0 - 2.0 * (g - 0.45) ** 2, 0.2, 1.0) * self.blk_noise[b] / 3.0

    def _illumina(self, depth):
        rng = self.rng
        n = len(self.padded_seq)
        rl = 150
        self.ins_mean, self.ins_sd = 400.0, 50.0
        v = self.ins_sd ** 2
        nb_n, nb_p = self.ins_mean ** 2 / (v - self.ins_mean), self.ins_mean / v
        n_frag = int(depth * n / (2 * rl))
        starts = rng.integers(0, n - 1200, int(n_frag * 4.5))
        keep = rng.random(len(starts)) < self._depth_weight(starts)
        starts = np.sort(starts[keep][:n_frag])
        inserts = rng.negative_binomial(nb_n, nb_p, len(starts))
        inserts = np.clip(inserts, 2 * rl, 1000)
        recs = []
        clean = []                                                    # middles of the first ends of pairs that no filter removes
        for i, (s, isz) in enumerate(zip(starts.tolist(), inserts.tolist())):
            name = f"p{i}"
            eqx = i % 17 == 0
            c1, q1, r1 = self._read(s, rl, eqx)
            c2, q2, r2 = self._read(0, rl, eqx)
            s2 = s + isz - r2
            c2, q2, r2 = self._read(s2, rl, eqx)
            first_fwd = rng.random() < 0.5
            fl1 = 0x1 | 0x2 | 0x40 | (0 if first_fwd else 0x10)
            fl2 = 0x1 | 0x2 | 0x80 | (0x10 if first_fwd else 0)
            mq1 = mq2 = 60
            kind = rng.random()
            if kind < 0.02:
                mq1 = 10                                              # MAPQ < 30
            elif kind < 0.03:
                fl1 |= 0x400                                          # duplicate
            elif kind < 0.035:
                fl2 |= 0x200                                          # QC fail
            elif kind < 0.045:
                c1, q1 = self._clip(s, rl, 10)                        # 10 / 150 clipped: > 2 %
            elif kind < 0.06:
                c1, q1 = self._clip(s, rl, 2)                         # 2 / 150: kept, S counted
            elif kind < 0.065:
                c1, q1 = self._lead_ins(s, rl, 2)                     # leading I counts as clipping
            recs.append((0, self.padded_start + s, name, mq1, fl1, c1, q1))
            recs.append((0, self.padded_start + s2, name, mq2, fl2, c2, q2))
            if kind >= 0.045:
                clean.append(self.padded_start + s + r1 // 2)
            if i % 97 == 0:                                           # a secondary and a supplementary record
                recs.append((0, self.padded_start + s + 5, name, 0, (fl1 | 0x100), c1, q1))
                recs.append((0, self.padded_start + s2 + 7, name, 60, (fl2 | 0x800), c2, q2))
        self._edge_records(recs, rl, paired=True)
        recs.sort(key=lambda r: (r[0], r[1]))
        self.records = recs
        self.clean_mid1 = np.array(clean, dtype=np.int64)
        self.paired = True

    def _clip(self, s, rl, nclip):
        rng = self.rng
        ref = self.padded_seq
        q = bytes(rng.choice(list(b"ACGT"), nclip).tolist()) + ref[s:s + rl - nclip]
        return [("S", nclip), ("M", rl - nclip)], q

    def _lead_ins(self, s, rl, nins):
        ref = self.padded_seq
        q = b"AC"[:nins].ljust(nins, b"A") + ref[s:s + rl - nins]
        return [("I", nins), ("M", rl - nins)], q

    def _edge_records(self, recs, rl, paired):
        """Alignments that leave the padded sequence, one that ends a base short of its end, and records of another contig."""
        ref = self.padded_seq
        P = self.padded_start
        re_ = self.end - P                                            # region end in padded coordinates
        fl = (0x1 | 0x2 | 0x40) if paired else 0
        # second M run ends exactly at the padded end: dropped (>=)
        d = len(ref) - (re_ + 100)
        recs.append((0, P + re_ - 100, "edge_drop_end", 60, fl, [("M", 100), ("D", d), ("M", 100)],
                     ref[re_ - 100:re_] + ref[len(ref) - 100:]))
        # ... one base earlier: kept
        recs.append((0, P + re_ - 100, "edge_keep_end", 60, fl, [("M", 100), ("D", d - 1), ("M", 100)],
                     ref[re_ - 100:re_] + ref[len(ref) - 101:len(ref) - 1]))
        # first M run before the padded start: dropped
        rs_ = self.start - P
        recs.append((0, P - 100, "edge_drop_start", 60, fl, [("M", 100), ("D", rs_ + 50), ("M", 100)],
                     b"A" * 100 + ref[rs_ - 50:rs_ + 50]))
        # records without M are taken as they are, even outside the padded sequence
        recs.append((0, P + re_ - 60, "edge_eqx", 60, fl, [("=", 60), ("D", d), ("=", 40)], b"C" * 100))
        # another contig
        for j in range(5):
            recs.append((1, 1000 + j * 300, f"other{j}", 60, fl, [("M", rl)], ref[:rl]))

    def _ont(self, depth):
        rng = self.rng
        n = len(self.padded_seq)
        rl = 10_000
        n_reads = int(depth * n / rl)
        starts = rng.integers(0, n - int(rl * 1.3), n_reads * 4)
        b = np.minimum(starts // 1500, len(self.gc_blk) - 1)
        starts = np.sort(starts[rng.random(len(starts)) < self.blk_noise[b] / 3.0][:n_reads])
        recs = []
        for i, s in enumerate(starts.tolist()):
            c, q, _ = self._read(s, int(rng.integers(8000, 12000)))
            fl = 0x10 if rng.random() < 0.5 else 0
            mq = 10 if i % 50 == 0 else 60
            recs.append((0, self.padded_start + s, f"r{i}", mq, fl, c, q))
        self._edge_records(recs, 150, paired=False)
        recs.sort(key=lambda r: (r[0], r[1]))
        self.records = recs
        self.paired = False

    def refs(self):
        return [(self.contig, self.padded_start + len(self.padded_seq) + 100_000), ("chrO", 100_000)]

    def write(self, path, records=None):
        write_bam(path, self.refs(), self.records if records is None else records)
        return path

    def padded_len(self):
        return len(self.padded_seq)


def ont_sample(seed=11, region_len=400_000, depth=30.0):
    return Sample(seed=seed, region_len=region_len, tech="ont", depth=depth, sub=0.02, ins=0.01, dele=0.01)
