"""Files for lcty_bg_reads_fetch: the record tuples of bg_synth written as coordinate-sorted, indexed BAM files by
pyref_sample_bam.write_bam, foreign records around a seeded sample, and a hand-made file of the record kinds the background route
filters, drops, keeps or refuses."""
import numpy as np

from tests import bg_synth, pyref_sample_bam as SB


def to_rec(t):
    """bg_synth tuple (tid, pos, name, mapq, flag, cigar, seq bytes) -> pyref_sample_bam.rec dict"""
    tid, pos, name, mapq, flag, cigar, seq = t
    return SB.rec(tid, pos, name, flag, cigar, bytes(seq).decode(), mapq=mapq)


def by_coordinate(tuples):
    return sorted(tuples, key=lambda r: (r[0], r[1]))


def write_indexed(path, refs, tuples, block_size=0xff00):
    """The tuples in the order given (sorted by the caller, or not on purpose) as path + path.bai; returns path."""
    SB.write_bam(str(path), refs, [to_rec(t) for t in tuples], block_size=block_size, index=True)
    return path


def write_plain(path, refs, tuples):
    """The same records as bg_synth writes them: no index, blocks of 0xff00 bytes."""
    bg_synth.write_bam(path, refs, tuples)
    return path


def seq_of(n, seed=0):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()


def wide_refs(s):
    """contigs long enough for records far behind the padded region of a bg_synth.Sample"""
    return [(s.contig, s.padded_start + len(s.padded_seq) + 2_000_000), ("chrO", 2_000_000)]


def with_foreign(s, n=2000, behind=300_000):
    """The sample's records followed, on its contig, by n / 2 records `behind` bases behind the padded region and, on the other
    contig, by n / 2 more: what a whole-genome file holds next to the background region."""
    fl = (0x1 | 0x2 | 0x40) if s.paired else 0
    q = seq_of(150, 3)
    at = s.padded_start + len(s.padded_seq) + behind
    own = [(0, at + 40 * i, f"far{i}", 60, fl, [("M", 150)], q) for i in range(n // 2)]
    other = [(1, 10_000 + 40 * i, f"alt{i}", 60, fl, [("M", 150)], q) for i in range(n - n // 2)]
    return by_coordinate(list(s.records) + own + other)


# ---- the hand file ---------------------------------------------------------------------------------------------------------------
class Hand:
    """Two contigs with the same geometry: padded sequence [P, P + PLEN), background interval [S, E)."""
    P, PLEN, S, E = 100_000, 20_000, 105_000, 115_000
    refs = [("chrA", 1_000_000), ("chrB", 1_000_000)]
    F1, F2 = 0x1 | 0x40, 0x1 | 0x80

    def __init__(self):
        P, S, E, F1, F2 = self.P, self.S, self.E, self.F1, self.F2
        PE = P + self.PLEN
        r = []
        k = [0]

        def add(pos, name, cigar, seq=None, mapq=60, flag=F1, tid=0):
            if seq is None:
                k[0] += 1
                seq = seq_of(sum(n for o, n in cigar if o in "MIS=X"), 100 + k[0])
            r.append((tid, pos, name, mapq, flag, cigar, seq))
        m150 = [("M", 150)]
        # one flag each
        for j, f in enumerate((0x4, 0x100, 0x200, 0x400, 0x800)):
            add(S + 100 + j, f"flag{f:x}", m150, flag=F1 | f)
        add(S + 200, "mapq29", m150, mapq=29)
        add(S + 201, "mapq30", m150, mapq=30)
        add(S + 210, "clip3", [("S", 3), ("M", 147)])
        add(S + 211, "clip4", [("S", 4), ("M", 146)])
        add(S + 220, "lead_ins", [("I", 2), ("M", 148)])
        add(S + 230, "all_soft", [("S", 150)])
        # bg_synth's edge records
        d = PE - (E - 100) - 200
        add(E - 100, "edge_drop_end", [("M", 100), ("D", d), ("M", 100)])
        add(E - 100, "edge_keep_end", [("M", 100), ("D", d - 1), ("M", 100)])
        add(P - 100, "edge_drop_start", [("M", 100), ("D", S - P + 50), ("M", 100)])
        add(E - 60, "edge_eqx", [("=", 60), ("D", d), ("=", 40)])
        # the interval's ends
        add(E - 1, "pos_last", m150)
        add(E, "pos_end", m150)
        add(S - 150, "end_at_start", m150)
        add(S - 149, "end_past_start", m150)
        add(S - 1, "noref_before", [("I", 10)])
        add(S, "noref_at", [("I", 10)])
        # what is dropped or filtered is not looked at any further
        add(E - 100, "dropped_with_n", [("M", 100), ("N", d), ("M", 100)])
        add(S + 300, "filtered_with_h", [("H", 2), ("M", 150)], mapq=10)
        # long CIGARs: the wavefront's path
        add(S + 1000, "ops200", [("M", 2), ("I", 1), ("M", 2), ("D", 1)] * 50)
        add(E - 10, "ops130_cross", [("M", 1), ("I", 1)] * 35 + [("M", 6000)] + [("I", 1), ("M", 1)] * 29 + [("I", 1)])
        for n in (1, 31, 32, 33, 64, 65, 151):
            add(S + 2000 + n, f"len{n}", [("M", n)])
        add(S + 2300, "rev151", [("M", 151)], flag=F1 | 0x10)
        add(S + 2301, "rev64", [("M", 64)], flag=F1 | 0x10)
        add(S + 2400, "codes", [("M", 40)], seq=b"ACGT=NRACGTNN==RYACGTACGTACGTMKACGTACGTN")
        add(S + 2401, "codes_rev", [("M", 33)], seq=b"=NRACGTACGTACGTACGTACGTACGTACGTAN", flag=F1 | 0x10)
        for n in (1, 3, 4, 5, 254):
            add(S + 2500 + n, "n" * n, m150)
        pre = "q" * 250
        for nm, at in ((pre + "a", S + 3000), (pre + "b", S + 3001)):
            add(at, nm, m150, flag=F1)
            add(at + 300, nm, m150, flag=F2 | 0x10)
        for tid in (0, 1):
            add(S + 4000, "full", m150, flag=F1, tid=tid)
            add(S + 4300, "full", m150, flag=F2 | 0x10, tid=tid)
            add(S + 4400, "mate_mapq", m150, flag=F1, tid=tid)
            add(S + 4700, "mate_mapq", m150, flag=F2 | 0x10, mapq=5, tid=tid)
            add(E - 200, "mate_outside", m150, flag=F1, tid=tid)
            add(E + 1000, "mate_outside", m150, flag=F2 | 0x10, tid=tid)
        add(S + 5000, "only_b", [("M", 77)], tid=1)
        self.records = by_coordinate(r)
        self.padded_seq = seq_of(self.PLEN, 1)

    def good_pairs(self, n=4):
        """a few clean pairs inside the interval: the company of an offending record"""
        out = []
        for i in range(n):
            out.append((0, self.S + 500 + 10 * i, f"ok{i}", 60, self.F1, [("M", 150)], seq_of(150, i)))
            out.append((0, self.S + 800 + 10 * i, f"ok{i}", 60, self.F2 | 0x10, [("M", 150)], seq_of(150, 50 + i)))
        return out
