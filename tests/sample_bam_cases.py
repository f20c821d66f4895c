"""The BAM files of the sample-BAM tests (tests/test_sample_bam_host.py, tests/test_gpu_sample_bam*.py), written with
tests/pyref_sample_bam.py: a hand-made file whose answer is derived by hand, and a seeded one with everything the fetch must tell apart."""
import numpy as np

from tests import pyref_sample_bam as P

HAND_REFS = [("chrA", 100_000), ("chrB", 50_000)]
HAND_REGIONS = [(0, 1000, 2000), (0, 2000, 3000), (1, 0, 500)]
# by hand (see hand_records): the fetched stream, the pairs in the order of their completing records, the discarded records
HAND_STREAM = [2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 17]
HAND_PAIRS = [(2, 5), (7, 8), (6, 9), (10, 13), (15, 16)]
HAND_DISCARDED = 3


def _seq(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


def hand_records():
    rng = np.random.default_rng(1)
    M = [("M", 100)]
    s = lambda: _seq(rng, 100)
    q = lambda: bytes(rng.integers(2, 41, 100).tolist())
    R = P.rec
    return [
        R(0, 800, "a", 0x41, M, s(), q(), 0, 1200),            # 0  ends at 900 <= 1000: not fetched
        R(0, 900, "s", 0x41, M, s(), q(), 0, 5000),            # 1  ends exactly at the region's start: not fetched
        R(0, 950, "b", 0x41, M, s(), q(), 0, 1300),            # 2  starts before the region, reaches into it; waits
        R(0, 1000, "b", 0x141, M, s(), q(), 0, 1300),          # 3  secondary
        R(0, 1200, "a", 0x81, M, s(), q(), 0, 800),            # 4  its mate was never fetched and lies before it: discarded
        R(0, 1300, "b", 0x91, M, s(), q(), 0, 950),            # 5  completes (2, 5); reverse
        R(0, 1950, "c", 0x41, M, s(), q(), 0, 2500),           # 6  region 0 takes it; region 1 sees pos < min_start = 2000
        R(0, 2100, "d", 0x45, [], s(), q(), 0, 2100),          # 7  unmapped flag, placed at its mate: end = pos + 1; (2100) <= (2100) waits
        R(0, 2100, "d", 0x89, M, s(), None, 0, 2100),          # 8  completes (7, 8): mate 1 is the one with 0x40; no qualities
        R(0, 2500, "c", 0x81, M, s(), q(), 0, 1950),           # 9  completes (6, 9)
        R(0, 2600, "e", 0x41, M, s(), q(), 1, 100),            # 10 mate on a later contig: waits
        R(0, 2800, "c", 0x41, M, s(), q(), 0, 2900),           # 11 a third record of a name starts over: waits, discarded at the end
        R(0, 3000, "x", 0x41, M, s(), q(), 0, 3100),           # 12 pos == end of the region: not fetched
        R(1, 100, "e", 0x81, M, s(), q(), 0, 2600),            # 13 completes (10, 13)
        R(1, 600, "f", 0x41, M, s(), q(), 1, 900),             # 14 outside every region
        R(-1, -1, "g", 0x4d, [], s(), q(), -1, -1),            # 15 no coordinate: (-1 as u32, -1 as u64) <= the same: waits
        R(-1, -1, "g", 0x8d, [], s(), q(), -1, -1),            # 16 completes (15, 16)
        R(-1, -1, "h", 0x4d, [], s(), q(), -1, -1),            # 17 waits, discarded at the end
        R(-1, -1, "h", 0x88d, [], s(), q(), -1, -1),           # 18 supplementary
    ]


SEEDED_REFS = [("c0", 200_000), ("c1", 150_000), ("c2", 3_000)]
# two adjacent regions on c0, a third further on, one on c1, and the short contig as a whole
SEEDED_REGIONS = [(0, 10_000, 14_000), (0, 14_000, 18_000), (0, 60_000, 64_000), (1, 20_000, 26_000), (2, 0, 3_000)]


def seeded_records(seed=3, n_pairs=1200, loci=None, n_tail=60):
    """Pairs of 100-base reads with inserts of 250 - 450 on and around SEEDED_REGIONS (mates left and right of every region border, foreign
    records between the regions), single secondary / supplementary copies, reads with other BAM codes, pairs whose second mate has the
    unmapped flag and is placed at its mate, pairs without coordinate. loci: [[allele bytes]]: every third pair is drawn from an allele."""
    rng = np.random.default_rng(seed)
    recs = []
    spans = [(0, 9_000, 19_000), (0, 59_000, 65_000), (1, 19_000, 27_000), (2, 0, 2_500), (0, 30_000, 40_000), (1, 90_000, 95_000)]

    def pair_seqs(i):
        if loci is not None and i % 3 == 0:
            al = loci[i % len(loci)][int(rng.integers(0, len(loci[i % len(loci)])))]
            p = int(rng.integers(0, len(al) - 450))
            s1 = al[p:p + 100].decode()
            s2 = "".join(P.complement_nt(c) for c in reversed(al[p + 300:p + 400].decode()))
            return s1, s2
        return _seq(rng, 100), _seq(rng, 100)

    def stored(seq, reverse):
        return "".join(P.complement_nt(c) for c in reversed(seq)) if reverse else seq

    for i in range(n_pairs):
        t, lo, hi = spans[int(rng.integers(0, len(spans)))]
        ins = int(rng.integers(250, 450))
        p1 = int(rng.integers(lo, hi))
        p2 = min(p1 + ins - 100, SEEDED_REFS[t][1] - 100)
        s1, s2 = pair_seqs(i)
        if i % 11 == 0:                                       # other codes: N, IUPAC letters, '='
            k = int(rng.integers(0, 100))
            s1 = s1[:k] + "NRYKMSWBDHV="[(i // 11) % 12] + s1[k + 1:]
        first_rev = bool(rng.integers(0, 2))
        name = f"p{i}"
        q1, q2 = bytes(rng.integers(2, 41, 100).tolist()), bytes(rng.integers(2, 41, 100).tolist())
        if i % 13 == 5:                                       # the second mate unmapped, placed at the first
            recs.append(P.rec(t, p1, name, 0x49 | (0x10 if first_rev else 0), [("M", 100)], stored(s1, first_rev), q1, t, p1))
            recs.append(P.rec(t, p1, name, 0x85 | (0x20 if first_rev else 0), [], s2, q2, t, p1))
            continue
        c1 = [("M", 100)] if i % 5 else [("S", 10), ("M", 40), ("D", 7), ("M", 30), ("I", 5), ("M", 15)]
        recs.append(P.rec(t, p1, name, 0x41 | (0x10 if first_rev else 0x20), c1, stored(s1, first_rev), q1, t, p2))
        recs.append(P.rec(t, p2, name, 0x81 | (0x20 if first_rev else 0x10), [("M", 100)], stored(s2, not first_rev), q2, t, p1))
        if i % 17 == 0:
            recs.append(P.rec(t, p1 + 3, name, 0x141, [("M", 100)], s1, None, t, p2))          # secondary
        if i % 19 == 0:
            recs.append(P.rec(t, max(p2 - 2, 0), name, 0x881, [("H", 60), ("M", 40)], s2[:40], None, t, p1))   # supplementary
    order = sorted(range(len(recs)), key=lambda j: (recs[j]["tid"], recs[j]["pos"]))
    recs = [recs[j] for j in order]
    for i in range(n_tail):
        name = f"u{i}"
        recs.append(P.rec(-1, -1, name, 0x4d, [], _seq(rng, 100), bytes(rng.integers(2, 41, 100).tolist())))
        recs.append(P.rec(-1, -1, name, 0x8d, [], _seq(rng, 100), bytes(rng.integers(2, 41, 100).tolist())))
        if i % 9 == 0:
            recs.append(P.rec(-1, -1, name, 0x98d, [], _seq(rng, 30), None))
    return recs


def expected(records, regions, with_unmapped=True, paired=True, whole_file=False):
    """The restatement's answer: (src [2 n]: every mate's ordinal in the fetched stream, or 0xFFFFFFFF; mates [[seq, seq or None]];
    records kept; records discarded)"""
    stream = P.fetched_stream(records, regions, with_unmapped, whole_file)
    if paired:
        pairs, discarded = P.pairs_of(records, stream)
    else:
        pairs, discarded = [(j, None) for j in stream], 0
    at = {j: k for k, j in enumerate(stream)}
    src = np.array([0xFFFFFFFF if j is None else at[j] for pr in pairs for j in pr], dtype=np.uint32)
    mates = [[None if j is None else P.restored(records[j]) for j in pr] for pr in pairs]
    return src, mates, len(stream), discarded
