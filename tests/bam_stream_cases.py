"""Inputs of the reader of whole BAM files in windows (lcty_bam_stream_*), shared by tests/test_bam_stream_host.py (the host
half under the sanitizers) and tests/test_gpu_bam_stream.py: designed record lists, malformed records, and the files they become."""
import struct

import numpy as np

from tests import pyref_sample_bam as SB

REFS = [("chr1", 100_000)]
LENS = [1, 31, 32, 33, 63, 64, 65, 255, 300]


def seq_of(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=n)) if n else ""


def unaligned(name, flag, seq, qual=True):
    return SB.rec(-1, -1, name, flag | 4, [], seq, bytes((i * 7) % 40 + 2 for i in range(len(seq))) if qual else None)


def blob(r):
    """the bytes of a record; "short": l_seq says more than the record holds; "cut": the record without its last five bytes"""
    b = SB.record_bytes(r)
    if r.get("bad") == "short":
        return b[:20] + struct.pack("<I", len(r["seq"]) + 1000) + b[24:]
    if r.get("bad") == "cut":
        return b[:-5]
    return b


def write_files(tmp, name, files, block_size=0xff00):
    """files: [[record]] -> the paths of name.<i>.bam, written without an index"""
    paths = []
    for i, recs in enumerate(files):
        p = str(tmp / f"{name}.{i}.bam")
        SB.write_bam(p, REFS, recs, block_size=block_size, index=False, raw_records=[blob(r) for r in recs])
        paths.append(p)
    return paths


def single_end_records():
    """24 records: primaries of every length at which unpack takes another turn, one of 5 000 bases, reverse ones, IUPAC and '=' codes,
    0x100 and 0x800 records between them"""
    rng = np.random.default_rng(5)
    recs = []
    for i, n in enumerate(LENS + [5000]):
        flag = 0x10 if i % 3 == 1 else 0
        recs.append(unaligned(f"read{i}", flag, seq_of(rng, n), qual=i % 4 != 2))
    recs.insert(2, unaligned("read1", 0x100, seq_of(rng, 40)))
    recs.insert(5, unaligned("read3", 0x800 | 0x10, seq_of(rng, 77)))
    recs.append(unaligned("iupac", 0, "ACGTNRYKM=SWBDHVACGTNNA"))
    recs.append(unaligned("iupac-rev", 0x10, "=ACMGRSVTWYHKDBNACGTTTGCA" * 3))
    recs.append(SB.rec(0, 1000, "mapped", 0x10, [("M", 37)], seq_of(rng, 37), bytes([30] * 37)))
    recs.append(SB.rec(0, 1000, "placeholder", 0, [("S", 45), ("N", 10)], seq_of(rng, 45), None))          # a kSmN CIGAR is no error here
    recs.append(unaligned("sup-last", 0x800, seq_of(rng, 10)))
    for i, n in enumerate((129, 2, 97, 160, 47, 1, 640)):
        recs.append(unaligned(f"tail{i}", 0x10 if i & 1 else 0, seq_of(rng, n, "ACGTN")))
    assert len(recs) == 24
    return recs


def interleaved_records(n_pairs, length=150, seed=11, between=10, behind=20):
    """n_pairs name-grouped pairs; every `between`-th has a 0x800 or 0x100 record between its mates, every `behind`-th one behind them"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n_pairs):
        a = unaligned(f"p{i}/1", 0x41 | (0x10 if i % 5 == 0 else 0), seq_of(rng, length, "ACGTN" if i % 7 == 0 else "ACGT"))
        b = unaligned(f"p{i}/2", 0x81 | (0x10 if i % 3 == 0 else 0), seq_of(rng, length))
        recs.append(a)
        if between and i % between == 0:
            recs.append(unaligned(f"p{i}/1", 0x800 if i % (2 * between) else 0x100, seq_of(rng, 30)))
        recs.append(b)
        if behind and i % behind == 0:
            recs.append(unaligned(f"p{i}/2", 0x800, seq_of(rng, 20)))
    return recs


def pair(name_a, name_b, n=20, seed=3):
    rng = np.random.default_rng(seed)
    return [unaligned(name_a, 0x41, seq_of(rng, n)), unaligned(name_b, 0x81, seq_of(rng, n))]


def three_files():
    """file 1 ends with a first mate and a supplementary record, file 2 is a header alone, file 3 begins with a secondary record and
    then the second mate: one pair across the files, behind two ordinary ones and in front of one"""
    rng = np.random.default_rng(9)
    f1 = pair("a/1", "a/2", 40, 1) + pair("b/1", "b/2", 33, 2) + [unaligned("c/1", 0x41, seq_of(rng, 50)), unaligned("c/1", 0x800, seq_of(rng, 12))]
    f3 = [unaligned("c/2", 0x100, seq_of(rng, 9)), unaligned("c/2", 0x91, seq_of(rng, 64))] + pair("d/1", "d/2", 65, 4)
    return [f1, [], f3]


def error_cases():
    """name -> (files, interleaved): good pairs in front of the offending record"""
    rng = np.random.default_rng(21)
    front = interleaved_records(70, length=40, seed=2, between=9, behind=13)
    bad = lambda name, flag, what, n=30: dict(unaligned(name, flag, seq_of(rng, n)), bad=what)
    return {
        "odd": ([front + [unaligned("alone/1", 0x41, seq_of(rng, 25))]], True),
        "odd-two-files": ([front, [unaligned("alone/1", 0x41, seq_of(rng, 25)), unaligned("alone/1", 0x800, seq_of(rng, 5))]], True),
        "noseq-first": ([front + [unaligned("empty/1", 0x41, "")] + pair("z/1", "z/2")], True),
        "noseq-second": ([front + [unaligned("e/1", 0x41, seq_of(rng, 8)), unaligned("e/2", 0x81, "")] + pair("z/1", "z/2")], True),
        "noseq-single": ([front + [unaligned("empty", 0, "")] + pair("z/1", "z/2")], False),
        "noseq-dropped": ([front + [unaligned("empty", 0x800, "")] + pair("z/1", "z/2")], True),                  # not kept: no error
        "short": ([front + [bad("s/1", 0x41, "short")] + pair("z/1", "z/2")], True),
        "short-dropped": ([front + [bad("s/1", 0x900, "short")] + pair("z/1", "z/2")], True),                     # an error whatever its flags
        "cut": ([front, pair("y/1", "y/2") + [bad("cut/1", 0x41, "cut", 90)], pair("z/1", "z/2")], True),
        "mismatch-len": ([front + pair("abcd", "abcde") + pair("z/1", "z/2")], True),
        "mismatch-byte": ([front + pair("abcd", "aXcd") + pair("z/1", "z/2")], True),
        "mismatch-then-noseq": ([front + pair("abcd", "aXcd") + [unaligned("empty/1", 0x41, "")]], True),
        "noseq-then-mismatch": ([front + [unaligned("empty/1", 0x41, "")] + pair("abcd", "aXcd")], True),
        "names-pass": ([pair("r/1", "r/2") + pair("abc", "xyz") + pair("abcd", "xbzz") + pair("", "") + pair("q", "p")], True),
    }


def corpus():
    """name -> (files, interleaved), the valid cases and the refused ones"""
    cases = {
        "single": ([single_end_records()], False),
        "single-two-files": ([single_end_records()[:11], single_end_records()[11:]], False),
        "pairs": ([interleaved_records(300)], True),
        "pairs-129": ([interleaved_records(129, between=0, behind=0)], True),
        "three-files": (three_files(), True),
        "empty": ([[], []], True),
    }
    cases.update(error_cases())
    return cases


def write_corpus(tmp, block_sizes=(64, 200, 0xff00)):
    """Every case of corpus() at every block size -> tmp/corpus.tsv (name, interleaved, paths joined by ','), and [(name, files,
    interleaved, paths)]"""
    out = []
    with open(tmp / "corpus.tsv", "w") as f:
        for name, (files, interleaved) in corpus().items():
            for bsz in block_sizes:
                paths = write_files(tmp, f"{name}.b{bsz}", files, bsz)
                f.write(f"{name}.b{bsz}\t{int(interleaved)}\t{','.join(paths)}\n")
                out.append((f"{name}.b{bsz}", files, interleaved, paths))
    return out
