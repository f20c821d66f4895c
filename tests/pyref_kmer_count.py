"""Genome k-mer counts as DESIGN.md 5m defines them (this build's statement of `jellyfish count -C` + `jellyfish query` as
JfKmerGetter::fetch uses them), restated serially: a dictionary of the canonical k-mers of the genome. No device, no library.

Genome: named contigs; A C G T a c g t are the bases (case folded); every other letter seq::standardize accepts is "not a base";
any other byte is an error. A k-mer occurrence is k consecutive bases of one contig. count(x) = occurrences whose canonical form
(the smaller of the forward and the reverse-complement value) equals canonical(x). A query value is max(min(count, max_value), 1)."""
import numpy as np

BASES = {ord(c): i for i, c in enumerate("ACGT")}
BASES.update({ord(c): i for i, c in enumerate("acgt")})
NOT_A_BASE = set(b"NRYKMSWBDHVnrykmswbdhv")


class GenomeByteError(ValueError):
    def __init__(self, contig, pos, byte):
        super().__init__(f"contig {contig}: byte {byte:#04x} at position {pos} is not a nucleotide")
        self.contig, self.pos, self.byte = contig, pos, byte


def canonical_kmers(seq, k, enc):
    """(start, canonical k-mer) for every window of k consecutive bytes of seq that `enc` maps to a base."""
    mask = (1 << (2 * k)) - 1
    shift = 2 * k - 2
    fw = rv = 0
    valid = 0
    for i, c in enumerate(seq):
        e = enc.get(c)
        if e is None:
            valid = 0
            continue
        fw = ((fw << 2) | e) & mask
        rv = (rv >> 2) | ((3 - e) << shift)
        valid += 1
        if valid >= k:
            yield i + 1 - k, min(fw, rv)


def check_genome(contigs):
    for ci, (name, seq) in enumerate(contigs):
        for p, c in enumerate(seq):
            if c not in BASES and c not in NOT_A_BASE:
                raise GenomeByteError(name, p, c)


def genome_table(contigs, k):
    """contigs: [(name, bytes)] -> {canonical k-mer: occurrences}"""
    check_genome(contigs)
    table = {}
    for _, seq in contigs:
        for _, km in canonical_kmers(seq, k, BASES):
            table[km] = table.get(km, 0) + 1
    return table


def max_value(counter_bytes):
    return 65535 if counter_bytes >= 2 else (1 << (8 * counter_bytes)) - 1


UPPER = {ord(c): i for i, c in enumerate("ACGT")}


def query(table, seqs, k, counter_bytes=2):
    """One u16 array of max(len + 1 - k, 0) values per sequence."""
    out = []
    mx = max_value(counter_bytes)
    for s in seqs:
        if b"N" in s:
            raise RuntimeError("Cannot count k-mers for sequence with Ns")
        if any(c not in UPPER for c in s):
            raise ValueError("a query sequence holds a byte outside A, C, G, T")
        vals = np.ones(max(len(s) + 1 - k, 0), dtype=np.uint16)
        for p, km in canonical_kmers(s, k, UPPER):
            vals[p] = max(min(table.get(km, 0), mx), 1)
        out.append(vals)
    return out


def kmer_counts(contigs, seqs, k, counter_bytes=2):
    return query(genome_table(contigs, k), seqs, k, counter_bytes)


def standardize(seq):
    """What fetch_seq + standardize leave of a contig: capitals A C G T, N for everything else."""
    return bytes(b"ACGT"[BASES[c]] if c in BASES else ord("N") for c in seq)


def fill_n(seq):
    """The reference record as process_alleles counts it: every N replaced with A."""
    return seq.replace(b"N", b"A")
