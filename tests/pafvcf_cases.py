"""Inputs of `locityper paf-vcf` for tests/test_pafvcf_host.py and tests/test_gpu_pafvcf.py: a reference haplotype, haplotypes made from it
by planted edits, and the TRUE CIGAR of every haplotype (no aligner: the items are the edits). Seeded; nothing is drawn and thrown away."""
import numpy as np

BASES = b"ACGT"
OPS = {b"M": 0, b"I": 1, b"D": 2, b"S": 4, b"H": 5, b"=": 7, b"X": 8}


def random_seq(rng, n):
    return bytes(np.frombuffer(BASES, dtype=np.uint8)[rng.integers(0, 4, n)])


def repetitive_ref(rng, n, repeat_share=0.3):
    """random bases with homopolymers (5-20) and tandem repeats (unit 2-4, 3-8 copies) over about repeat_share of the length, so that
    planted indels fall into them and the left shift has something to do"""
    out = bytearray()
    while len(out) < n:
        if rng.random() < repeat_share / 6:
            if rng.random() < 0.5:
                out += BASES[rng.integers(0, 4):][:1] * int(rng.integers(5, 21))
            else:
                out += random_seq(rng, int(rng.integers(2, 5))) * int(rng.integers(3, 9))
        else:
            out += random_seq(rng, int(rng.integers(1, 12)))
    return bytes(out[:n])


def words(cigar):
    """[(op, len)] -> the CIGAR words of lcty_paf_read (len << 4 | BAM operation)"""
    return np.array([(n << 4) | OPS[op] for op, n in cigar], dtype=np.uint32)


def invert(cigar):
    return [({b"I": b"D", b"D": b"I"}.get(op, op), n) for op, n in cigar]


def plan_ops(rng, n_items, run_rate, indel_at_0, no_quirk):
    """the operations of a CIGAR of exactly n_items items: '=' and edits alternate, and with probability run_rate an '=' between two
    edits is replaced by an edit of another kind (runs of adjacent X / I / D); no two neighbours are equal"""
    if n_items == 0:
        return []
    if n_items == 1:
        return [b"="]
    ops = []
    for i in range(n_items):
        prev = ops[-1] if ops else None
        if i == 0:
            op = (b"I", b"D")[int(rng.integers(0, 2))] if indel_at_0 else b"="
        elif prev == b"=":
            op = (b"X", b"I", b"D")[int(rng.integers(0, 3))]
        elif i + 1 < n_items and rng.random() < run_rate:
            op = [o for o in (b"X", b"I", b"D") if o != prev][int(rng.integers(0, 2))]
        else:
            op = b"="
        if no_quirk and i == 1 and {ops[0], op} == {b"I", b"D"}:
            op = b"X"
        ops.append(op)
    return ops


def make_haplotype(rng, ref, n_items, run_rate=0.2, indel_at_0=False, no_quirk=False, long_edit=0, n_rate=0.0):
    """(sequence, true CIGAR) of exactly n_items items (0: the reference itself and an EMPTY CIGAR, which process_paf skips for its lengths)"""
    if n_items == 0:
        return ref, []
    ops = plan_ops(rng, n_items, run_rate, indel_at_0, no_quirk)
    lens = [0] * len(ops)
    for i, op in enumerate(ops):
        if op != b"=":
            lens[i] = int(rng.integers(1, 4)) if rng.random() < 0.9 else int(rng.integers(4, 30))
    edits = [i for i, op in enumerate(ops) if op != b"="]
    if long_edit and edits:                       # one long INSERTION (a substitution or deletion of that length needs a reference as long)
        i = next((i for i in edits if ops[i] == b"I"), None)
        if i is None:
            i = next(i for i in edits if b"I" not in (ops[i - 1] if i else b"", ops[i + 1] if i + 1 < len(ops) else b""))
            ops[i] = b"I"
        lens[i] = long_edit
    used = sum(n for op, n in zip(ops, lens) if op in (b"X", b"D"))
    eq = [i for i, op in enumerate(ops) if op == b"="]
    rest = len(ref) - used
    assert rest >= len(eq) and (eq or rest == 0), "the reference is too short for this many items"
    # a random composition of `rest` into len(eq) positive parts
    cuts = np.sort(rng.choice(np.arange(1, rest), size=len(eq) - 1, replace=False)) if len(eq) > 1 else np.zeros(0, dtype=np.int64)
    for i, n in zip(eq, np.diff(np.concatenate([[0], cuts, [rest]]))):
        lens[i] = int(n)
    out = bytearray()
    rpos = 0
    for op, n in zip(ops, lens):
        if op == b"=":
            out += ref[rpos:rpos + n]
            rpos += n
        elif op == b"X":
            for c in ref[rpos:rpos + n]:
                out.append(ord("N") if rng.random() < n_rate else [b for b in BASES if b != c][int(rng.integers(0, 3))] if c in BASES else BASES[0])
            rpos += n
        elif op == b"D":
            rpos += n
        else:                       # an insertion: half of them copy what stands in front of them, so that they can move left
            if rpos >= n and rng.random() < 0.5:
                out += ref[rpos - n:rpos]
            else:
                out += random_seq(rng, n)
    assert rpos == len(ref)
    return bytes(out), list(zip(ops, lens))


def make_case(seed, n_haps, ref_len, n_items, run_rate=0.2, indel_at_0_rate=0.1, n_rate=0.0, missing_rate=0.0, as_query_rate=0.3, dup_rate=0.1,
              round_trip=False, long_edit=0, ref_n=0):
    """names, seqs, entries [(query id, target id, [(op, len)])], the name of the reference haplotype. n_items: one number or a list the
    haplotypes cycle through. round_trip: what the identity through lcty_panvcf_reconstruct needs — every haplotype with an entry, no N,
    no CIGAR that starts with gaps of two kinds, samples with all their haplotypes."""
    rng = np.random.default_rng(seed)
    ref = bytearray(repetitive_ref(rng, ref_len))
    if not round_trip:
        for p in rng.integers(0, ref_len, ref_n):
            ref[int(p)] = ord("N")
    ref = bytes(ref)
    items = list(n_items) if isinstance(n_items, (list, tuple)) else [n_items]
    names, seqs, entries = [b"ref"], [ref], []
    for h in range(n_haps):
        k = items[h % len(items)]
        if round_trip and k == 0:
            k = 1
        seq, cigar = make_haplotype(rng, ref, k, run_rate, indel_at_0=k >= 2 and rng.random() < indel_at_0_rate, no_quirk=round_trip, long_edit=long_edit,
                                    n_rate=0.0 if round_trip else n_rate)
        # samples: pairs S<i>.1 / S<i>.2 (the last may lack its second haplotype), `_` suffixes and haploid names in between
        pair, slot = divmod(h, 2)
        if round_trip:
            name = b"S%d.%d" % (pair, slot + 1) if (h | 1) < n_haps else b"H%d" % pair
        else:
            name = b"H%d" % pair if pair % 5 == 4 and slot == 0 else b"S%d%s%d" % (pair, b"_" if pair % 3 == 2 else b".", slot + 1)
            if pair % 5 == 4 and slot == 1:
                name = b"G%d" % pair
        names.append(name)
        seqs.append(seq)
        hid = h + 1
        if not round_trip and rng.random() < missing_rate:
            continue
        if not round_trip and cigar and rng.random() < dup_rate:
            # an earlier entry for the same haplotype that the true one replaces: substitutions over the common length, then one gap
            m = min(len(seq), len(ref))
            alt = [(b"X", m)] + ([(b"I", len(seq) - m)] if len(seq) > m else []) + ([(b"D", len(ref) - m)] if len(ref) > m else [])
            entries.append((hid, 0, alt))
        if rng.random() < as_query_rate:
            entries.append((0, hid, invert(cigar)))
        else:
            entries.append((hid, 0, cigar))
        if not round_trip and cigar and rng.random() < dup_rate:
            entries.append((hid, 0, cigar + [(b"=", 1)]))          # a later entry of the wrong length: skipped and counted
    return names, seqs, entries, b"ref"


def flat(seqs):
    """(concatenated u8, seq_off[n + 1])"""
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:-1].copy() if off[-1] else np.zeros(0, dtype=np.uint8), off


def api_entries(entries):
    """the entries as io.paf_read gives them: (id1 query, id2 target, CIGAR words)"""
    return [(q, t, words(c)) for q, t, c in entries]
