"""Serial Python restatement of the basis step of `locityper augment` (src/command/augment.rs:258-348, src/seq/cigar.rs:656-751,
src/algo/dom_set.rs): the loops as the reference writes them, one CIGAR item at a time. Nothing here shares a closed form with
locityper_amd/csrc/lcty_basis.hip: the kernel takes prefix sums and bisects, this file walks.

A CIGAR is a list of (op, len) with op one of "=XIDM"; an entry is (query id, target id, raw BAM CIGAR words, n_matches, aln_len), what
SynthLocus.hap_alns() returns and lcty_paf_read parses."""
import itertools
import math
import re

OPS = "MIDNSHP=X"
U32_MAX = 2 ** 32 - 1


def parse_cigar(text):
    return [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def cigar_words(cigar):
    return [(n << 4) | OPS.index(op) for op, n in cigar]


def words_cigar(words):
    return [(OPS[int(w) & 15], int(w) >> 4) for w in words]


def consumes_query(op):
    return op in "M=XIS"


def consumes_ref(op):
    return op in "M=XD"


def query_len(cigar):
    return sum(n for op, n in cigar if consumes_query(op))


def ref_len(cigar):
    return sum(n for op, n in cigar if consumes_ref(op))


def locally_similar(cigar, in_query, window, step, max_edit):
    """Cigar::locally_similar::<IN_QUERY> (cigar.rs:660-751): the window indices it pushes, in its order (an index may repeat)."""
    moves = consumes_query if in_query else consumes_ref
    indices = []
    pos2 = 0
    iter2 = iter(cigar)
    edit = 0
    while True:
        item = next(iter2, None)
        if item is None:
            if edit <= max_edit:
                indices.append(0)
            return indices
        op, ln = item
        if moves(op):
            window_rem = window - pos2
            shift = min(ln, window_rem)
            edit += shift if op != "=" else 0
            pos2 += shift
            if ln > window_rem:
                rem2, op2 = ln - window_rem, op
                break
        else:
            edit += ln

    iter1 = iter(cigar)
    op1, rem1 = next(iter1)
    pos1 = 0
    while True:
        shift = min(rem1, rem2)
        moves1, moves2 = moves(op1), moves(op2)
        upd1 = (moves1 == moves2) or not moves1
        upd2 = (moves1 == moves2) or not moves2
        if moves1 and moves2:
            m1 = op1 != "="
            m2 = op2 != "="
            next_saved = pos1 + (-pos1) % step
            for pos in range(next_saved, pos1 + shift, step):
                cs = pos - pos1
                if edit + (cs if m2 else 0) - (cs if m1 else 0) <= max_edit:
                    indices.append(pos // step)
            pos1 += shift
            pos2 += shift
            edit = edit + (shift if m2 else 0) - (shift if m1 else 0)
        else:
            edit = edit + (shift if upd2 else 0) - (shift if upd1 else 0)
        assert edit >= 0
        if upd2:
            if shift == rem2:
                item = next(iter2, None)
                if item is None:
                    break
                op2, rem2 = item
            else:
                rem2 -= shift
        if upd1:
            if shift == rem1:
                op1, rem1 = next(iter1)           # "Left iterator could not overtake the right one"
            else:
                rem1 -= shift
    if edit <= max_edit:
        indices.append(-(-pos1 // step))
    assert pos1 + window == pos2
    assert pos2 == (query_len(cigar) if in_query else ref_len(cigar))
    return indices


def global_div(n_matches, aln_len):
    """PafEntry::divergence().unwrap_or(1.0) (paf.rs:201-208, augment.rs:336)"""
    return 1.0 if aln_len == 0 else (aln_len - n_matches) / aln_len


def update_bitarray(cigar, in_query, gdiv, window, step, max_window_edit, divergence):
    """update_bitarray (augment.rs:291-312): the windows of this side whose bit is set."""
    ln = query_len(cigar) if in_query else ref_len(cigar)
    if ln <= window:
        return [0] if gdiv <= divergence else []
    return locally_similar(cigar, in_query, window, step, max_window_edit)


def resolve(divergence, window, step):
    """(max_window_edit, step) of augment.rs:319-320; step None or 0 = not given"""
    return int(math.floor(window * divergence)), (step if step else max(window >> 1, 1))


def n_windows(length, window, step):
    """augment.rs:323; a contig not longer than the window has one window (there the reference's u32 subtraction underflows)"""
    return 1 if length <= window else -(-(length - window) // step) + 1


def row_table(lengths, entries, divergence=0.01, window=250, step=None, leave_out=()):
    """inner_construct_dominant_set up to line 339: rows[contig][window] = set of contig ids (the BitArray as a Python int).
    Entries naming a left-out contig are skipped (the reference builds the subset first, so the PAF reader drops them); left-out
    contigs have no rows. Ids stay those of the full set."""
    mwe, st = resolve(divergence, window, step)
    out = set(leave_out)
    rows = [[] if i in out else [1 << i] * n_windows(l, window, st) for i, l in enumerate(lengths)]
    for q, t, words, nm, al in entries:
        if q == t or q in out or t in out or len(words) == 0:
            continue
        cigar = words_cigar(words)
        gd = global_div(nm, al)
        for w in update_bitarray(cigar, True, gd, window, st, mwe, divergence):
            rows[q][w] |= 1 << t
        for w in update_bitarray(cigar, False, gd, window, st, mwe, divergence):
            rows[t][w] |= 1 << q
    return rows


def unique_rows(rows):
    """the HashSet of augment.rs:341-344"""
    return {r for contig in rows for r in contig}


def minimal_rows(uniq):
    """rows that have no proper subset among the rows: the presolve of lcty_basis_constraints (not the reference's)"""
    return {r for r in uniq if not any(o != r and (o & r) == o for o in uniq)}


def is_cover(chosen, uniq):
    mask = sum(1 << int(i) for i in chosen)
    return all(r & mask for r in uniq)


def greedy_cover(n, uniq):
    """the textbook greedy: the id in most uncovered rows, lowest id on ties"""
    left = list(uniq)
    chosen = []
    while left:
        best = max(range(n), key=lambda i: (sum(1 for r in left if r >> i & 1), -i))
        chosen.append(best)
        left = [r for r in left if not r >> best & 1]
    return sorted(chosen)


def brute_force_min(n, uniq):
    """size of a minimum hitting set by enumeration, n <= 20"""
    assert n <= 20
    rows = list(minimal_rows(uniq))
    for size in range(0, n + 1):
        for comb in itertools.combinations(range(n), size):
            mask = sum(1 << i for i in comb)
            if all(r & mask for r in rows):
                return size
    raise AssertionError("an empty row cannot be hit")


def num_digits(x):
    return int(math.floor(math.log10(abs(x)))) + 1


def fmt_signif(x, digits):
    """math::fmt_signif (src/math/mod.rs:159-174)"""
    if x == 0.0:
        return "0"
    shift = num_digits(x) - digits
    fct = 10.0 ** shift
    if shift < 0:
        s = "%.*f" % (-shift, x)
        return s.rstrip("0").rstrip(".")
    half_away = lambda v: math.copysign(math.floor(abs(v) + 0.5), v)         # f64::round
    return str(int(half_away(half_away(x / fct) * fct)))


def pretty_u32(v):
    """ext::fmt::PrettyU32 (src/ext/fmt.rs:93-113)"""
    if v == 0:
        return "0"
    if v == U32_MAX:
        return "inf"
    for unit, suffix in ((10 ** 9, "G"), (10 ** 6, "M"), (1000, "k")):
        if v % unit == 0:
            return f"{v // unit}{suffix}"
    return str(v)


def basis_tag(divergence=0.01, window=250, step=None, leave_out=()):
    """construct_basis_tag (augment.rs:259-279); ValueError where the reference returns its RuntimeError"""
    tag = "x" + fmt_signif(divergence, 5)
    if window == U32_MAX:
        tag += "-global"
    else:
        tag += "-w" + pretty_u32(window)
        if step is not None:
            tag += "-s" + pretty_u32(step)
    if leave_out:
        tag += "-lo" + ",".join(leave_out)
    if len(tag) >= 128:
        raise ValueError(f"Automatic tag name is too long ({len(tag)} chars.), please provide tag using --tag")
    return tag
