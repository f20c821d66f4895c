"""Designed likelihood matrices for the prefilter tests (tests/test_prefilter_cases.py on the oracle, tests/test_gpu_prefilter.py on the
device). A matrix row is only reachable through a loaded read pair, so a row is steered through the pair's records: pair r gets one
alignment per read end on every allele a with design[r][a] >= 0, whose edit profile and insert size are those of the level id
design[r][a]; an allele with design[r][a] == NOALN gets no record and with it the pair's no-alignment value. Equal level ids in a row
give bit-equal entries (the likelihood of a record depends on its operation counts and the insert size only), different ids
different entries. Nothing here predicts a value: the tests read the matrix back and count (`row_levels`, `gram_geometry`).

The level of id l: base profile l % 12 (mismatches on both ends, a one-base deletion on end 1: at most three edits per end, so every
pair stays good under the 3 % threshold of 150-base reads and a paired alignment stays above the lone-end alternative) and an insert
size of `insert0 + l // 12` bases.
"""
import numpy as np

from locityper_amd import cdefs
from locityper_amd.cdefs import ReadsChunk

NOALN = -1
READ_LEN = 150
# (mismatches end 1, mismatches end 2, deleted bases end 1): distinct (x1 + x2, d1), at most 3 edits per end
BASE_PROFILES = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0), (3, 2, 0), (3, 3, 0),
                 (0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 2, 1), (2, 2, 1)]
N_BASE = len(BASE_PROFILES)
EDGE_ALLELES = (0, 31, 32, 63, 64, 127, 128)      # and A - 1: the lanes / tiles where an operand or C/D layout mistake would show
GR_LMAX, GR_RB = 16, 128                          # lcty_gram.hip: levels of a row the Gram form takes; rows per block of the level kernel


def level_id(base=0, shift=0):
    return base + N_BASE * shift


def mean_insert(bg):
    return int(round(bg.ins_n * (1.0 - bg.ins_p) / bg.ins_p))


def _cigar_words(x, d):
    """150 read bases with x mismatches (and a d-base deletion in the middle)."""
    EQ, X, D = cdefs.CIGAR_EQ, cdefs.CIGAR_X, cdefs.CIGAR_D
    w = []
    if d:
        w += [(70 << 4) | EQ, (d << 4) | D, ((READ_LEN - 70 - x) << 4) | EQ]
    else:
        w += [((READ_LEN - x) << 4) | EQ]
    if x:
        w += [(x << 4) | X]
    return w


def build_chunk(design, seqs, seq_off, insert0, pos1=400):
    """design: int array [R][A] of level ids (NOALN = no record). seqs / seq_off: the locus' alleles (the read ends are copied from
    allele 0, so that they carry its k-mers). -> ReadsChunk of R pairs, built with numpy (a pair at 4 096 alleles has 8 192 records)."""
    design = np.asarray(design, dtype=np.int64)
    R, A = design.shape
    assert A == len(seq_off) - 1 and (design >= NOALN).all()
    assert ((design >= 0).sum(axis=1) >= 1).all(), "a pair needs a primary record"
    allele_len = np.diff(np.asarray(seq_off).astype(np.int64))
    max_shift = int(design.max()) // N_BASE
    assert pos1 + 8 * 20 + insert0 + max_shift + 200 <= int(allele_len.min()), "alleles too short for the designed pairs"
    M2, REV, SEC = cdefs.FLAG_MATE2, cdefs.FLAG_REVERSE, cdefs.FLAG_SECONDARY
    # the CIGARs of every profile once
    cig1 = {b: _cigar_words(x1, d1) for b, (x1, x2, d1) in enumerate(BASE_PROFILES)}
    cig2 = {b: _cigar_words(x2, 0) for b, (x1, x2, d1) in enumerate(BASE_PROFILES)}
    n1 = np.array([len(cig1[b]) for b in range(N_BASE)]); n2 = np.array([len(cig2[b]) for b in range(N_BASE)])
    w1 = np.zeros((N_BASE, 4), dtype=np.uint32); w2 = np.zeros((N_BASE, 4), dtype=np.uint32)
    for b in range(N_BASE):
        w1[b, :n1[b]] = cig1[b]; w2[b, :n2[b]] = cig2[b]
    a0 = np.asarray(seqs[int(seq_off[0]):int(seq_off[1])])
    code = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"): code[ch] = i
    rec_parts, cig_parts, aln_off, cigar_off = [], [], [0], [0]
    mate_len = np.full(2 * R, READ_LEN, dtype=np.uint32)
    stride = (READ_LEN + 31) // 32 * 32
    mate_off = np.arange(2 * R + 1, dtype=np.uint64) * stride
    bases = np.zeros(2 * R * stride, dtype=np.uint8)
    nmask_bits = np.zeros(2 * R * stride, dtype=bool)
    for r in range(R):
        p1 = pos1 + 8 * (r % 20)
        al = np.nonzero(design[r] >= 0)[0]
        lv = design[r, al]
        base, shift = lv % N_BASE, lv // N_BASE
        n = len(al)
        recs = np.zeros(2 * n, dtype=cdefs.ALN_REC_DTYPE)
        recs["contig"][:n] = al; recs["contig"][n:] = al
        recs["pos"][:n] = p1
        recs["pos"][n:] = p1 + insert0 - READ_LEN + shift                     # insert size = insert0 + shift
        recs["flags"][:n] = SEC; recs["flags"][n:] = SEC | M2 | REV
        recs["flags"][0] = 0; recs["flags"][n] = M2 | REV                     # the first record of an end is its primary
        nc = np.concatenate([n1[base], n2[base]])
        recs["n_cigar"] = nc
        rel = np.zeros(2 * n, dtype=np.int64); np.cumsum(nc[:-1], out=rel[1:])
        recs["cigar_rel"] = rel
        words = np.concatenate([w1[base], w2[base]])                           # [2n][4], the first n_cigar of each row count
        keep = np.arange(4)[None, :] < nc[:, None]
        cig_parts.append(words[keep])
        rec_parts.append(recs)
        aln_off.append(aln_off[-1] + 2 * n); cigar_off.append(cigar_off[-1] + int(nc.sum()))
        p2 = p1 + insert0 - READ_LEN
        for e, q in ((0, p1), (1, p2)):
            c = code[a0[q:q + READ_LEN]]
            o = (2 * r + e) * stride
            nmask_bits[o:o + READ_LEN] = c == 255
            bases[o:o + READ_LEN] = np.where(c == 255, 0, c)
    b16 = bases.reshape(-1, 16).astype(np.uint32)
    bases2 = (b16 << (2 * np.arange(16, dtype=np.uint32))[None, :]).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    m32 = nmask_bits.reshape(-1, 32).astype(np.uint64)
    nmask = (m32 << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    if R == 0:
        return ReadsChunk.from_pairs([])
    return ReadsChunk(mate_len, mate_off, bases2, nmask, aln_off, np.concatenate(rec_parts), cigar_off, np.concatenate(cig_parts))


def concat_chunks(chunks):
    """One chunk holding the pairs of `chunks` in order (what appending them one after the other loads)."""
    mo, ao, co = [np.zeros(1, dtype=np.uint64)], [np.zeros(1, dtype=np.uint64)], [np.zeros(1, dtype=np.uint64)]
    for c in chunks:
        mo.append(c.mate_off[1:] + mo[-1][-1]); ao.append(c.aln_off[1:] + ao[-1][-1]); co.append(c.cigar_off[1:] + co[-1][-1])
    return ReadsChunk(np.concatenate([c.mate_len for c in chunks]), np.concatenate(mo),
                      np.concatenate([c.bases2[:c.n_bases // 16] for c in chunks]), np.concatenate([c.nmask[:c.n_bases // 32] for c in chunks]),
                      np.concatenate(ao), np.concatenate([c.recs for c in chunks]), np.concatenate(co),
                      np.concatenate([c.cigar[:int(c.cigar_off[-1])] for c in chunks]))


# ------------------------------------------------------------------ designs
def _row_with(rng, A, ids):
    """A row over A alleles that takes exactly the level ids `ids`, each at least once."""
    ids = np.asarray(ids, dtype=np.int64)
    assert len(ids) <= A
    row = ids[rng.integers(0, len(ids), A)]
    row[rng.permutation(A)[:len(ids)]] = ids
    return row


def _pick(rng, n, pool=40):
    """n distinct level ids; from 13 on one of them is NOALN."""
    if n == 1:
        return np.array([int(rng.integers(0, pool))])
    ids = rng.permutation(pool)[:n]
    if n >= 13 or rng.random() < 0.5:
        ids[0] = NOALN
    return ids


LEVEL_CYCLE = (1, 2, 15, 16, 17, 22)


def levels_1_2_16_17(A, R, seed=1):
    """Rows with exactly 1, 2, 15, 16, 17 and 22 distinct values in turn: every block of 128 rows mixes them. -> design, counts."""
    rng = np.random.default_rng(seed)
    counts = np.array([LEVEL_CYCLE[r % len(LEVEL_CYCLE)] for r in range(R)])
    return np.stack([_row_with(rng, A, _pick(rng, int(n))) for n in counts]), counts


def block_edges(A, totals, tail, seed=2):
    """One block of 128 rows per entry of `totals` (the last one of `tail` rows only): the rows the Gram form takes have
    sum(levels - 1) == totals[b] columns; every block but a one-row one also holds a 17-level row, which has none. -> design, counts."""
    rng = np.random.default_rng(seed)
    rows, counts = [], []
    for b, T in enumerate(totals):
        n_rows = tail if b == len(totals) - 1 else GR_RB
        per_row = [1] * n_rows
        slots = list(rng.permutation(n_rows))
        if n_rows > 1:
            per_row[slots.pop()] = GR_LMAX + 1                                  # residual: no columns
        left = T
        while left > 0:
            c = min(left, GR_LMAX - 1)
            per_row[slots.pop()] = c + 1
            left -= c
        for n in per_row:
            rows.append(_row_with(rng, A, _pick(rng, n))); counts.append(n)
    return np.stack(rows), np.array(counts)


def edge_alleles(A):
    return sorted({e for e in EDGE_ALLELES + (A - 1,) if e < A})


def tile_edges(A, R, seed=3):
    """Steps and spikes at the edge alleles: rows in which the alleles up to e sit at one level and those behind it at another
    (e and e - 1 as the last allele of the first group), and rows in which e alone differs from everybody else. Each edge allele then
    differs from both neighbours in some row, with a weight of its own. -> design, counts (2 everywhere)."""
    rng = np.random.default_rng(seed)
    kinds = [(e, k) for e in edge_alleles(A) for k in ("step", "step_before", "spike") if not (k == "step" and e == A - 1)]
    rows = []
    for r in range(R):
        e, k = kinds[r % len(kinds)]
        hi, lo = rng.permutation(40)[:2]
        if rng.random() < 0.3: lo = NOALN
        row = np.full(A, lo, dtype=np.int64)
        if k == "spike": row[e] = hi
        elif k == "step": row[:e + 1] = hi
        else: row[:max(e, 1)] = hi
        rows.append(row)
    return np.stack(rows), np.array([len(np.unique(x)) for x in rows])


def wide_range(A, R, near_shifts, n_wide=4, seed=4):
    """`n_wide` rows whose alleles either carry a perfect pair or no alignment at all (the largest difference two entries of a row can
    have) among rows that take two insert sizes with nearly the same probability (`near_shifts`, see closest_insert_shifts) and nothing
    else. -> design, counts (2 everywhere)."""
    rng = np.random.default_rng(seed)
    rows = []
    wide_at = set(np.linspace(0, R - 1, n_wide).astype(int).tolist())
    for r in range(R):
        ids = [level_id(0, near_shifts[0]), NOALN] if r in wide_at else [level_id(0, near_shifts[0]), level_id(0, near_shifts[1])]
        rows.append(_row_with(rng, A, ids))
    return np.stack(rows), np.full(R, 2)


def closest_insert_shifts(insert_lnprob, insert0, span=300):
    """The two insert sizes in [insert0, insert0 + span) whose ln-probabilities are closest without being equal, as shifts from insert0
    (around the mode of the insert size distribution two sizes on either side of it can be very close)."""
    v = np.array([insert_lnprob(insert0 + s) for s in range(span)])
    o = np.argsort(v, kind="stable")
    d = np.diff(v[o])
    d[d == 0.0] = np.inf
    t = int(np.argmin(d))
    return int(o[t + 1]), int(o[t])


def mostly_many_valued(A, R, many=20, few=3, seed=5):
    """Two rows in five with `many` levels, the others with `few`. -> design, counts."""
    rng = np.random.default_rng(seed)
    counts = np.array([many if r % 5 in (1, 3) else few for r in range(R)])
    return np.stack([_row_with(rng, A, _pick(rng, int(n))) for n in counts]), counts


def many_sixteens(A, R, seed=6):
    """Three rows in ten with exactly 16 levels — the most the Gram form takes —, the others with 2: more than a quarter of the rows would be
    residual if a 16-level row were taken for one, and the columns (5.2 per row) still fit the room of 6 per row. -> design, counts."""
    rng = np.random.default_rng(seed)
    counts = np.array([GR_LMAX if r % 10 in (1, 4, 7) else 2 for r in range(R)])
    return np.stack([_row_with(rng, A, _pick(rng, int(n))) for n in counts]), counts


# ------------------------------------------------------------------ reading a matrix back
def row_levels(M):
    """Distinct values per row of the [A][n_good] matrix (what np.unique counts: exact equality)."""
    return np.array([len(np.unique(M[:, j])) for j in range(M.shape[1])], dtype=np.int64)


def device_rows(M, status):
    """Levels per row of the matrix the device holds: [n_pairs][A], the rows of pairs that are not good are all 0.0 (one level)."""
    good = np.asarray(status) == cdefs.READ_GOOD
    assert int(good.sum()) == M.shape[1]
    lv = np.ones(len(good), dtype=np.int64)
    lv[good] = row_levels(M)
    return lv


def gram_geometry(M, status, lmax=GR_LMAX):
    """What lcty_gram.hip makes of the batch, derived from the matrix the way the kernels define it: levels per device row, the rows left
    to the f64 kernel, the columns per block of 128 rows, the column total (blocks padded to whole 32-column words), the largest level
    difference and the sum of |largest value| over the Gram rows."""
    lv = device_rows(M, status)
    res = lv > lmax
    cols = np.where(res, 0, lv - 1)
    n_blocks = (len(lv) + GR_RB - 1) // GR_RB
    per_block = np.array([int(cols[b * GR_RB:(b + 1) * GR_RB].sum()) for b in range(n_blocks)], dtype=np.int64)
    padded = (per_block + 31) // 32 * 32
    good_ix = np.nonzero(np.asarray(status) == cdefs.READ_GOOD)[0]
    dmax, dmin, c_abs = 0.0, np.inf, 0.0
    for j, r in enumerate(good_ix):
        if res[r]: continue
        u = np.unique(M[:, j])
        c_abs += abs(float(u[-1]))
        if len(u) > 1:
            d = np.diff(u)
            dmax = max(dmax, float(d.max())); dmin = min(dmin, float(d.min()))
    return dict(levels=lv, residual=res, n_res=int(res.sum()), block_cols=per_block, n_cols=int(cols.sum()), n_cols_padded=int(padded.sum()),
                dmax=dmax, dmin=dmin, c_abs=c_abs, n_rows=len(lv), A=M.shape[0])


def level_kernel_width(A):
    """The instantiation of gram_levels_kernel (values per lane) an allele count gets."""
    v = (A + 63) // 64
    return next(w for w in (4, 8, 16, 32, 64) if v <= w)


# ------------------------------------------------------------------ the higher-precision sum and the bounds
U = 2.0 ** -53                                     # unit roundoff of f64


def gt_index(i, j, A):
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return i * A - i * (i - 1) // 2 + (j - i)


def sample_genotypes(A, n_random, seed=11):
    """Every pair among the edge alleles and their neighbours, the whole diagonal {i, i}, and n_random genotypes drawn with `seed`."""
    e = sorted({x for a in edge_alleles(A) for x in (a - 1, a, a + 1) if 0 <= x < A})
    pairs = {(i, j) for i in e for j in e if i <= j} | {(i, i) for i in range(A)}
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, A, n_random), rng.integers(0, A, n_random)
    pairs |= set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))
    out = np.array(sorted(pairs), dtype=np.int64)
    return out[:, 0], out[:, 1]


def long_sum(M, i, j, chunk=512):
    """sum_r max(M[i][r], M[j][r]) in np.longdouble (64-bit significand on x86-64) -> (sums, sums of absolute values)."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than f64 here"
    s = np.zeros(len(i), dtype=np.longdouble); sa = np.zeros(len(i), dtype=np.longdouble)
    for o in range(0, len(i), chunk):
        m = np.maximum(M[i[o:o + chunk]], M[j[o:o + chunk]]).astype(np.longdouble)
        s[o:o + chunk] = m.sum(axis=1); sa[o:o + chunk] = np.abs(m).sum(axis=1)
    return s, sa


def tile_bound(n_terms, sum_abs):
    """|fl(sum) - sum| of f64 terms added in any order is at most gamma_(additions) * sum |x| (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2). The tile kernel adds the n terms of a genotype one by one to 0.0, split by split, and then the splits' partial
    sums in order; a split holds at least one term, so there are at most 2 n additions."""
    n = 2 * max(int(n_terms), 1)
    return n * U / (1.0 - n * U) * sum_abs


def gram_bound(geo, sum_abs_max, score_abs_max):
    """What the Gram form may differ by from the exact sum, from lcty_gram.hip:
      - a column's weight is q = llrint(ldexp(delta, F)) with F such that the largest delta * 2^F lies in [2^34, 2^35): |q 2^-F - delta| <=
        2^-(F+1) (the clamp to 2^35 - 1 can cost one more unit when the largest weight rounds up to 2^35: 2^-F then);
        delta = lv[k] - lv[k+1] is itself an f64 difference: U * delta <= U * dmax more. At most all n_cols columns count for a genotype.
      - the integer sum S is exact; its conversion to f64 rounds once when S >= 2^53: U * (n_cols * dmax).
      - C, the sum of the rows' largest values, is added serially (rows of a block, then the blocks): gamma_(rows) * sum |v_1|.
      - (C - S 2^-F) rounds once, and adding the residual rows' f64 partial rounds once more: 2 U * max |score| (intermediate results are
        bounded by sum_r |max|, which is what is passed in), and that partial is a tile-kernel sum over the residual rows.
    """
    if geo["dmax"] > 0.0:
        F = 34 - int(np.floor(np.log2(geo["dmax"])))
        per_col = 2.0 ** -(F + 1) + 2.0 ** -F * (geo["dmax"] * 2.0 ** F >= 2.0 ** 35 - 0.5) + U * geo["dmax"]
    else:
        per_col = 0.0
    K = geo["n_cols"]
    n_gram = geo["n_rows"] - geo["n_res"]
    return (K * per_col + U * K * geo["dmax"] + tile_bound(n_gram, geo["c_abs"]) + 2.0 * U * (score_abs_max + geo["c_abs"])
            + tile_bound(geo["n_res"], sum_abs_max))
