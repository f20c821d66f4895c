"""Transliteration of the transitive strategy of `locityper align` (TEST INFRASTRUCTURE), written from the Rust in plain Python: the
single-thread TransitiveStrategy (src/seq/align.rs:428-514) with save_cigar and the dv of process_pair (652-665),
Cigar::find_transitive_alignment / transfer_alignment::<true> (src/seq/cigar.rs:1248-1368, 1389-1414) and Cigar::optimize (1167-1237).
double_move, the operation classes and Cig are those of tests/pyref_transfer.py; the backbone route, smart_align at accuracy 9, the
counts and calculate_score those of tests/pyref_align.py (pyref_transfer.optimize does not fit: its aligner is level 6's).

The library's stated difference is applied here too: equal neighbouring operations are merged — the CIGARs the walk reads are merged,
and the walk's own CIGAR is merged before optimize looks for its anchors.

run() also returns the round boundaries of the library's schedule: a round is the longest prefix of the remaining pairs in which no
pair reads a cell (closest[ref], closest[query], the CIGAR cells its clause tests) that an earlier pair of the prefix writes (its own
CIGAR cell, closest[query])."""
from tests import pyref_align as A
from tests import pyref_db as D
from tests.pyref_transfer import Cig, consumes, invert_op, double_move

NONE = 0xFFFFFFFF
NO_GAP = 0xFFFFFFFF
ANCHOR_MARGIN = 5
OPT_GAP, OPT_ANCHOR = 1000, 51


def route_name(n, m, max_gap):                               # smart_align's routing, wfa.rs:280-321
    if n > 0 and m > 0:
        if max_gap < n or max_gap < m: return "simple"
        if n == m and n <= A.SAFE_MISMATCH: return "straight"
        return "exact"
    return "del" if n > 0 else "ins" if m > 0 else "none"


def _smart(seq_k, i1, i2, seq_i, j1, j2, max_gap, cig, dp_cells, counters, trace, phase):
    trace.append((phase, route_name(i2 - i1, j2 - j1, max_gap), i2 - i1, j2 - j1))
    return A.smart_align(seq_k, i1, i2, seq_i, j1, j2, max_gap, cig, dp_cells, counters)


def merged(cig):
    out = Cig()
    for op, ln in A.normalize(cig):
        out.push_unchecked(op, ln)
    return out


def optimize(self, ref_seq, query_seq, max_gap, anchor_size, dp_cells, counters, trace):    # cigar.rs:1167-1237
    i = qpos1 = rpos1 = flag = qpos2 = rpos2 = 0
    new = None

    def begin():
        c = Cig(); c.t = [list(x) for x in self.t[:i]]; c.qlen, c.rlen = qpos1, rpos1
        return c
    for j, (op, ln) in enumerate([tuple(x) for x in self.t]):
        cq, cr = consumes(op)
        if cq and cr and ln >= anchor_size:
            if flag == 3 and not max_gap < qpos2 - qpos1 and not max_gap < rpos2 - rpos1:
                if new is None: new = begin()
                _smart(ref_seq, rpos1, rpos2, query_seq, qpos1, qpos2, NO_GAP, new, dp_cells, counters, trace, "optimize")
                i = j
            qpos2 += ln; rpos2 += ln; qpos1, rpos1, flag = qpos2, rpos2, 0
            if new is not None:
                new.t.extend([list(x) for x in self.t[i:j]])
                new.push_checked(op, ln)
                new.qlen, new.rlen = qpos2, rpos2
            i = j + 1
        else:
            qpos2 += ln if cq else 0; rpos2 += ln if cr else 0
            flag |= (0 if cq else 1) | ((0 if cr else 1) << 1)
    if flag == 3 and not max_gap < qpos2 - qpos1 and not max_gap < rpos2 - rpos1:
        if new is None: new = begin()
        _smart(ref_seq, rpos1, rpos2, query_seq, qpos1, qpos2, NO_GAP, new, dp_cells, counters, trace, "optimize")
        i = len(self.t)
    if new is not None:
        new.t.extend([list(x) for x in self.t[i:]])
        self.t = new.t


def find_transitive_alignment(items_ij, j_ref_ij, items_jk, k_ref_jk, seq_i, seq_k, max_gap, anchor_size, dp_cells=A.DP_CELLS, counters=None,
                              trace=None):
    """(normalized items of i (query) against k (reference), which shortcut: None, "ij" or "jk"). items_*: normalized [(op, len)]."""
    counters = counters if counters is not None else {}
    trace = trace if trace is not None else []
    seq_i, seq_k = A.norm(seq_i), A.norm(seq_k)
    d1 = (lambda o: o) if j_ref_ij else invert_op            # QueryToRef / RefToQuery
    d2 = (lambda o: o) if k_ref_jk else invert_op
    full = lambda t: len(t) == 1 and t[0][0] == "="          # full_sequence_match, cigar.rs:514-516
    if full(items_ij):
        return A.normalize(Cig([(d2(op), ln) for op, ln in items_jk])), "ij"
    if full(items_jk):
        return A.normalize(Cig([(d1(op), ln) for op, ln in items_ij])), "jk"
    new = Cig()
    last1 = last2 = 0
    if items_ij and items_jk:
        ij, jk = iter(items_ij), iter(items_jk)
        op2, len2 = next(jk); op2 = d2(op2)
        op1, len1 = next(ij); op1 = d1(op1)
        st = [0, len1, 0, len2]                              # pos1, rem1, pos2, rem2
        while True:
            pos1, rem1, pos2, rem2 = st
            e1, e2 = op1 == "=", op2 == "="
            add = None
            if e1 and e2:
                if min(rem1, rem2) >= anchor_size: add = "="
            elif e1 and not e2:
                if rem1 >= anchor_size and len1 - rem1 >= ANCHOR_MARGIN: add = op2
            elif not e1 and e2:
                if rem2 >= anchor_size and len2 - rem2 >= ANCHOR_MARGIN: add = op1
            if add is not None:
                _smart(seq_k, last2, pos2, seq_i, last1, pos1, max_gap, new, dp_cells, counters, trace, "walk")
            shift = double_move(op1, op2, st)
            if add is not None:
                new.push_checked(add, shift); last1, last2 = st[0], st[2]
            if st[1] == 0:
                nxt = next(ij, None)
                if nxt is None: break
                op1, len1 = nxt; op1 = d1(op1); st[1] = len1
            if st[3] == 0:
                nxt = next(jk, None)
                if nxt is None: break
                op2, len2 = nxt; op2 = d2(op2); st[3] = len2
    if last1 != len(seq_i) or last2 != len(seq_k):
        _smart(seq_k, last2, len(seq_k), seq_i, last1, len(seq_i), max_gap, new, dp_cells, counters, trace, "tail")
    assert new.qlen == len(seq_i) and new.rlen == len(seq_k), (new.qlen, len(seq_i), new.rlen, len(seq_k))
    new = merged(new)
    optimize(new, seq_k, seq_i, OPT_GAP, OPT_ANCHOR, dp_cells, counters, trace)
    return A.normalize(new), None


def run(seqs, pairs, ks, max_gap=10000, tr_div=0.01, anchor=101, thresh_div=1.0, against=None, against_div=1.0, div_k=15, div_w=15,
        dp_cells=A.DP_CELLS):
    """The strategy over `pairs` [(ref, query)] in order. Returns a dict: per pair `route` (0 skipped, 1 backbone, 2 first clause,
    3 second clause), `via`, `items` (normalized CIGAR or None), `score`, `best_k`, `div` (um, md); `rounds` = the index of the first
    pair of every round (n_rounds = its length; empty when nothing is accelerated by rule); `events` for the coverage assertions."""
    n, P = len(seqs), len(pairs)
    uniq, dv = D.divergences(seqs, div_k, div_w)
    tri = {p: x for x, p in enumerate(D.triangle_indices(n))}
    div = [(int(uniq[tri[(min(r, q), max(r, q))]]), float(dv[tri[(min(r, q), max(r, q))]])) for r, q in pairs]
    ag = against if against is not None else [0] * n
    taken = [div[x][1] <= (against_div if ag[r] or ag[q] else (-1.0 if thresh_div == 0.0 else thresh_div)) for x, (r, q) in enumerate(pairs)]
    res = {"route": [0] * P, "via": [NONE] * P, "items": [None] * P, "score": [0] * P, "best_k": [0] * P, "div": div, "rounds": [],
           "events": {"dirs": set(), "shortcuts": set(), "replaced": 0, "kept_equal": 0, "trace": [], "dropped": 0}}
    ev = res["events"]
    accelerate = tr_div > 0 and P >= 16                      # align.rs:784
    closest = [None] * n                                     # query -> (ref, pair index, dv)
    cells = {}                                               # frozenset{a, b} -> pair index
    w_closest, w_cells = set(), set()
    counters = {}
    for x, (k, i) in enumerate(pairs):
        if not taken[x]:
            continue
        edge = None
        if accelerate:
            tested = []
            if closest[k] is not None: tested.append(frozenset((i, closest[k][0])))
            if not (tested and tested[0] in cells) and closest[i] is not None: tested.append(frozenset((k, closest[i][0])))
            if not res["rounds"] or k in w_closest or i in w_closest or any(c in w_cells for c in tested):
                res["rounds"].append(x); w_closest.clear(); w_cells.clear()
            if closest[k] is not None and frozenset((i, closest[k][0])) in cells:
                j = closest[k][0]; edge = (2, j, cells[frozenset((i, j))], closest[k][1])
            elif closest[i] is not None and frozenset((k, closest[i][0])) in cells:
                j = closest[i][0]; edge = (3, j, closest[i][1], cells[frozenset((k, j))])
            w_closest.add(i); w_cells.add(frozenset((k, i)))
        if edge is not None:
            rt, j, pij, pjk = edge
            j_ref_ij, k_ref_jk = pairs[pij][0] == j, pairs[pjk][0] == k
            trace = []
            items, shortcut = find_transitive_alignment(res["items"][pij], j_ref_ij, res["items"][pjk], k_ref_jk, seqs[i], seqs[k], max_gap,
                                                        anchor, dp_cells, counters, trace)
            ev["dirs"].add((j_ref_ij, k_ref_jk)); ev["trace"] += trace
            if shortcut: ev["shortcuts"].add(shortcut)
            res["route"][x], res["via"][x], res["items"][x], res["score"][x] = rt, j, items, A.calculate_score(items)
        else:
            cig, score, bk = A.align_multik(seqs[k], seqs[i], ks, max_gap, dp_cells)
            res["route"][x], res["items"][x], res["score"][x], res["best_k"][x] = 1, A.normalize(cig), score, bk
        nm, ne = A.counts(res["items"][x])
        d = ne / (nm + ne) if nm + ne else float("nan")
        if accelerate:                                       # save_cigar, align.rs:504-513
            if d <= tr_div:
                if closest[i] is not None and closest[i][2] <= d:
                    ev["kept_equal"] += closest[i][2] == d
                else:
                    ev["replaced"] += closest[i] is not None
                    closest[i] = (k, x, d)
            cells[frozenset((k, i))] = x
    ev["dropped"] = counters.get("dropped", 0)
    return res
