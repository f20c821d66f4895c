"""Pairwise haplotype alignments on the device (lcty_align.hip) against the transliteration tests/pyref_align.py, stage by stage through
lcty_align_backbone and end to end through lcty_align_haplotypes, on the designed cases of tests/align_cases.py (tests/test_align_host.py
shows that the "unique chain" ones are solved optimally by the reference route itself)."""
import numpy as np
import pytest

from locityper_amd import api, io
from locityper_amd._lib import LocityperError
from tests import align_cases as AC
from tests import pyref_align as R

pytestmark = pytest.mark.gpu

TASKS = [(c.name, r, q, k) for c in AC.cases() for r, q in c.pairs for k in c.ks]
backbone, check_cigar = AC.backbone, AC.check_cigar


_full = {}


def full(ctx, name):
    """lcty_align_haplotypes over the pairs of a case"""
    if name not in _full:
        c = AC.by_name(name)
        seqs, off = c.arrays()
        # a call refuses a pair given in both orders: the second direction of a pair goes into a second call, the results are put
        # back into the order of c.pairs
        calls, seen = [[], []], set()
        for x, (r, q) in enumerate(c.pairs):
            calls[1 if frozenset((r, q)) in seen else 0].append(x)
            seen.add(frozenset((r, q)))
        parts, stats = {}, {}
        for xs in calls:
            if not xs:
                continue
            res, st = api.align_haplotypes(ctx, seqs, off, [c.pairs[x][0] for x in xs], [c.pairs[x][1] for x in xs],
                                           api.align_params(backbone_ks=c.ks, max_gap=c.max_gap))
            for t, x in enumerate(xs):
                parts[x] = {k: v[t] for k, v in res.items() if k not in ("cigar", "cigar_off")}
                parts[x]["words"] = res["cigar"][int(res["cigar_off"][t]):int(res["cigar_off"][t + 1])]
            for k, v in st.items():
                stats[k] = v if k not in stats else ([a + b for a, b in zip(stats[k], v)] if isinstance(v, list) else stats[k] + v)
        n = len(c.pairs)
        merged = {k: np.array([parts[x][k] for x in range(n)]) for k in parts[0] if k != "words"}
        merged["cigar_off"] = np.concatenate([[0], np.cumsum([len(parts[x]["words"]) for x in range(n)])]).astype(np.uint64)
        merged["cigar"] = np.concatenate([parts[x]["words"] for x in range(n)]).astype(np.uint32)
        _full[name] = (merged, stats)
    return _full[name]


# ---- 1. stage A -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,query,k", TASKS)
def test_stage_a_matches(gpu_ctx, name, ref, query, k):
    AC.check_stage_a(gpu_ctx, name, ref, query, k)


# ---- 2. stage B -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,query,k", TASKS)
def test_stage_b_chain(gpu_ctx, name, ref, query, k):
    AC.check_stage_b(gpu_ctx, name, ref, query, k)


# ---- 3. stage C -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,query,k", TASKS)
def test_stage_c_gap_fill(gpu_ctx, name, ref, query, k):
    AC.check_stage_c(gpu_ctx, name, ref, query, k)


# ---- 4. + 5. end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in AC.cases()])
def test_end_to_end(gpu_ctx, name):
    c = AC.by_name(name)
    res, st = full(gpu_ctx, name)
    assert st["n_aligned"] == len(c.pairs) and st["n_skipped"] == 0 and st["n_dropped"] == 0
    assert res["aligned"].all()
    for x, (r, q) in enumerate(c.pairs):
        items = R.items_of(res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])])
        score = int(res["score"][x])
        opt = AC.optimum(name, r, q)
        check_cigar(items, score, c.seqs[r], c.seqs[q], opt)
        nm, ne = R.counts(items)
        assert (int(res["n_matches"][x]), int(res["nerrs"][x]), int(res["aln_len"][x])) == (nm, ne, nm + ne)
        assert int(res["best_k"][x]) in c.ks
        # the winner is the best of the single-k runs, the first k on a tie
        singles = [backbone(gpu_ctx, name, r, q, k) for k in c.ks]
        if singles:
            best = max(range(len(c.ks)), key=lambda t: (singles[t]["score"], -t))
            assert int(res["best_k"][x]) == c.ks[best] and score == singles[best]["score"]
            assert np.array_equal(R.words(items), singles[best]["cigar"])
        if c.unique:
            want_items, want_score, want_k = AC.reference_multik(name, r, q)
            assert items == want_items and score == want_score == opt and int(res["best_k"][x]) == want_k
            assert (nm, ne) == R.counts(want_items)
    # dv == nerrs / aln_len: the PAF line is the transliteration's
    seqs, off = c.arrays()
    text = io.paf_write(c.names, off, [p[0] for p in c.pairs], [p[1] for p in c.pairs], res, api.align_params(backbone_ks=c.ks, max_gap=c.max_gap)).decode()
    lines = text.split("\n")[1:-1]
    for x, (r, q) in enumerate(c.pairs):
        items = R.items_of(res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])])
        assert lines[x] + "\n" == R.paf_line(c.names[q], len(c.seqs[q]), c.names[r], len(c.seqs[r]), (items, int(res["score"][x])),
                                             (int(res["um"][x]), float(res["md"][x])))
        ne, ln = int(res["nerrs"][x]), int(res["aln_len"][x])
        assert f"dv:f:{ne / ln:.9f}" in lines[x]


def test_identical_pair_is_one_run(gpu_ctx):
    c = AC.by_name("ends")
    res, _ = full(gpu_ctx, "ends")
    x = c.pairs.index((0, 3))
    assert R.items_of(res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])]) == [("=", len(c.seqs[0]))]
    assert int(res["score"][x]) == 0 and int(res["nerrs"][x]) == 0
    x = c.pairs.index((0, 4))                                                # differs only in length
    assert R.items_of(res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])]) == [("=", len(c.seqs[4])), ("D", 37)]


def test_max_gap_routes(gpu_ctx):
    c = AC.by_name("maxgap")
    res, st = full(gpu_ctx, "maxgap")
    assert st["n_simple"] > 0
    x = c.pairs.index((0, 1))
    assert R.items_of(res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])]) == [("=", 500), ("I", 300), ("=", 700)]


def test_tie_cases_take_the_reference_choice(gpu_ctx):
    """The stretches of AC.TIE_CASES, where the optimal alignment is not unique or a route changes, each way round: both sequences are
    shorter than k, so a pair has no match and is one stretch of smart_align. CIGAR and score are pyref_align's, and the stretches
    meant for the exact aligner reach it (tests/test_align_host.py puts the same list through the host instantiation)."""
    seqs = [s for _, r, q, _, _ in AC.TIE_CASES for s in (r, q)]
    arr = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    n_exact = 0
    for x, (name, r, q, max_gap, _) in enumerate(AC.TIE_CASES):
        for ri, qi in ((2 * x, 2 * x + 1), (2 * x + 1, 2 * x)):
            ref, query = seqs[ri], seqs[qi]
            got, st = api.align_backbone(gpu_ctx, arr, off, ri, qi, 25, api.align_params(max_gap=max_gap))
            cig, score = R.align_from_backbone(ref, query, 25, max_gap)
            assert len(got["matches"]) == 0 and got["n_dropped"] == 0, name
            assert np.array_equal(got["cigar"], R.words(R.normalize(cig))), (name, R.items_of(got["cigar"]), R.normalize(cig))
            assert got["score"] == score, name
            exact = bool(ref) and bool(query) and max_gap >= max(len(ref), len(query)) and not (len(ref) == len(query) <= R.SAFE_MISMATCH)
            assert st["n_small_dp"] + st["n_general_dp"] == int(exact), name
            if exact:
                assert score == R.full_dp_score(ref, query), name
            n_exact += exact
    assert n_exact >= 10


# ---- 6. divergences and skipping ---------------------------------------------------------------------------------------------------------
def _mixed_set():
    rng = np.random.default_rng(23)
    base = AC.rand_seq(rng, 1500)
    seqs = [base]
    for n_edits in (2, 10, 40, 120, 300):
        pos = sorted(rng.choice(np.arange(5, 1495), n_edits, replace=False).tolist())
        seqs.append(AC.apply_edits(base, [(p, "X", AC.other_base(base[p], rng)) for p in pos]))
    return AC.Case("mixed", seqs, [25], False)


def test_divergence_and_skipping(gpu_ctx):
    c = _mixed_set()
    seqs, off = c.arrays()
    r, q = api.align_all_pairs(len(c.seqs))
    uniq, div, _, _ = api.db_divergences(gpu_ctx, seqs, off, 15, 15)
    res, st = api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(backbone_ks=[25]))
    assert np.array_equal(res["um"], uniq) and np.array_equal(res["md"].view(np.uint64), div.view(np.uint64))
    assert res["aligned"].all()
    thresh = float(np.sort(div)[len(div) // 2])
    assert 0 < thresh < div.max()
    res, st = api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(backbone_ks=[25], thresh_div=thresh))
    assert np.array_equal(res["aligned"].astype(bool), div <= thresh) and st["n_skipped"] == int((div > thresh).sum()) > 0
    skipped = ~res["aligned"].astype(bool)
    assert not res["aln_len"][skipped].any() and np.array_equal(np.diff(res["cigar_off"].astype(np.int64))[skipped], np.zeros(skipped.sum(), dtype=np.int64))
    assert np.array_equal(res["um"], uniq)
    # against: pairs that touch haplotype 5 take against_div instead
    against = np.zeros(len(c.seqs), dtype=np.uint8); against[5] = 1
    res, _ = api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(backbone_ks=[25], thresh_div=thresh, against_div=1.0), against=against)
    touches = (r == 5) | (q == 5)
    assert np.array_equal(res["aligned"].astype(bool), np.where(touches, True, div <= thresh))
    res, _ = api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(backbone_ks=[25], thresh_div=1.0, against_div=0.0), against=against)
    assert np.array_equal(res["aligned"].astype(bool), np.where(touches, div <= 0.0, True))
    # skip_div: nothing is skipped, whatever the threshold; thresh_div == 0: nothing is aligned
    res, st = api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(backbone_ks=[25], thresh_div=thresh, skip_div=1))
    assert res["aligned"].all() and not res["um"].any() and st["n_skipped"] == 0
    res, st = api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(backbone_ks=[25], thresh_div=0.0))
    assert not res["aligned"].any() and st["n_aligned"] == 0 and np.array_equal(res["um"], uniq)
    # ... and a pair that passes all the same has no alignment to get, as in the reference (the ks are cleared): an error
    for kw in ({"skip_div": 1}, {"against_div": 1.0}):
        with pytest.raises(LocityperError) as e:
            api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(backbone_ks=[25], thresh_div=0.0, **kw), against=against)
        assert e.value.code == 3 and "No alignment found" in str(e.value)


# ---- 7. batching and limits ----------------------------------------------------------------------------------------------------------------
def _twelve():
    rng = np.random.default_rng(29)
    base = AC.rand_seq(rng, 800)
    seqs = []
    for h in range(12):
        pos = sorted(rng.choice(np.arange(5, 795), 6, replace=False).tolist())
        seqs.append(AC.apply_edits(base, [(p, "X", AC.other_base(base[p], rng)) if t % 2 else (p, "D", 1 + t) for t, p in enumerate(pos)]))
    return AC.Case("twelve", seqs, [25, 51], False)


def test_batches_of_three_pairs(gpu_ctx):
    c = _twelve()
    seqs, off = c.arrays()
    r, q = api.align_all_pairs(12)
    p = api.align_params(backbone_ks=c.ks)
    one, st1 = api.align_haplotypes(gpu_ctx, seqs, off, r, q, p)
    gpu_ctx.set_knob("align_batch_pairs", 3)
    try:
        many, st3 = api.align_haplotypes(gpu_ctx, seqs, off, r, q, p)
    finally:
        gpu_ctx.set_knob("align_batch_pairs", -1)
    assert st1["n_batches"] == 1 and st3["n_batches"] == 22
    for k in one:
        assert np.array_equal(one[k], many[k]), k
    for x in range(len(r)):
        check_cigar(R.items_of(one["cigar"][int(one["cigar_off"][x]):int(one["cigar_off"][x + 1])]), int(one["score"][x]), c.seqs[int(r[x])], c.seqs[int(q[x])])


def test_dropped_stretch(gpu_ctx):
    c = AC.by_name("unrelated")
    seqs, off = c.arrays()
    gpu_ctx.set_knob("align_dp_cells", 10000)
    try:
        res, st = api.align_haplotypes(gpu_ctx, seqs, off, [0], [1], api.align_params(backbone_ks=[25]))
    finally:
        gpu_ctx.set_knob("align_dp_cells", -1)
    assert st["n_dropped"] == 1 and st["dp_cells"] == 0
    items = R.items_of(res["cigar"])
    cig = R.Cig()
    want_score = R.align_simple(R.norm(c.seqs[0]), R.norm(c.seqs[1]), cig)
    assert items == R.normalize(cig) and items[0] == ("I", 40) and int(res["score"][0]) == want_score
    check_cigar(items, int(res["score"][0]), c.seqs[0], c.seqs[1], AC.optimum("unrelated", 0, 1))
    # the transliteration drops the same stretch under the same limit
    cig2, s2 = R.align_from_backbone(c.seqs[0], c.seqs[1], 25, 10000, dp_cells=10000)
    assert R.normalize(cig2) == items and s2 == want_score


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    c = AC.by_name("subs")
    seqs, off = c.arrays()

    def code(r, q, **kw):
        with pytest.raises(LocityperError) as e:
            api.align_haplotypes(gpu_ctx, seqs, off, r, q, api.align_params(**kw))
        return e.value.code
    assert code([0, 1], [1, 1]) == 1                                         # ref_id == query_id
    assert code([0, 1], [1, 0]) == 1                                         # the same pair in the other order
    assert code([0, 0], [1, 1]) == 1
    assert code([0], [4]) == 1                                               # out of range
    assert code([0], [1], backbone_ks=[4]) == 1 and code([0], [1], backbone_ks=[128]) == 1 and code([0], [1], backbone_ks=[]) == 1
    assert code([0], [1], thresh_div=1.5) == 1
    assert code([0], [1], mismatch=5) == 5 and code([0], [1], gap_open=4) == 5    # LCTY_ERR_UNSUPPORTED
    res, _ = api.align_haplotypes(gpu_ctx, seqs, off, [0], [1], api.align_params(backbone_ks=[127]))
    assert res["aligned"][0] == 1 and res["best_k"][0] == 127


# ---- 9. downstream -------------------------------------------------------------------------------------------------------------------------
def test_paf_feeds_hap_alns_and_basis(gpu_ctx, tmp_path):
    from locityper_amd import synth
    L = synth.SynthLocus(8, 256, base_len=3000)
    seqs, off = np.asarray(L.seqs, dtype=np.uint8), np.asarray(L.seq_off, dtype=np.uint64)
    names = [f"hap{i}" for i in range(8)]
    r, q = api.align_all_pairs(8)
    res, _ = api.align_haplotypes(gpu_ctx, seqs, off, r, q)
    path = tmp_path / "haplotypes.paf.gz"
    io.write_gz(path, io.paf_write(names, off, r, q, res))
    ents = io.paf_read(path, names)
    assert len(ents) == 28 and [(e[0], e[1]) for e in ents] == list(zip(q.tolist(), r.tolist()))
    for x, e in enumerate(ents):
        assert np.array_equal(e[2], res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])])
        assert (e[3], e[4]) == (int(res["n_matches"][x]), int(res["aln_len"][x]))
    p = api.resolve_params(api.default_params(), L.bg)
    loc = api.Locus(gpu_ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    loc.set_hap_alns(ents)
    lengths = np.diff(off.astype(np.int64)).astype(np.uint32)
    bp = api.basis_params(divergence=0.02, window=250)
    ids, bound, optimal, _ = api.basis_build(gpu_ctx, lengths, ents, bp)
    assert 1 <= len(ids) <= 8 and bound <= len(ids)
    win_off, rows, _ = api.basis_windows(gpu_ctx, lengths, ents, bp)
    mask = np.zeros(rows.shape[1], dtype=np.uint32)
    for i in ids:
        mask[int(i) >> 5] |= np.uint32(1 << (int(i) & 31))
    assert ((rows & mask) != 0).any(axis=1).all(), "the basis does not dominate its own rows"
