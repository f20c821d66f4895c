"""The pairwise haplotype alignments of lcty_align.hip where tests/test_gpu_align.py does not reach: every scratch level of the exact
aligner at its limits and beyond the largest, a level's list longer than its lanes (a lane's scratch used again with another row
width), a batch cut by the match budget, the refusal of more than 2^24 matches, a CIGAR that fills its planned bound, low-complexity
sequence, and lengths around k and around the block of align_prefix_kernel; then a random differential run. The sets are those of
tests/align_cases.py (tests/test_align_host.py shows that each is what it is meant to be), the reference is the transliteration
tests/pyref_align.py, stage by stage."""
import re

import numpy as np
import pytest

from locityper_amd import api
from locityper_amd._lib import LocityperError
from tests import align_cases as AC
from tests import pyref_align as R
from tests import test_gpu_align as TG

pytestmark = pytest.mark.gpu


def _words(res, x):
    return res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])]


def _stage_tasks(names):
    return [(n, r, q, k) for n in names for c in [AC.by_name(n)] for r, q in c.pairs for k in c.ks]


# ---- 1. the scratch levels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pair", [(s, p) for s in AC.LEVEL_SHAPES for p in s[3]], ids=lambda v: v[0] if len(v) == 7 else f"{v[0]}-{v[1]}")
def test_levels(gpu_ctx, shape, pair):
    """One stretch at, or just beyond, a limit of lim_takes: the task runs at the level the shape is meant for (n_level), alone in
    that level's scratch with rows of dim + 1 cells and exactly `cells` direction bytes behind them."""
    name, _, _, _, max_gap, n_level, n_dropped = shape
    c = AC.by_name("lv_" + name)
    r, q = pair
    got, st = AC.backbone_run(gpu_ctx, c.name, r, q, AC.K)
    a, b = c.stretch[pair]
    print(f"{name} as {a} x {b}: fill_ms {st['fill_ms']:.1f}, chain_ms {st['chain_ms']:.1f}, total_ms {st['total_ms']:.1f}")
    matches, score, path = AC.reference(c.name, r, q, AC.K)
    assert np.array_equal(got["matches"], np.array(matches, dtype=np.uint32).reshape(-1, 2))
    # two diagonals, 60 + 60; the optimal chain is not unique (a jump of k within a diagonal is worth k single steps): any valid one
    AC.check_stage_b(gpu_ctx, c.name, r, q, AC.K)
    assert got["chain_score"] == score == 2 * AC.FLANK
    assert st["n_level"] == n_level and st["n_dropped"] == got["n_dropped"] == n_dropped
    assert st["n_general_dp"] == 1 - n_dropped and st["dp_cells"] == (0 if n_dropped else (a + 1) * (b + 1))
    items = R.items_of(got["cigar"])
    mid_r, mid_q = c.seqs[r][AC.FLANK:-AC.FLANK], c.seqs[q][AC.FLANK:-AC.FLANK]
    if name in AC.BEYOND_ORACLE:
        # the oracle's aligner refuses a gap of 16 000 columns: an independent full-matrix optimum of the stretch (the anchors cost nothing)
        AC.check_cigar(items, got["score"], c.seqs[r], c.seqs[q])
        assert got["score"] == R.full_dp_score(mid_r, mid_q)
        assert items[0] == ("=", AC.FLANK) and items[-1] == ("=", AC.FLANK)
        return
    counters = {}
    cig, want = R.align_from_path(c.seqs[r], c.seqs[q], matches, got["path"].tolist(), AC.K, max_gap, counters=counters)
    assert np.array_equal(got["cigar"], R.words(R.normalize(cig))) and got["score"] == want
    assert counters.get("dropped", 0) == n_dropped and st["n_simple"] == n_dropped
    AC.check_cigar(items, got["score"], c.seqs[r], c.seqs[q])
    if n_dropped:
        assert got["score"] <= R.full_dp_score(mid_r, mid_q)
    else:
        assert got["score"] == R.full_dp_score(mid_r, mid_q)


# ---- 2. a lane's scratch used again ---------------------------------------------------------------------------------------------------------
def _against_transliteration(c, pairs, res):
    for x, (r, q) in enumerate(pairs):
        matches, _, path = AC.reference(c.name, r, q, AC.K)
        cig, score = R.align_from_path(c.seqs[r], c.seqs[q], matches, path, AC.K, c.max_gap)
        assert np.array_equal(_words(res, x), R.words(R.normalize(cig))), (r, q)
        assert int(res["score"][x]) == score, (r, q)


def test_reuse_of_level_1_lanes(gpu_ctx):
    """136 tasks of level 1 in one call, 128 lanes: eight lanes take a second task, with another row width W, in the same scratch"""
    c = AC.by_name("reuse1")
    seqs, off = c.arrays()
    res, st = api.align_haplotypes(gpu_ctx, seqs, off, [p[0] for p in c.pairs], [p[1] for p in c.pairs], api.align_params(backbone_ks=c.ks))
    print(f"reuse1: fill_ms {st['fill_ms']:.1f}, total_ms {st['total_ms']:.1f}")
    assert st["n_level"] == [0, 136, 0] and st["n_batches"] == 1 and st["n_dropped"] == 0 and res["aligned"].all()
    _against_transliteration(c, c.pairs, res)


@pytest.mark.parametrize("way", [0, 1])
def test_reuse_of_level_2_lanes(gpu_ctx, way):
    """twelve tasks of level 2 in one call, eight lanes"""
    c = AC.by_name("reuse2")
    seqs, off = c.arrays()
    pairs = c.pairs[12 * way:12 * way + 12]
    res, st = api.align_haplotypes(gpu_ctx, seqs, off, [p[0] for p in pairs], [p[1] for p in pairs], api.align_params(backbone_ks=c.ks))
    print(f"reuse2 way {way}: fill_ms {st['fill_ms']:.1f}, total_ms {st['total_ms']:.1f}")
    assert st["n_level"] == [0, 0, 12] and st["n_batches"] == 1 and st["n_dropped"] == 0 and res["aligned"].all()
    _against_transliteration(c, pairs, res)


# ---- 3. the batch cut by the match budget -------------------------------------------------------------------------------------------------
def _simulated_batches(counts, budget, per_batch):
    """the loop of lcty_align_haplotypes around run_batch, from match counts alone: a batch of more than one pair whose matches (20
    bytes each) exceed the budget is cut to its longest prefix that fits, at least one pair"""
    at, batches = 0, 0
    while at < len(counts):
        n = min(per_batch, len(counts) - at)
        if n > 1 and 20 * sum(counts[at:at + n]) > budget:
            fit = 1
            while fit < n and 20 * sum(counts[at:at + fit + 1]) <= budget:
                fit += 1
            n = fit
        at += n; batches += 1
    return batches


def test_batches_cut_by_the_match_budget(gpu_ctx):
    c = TG._twelve()
    seqs, off = c.arrays()
    r, q = api.align_all_pairs(12)
    p = api.align_params(backbone_ks=c.ks)
    counts = [sum(len(R.kmer_matches(c.seqs[int(a)], c.seqs[int(b)], k)) for k in c.ks) for a, b in zip(r, q)]
    five, below = 20 * sum(counts[:5]), 20 * min(counts) - 1
    runs = [api.align_haplotypes(gpu_ctx, seqs, off, r, q, p)]
    # the default number of pairs per batch is sized from the same budget: held at all 66, so that the budget alone cuts
    for budget in (five, below):
        gpu_ctx.set_knob("align_match_budget", budget)
        gpu_ctx.set_knob("align_batch_pairs", 66)
        try:
            runs.append(api.align_haplotypes(gpu_ctx, seqs, off, r, q, p))
        finally:
            gpu_ctx.set_knob("align_match_budget", -1)
            gpu_ctx.set_knob("align_batch_pairs", -1)
    assert [st["n_batches"] for _, st in runs] == [1, _simulated_batches(counts, five, 66), 66]
    assert _simulated_batches(counts, below, 66) == 66 and 8 <= _simulated_batches(counts, five, 66) <= 20
    for res, st in runs[1:]:
        assert st["n_kmer_matches"] == runs[0][1]["n_kmer_matches"] == sum(counts)
        for k in runs[0][0]:
            assert np.array_equal(res[k], runs[0][0][k]), k
    for x in range(len(r)):
        AC.check_cigar(R.items_of(_words(runs[2][0], x)), int(runs[2][0]["score"][x]), c.seqs[int(r[x])], c.seqs[int(q[x])])


# ---- 4. the refusal ------------------------------------------------------------------------------------------------------------------------
def test_more_than_2_24_matches_are_refused(gpu_ctx):
    """4 196 windows a side, all equal: 17 606 416 matches of one (pair, k). The counting pass finds that out; nothing is emitted."""
    seqs = [b"A" * 4200, b"A" * 4200]
    arr = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    off = np.array([0, 4200, 8400], dtype=np.uint64)
    with pytest.raises(LocityperError) as e:
        api.align_backbone(gpu_ctx, arr, off, 0, 1, 5)
    assert e.value.code == 5
    assert re.search(r"sequences 0 and 1 share 17606416 5-mer matches", str(e.value)) and 4196 * 4196 == 17606416 > 1 << 24


# ---- 5. a CIGAR that fills its bound --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(0, 1), (1, 0), (2, 3), (3, 2)])
def test_cigar_fills_its_bound(gpu_ctx, pair):
    """PlanVisitor's bound is met but for its start of 2: were it one short on every stretch of any one route, three stretches of that
    route would outgrow it ("a CIGAR outgrew its bound")"""
    c = AC.by_name("tight_bound")
    r, q = pair
    got, st = AC.backbone_run(gpu_ctx, c.name, r, q, AC.K)
    items, count = AC.tight_bound_items(r, q)
    assert np.array_equal(got["cigar"], R.words(items)) and len(got["cigar"]) == count
    assert st["n_simple"] == sum(kd in ("9x12", "12x9") for kd in c.kinds[pair]) and st["n_general_dp"] + st["n_small_dp"] == 0
    AC.check_stage_a(gpu_ctx, c.name, r, q, AC.K)
    AC.check_stage_b(gpu_ctx, c.name, r, q, AC.K)
    AC.check_stage_c(gpu_ctx, c.name, r, q, AC.K)


# ---- 6. low complexity, 7. lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,query,k", _stage_tasks(["lowcomplexity", "lengths"]))
def test_stages_on_designed_sets(gpu_ctx, name, ref, query, k):
    AC.check_stage_a(gpu_ctx, name, ref, query, k)
    AC.check_stage_b(gpu_ctx, name, ref, query, k)
    AC.check_stage_c(gpu_ctx, name, ref, query, k)


# ---- 8. the random differential run (not designed; last) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,query,k", _stage_tasks([f"random_k{k}" for k in AC.RANDOM_KS]))
def test_random_pairs(gpu_ctx, name, ref, query, k):
    AC.check_stage_a(gpu_ctx, name, ref, query, k)
    AC.check_stage_b(gpu_ctx, name, ref, query, k)
    AC.check_stage_c(gpu_ctx, name, ref, query, k)
