"""The rare paths of the greedy loop: reads with more than four locations (the ones beyond the fourth come from the chain's run, and the
current location itself may be one of them), alternatives that share a window with the current pair (the two halves of depth_lik_diff
are then not independent), samples that repeat an index (the row draws again), rows of 10, 12 and 16 lanes, and a depth table that a
chain outgrows inside the loop. The common path is covered by tests/test_gpu_solve.py and tests/test_gpu_greedy_trivial_alternatives.py;
every test here first asserts, from the oracle's arrays on the CPU, that its input holds the case, and then compares the device's chains
with the oracle's as the other greedy tests do (stages.compare_stage: likelihood of every chain, mean and variance per genotype). The
oracle reports no iteration counts: iterations and accepted moves (api.solve_stats) are compared between the layouts of the loop, which
run the same chains."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, synth
from tests import oracle_ffi as O
from tests import test_gpu_solve as stages

pytestmark = pytest.mark.gpu

# name -> (alleles, read pairs, allele length, model parameters; "window": the depth windows' size instead of the background's 100)
INPUTS = {
    "many locations": (8, 3000, 20000, dict(prob_diff=60.0, unmapped_penalty=-5.0)),
    "many locations, no tweak": (8, 3000, 20000, dict(prob_diff=60.0, unmapped_penalty=-5.0, tweak=0)),
    "short alleles, no tweak": (6, 1500, 1500, dict(tweak=0)),
    "windows of 400, no tweak": (8, 3000, 20000, dict(prob_diff=60.0, unmapped_penalty=-5.0, tweak=0, window=400)),
    "16 non-trivial reads": (4, 20, 5000, {}),
    "36 non-trivial reads": (4, 40, 5000, {}),
    "7 non-trivial reads": (4, 8, 5000, {}),
    "1 non-trivial read": (4, 1, 5000, {}),
}
_made = {}


def setup_with_windows(ctx, n_alleles, n_pairs, base_len, window, **prm):
    """stages.setup() with depth windows of another size (the mates of a pair, some 300 bases apart, then often lie in ONE window)."""
    L = synth.SynthLocus(n_alleles, n_pairs, seed=31, base_len=base_len)
    L.bg.window = window
    L.bg.neighb = max(L.bg.neighb, window)
    p = api.default_params()
    for k, v in prm.items():
        setattr(p, k, v)
    api.resolve_params(p, L.bg)
    loc = api.Locus(ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    aa = api.AllAlignments.load(loc, L.reads(0, n_pairs))
    st, w, unm, uk = aa.status()
    off, pa = aa.pair_alns()
    ol = O.OracleLocus(L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    ol.inject_tables(loc.depth_lut(), loc.window_weights())
    oa = O.alns_from_arrays(n_alleles, st, w, unm, off, pa)
    return L, p, loc, aa, ol, oa


def the_input(ctx, name):
    """The set-up of an input, once for the tests of this file: (batch, oracle locus, oracle alignments, diploid genotypes)."""
    if name not in _made:
        n_alleles, n_pairs, base_len, prm = INPUTS[name]
        prm = dict(prm)
        window = prm.pop("window", None)
        if window is None:
            L, p, loc, aa, ol, oa = stages.setup(ctx, n_alleles, n_pairs, base_len, **prm)
        else:
            L, p, loc, aa, ol, oa = setup_with_windows(ctx, n_alleles, n_pairs, base_len, window, **prm)
        _made[name] = (aa, ol, oa, api.generate_genotypes(n_alleles, 2))
    return _made[name]


def rare_reads(ol, oa, gts, tweak_key=99):
    """Over the genotypes, from the oracle's GenotypeAlignments after apply_tweak: reads with more than four locations; reads with an
    alternative location that shares a window which carries a distribution (a window above 1) with their best (first) location — all of
    them, and those where one of the two locations has both mates in ONE window (a depth then changes by two against a change by one; with
    two windows each the shared window simply does not change); and the number of non-trivial reads of every genotype."""
    deep = shared = shared_one = 0
    non_trivial = []
    for ids in gts:
        g = O.OracleGtAlns(ol, oa, ids)
        g.apply_tweak(tweak_key)
        a = g.arrays()
        rix = a["read_ixs"].astype(np.int64)
        win = a["windows"].astype(np.int64)
        n_loc = np.diff(rix)
        first = np.repeat(rix[:-1], n_loc)                                  # the read's first location, for each of its locations
        alternative = np.arange(len(win)) != first
        hit = np.zeros(len(win), dtype=bool)
        for c in (0, 1):
            hit |= (win[:, c] >= 2) & ((win[:, c] == win[first, 0]) | (win[:, c] == win[first, 1]))
        hit &= alternative
        one_window = hit & ((win[first, 0] == win[first, 1]) | (win[:, 0] == win[:, 1]))
        deep += int(np.sum(n_loc > 4))
        shared += int(np.sum((np.add.reduceat(hit.astype(np.int64), rix[:-1]) > 0) & (n_loc >= 2)))
        shared_one += int(np.sum((np.add.reduceat(one_window.astype(np.int64), rix[:-1]) > 0) & (n_loc >= 2)))
        non_trivial.append(g.n_nontrivial)
    return deep, (shared, shared_one), non_trivial


def device_chains(aa, gts, solver, attempts, seeds, ref):
    """The device's stage against likelihoods the oracle gave before (compare_stage's bound); returns likelihoods and solve_stats."""
    gm, gv, gl = api.solve_stage(aa, gts, solver, attempts, seeds)
    assert np.abs(gl - ref).max() <= 1e-9 * np.abs(ref).max()
    return gl, api.solve_stats(aa)


def test_reads_with_more_than_four_locations_and_a_current_location_beyond_the_fourth(gpu_ctx):
    """13 genotypes x 2 attempts from the best start and from a random one. A random start puts a read with n > 4 locations beyond the
    fourth with probability (n - 4) / n >= 1 / 5: with the 1 000 such reads asserted, some hundred candidates of the first iterations have
    their current location in the chain's run."""
    aa, ol, oa, gts = the_input(gpu_ctx, "many locations")
    sub = np.ascontiguousarray(gts[:13])
    deep, shared, nnt = rare_reads(ol, oa, sub)
    print("reads with more than four locations:", deep, "with a shared window (all, one-window pairs):", shared)
    assert deep >= 1000
    seeds = api.chain_seeds(1234, 26)
    for best_start in (0, 1):
        g = api.default_solver(cdefs.SOLVER_GREEDY)
        g.best_start = best_start
        stages.compare_stage(aa, ol, oa, sub, g, 2, seeds)


@pytest.mark.parametrize("name,one_window", [("many locations, no tweak", 0), ("short alleles, no tweak", 0), ("windows of 400, no tweak", 1000)])
def test_alternatives_that_share_a_window_with_the_current_pair(gpu_ctx, name, one_window):
    """A read's several pair-alignments on one contig lie close to each other: without the tweak many of them share a window, and on short
    alleles the locations fall into few windows. With windows of 400 bases a third of these reads has both mates of a location in one
    window: the case in which the depths of the shared window are not the gathered ones."""
    aa, ol, oa, gts = the_input(gpu_ctx, name)
    sub = np.ascontiguousarray(gts[:13])
    deep, shared, nnt = rare_reads(ol, oa, sub)
    print(name, "- reads with a shared window (all, one-window pairs):", shared, "with more than four locations:", deep)
    assert shared[0] - shared[1] >= 100 and shared[1] >= one_window
    seeds = api.chain_seeds(77, 26)
    for best_start in (1, 0):
        g = api.default_solver(cdefs.SOLVER_GREEDY)
        g.best_start = best_start
        stages.compare_stage(aa, ol, oa, sub, g, 2, seeds)


@pytest.mark.parametrize("name,lo,hi", [("16 non-trivial reads", 12, 40), ("36 non-trivial reads", 12, 40), ("7 non-trivial reads", 2, 9),
                                        ("1 non-trivial read", 1, 1)])
def test_samples_that_repeat_an_index(gpu_ctx, name, lo, hi):
    """A sample of 10 out of n reads is without a repeat with probability n! / ((n - 10)! n^10): 0.026 for n = 16, 0.25 for n = 36 — the
    row draws again in most iterations. Fewer than 10 non-trivial reads: the sample is all of them (S = n) and every draw beyond the
    first collides with probability up to (n - 1) / n. One read: a sample of one. These chains end at the plateau."""
    aa, ol, oa, gts = the_input(gpu_ctx, name)
    deep, shared, nnt = rare_reads(ol, oa, gts)
    print(name, "- non-trivial reads per genotype:", nnt)
    assert all(lo <= n <= hi for n in nnt)
    seeds = api.chain_seeds(5, 3 * len(gts))
    for best_start in (1, 0):
        g = api.default_solver(cdefs.SOLVER_GREEDY)
        g.best_start = best_start
        ref = stages.compare_stage(aa, ol, oa, gts, g, 3, seeds)[2]
        chains, iterations, accepted = api.solve_stats(aa)
        assert chains == 3 * len(gts) and iterations < chains * 100000          # no chain ran to the limit of iterations
        for cpw in (5, 6):                                                   # the rows of 12 and 10 lanes draw again through another exchange
            gpu_ctx.set_knob("solve_chains_per_wave", cpw)
            try:
                gl, stats = device_chains(aa, gts, g, 3, seeds, ref)
            finally:
                gpu_ctx.set_knob("solve_chains_per_wave", -1)
            assert stats == (chains, iterations, accepted), cpw


def test_rows_of_10_12_and_16_lanes_on_the_input_with_most_locations(gpu_ctx):
    """Six, five and four chains per wavefront and both homes of the window weights, from a random start: the oracle's chains (computed
    once), the same iterations and accepted moves in every layout, the two weight layouts bit for bit."""
    aa, ol, oa, gts = the_input(gpu_ctx, "many locations")
    sub = np.ascontiguousarray(gts[:13])
    assert rare_reads(ol, oa, sub)[0] >= 1000
    seeds = api.chain_seeds(1234, 26)
    g = api.default_solver(cdefs.SOLVER_GREEDY)
    g.best_start = 0
    ref = stages.compare_stage(aa, ol, oa, sub, g, 2, seeds)[2]
    stats = api.solve_stats(aa)
    for cpw in (4, 5, 6):
        gpu_ctx.set_knob("solve_chains_per_wave", cpw)
        try:
            tables, st_t = device_chains(aa, sub, g, 2, seeds, ref)
            gpu_ctx.set_knob("solve_lds_weights", 0)
            gathered, st_g = device_chains(aa, sub, g, 2, seeds, ref)
        finally:
            gpu_ctx.set_knob("solve_lds_weights", -1)
            gpu_ctx.set_knob("solve_chains_per_wave", -1)
        assert np.array_equal(tables, gathered), cpw
        assert st_t == stats and st_g == stats, cpw


_M64 = (1 << 64) - 1


def _counter_u64(key, i):
    """oracle/lcty_oracle_solve.c: orc_counter_u64."""
    z = (key + (i + 1) * 0x9e3779b97f4a7c15) & _M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M64
    return z ^ (z >> 31)


def start_and_final_depth(ol, oa, ids, solver, seed):
    """The deepest window that carries a distribution in the random start of the oracle's chain (rassgn_init: a counter draw per
    non-trivial read under key ^ INIT_KEY_XOR) and in the assignment the chain ends with."""
    seed = int(seed)
    g = O.OracleGtAlns(ol, oa, ids)
    g.apply_tweak(seed)
    a = g.arrays()
    weight = g.window_distr()[1]
    rix = a["read_ixs"].astype(np.int64)
    win = a["windows"].astype(np.int64)
    n_loc = np.diff(rix)
    start = np.array([(_counter_u64(seed ^ 0x8CB92BA72F3D8DD7, r) * int(n_loc[r])) >> 64 if n_loc[r] > 1 else 0 for r in range(len(n_loc))],
                     dtype=np.int64)
    final = g.solve(solver, seed)[1].astype(np.int64)
    deepest = []
    for assignment in (start, final):
        depth = np.bincount(win[rix[:-1] + assignment].ravel(), minlength=len(weight))
        deepest.append(int(depth[weight != 0.0].max()))
    return deepest


def test_a_depth_table_that_a_chain_outgrows_inside_the_loop(gpu_ctx):
    """A table of 256 depths (the narrowest) and chains that start, from a random assignment, below depth 256 in every window and end with a
    window above it: the initialisation raises no flag, a candidate of the loop is the first to look past the table (`overflow` = 1), the
    host widens the table and repeats the batch. The result is the oracle's. (tests/test_gpu_solve.py starts a table far below the depths
    of the chains' start: there the flag is raised before the loop's first iteration.)"""
    gpu_ctx.set_knob("depth_table_start", 256)
    try:
        L, p, loc, aa, ol, oa = stages.setup(gpu_ctx, 4, 7000, 4000)
        pick = [3, 5, 6, 8]
        sub = np.ascontiguousarray(api.generate_genotypes(4, 2)[pick])
        seeds = np.ascontiguousarray(api.chain_seeds(8, 10)[pick])
        g = api.default_solver(cdefs.SOLVER_GREEDY)
        g.best_start = 0
        for ids, seed in zip(sub, seeds):
            d_start, d_final = start_and_final_depth(ol, oa, ids, g, seed)
            print(tuple(int(x) for x in ids), "deepest window at the start", d_start, "at the end", d_final)
            assert d_start <= 255 < d_final
        stages.compare_stage(aa, ol, oa, sub, g, 1, seeds)
    finally:
        gpu_ctx.set_knob("depth_table_start", -1)
