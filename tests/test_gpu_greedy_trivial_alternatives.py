"""The greedy loop takes no depth gathers for an alternative location that lies in windows 0 and 1 only ("both mates unmapped", out of
region): those two windows carry WindowDistr::TRIVIAL (assgn.rs:71-76, 140), so both of the alternative's terms are 0.0 whatever the depths.
Only alternatives with a window above 1 take gathers, and an iteration a second round only for those. Every chain must stay the oracle's chain, on inputs that hold every class of
read the slot rule could get wrong, and a caller of lcty_solve_given who DOES give windows 0 and 1 a weight must get them honoured."""
import numpy as np
import pytest

from locityper_amd import api, cdefs
from tests import oracle_ffi as O
from tests import test_gpu_solve as stages
from tests import test_gpu_solve_given as given

pytestmark = pytest.mark.gpu

# name -> (alleles, read pairs, allele length, ploidy, model parameters)
INPUTS = {
    "defaults": (8, 3000, 20000, 2, {}),
    "prob_diff 60": (8, 3000, 20000, 2, dict(prob_diff=60.0)),
    "unmapped_penalty -10": (8, 3000, 20000, 2, dict(unmapped_penalty=-10.0)),
    "prob_diff 60, unmapped_penalty -5": (8, 3000, 20000, 2, dict(prob_diff=60.0, unmapped_penalty=-5.0)),
    "ploidy 3": (6, 2500, 12000, 3, {}),
}
CLASSES = ("non-trivial", "2 locations, one trivial", "3 locations, one trivial", "3 locations, none trivial", "4 locations",
           "more than 4 locations", "3 or more locations and the best is trivial", "a location with one window below 2")
_made = {}


def the_input(ctx, name):
    """stages.setup() of an input, once for the tests of this file."""
    if name not in _made:
        n_alleles, n_pairs, base_len, ploidy, prm = INPUTS[name]
        L, p, loc, aa, ol, oa = stages.setup(ctx, n_alleles, n_pairs, base_len, **prm)
        _made[name] = (aa, ol, oa, api.generate_genotypes(n_alleles, ploidy))
    return _made[name]


def read_classes(ol, oa, gts, tweak_key=99):
    """Reads of each class, summed over the genotypes, from the oracle's GenotypeAlignments after apply_tweak."""
    n = dict.fromkeys(CLASSES, 0)
    for ids in gts:
        g = O.OracleGtAlns(ol, oa, ids)
        g.apply_tweak(tweak_key)
        a = g.arrays()
        rix = a["read_ixs"].astype(np.int64)
        win = a["windows"]
        low = win < 2
        trivial = (low[:, 0] & low[:, 1]).astype(np.int64)               # the location changes no window that carries a distribution
        one_low = (low[:, 0] ^ low[:, 1]).astype(np.int64)
        n_loc = np.diff(rix)
        n_triv = np.add.reduceat(trivial, rix[:-1])
        n_one = np.add.reduceat(one_low, rix[:-1])
        best_triv = trivial[rix[:-1]] == 1
        n[CLASSES[0]] += int(np.sum(n_loc >= 2))
        n[CLASSES[1]] += int(np.sum((n_loc == 2) & (n_triv == 1)))
        n[CLASSES[2]] += int(np.sum((n_loc == 3) & (n_triv == 1)))
        n[CLASSES[3]] += int(np.sum((n_loc == 3) & (n_triv == 0)))
        n[CLASSES[4]] += int(np.sum(n_loc == 4))
        n[CLASSES[5]] += int(np.sum(n_loc > 4))
        n[CLASSES[6]] += int(np.sum((n_loc >= 3) & best_triv))
        n[CLASSES[7]] += int(np.sum((n_loc >= 2) & (n_one > 0)))
    return n


def test_every_class_of_read_is_among_the_inputs(gpu_ctx):
    """A condition on the inputs, not on the solver: each class of read has at least five reads in at least one of them (first six
    genotypes, tweak key 99)."""
    most = dict.fromkeys(CLASSES, 0)
    for name in INPUTS:
        aa, ol, oa, gts = the_input(gpu_ctx, name)
        counts = read_classes(ol, oa, gts[:6])
        print(name, counts)
        for c in CLASSES:
            most[c] = max(most[c], counts[c])
    for c in CLASSES:
        assert most[c] >= 5, f"no input with five reads of the class '{c}'"


@pytest.mark.parametrize("name", list(INPUTS))
def test_greedy_chains_equal_the_oracle(gpu_ctx, name):
    """The first 13 genotypes x 2 attempts (26 chains: a last wavefront with spare rows), from the best start and from a random one — which
    puts reads on the trivial location, so that two real alternatives and the second round of gathers occur —, samples of 10 and of 3."""
    aa, ol, oa, gts = the_input(gpu_ctx, name)
    sub = np.ascontiguousarray(gts[:13])
    seeds = api.chain_seeds(1234, 26)
    for best_start in (1, 0):
        for sample in (10, 3):
            g = api.default_solver(cdefs.SOLVER_GREEDY)
            g.best_start, g.sample_size = best_start, sample
            stages.compare_stage(aa, ol, oa, sub, g, 2, seeds)


def test_layouts_of_the_loop_agree_on_the_input_with_most_locations(gpu_ctx):
    """Four, five and six chains per wavefront and both homes of the window weights on the fourth input: the oracle's chains in every
    layout; the two weight layouts bit for bit, the numbers of chains per wavefront within the order of a sum."""
    aa, ol, oa, gts = the_input(gpu_ctx, "prob_diff 60, unmapped_penalty -5")
    sub = np.ascontiguousarray(gts[:13])
    seeds = api.chain_seeds(1234, 26)
    for best_start in (1, 0):
        g = api.default_solver(cdefs.SOLVER_GREEDY)
        g.best_start = best_start
        ref = stages.compare_stage(aa, ol, oa, sub, g, 2, seeds)[2]
        for cpw in (4, 5, 6):
            gpu_ctx.set_knob("solve_chains_per_wave", cpw)
            try:
                tables = stages.compare_stage(aa, ol, oa, sub, g, 2, seeds)[2]
                gpu_ctx.set_knob("solve_lds_weights", 0)
                gathered = stages.compare_stage(aa, ol, oa, sub, g, 2, seeds)[2]
            finally:
                gpu_ctx.set_knob("solve_lds_weights", -1)
                gpu_ctx.set_knob("solve_chains_per_wave", -1)
            assert np.array_equal(tables, gathered), cpw
            assert np.allclose(tables, ref, rtol=1e-12, atol=0), cpw


def test_without_tweak(gpu_ctx):
    L, p, loc, aa, ol, oa = stages.setup(gpu_ctx, 8, 3000, 20000, tweak=0)
    sub = np.ascontiguousarray(api.generate_genotypes(8, 2)[:13])
    g = api.default_solver(cdefs.SOLVER_GREEDY)
    g.best_start = 0
    stages.compare_stage(aa, ol, oa, sub, g, 2, api.chain_seeds(1234, 26))


def test_given_weights_on_windows_0_and_1_are_honoured(gpu_ctx):
    """lcty_solve_given takes the caller's weight for EVERY window. With weights on windows 0 and 1 no location is trivial: the chain must
    be, bit for bit, the chain of the same object with every window moved up by two behind two windows of weight 0 — the random stream
    does not see window numbers, and that form has nothing in windows 0 and 1 to take the short way with."""
    L, p, loc, ol, oa = given.make(gpu_ctx, 6, 1200, 9000)
    table = loc.depth_table(1 << 13)
    rnd = np.random.default_rng(11)
    g = O.OracleGtAlns(ol, oa, (1, 4))
    v = given.view_of(g, p, 77)
    W = len(v["window_weight"])
    perm = np.concatenate([[0, 1], 2 + rnd.permutation(W - 2)]).astype(np.uint32)
    v["windows"] = perm[v["windows"]]
    v["window_weight"] = np.where(rnd.random(W) < 0.2, 0.0, rnd.random(W)); v["window_weight"][:2] = (0.7, 0.4)
    v["window_gc"] = rnd.integers(30, 70, W).astype(np.uint8)
    v["ln_prob"] = v["ln_prob"] - rnd.random(len(v["ln_prob"]))
    v["depth_contrib"], v["aln_contrib"] = 1.3, 0.7
    low = v["windows"] < 2
    n_loc = np.diff(v["read_ixs"]).astype(np.int64)
    several = np.repeat(n_loc >= 2, n_loc)
    assert int(np.sum(low[:, 0] & low[:, 1] & several)) >= 5              # locations that the stages' chains call trivial
    shifted = dict(v)
    shifted["windows"] = v["windows"] + 2
    shifted["window_weight"] = np.concatenate([[0.0, 0.0], v["window_weight"]])
    shifted["window_gc"] = np.concatenate([[0, 0], v["window_gc"]]).astype(np.uint8)
    for solver in given.solvers()[:2]:                                    # the two greedy ones: from the best start, from a random one
        lik, assgn, parts = api.solve_given(loc, solver=solver, rng_state=api.rng_seed_from_u64(3), **v)
        lik2, assgn2, parts2 = api.solve_given(loc, solver=solver, rng_state=api.rng_seed_from_u64(3), **shifted)
        assert np.array_equal(assgn, assgn2), f"{int((assgn != assgn2).sum())} of {len(assgn)} reads assigned differently"
        assert lik == lik2 and np.array_equal(parts, parts2)
        want, aln, dl = given.recompute(v, assgn, table)
        assert abs(lik - want) <= 1e-9 * abs(want) and abs(parts[1] - dl) <= 1e-9 * max(1.0, abs(dl))
