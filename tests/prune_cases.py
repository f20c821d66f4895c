"""Designed inputs of the pruning tests (tests/test_prune_host.py, tests/test_gpu_prune.py): triangles for the clustering, and
(triangle, multiplicities, parameters) for the cut and the representatives. Expected values come from tests/pyref_prune.py, once per process."""
import functools

import numpy as np

from tests import pyref_prune as R


class Case:
    def __init__(self, name, n, tri, distinct, mult=None, **params):
        self.name, self.n, self.tri, self.distinct = name, n, np.ascontiguousarray(tri, dtype=np.float64), distinct
        assert len(self.tri) == n * (n - 1) // 2
        self.mult = None if mult is None else np.ascontiguousarray(mult, dtype=np.uint32)
        self.params = params                     # threshold, n_clusters, power as pyref_prune.cluster_haplotypes names them


def _from_matrix(M):
    n = len(M)
    return np.array([M[i][j] for i, j in R.triangle_indices(n)], dtype=np.float64)


def _distinct(n, seed):
    """a shuffled arange scaled into 1e-5 .. 1e-2: every value once"""
    m = n * (n - 1) // 2
    v = 1e-5 + (1e-2 - 1e-5) * np.arange(m, dtype=np.float64) / max(m - 1, 1)
    np.random.default_rng(seed).shuffle(v)
    assert len(np.unique(v)) == m
    return v


def _blocks(sizes, seed, inside=(1e-5, 1e-4), across=(1e-2, 2e-2)):
    """cliques: distinct values inside a block well below distinct values across blocks; the members of a block are interleaved"""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    owner = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(owner)
    pairs = R.triangle_indices(n)
    same = np.array([owner[i] == owner[j] for i, j in pairs])
    tri = np.zeros(len(pairs))
    a = np.linspace(inside[0], inside[1], int(same.sum())); rng.shuffle(a)
    b = np.linspace(across[0], across[1], int((~same).sum())); rng.shuffle(b)
    tri[same], tri[~same] = a, b
    return n, tri, owner


def _linkage_cases():
    cs = [Case("n1", 1, [], True), Case("n2", 2, [3e-4], True), Case("n3", 3, [3e-4, 1e-4, 2e-4], True)]
    for n in (65, 257, 1025):                    # one past a wavefront, a 256-thread block, the 1 024-thread workgroup of the merge loop
        cs.append(Case(f"distinct{n}", n, _distinct(n, n), True))
    cs.append(Case("all_equal9", 9, np.full(36, 2e-4), False))
    M = np.full((20, 20), 5e-3)
    for b in range(4):
        M[5 * b:5 * b + 5, 5 * b:5 * b + 5] = 1e-4
    cs.append(Case("two_level", 20, _from_matrix(M), False))
    rng = np.random.default_rng(40)
    cs.append(Case("five_values40", 40, rng.choice([1e-4, 2e-4, 3e-4, 1e-3, 5e-3], 40 * 39 // 2), False))
    # star: haplotype 0 is every other's nearest, so the first merge sends every row back to a scan
    n = 130
    M = np.zeros((n, n))
    far = _distinct(n, 7) + 2e-2
    for t, (i, j) in enumerate(R.triangle_indices(n)):
        M[i][j] = M[j][i] = far[t]
    for x in range(1, n):
        M[0][x] = M[x][0] = 1e-4 + 1e-6 * x
    cs.append(Case("star130", n, _from_matrix(M), True))
    # 30 % of the pairs missing, n_clusters mode: the missing ones are +inf
    n = 30
    tri = _distinct(n, 30)
    tri[np.random.default_rng(31).random(len(tri)) < 0.3] = np.inf
    cs.append(Case("inf30", n, tri, False, n_clusters=6))
    return cs


def _cluster_cases():
    cs = []
    # cut boundaries on a small distinct triangle
    n = 12
    tri = _distinct(n, 12)
    steps = R.linkage(list(tri), n)
    at = steps[5][2]
    cs.append(Case("cut_equal_to_step", n, tri, True, threshold=at))             # merged at the step, not cut: strictly greater cuts
    cs.append(Case("cut_just_below_step", n, tri, True, threshold=float(np.nextafter(at, 0.0))))
    cs.append(Case("cut_zero", n, tri, True, threshold=0.0))
    cs.append(Case("cut_below_min", n, tri + 1.0, True, threshold=0.5))         # minimal divergence above the threshold: all kept
    cs.append(Case("cut_above_all", n, tri, True, threshold=1.0))               # nothing exceeds: the root is the one cluster
    for k in (1, n - 1, n, n + 3):
        cs.append(Case(f"n_clusters_{k}", n, tri, True, n_clusters=k))
    cs.append(Case("n_clusters_ties", 20, _by_name_linkage("two_level").tri, False, n_clusters=7))
    # representatives: cliques of 2, 64, 65 and 300 (below, at, one past a wavefront; more than the 256 threads of a workgroup)
    n, tri, owner = _blocks([2, 64, 65, 300], 5)
    mult = np.random.default_rng(6).choice([1, 2, 7], n).astype(np.uint32)
    for p in (2, 1, 3, -1, -2, R.POWER_MIN, R.POWER_MAX):
        cs.append(Case(f"repr_power_{p}", n, tri, True, mult=mult, threshold=1e-3, power=p))
    cs.append(Case("repr_no_mult", n, tri, True, threshold=1e-3, power=2))
    cs.append(Case("repr_power_0", n, tri, True, mult=mult, threshold=1e-3, power=0))
    # two equal best sums: in a clique of equal distances without multiplicities every member adds the same terms, the first member wins
    M = np.full((7, 7), 3e-2)
    for grp in ((1, 3, 5), (0, 2, 4, 6)):
        for i in grp:
            for j in grp:
                M[i][j] = 1e-4
    cs.append(Case("repr_tie", 7, _from_matrix(M), False, threshold=1e-3, power=2))
    cs.append(Case("repr_tie_neg", 7, _from_matrix(M), False, threshold=1e-3, power=-1))
    return cs


LINKAGE = _linkage_cases()


def _by_name_linkage(name):
    return next(c for c in LINKAGE if c.name == name)


CLUSTER = LINKAGE + _cluster_cases()
assert len({c.name for c in CLUSTER}) == len(CLUSTER)


def by_name(name):
    return next(c for c in CLUSTER if c.name == name)


@functools.lru_cache(maxsize=None)
def _steps_of(key):
    c = by_name(key)
    return R.linkage(list(c.tri), c.n)


def expected_steps(name):
    """pyref steps of a case; cases that share a triangle share the computation"""
    c = by_name(name)
    for o in CLUSTER:                            # the first case with the same triangle owns the result
        if o.n == c.n and (o.tri is c.tri or np.array_equal(o.tri, c.tri)):
            return _steps_of(o.name)
    raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """pyref_prune.cluster_haplotypes of a case (names h0 .. h<n-1>, no old discarded file)"""
    c = by_name(name)
    p = c.params
    disc = None if c.mult is None else {i: [f"d{i}_{t}" for t in range(int(m) - 1)] for i, m in enumerate(c.mult) if m > 1}
    return R.cluster_haplotypes(names(c), list(c.tri), p.get("threshold", 0.0002), p.get("n_clusters"), p.get("power", 2), disc,
                                steps=expected_steps(name))


def names(c):
    return [f"h{i}" for i in range(c.n)]
