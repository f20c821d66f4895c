"""Pruning on the device: lcty_prune_linkage and lcty_prune_cluster against tests/pyref_prune.py on the designed inputs of
tests/prune_cases.py. Dissimilarities and accumulators bit for bit (power 0: rtol 1e-12, the device's log is not libm's)."""
import ctypes as C

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from tests import prune_cases as PC
from tests import pyref_prune as R

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _check_steps(got, want):
    assert len(got) == len(want)
    w = np.array([(a, b, d, sz, 0) for a, b, d, sz in want], dtype=cdefs.PRUNE_STEP_DTYPE) if want else np.zeros(0, dtype=cdefs.PRUNE_STEP_DTYPE)
    for f in ("cluster1", "cluster2", "size"):
        bad = np.nonzero(got[f] != w[f])[0]
        assert len(bad) == 0, f"{f} differs first at step {bad[0]}: {got[bad[0]]} != {w[bad[0]]}"
    assert _same_bits(got["dissimilarity"], w["dissimilarity"])


@pytest.mark.parametrize("name", [c.name for c in PC.LINKAGE])
def test_linkage_equals_the_transliteration(gpu_ctx, name):
    c = PC.by_name(name)
    steps, st = api.prune_linkage(gpu_ctx, c.n, c.tri)
    _check_steps(steps, PC.expected_steps(name))
    assert np.all(steps["dissimilarity"][1:] >= steps["dissimilarity"][:-1])   # complete linkage is monotone (inf >= inf holds)
    if c.n > 1:
        assert st["matrix_bytes"] == 8 * c.n * c.n and st["n_rescans"] >= c.n - 1
    if name == "star130":
        assert st["n_rescans"] >= 2 * c.n - 3                                   # the first merge sends every other row back to a scan


def _power_arg(p):
    return {R.POWER_MIN: "min", R.POWER_MAX: "max"}.get(p, p)


@pytest.mark.parametrize("name", [c.name for c in PC.CLUSTER])
def test_cluster_equals_the_transliteration(gpu_ctx, name):
    c, want = PC.by_name(name), PC.expected(name)
    power = c.params.get("power", 2)
    prm = api.prune_params(threshold=c.params.get("threshold", 0.0002), n_clusters=c.params.get("n_clusters") or 0, power=_power_arg(power))
    got = api.prune_cluster(gpu_ctx, c.n, c.tri, c.mult, prm)
    _check_steps(got["steps"], want["steps"])
    assert _same_bits([got["threshold"]], [want["threshold"]]) and _same_bits([got["epsilon"]], [want["epsilon"]])
    assert [list(m) for m in got["clusters"]] == want["clusters"]               # cluster order and member order
    assert list(got["keep_ids"]) == want["keep_ids"]
    for k, (acc, wacc) in enumerate(zip(got["acc"], want["acc"])):
        if not wacc:
            assert len(acc) == 1 and acc[0] == 0.0
            continue
        if power == 0:
            srt = sorted(wacc)
            assert srt[1] - srt[0] > 1e-9 * abs(srt[0]), f"cluster {k}: the case must keep its two best sums apart"
            assert np.allclose(acc, wacc, rtol=1e-12, atol=0.0)
        else:
            assert _same_bits(acc, wacc), f"accumulators of cluster {k} (power {power})"
    assert list(got["repr"]) == want["repr"]
    if "n_clusters" in c.params and c.distinct:
        assert len(got["keep_ids"]) == min(c.params["n_clusters"], c.n)


def test_refusal_above_the_size_limit(gpu_ctx):
    """n above LCTY_PRUNE_MAX_N is refused before the triangle is read or anything is allocated: a size-only call"""
    L = _lib.lib()
    tri = np.zeros(1)
    n = cdefs.PRUNE_MAX_N + 1
    assert cdefs.PRUNE_MAX_N >= 8192
    for call in (lambda: L.lcty_prune_linkage(gpu_ctx._h, n, tri.ctypes.data, None, None),
                 lambda: L.lcty_prune_cluster(gpu_ctx._h, n, tri.ctypes.data, None, C.byref(api.prune_params()), C.byref(cdefs.PruneOut()))):
        with pytest.raises(_lib.LocityperError) as e:
            _lib.check(call())
        assert e.value.code == cdefs.ERR_UNSUPPORTED and str(cdefs.PRUNE_MAX_N) in str(e.value)


def test_nan_is_refused(gpu_ctx):
    with pytest.raises(_lib.LocityperError) as e:
        api.prune_linkage(gpu_ctx, 3, [1e-3, np.nan, 2e-3])
    assert e.value.code == cdefs.ERR_INVALID_INPUT
