"""The basis step on the device (lcty_basis_windows / _constraints / _build) against tests/pyref_basis.py, the reference's serial walk:
bit rows for equality, unique and minimal rows as sets, the basis for cover, size and repeatability."""
import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, synth
from tests import pyref_basis as R
from tests.test_basis_host import DESIGNED

pytestmark = pytest.mark.gpu

# The synthetic cases. Chosen with pyref alone on the CPU so that the case cannot pass vacuously (asserted in _synth_case):
#   A = 8,  base_len 4 000, divergence 0.005, window 200 (max_window_edit 1): 26 unique rows, minimum basis 5
#   A = 64, base_len 6 000, divergence 0.004, window 250 (max_window_edit 1): 133 unique rows, greedy basis 8
SYNTH = {8: dict(base_len=4000, divergence=0.005, window=200), 64: dict(base_len=6000, divergence=0.004, window=250)}


@pytest.fixture(scope="module")
def gpu_ctx():
    return api.Context(0)


def _ints(rows):
    return api._rows_ints(rows)


def _table(win_off, rows):
    ints = _ints(rows)
    return [ints[int(win_off[a]):int(win_off[a + 1])] for a in range(len(win_off) - 1)]


def _params_for(window, step, max_edit, **kw):
    # floor(window * divergence) == max_edit, away from both neighbours
    return api.basis_params(divergence=(max_edit + 0.5) / window, window=window, step=step, **kw)


@pytest.mark.parametrize("case", DESIGNED, ids=[c[0] for c in DESIGNED])
def test_windows_on_designed_cigars(gpu_ctx, case):
    _, text, in_query, window, step, max_edit, want = case
    cg = R.parse_cigar(text)
    lens = [R.query_len(cg), R.ref_len(cg)]
    nm = sum(n for op, n in cg if op == "=")
    e = [(0, 1, np.array(R.cigar_words(cg), dtype=np.uint32), nm, sum(n for _, n in cg))]
    p = _params_for(window, step, max_edit)
    win_off, rows, st = api.basis_windows(gpu_ctx, lens, e, p)
    ref = R.row_table(lens, e, p.divergence, window, step)
    assert _table(win_off, rows) == ref
    side = 0 if in_query else 1
    if lens[side] > window:                                                       # the hand-derived answer, through the device
        assert [w for w, r in enumerate(ref[side]) if r >> (1 - side) & 1] == want
    assert st["n_walks"] == 2 and st["n_rows_raw"] == sum(len(r) for r in ref)


def test_windows_on_short_sides(gpu_ctx):
    # length == window, < window, and one side short while the other is not; the short side asks n_matches / aln_len
    for text, nm, al, div in (("4=", 4, 4, 0.3), ("3=1X", 3, 4, 0.25), ("3=1X", 3, 4, 0.2), ("3=", 3, 3, 0.0), ("4=6I", 4, 10, 0.6), ("4=6I", 4, 10, 0.5),
                              ("4=", 0, 0, 0.99), ("4=", 0, 0, 1.0)):
        cg = R.parse_cigar(text)
        lens = [R.query_len(cg), R.ref_len(cg)]
        e = [(0, 1, np.array(R.cigar_words(cg), dtype=np.uint32), nm, al)]
        p = api.basis_params(divergence=div, window=4, step=2)
        win_off, rows, _ = api.basis_windows(gpu_ctx, lens, e, p)
        assert _table(win_off, rows) == R.row_table(lens, e, div, 4, 2), (text, div)


def _long_cigar(n_blocks, rng):
    """more runs than one LDS chunk of the kernel (1 024): short blocks of =, X, I, D in seeded order, gaps next to each other included"""
    cg = []
    for _ in range(n_blocks):
        op = "=XID="[int(rng.integers(5))]
        ln = int(rng.integers(1, 9)) if op == "=" else int(rng.integers(1, 3))
        if cg and cg[-1][0] == op:
            cg[-1] = (op, cg[-1][1] + ln)
        else:
            cg.append((op, ln))
    return cg


@pytest.mark.parametrize("window,step,max_edit", [(40, 0, 12), (300, 7, 100), (2500, 1, 900), (16, 16, 5)])
def test_windows_on_cigars_longer_than_one_lds_chunk(gpu_ctx, window, step, max_edit):
    rng = np.random.default_rng(window)
    ents, lens = [], []
    for i, blocks in enumerate((2500, 3500, 6000, 2000)):
        cg = _long_cigar(blocks, rng)
        if i == 2:
            cg = [("I", 3)] + cg + [("D", 2), ("I", 4)]                           # leading and trailing gaps on both sides
        assert len(cg) > 1024
        lens += [R.query_len(cg), R.ref_len(cg)]
        ents.append((2 * i, 2 * i + 1, np.array(R.cigar_words(cg), dtype=np.uint32), sum(n for op, n in cg if op == "="), sum(n for _, n in cg)))
    p = _params_for(window, step, max_edit)
    win_off, rows, _ = api.basis_windows(gpu_ctx, lens, ents, p)
    ref = R.row_table(lens, ents, p.divergence, window, step or None)
    got = _table(win_off, rows)
    assert got == ref
    assert any(r != 1 << a for a, rr in enumerate(ref) for r in rr) and any(r == 1 << a for a, rr in enumerate(ref) for r in rr)


_cache = {}


def _synth_case(A):
    if A not in _cache:
        c = SYNTH[A]
        L = synth.SynthLocus(A, 16, base_len=c["base_len"])
        lens = [int(x) for x in np.diff(L.seq_off.astype(np.int64))]
        ents = L.hap_alns()
        rows = R.row_table(lens, ents, c["divergence"], c["window"])
        uniq = R.unique_rows(rows)
        greedy = R.greedy_cover(A, uniq)
        assert len(uniq) > A and 1 < len(greedy) < A                              # the conditions the case was chosen for
        _cache[A] = (lens, ents, rows, uniq, greedy)
    return _cache[A]


@pytest.mark.parametrize("A", [8, 64])
def test_windows_equal_pyref_on_a_synthetic_locus(gpu_ctx, A):
    lens, ents, rows, uniq, greedy = _synth_case(A)
    p = api.basis_params(divergence=SYNTH[A]["divergence"], window=SYNTH[A]["window"])
    win_off, got, st = api.basis_windows(gpu_ctx, lens, ents, p)
    assert _table(win_off, got) == rows
    assert st["n_entries"] == A * (A - 1) // 2 and st["n_walks"] == A * (A - 1)


@pytest.mark.parametrize("A", [8, 64])
def test_constraints_equal_pyref_as_sets(gpu_ctx, A):
    lens, ents, rows, uniq, greedy = _synth_case(A)
    raw = api.basis_rows_from_ints(A, [r for contig in rows for r in contig])
    u, st = api.basis_constraints(gpu_ctx, A, raw, minimal=False)
    assert len(u) == len(uniq) == st["n_rows_unique"] and set(_ints(u)) == uniq
    m, st = api.basis_constraints(gpu_ctx, A, raw, minimal=True)
    want = {r for r in uniq if not any(o != r and o & r == o for o in uniq)}      # the subset filter, written out
    assert len(m) == len(want) == st["n_rows_minimal"] and set(_ints(m)) == want
    assert 0 < len(want) < len(uniq)
    # a fixed order: by number of bits, and the same from call to call
    pops = [bin(v).count("1") for v in _ints(u)]
    assert pops == sorted(pops)
    u2, _ = api.basis_constraints(gpu_ctx, A, raw[::-1].copy(), minimal=False)
    assert np.array_equal(u, u2)


def test_constraints_on_wide_rows_and_repeats(gpu_ctx):
    # 200 haplotypes = 7 words; many repeats, nested rows, rows that differ in the last word only
    rng = np.random.default_rng(3)
    n = 200
    base = [int(sum(1 << int(i) for i in rng.choice(n, int(rng.integers(1, 12)), replace=False))) for _ in range(300)]
    ints = base * 5 + [b | 1 << 199 for b in base[:100]] + [b | 1 << int(rng.integers(n)) for b in base[:150]]
    order = rng.permutation(len(ints))
    raw = api.basis_rows_from_ints(n, [ints[i] for i in order])
    u, _ = api.basis_constraints(gpu_ctx, n, raw, minimal=False)
    assert set(_ints(u)) == set(ints) and len(u) == len(set(ints))
    m, _ = api.basis_constraints(gpu_ctx, n, raw, minimal=True)
    assert set(_ints(m)) == R.minimal_rows(set(ints)) and len(m) == len(R.minimal_rows(set(ints)))


def test_build_at_8_alleles_equals_brute_force(gpu_ctx):
    lens, ents, rows, uniq, greedy = _synth_case(8)
    p = api.basis_params(divergence=SYNTH[8]["divergence"], window=SYNTH[8]["window"])
    ids, bound, optimal, st = api.basis_build(gpu_ctx, lens, ents, p)
    assert R.is_cover(ids, uniq)                                                  # every pyref row is hit
    assert optimal and len(ids) == bound == R.brute_force_min(8, uniq)
    assert 1 < len(ids) < 8
    assert (st["n_rows_raw"], st["n_rows_unique"]) == (sum(len(r) for r in rows), len(uniq))
    assert st["n_rows_minimal"] == len(R.minimal_rows(uniq))
    ids2, bound2, optimal2, _ = api.basis_build(gpu_ctx, lens, ents, p)
    assert list(ids2) == list(ids) and (bound2, optimal2) == (bound, optimal)
    ids3, bound3, optimal3, st3 = api.basis_build(gpu_ctx, lens, ents, api.basis_params(divergence=p.divergence, window=p.window, minimal=0))
    assert optimal3 and len(ids3) == len(ids) and st3["n_rows_minimal"] == len(uniq)     # without the presolve: the same size


def test_build_at_64_alleles(gpu_ctx):
    lens, ents, rows, uniq, greedy = _synth_case(64)
    p = api.basis_params(divergence=SYNTH[64]["divergence"], window=SYNTH[64]["window"])
    ids, bound, optimal, st = api.basis_build(gpu_ctx, lens, ents, p)
    assert R.is_cover(ids, uniq)
    assert bound <= len(ids) <= len(greedy) and (not optimal or bound == len(ids))
    assert list(ids) == sorted(set(int(i) for i in ids))
    ids2, bound2, optimal2, _ = api.basis_build(gpu_ctx, lens, ents, p)
    assert list(ids2) == list(ids) and (bound2, optimal2) == (bound, optimal)


def test_leave_out_and_small_batches_give_the_same_rows(gpu_ctx):
    lens, ents, rows, uniq, greedy = _synth_case(64)
    c = SYNTH[64]
    p = api.basis_params(divergence=c["divergence"], window=c["window"])
    out = [3, 17, 63]
    ref = R.row_table(lens, ents, c["divergence"], c["window"], leave_out=out)
    assert all(not any(r >> o & 1 for o in out) for contig in ref for r in contig) and [len(ref[o]) for o in out] == [0, 0, 0]
    win_off, got, st1 = api.basis_windows(gpu_ctx, lens, ents, p, leave_out=out)
    assert _table(win_off, got) == ref and st1["n_batches"] == 1
    gpu_ctx.set_knob("basis_batch_words", 100)                                    # a few entries per batch
    try:
        win_off2, got2, st2 = api.basis_windows(gpu_ctx, lens, ents, p, leave_out=out)
        win_off3, got3, st3 = api.basis_windows(gpu_ctx, lens, ents, p)
        ids_small, _, _, _ = api.basis_build(gpu_ctx, lens, ents, p, leave_out=out)
    finally:
        gpu_ctx.set_knob("basis_batch_words", -1)
    assert st2["n_batches"] > 10 and np.array_equal(win_off, win_off2) and np.array_equal(got, got2)
    assert _table(win_off3, got3) == rows and st3["n_batches"] > 10
    ids, _, _, _ = api.basis_build(gpu_ctx, lens, ents, p, leave_out=out)
    assert list(ids) == list(ids_small) and not set(int(i) for i in ids) & set(out)
    assert R.is_cover(ids, R.unique_rows(ref))


def test_device_errors(gpu_ctx):
    def raises(code, fn):
        with pytest.raises(_lib.LocityperError) as e:
            fn()
        assert e.value.code == code
    w = np.array(R.cigar_words(R.parse_cigar("10=")), dtype=np.uint32)
    p = api.basis_params(divergence=0.1, window=4, step=2)
    raises(cdefs.ERR_INVALID_DATA, lambda: api.basis_windows(gpu_ctx, [10, 12], [(0, 1, w, 10, 10)], p))          # the target is longer than the CIGAR
    raises(cdefs.ERR_INVALID_DATA, lambda: api.basis_windows(gpu_ctx, [8, 10], [(0, 1, w, 10, 10)], p))           # the CIGAR is longer than the query
    s = np.array(R.cigar_words([("S", 2), ("=", 8)]), dtype=np.uint32)
    raises(cdefs.ERR_INVALID_DATA, lambda: api.basis_windows(gpu_ctx, [10, 8], [(0, 1, s, 8, 10)], p))            # an operation outside M = X I D
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.basis_windows(gpu_ctx, [10, 10], [(0, 2, w, 10, 10)], p))         # a contig the locus does not have
    raises(cdefs.ERR_INVALID_INPUT, lambda: api.basis_windows(gpu_ctx, [10, 10], [(0, 1, w, 10, 10)], api.basis_params(window=0)))
    # self-alignments and entries without a CIGAR are passed over, as in the reference
    win_off, rows, st = api.basis_windows(gpu_ctx, [10, 10], [(0, 0, w, 10, 10), (0, 1, w[:0], 10, 10)], p)
    assert st["n_entries"] == 0 and _ints(rows) == [1] * 4 + [2] * 4
