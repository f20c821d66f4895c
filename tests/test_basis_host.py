"""Host side of the basis step (`locityper augment`): tests/pyref_basis.py — the reference's serial walk — against hand-derived answers
on designed CIGARs, lcty_basis_tag and lcty_basis_select (the host branch and bound) against pyref and brute force, error statuses.
No device."""
import ctypes as C

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from tests import pyref_basis as R

# (name, CIGAR, IN_QUERY, window, step, max_edit, windows) — every answer below is derived by hand from the walk of cigar.rs:660-751:
# a window [s, s + window) counts the X / consuming-gap bases inside it and the non-consuming gaps at boundaries s < b <= s + window;
# the last window (s = len - window, index ceil(s / step)) also counts a non-consuming gap AT b = s, less what a trailing gap takes off.
DESIGNED = [
    ("all_equal_query", "10=", True, 4, 2, 0, [0, 1, 2, 3]),
    ("all_equal_ref", "10=", False, 4, 2, 0, [0, 1, 2, 3]),
    ("x_run_crosses_window_edge", "3=2X5=", True, 4, 2, 1, [0, 2, 3]),             # X at 3, 4: [0,4) has 1, [2,6) has 2, [4,8) has 1
    ("leading_I_query", "2I8=", True, 4, 2, 0, [1, 2, 3]),                         # I consumes the query: bases 0, 1 are edits
    ("leading_I_ref", "2I8=", False, 4, 2, 0, [0, 1, 2]),                          # gap at b = 0 is removed before s = 0 is emitted
    ("leading_D_query", "2D8=", True, 4, 2, 0, [0, 1, 2]),
    ("leading_D_ref", "2D8=", False, 4, 2, 0, [1, 2, 3]),
    ("trailing_I_query", "8=2I", True, 4, 2, 0, [0, 1, 2]),                        # bases 8, 9 are edits of the last window only
    ("trailing_I_ref", "8=2I", False, 4, 2, 0, [0, 1]),                            # gap at b = len: the last window has it
    ("trailing_I_ref_allowed", "8=2I", False, 4, 2, 2, [0, 1, 2]),
    ("trailing_D_query", "8=2D", True, 4, 2, 0, [0, 1]),
    ("trailing_D_ref", "8=2D", False, 4, 2, 0, [0, 1, 2]),
    ("gap_at_s_and_at_s_plus_window", "4=2I6=", False, 4, 2, 0, [2, 3]),           # b = 4: in [0,4] (b = s + window), in (2,6], not in s = 4
    ("gap_at_start_of_last_window", "6=2I4=", False, 4, 2, 0, [0]),                # b = 6 = s of the last window: counted there
    ("gap_at_last_start_and_trailing", "6=2I4=2I", False, 4, 2, 2, [0, 1, 2, 3]),  # G = 2 at s, c = 2 trailing: 2 + 2 - min(2, 2) = 2
    ("gap_at_last_start_and_trailing_tight", "6=2I4=2I", False, 4, 2, 1, [0]),
    ("gap_at_last_start_longer_than_trailing", "6=3D4=1D", True, 4, 2, 2, [0]),    # last: 3 + 1 - min(3, 1) = 3; [2,6] and (4,8] hold 3
    ("len_window_plus_1", "5=", True, 4, 2, 0, [0, 1]),
    ("step_not_dividing", "11=", True, 4, 3, 0, [0, 1, 2, 3]),
    ("step_not_dividing_last_bad", "10=1X", True, 4, 3, 0, [0, 1, 2]),
    ("step_equals_window", "12=", True, 4, 4, 0, [0, 1, 2]),
    ("step_one", "6=", True, 4, 1, 0, [0, 1, 2]),
    ("step_one_x", "2=1X3=", True, 4, 1, 0, []),                                   # X at base 2 lies in [0,4), [1,5) and the last window [2,6) alike
    ("step_one_x_front", "1X5=", True, 4, 1, 0, [1, 2]),
]


@pytest.mark.parametrize("case", DESIGNED, ids=[c[0] for c in DESIGNED])
def test_walk_on_designed_cigars(case):
    _, text, in_query, window, step, max_edit, want = case
    got = R.locally_similar(R.parse_cigar(text), in_query, window, step, max_edit)
    assert sorted(set(got)) == want


def test_short_sides_take_the_global_divergence():
    # update_bitarray: a side not longer than the window asks the PAF columns, not the CIGAR
    for text, ln in (("4=", 4), ("3=", 3)):                      # length == window, length < window
        cg = R.parse_cigar(text)
        assert R.update_bitarray(cg, True, 0.01, 4, 2, 0, 0.01) == [0]
        assert R.update_bitarray(cg, True, 0.0100001, 4, 2, 0, 0.01) == []
    assert R.global_div(0, 0) == 1.0 and R.global_div(99, 100) == 0.01
    assert R.n_windows(3, 4, 2) == 1 and R.n_windows(4, 4, 2) == 1 and R.n_windows(5, 4, 2) == 2 and R.n_windows(11, 4, 3) == 4


def test_row_table_of_two_contigs():
    # query 10 bases, target 8: "2I8=" — the query's windows 1..3 see the target, the target's windows 0..2 see the query
    e = [(0, 1, R.cigar_words(R.parse_cigar("2I8=")), 8, 10)]
    rows = R.row_table([10, 8], e, divergence=0.1, window=4, step=2)
    assert rows == [[0b01, 0b11, 0b11, 0b11], [0b11, 0b11, 0b11]]
    assert R.unique_rows(rows) == {0b01, 0b11} and R.minimal_rows({0b01, 0b11}) == {0b01}
    assert R.row_table([10, 8], e, divergence=0.1, window=4, step=2, leave_out=[1]) == [[1, 1, 1, 1], []]


def test_tag_against_pyref_and_hand_strings():
    assert api.basis_tag() == "x0.01-w250" == R.basis_tag()
    assert api.basis_tag(api.basis_params(step=100)) == "x0.01-w250-s100" == R.basis_tag(step=100)
    assert api.basis_tag(api.basis_params(window=cdefs.NONE_U32)) == "x0.01-global" == R.basis_tag(window=R.U32_MAX)
    assert api.basis_tag(leave_out_names=["A", "B"]) == "x0.01-w250-loA,B" == R.basis_tag(leave_out=["A", "B"])
    assert api.basis_tag(api.basis_params(window=1000, step=250000)) == "x0.01-w1k-s250k"        # PrettyU32
    for div in (0.0, 0.5, 0.123456789, 0.0002, 1.0, 0.05, 1e-7):
        for window, step in ((250, 0), (3000, 7), (2000000, 1000)):
            assert api.basis_tag(api.basis_params(divergence=div, window=window, step=step)) == R.basis_tag(div, window, step or None)
    assert api.basis_tag(api.basis_params(divergence=0.123456789)) == "x0.12346-w250"
    long_names = ["HG%05d.1" % i for i in range(14)]
    with pytest.raises(ValueError):
        R.basis_tag(leave_out=long_names)
    with pytest.raises(_lib.LocityperError) as e:
        api.basis_tag(leave_out_names=long_names)
    assert e.value.code == cdefs.ERR_RUNTIME and "too long" in str(e.value)
    ok = ["n%02d" % i for i in range(28)]                         # 10 + 3 + 28 * 3 + 27 = 124 characters... one below the limit is fine
    assert api.basis_tag(leave_out_names=ok) == R.basis_tag(leave_out=ok)


def _select(n, ints, node_limit=0):
    return api.basis_select(n, api.basis_rows_from_ints(n, ints), node_limit)


@pytest.mark.parametrize("seed", range(12))
def test_select_size_equals_brute_force_on_random_rows(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(3, 21))
    n_rows = int(rng.integers(1, 60))
    dens = rng.choice([0.1, 0.2, 0.4])
    ints = []
    for _ in range(n_rows):
        v = 0
        for i in range(n):
            if rng.random() < dens:
                v |= 1 << i
        ints.append(v or 1 << int(rng.integers(n)))
    ids, bound, optimal, nodes = _select(n, ints)
    assert optimal and bound == len(ids) == R.brute_force_min(n, set(ints))
    assert R.is_cover(ids, ints) and list(ids) == sorted(set(int(i) for i in ids))
    assert len(ids) <= len(R.greedy_cover(n, set(ints)))
    again = _select(n, ints)
    assert list(again[0]) == list(ids) and again[1:] == (bound, optimal, nodes)


def test_select_on_designed_row_sets():
    ids, bound, optimal, _ = _select(5, [1 << i for i in range(5)])              # all singletons: everything is forced
    assert list(ids) == [0, 1, 2, 3, 4] and bound == 5 and optimal
    ids, bound, optimal, _ = _select(5, [0b11111])                                # one full row: the lowest id
    assert list(ids) == [0] and bound == 1 and optimal
    # a forced chain: {0} forces 0, which hits {0,1}; {1,2} and {2,3} are left and share 2
    ids, bound, optimal, _ = _select(4, [0b0001, 0b0011, 0b0110, 0b1100])
    assert list(ids) == [0, 2] and bound == 2 and optimal
    # a triangle needs two, and the greedy tie goes to the lowest ids
    ids, bound, optimal, _ = _select(3, [0b011, 0b110, 0b101])
    assert len(ids) == 2 and bound == 2 and optimal
    ids, bound, optimal, _ = _select(70, [1 << 69 | 1 << 3, 1 << 69 | 1 << 40])   # more than two words of bits
    assert list(ids) == [69] and optimal


def test_select_node_limit_returns_a_cover_that_is_not_proved():
    rng = np.random.default_rng(7)
    n = 20
    ints = list({int(sum(1 << int(i) for i in rng.choice(n, 3, replace=False))) for _ in range(40)})
    full = _select(n, ints)
    assert full[2] and full[3] > 1                                                # the search needs more than one node here
    ids, bound, optimal, nodes = _select(n, ints, node_limit=1)
    assert not optimal and R.is_cover(ids, ints)
    assert bound <= len(full[0]) <= len(ids)


def _raises(code, fn):
    with pytest.raises(_lib.LocityperError) as e:
        fn()
    assert e.value.code == code
    assert _lib.lib().lcty_last_error() != b""


def test_error_statuses():
    L = _lib.lib()
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _select(4, [0b0011, 0]))                                   # a row nobody can hit
    n_ids = C.c_uint32()
    one = np.ones(1, dtype=np.uint32)
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_basis_select(0, 0, None, 0, one.ctypes.data, C.byref(n_ids), None, None, None)))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_basis_select(3, 1, one.ctypes.data, 0, None, C.byref(n_ids), None, None, None)))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.basis_tag(api.basis_params(window=0)))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.basis_tag(api.basis_params(divergence=1.5)))
    buf = C.create_string_buffer(4)
    p = api.basis_params()
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_basis_tag(C.byref(p), None, 0, buf, 4)))  # buffer too small
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_basis_tag(None, None, 0, buf, 4)))
    # the device entries refuse a missing context before anything else: there is no host fallback
    lens = np.array([10, 8], dtype=np.uint32)
    win_off = np.zeros(3, dtype=np.uint64)
    h, n_out = C.c_void_p(), C.c_uint64()
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_basis_windows(None, 2, lens.ctypes.data, 0, None, None, None, None, None, None, None,
                                                                             C.byref(p), win_off.ctypes.data, C.byref(h), None)))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_basis_constraints(None, 2, 1, one.ctypes.data, 0, C.byref(n_out), C.byref(h), None)))
    ids = np.zeros(2, dtype=np.uint32)
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_basis_build(None, 2, lens.ctypes.data, 0, None, None, None, None, None, None, None,
                                                                           C.byref(p), ids.ctypes.data, C.byref(n_ids), None, None, None)))


def test_basis_params_default():
    p = api.basis_params()
    assert (p.divergence, p.window, p.step, p.minimal, p.node_limit) == (0.01, 250, 0, 1, 2000000)     # augment.rs:59-61
    assert api.basis_params(step=100).step == 100
