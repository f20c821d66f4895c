"""The hand-offs between the scoring kernels of a counted batch on designed pairs (tests/score_route_cases.py; held against pyref on
the CPU by tests/test_score_route_cases.py). For every case: AllAlignments.score_routes() says that each pair went to the kernel its
group sizes and mate lengths send it to; the default flow gives the same products bit for bit as the flow with each of the knobs
"score_lean", "score_lean_two" and "score_lean_keep" at 0, and as the record batch of the same pairs, with the routes those
settings imply; and the products are the oracle's."""
import ctypes as C

import numpy as np
import pytest

from locityper_amd import api, cdefs
from tests import oracle_ffi as O
from tests import pyref
from tests import score_route_cases as SC
from tests.helpers import locus_arrays
from tests.test_gpu_counted import _same

pytestmark = pytest.mark.gpu

KNOBS = ("score_lean", "score_lean_two", "score_lean_keep")


@pytest.fixture(scope="module")
def loci(gpu_ctx):
    """The design's locus on the device, the oracle's, and pyref's for the walk: once per design, released with the module."""
    made = {}

    def get(D):
        if D.key not in made:
            p = api.resolve_params(api.default_params(), D.bg)
            seqs, seq_off, cflat, cnt_off, _ = locus_arrays(D.alleles, D.k, D.counts)
            loc = api.Locus(gpu_ctx, seqs, seq_off, cflat, cnt_off, D.k, D.bg, p)
            ol = O.OracleLocus(seqs, seq_off, cflat, cnt_off, D.k, D.bg, p)

            def edit_thr(rl):
                g, q = C.c_uint32(), C.c_uint32()
                O.lib().orc_edit_thresholds(C.byref(D.bg), rl, C.byref(g), C.byref(q))
                return g.value, q.value
            made[D.key] = (loc, ol, SC.WalkLocus(D.alleles, D.k, D.bg, p, edit_thr))
        return made[D.key]
    yield get
    for loc, _, _ in made.values():
        loc.close()


def check_routes(aa, D, facts, knobs=(), counted=True):
    want = np.array([SC.route_from_facts(f, D.n_alleles, D.k, knobs, counted) for f in facts], dtype=np.uint8)
    got = aa.score_routes()
    print(f"{D.key}: knobs off {knobs or '-'}, counted {counted}: lean {got['n_lean']}, two {got['n_two']}, general {got['n_general']} "
          f"of {got['n_pairs']}; lean form {got['lean_form']}, two-slot form ran {got['two_ran']}")
    assert got["n_pairs"] == len(facts) == got["n_lean"] + got["n_two"] + got["n_general"]
    assert np.array_equal(got["route"], want), np.nonzero(got["route"] != want)[0]
    assert [got["n_lean"], got["n_two"], got["n_general"]] == [int((want == r).sum()) for r in (SC.LEAN, SC.TWO, SC.GENERAL)]
    form = SC.lean_form(D.n_alleles, D.k, knobs, counted)
    assert got["lean_form"] == form
    assert got["two_ran"] == (form == cdefs.LEAN_FORM_KEEP and SC.two_runs(D.n_alleles, knobs))
    if form == cdefs.LEAN_FORM_NONE:
        assert got["n_general"] == got["n_pairs"]
    return got


@pytest.mark.parametrize("key,name", SC.case_ids())
def test_designed_pairs_take_their_routes(gpu_ctx, loci, key, name):
    D = SC.design(key)
    pairs = D.cases[name]
    loc, ol, wl = loci(D)
    ch = SC.chunk_of(pairs)
    facts = [SC.walk(wl, q) for q in pyref._decode_chunk(ch)]
    designed = np.array([q["route"] for q in pairs], dtype=np.uint8)
    try:
        for knob in KNOBS:
            gpu_ctx.set_knob(knob, -1)
        lean = api.AllAlignments.load(loc, ch, counted=True)
        got = check_routes(lean, D, facts)
        assert np.array_equal(got["route"], designed)                        # what the case says, pair by pair
        for knob in KNOBS:
            gpu_ctx.set_knob(knob, 0)
            other = api.AllAlignments.load(loc, ch, counted=True)
            check_routes(other, D, facts, (knob,))
            _same(lean, other)
            gpu_ctx.set_knob(knob, -1)
        # the record batch of the same pairs: the general kernel on CIGARs (and the flag of the mates' lengths picks its k-mer path)
        raw = api.AllAlignments.load(loc, ch)
        check_routes(raw, D, facts, counted=False)
        _same(lean, raw)
    finally:
        for knob in KNOBS:
            gpu_ctx.set_knob(knob, -1)
    oa = ol.load(ch)
    st, w, unm, uk = lean.status()
    assert np.array_equal(st, oa.status) and np.array_equal(uk, oa.uniq_kmers) and lean.n_good() == oa.n_good
    M, Mo = lean.best_aln_matrix(), oa.best_aln_matrix()
    assert M.shape == Mo.shape and (M.size == 0 or np.abs(M - Mo).max() < 1e-9)
    off, pa = lean.pair_alns()
    assert np.array_equal(off, oa.pa_off)
    assert np.array_equal(pa["contig"], oa.pair_alns["contig"]) and np.array_equal(pa["mid1"], oa.pair_alns["mid1"])
    # a case is about pairs that are scored: most of them are good, every kind of route among them
    good = st == cdefs.READ_GOOD
    assert good.sum() * 2 >= len(pairs)
    for r in set(designed.tolist()):
        assert (good & (designed == r)).any(), r


def test_routes_of_an_unscored_and_a_rescored_batch(gpu_ctx, loci):
    """score_routes() speaks of the last scoring launch: asked before one it fails loudly; after a second score() under another
    knob it reports that launch."""
    from locityper_amd import _lib
    D = SC.design("small")
    loc, ol, wl = loci(D)
    pairs = D.cases["group sizes"]
    ch = SC.chunk_of(pairs)
    facts = [SC.walk(wl, q) for q in pyref._decode_chunk(ch)]
    aa = api.AllAlignments(loc, ch.n_pairs, ch.n_bases, len(ch.recs), 0)
    aa.append(ch, counted=True)
    with pytest.raises(_lib.LocityperError) as e:
        aa.score_routes()
    assert e.value.code == cdefs.ERR_INVALID_INPUT
    try:
        aa.score()
        first = check_routes(aa, D, facts)
        assert first["n_two"] > 0 and first["n_general"] > 0 and first["n_lean"] > 0
        gpu_ctx.set_knob("score_lean", 0)
        aa.score()
        check_routes(aa, D, facts, ("score_lean",))
    finally:
        gpu_ctx.set_knob("score_lean", -1)
