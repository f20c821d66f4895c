"""Transitive haplotype alignments on the device (lcty_align_haplotypes_transitive) against the transliteration
tests/pyref_transitive.py on the designed families of tests/transitive_cases.py (tests/test_transitive_host.py shows that the families
cover the branches they were designed for): routes, via, CIGAR words, counts, scores and the number of rounds, pair for pair."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, io
from locityper_amd._lib import LocityperError
from tests import pyref_align as R
from tests import transitive_cases as TC

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in TC.cases()]
KEYS = ("aligned", "n_matches", "aln_len", "nerrs", "score", "best_k", "um", "md", "cigar_off", "cigar", "route", "via")


def run(ctx, c, **over):
    seqs, off = c.arrays()
    kw = dict(backbone_ks=c.ks, max_gap=c.max_gap, thresh_div=c.thresh_div)
    return api.align_haplotypes_transitive(ctx, seqs, off, [p[0] for p in c.pairs], [p[1] for p in c.pairs], api.align_params(**kw),
                                           api.align_tr_params(transitive_div=over.get("tr_div", c.tr_div), transitive_anchor=c.anchor),
                                           against=c.against)


_dev = {}


def device(ctx, name):
    if name not in _dev:
        _dev[name] = run(ctx, TC.by_name(name))
    return _dev[name]


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS if k in a and k in b)


@pytest.mark.parametrize("name", NAMES + [c.name for c in TC.level_cases()])
def test_every_pair_equals_the_transliteration(gpu_ctx, name):
    c, want = TC.by_name(name), TC.expected(name)
    res, st = device(gpu_ctx, name)
    assert res["route"].tolist() == want["route"] and res["via"].tolist() == want["via"]
    assert st["n_rounds"] == len(want["rounds"]) and st["n_accelerated"] == sum(r >= 2 for r in want["route"])
    assert st["n_dropped"] == want["events"]["dropped"]
    for x in range(len(c.pairs)):
        words = res["cigar"][int(res["cigar_off"][x]):int(res["cigar_off"][x + 1])]
        if want["route"][x] == 0:
            assert not res["aligned"][x] and len(words) == 0
            continue
        items = want["items"][x]
        nm, ne = R.counts(items)
        assert np.array_equal(words, R.words(items)), (x, c.pairs[x], want["route"][x], R.items_of(words), items)
        assert (int(res["n_matches"][x]), int(res["aln_len"][x]), int(res["nerrs"][x])) == (nm, nm + ne, ne)
        assert int(res["score"][x]) == want["score"][x] and int(res["best_k"][x]) == want["best_k"][x]
        assert (int(res["um"][x]), float(res["md"][x])) == want["div"][x]


@pytest.mark.parametrize("name", ["tree", "fifteen"])
def test_without_acceleration_it_is_the_backbone_call(gpu_ctx, name):
    """transitive_div 0, and a call of 15 pairs: lcty_align_haplotypes bit for bit"""
    c = TC.by_name(name)
    seqs, off = c.arrays()
    res, st = run(gpu_ctx, c, tr_div=0.0) if name == "tree" else device(gpu_ctx, name)
    plain, _ = api.align_haplotypes(gpu_ctx, seqs, off, [p[0] for p in c.pairs], [p[1] for p in c.pairs],
                                    api.align_params(backbone_ks=c.ks, max_gap=c.max_gap, thresh_div=c.thresh_div), against=c.against)
    assert same(res, plain)
    assert (res["route"] == 1).all() and (res["via"] == 0xFFFFFFFF).all() and st["n_rounds"] == 0 and st["n_accelerated"] == 0


@pytest.mark.parametrize("knob,value", [("align_batch_pairs", 3), ("align_match_budget", 40000)])
def test_rounds_and_backbone_batches_do_not_interact(gpu_ctx, knob, value):
    base, st0 = device(gpu_ctx, "skips")
    gpu_ctx.set_knob(knob, value)
    try:
        res, st = run(gpu_ctx, TC.by_name("skips"))
    finally:
        gpu_ctx.set_knob(knob, -1)
    assert same(res, base) and st["n_batches"] > st0["n_batches"] and st["n_rounds"] == st0["n_rounds"]


def test_lane_scratch_is_reused_across_rounds(gpu_ctx):
    """rows of 7, 6, ... pairs, then again in one context: the lanes' scratch and the store hold nothing over from a round or a call"""
    first, _ = device(gpu_ctx, "tree")
    other, _ = run(gpu_ctx, TC.by_name("hand"))                                # rounds of other widths in between
    again, st = run(gpu_ctx, TC.by_name("tree"))
    assert same(first, again) and same(other, device(gpu_ctx, "hand")[0])
    assert st["n_rounds"] == 7 and st["n_tr_stretches"] > 0 and st["store_bytes"] == 4 * len(again["cigar"])


def test_a_store_that_is_too_small_is_an_error_naming_the_knob(gpu_ctx):
    gpu_ctx.set_knob("align_cigar_store_mb", 0)
    try:
        with pytest.raises(LocityperError) as e:
            run(gpu_ctx, TC.by_name("tree"))
        assert e.value.code == cdefs.ERR_UNSUPPORTED and "align_cigar_store_mb" in str(e.value)
    finally:
        gpu_ctx.set_knob("align_cigar_store_mb", -1)
    res, _ = run(gpu_ctx, TC.by_name("tree"))                                  # the context is as good as before
    assert same(res, device(gpu_ctx, "tree")[0])


def test_accelerated_paf_feeds_hap_alns_and_basis(gpu_ctx, tmp_path):
    from locityper_amd import synth
    L = synth.SynthLocus(8, 256, base_len=3000)
    seqs, off = np.asarray(L.seqs, dtype=np.uint8), np.asarray(L.seq_off, dtype=np.uint64)
    names = [f"hap{i}" for i in range(8)]
    r, q = api.align_all_pairs(8)
    res, st = api.align_haplotypes_transitive(gpu_ctx, seqs, off, r, q, tr_params=api.align_tr_params(transitive_div=0.05, transitive_anchor=31))
    assert st["n_accelerated"] > 0
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
    ids, bound, optimal, _ = api.basis_build(gpu_ctx, lengths, ents, api.basis_params(divergence=0.02, window=250))
    assert 1 <= len(ids) <= 8 and bound <= len(ids)
