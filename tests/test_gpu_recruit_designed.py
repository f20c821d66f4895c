"""recruit_kernel and recruit_single_kernel (lcty_recruit.hip) on the designed cases of tests/recruit_cases.py, through the C ABI,
against the oracle: every read of every case, sets of loci bit for bit. A refusal must be the stated error code and the call after
it on the same targets must still answer. The turn tests cap the workgroups of both launches with the knob "recruit_blocks", so
that one workgroup takes many chunks of pairs (many long reads) in turn and carries its LDS and scratch from one to the next.
tests/test_recruit_cases.py holds the cases to their shapes and the oracle to the restatement on the CPU."""
import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from locityper_amd.cdefs import ReadsChunk
from tests import recruit_cases as RC
from tests.test_recruit_cases import oracle_targets

pytestmark = pytest.mark.gpu

CODES = {"UNSUPPORTED": cdefs.ERR_UNSUPPORTED, "INVALID_INPUT": cdefs.ERR_INVALID_INPUT}


@pytest.fixture(scope="module")
def gpu_ctx():
    return api.Context(0)


def _device_targets(ctx, case):
    p = case.params
    gt = api.Targets(ctx, api.recruit_params(paired=case.paired, minimizer_k=p["k"], minimizer_w=p["w"], match_frac=p["match_frac"],
                                             match_length=p["match_length"], thresh_kmer_count=p["thresh_kmer_count"]))
    for alleles, counts in zip(case.loci, RC.case_counts(case)):
        seqs = np.frombuffer(b"".join(alleles), dtype=np.uint8)
        seq_off = np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64)
        cnt_off = np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64)
        gt.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, RC.BASE_K)
    gt.finalize()
    return gt


def _chunk(reads):
    return ReadsChunk.from_pairs([{"seq1": a.decode(), "seq2": None if b is None else b.decode(), "recs": []} for a, b in reads])


def _device_answers(gt, case, reads):
    cnt, out = gt.recruit(_chunk(reads), paired=case.paired, max_out=case.max_out)
    return [[int(x) for x in out[i, :cnt[i]]] for i in range(len(reads))]


def _oracle_answers(ot, reads):
    return [ot.recruit(a, b) for a, b in reads]


def _run(ctx, case):
    """-> number of reads the device answered like the oracle (all of them, or the test has failed)"""
    gt, ot = _device_targets(ctx, case), oracle_targets(case)
    try:
        reads = case.reads
        if case.error is not None:
            with pytest.raises(_lib.LocityperError) as ei:
                _device_answers(gt, case, reads)
            assert ei.value.code == CODES[case.error], (case.name, ei.value.code, str(ei.value))
            assert case.after
            reads = case.after                                                # the call after a refusal, on the same targets
        got, exp = _device_answers(gt, case, reads), _oracle_answers(ot, reads)
        for i, (g, e) in enumerate(zip(got, exp)):
            assert g == e, (case.name, i, case.tags[i] if reads is case.reads else "after", len(reads[i][0]))
        return len(reads), sum(bool(e) for e in exp)
    finally:
        gt.close()


def _run_all(ctx, cases):
    assert cases
    n = n_rec = 0
    for case in cases:
        a, b = _run(ctx, case)
        n += a; n_rec += b
    return n, n_rec


def test_every_switching_length(gpu_ctx):
    n, n_rec = _run_all(gpu_ctx, RC.length_cases())
    assert n_rec > n // 3


def test_equal_hashes_inside_a_window(gpu_ctx):
    n, n_rec = _run_all(gpu_ctx, RC.tie_cases())
    assert n_rec > n // 3


def test_other_bases_at_every_designed_place(gpu_ctx):
    n, n_rec = _run_all(gpu_ctx, RC.other_base_cases())
    assert n_rec > n // 3


def test_locus_slots_full_one_over_and_max_out(gpu_ctx):
    cases = RC.slot_cases()
    assert sum(c.error == "UNSUPPORTED" for c in cases) == 3 and sum(c.error == "INVALID_INPUT" for c in cases) == 3
    _run_all(gpu_ctx, cases)


def test_fractions_at_equality_and_just_below(gpu_ctx):
    _run_all(gpu_ctx, RC.fraction_cases())


def test_long_read_rule_at_its_boundaries(gpu_ctx):
    _run_all(gpu_ctx, RC.long_rule_cases())


@pytest.mark.parametrize("w", RC.WINDOWS)
def test_window_sizes(gpu_ctx, w):
    """w >= 52 asks for more than 64 KB of dynamic LDS in the pair kernel, w >= 33 in the single-read kernel."""
    cases = [c for c in RC.window_cases() if c.params["w"] == w]
    assert len(cases) == 2 * len(RC.KS)
    n, n_rec = _run_all(gpu_ctx, cases)
    assert n_rec > n // 5


@pytest.mark.parametrize("which", [0, 1])
def test_many_turns_of_one_workgroup(gpu_ctx, which):
    case = RC.turn_cases()[which]
    gt, ot = _device_targets(gpu_ctx, case), oracle_targets(case)
    try:
        exp = _oracle_answers(ot, case.reads)
        plain = _device_answers(gt, case, case.reads)
        assert plain == exp
        for blocks in (1, 3):
            gpu_ctx.set_knob("recruit_blocks", blocks)
            got = _device_answers(gt, case, case.reads)
            for i, (g, e) in enumerate(zip(got, exp)):
                assert g == e, (case.name, blocks, i, case.tags[i], len(case.reads[i][0]))
        assert sum(bool(e) for e in exp) > len(exp) // 3
    finally:
        gpu_ctx.set_knob("recruit_blocks", -1)
        gt.close()


def test_the_knob_is_a_cap_and_never_below_one(gpu_ctx):
    case = RC.length_cases()[0]
    gt, ot = _device_targets(gpu_ctx, case), oracle_targets(case)
    try:
        exp = _oracle_answers(ot, case.reads)
        for blocks in (0, 1, 1 << 40):
            gpu_ctx.set_knob("recruit_blocks", blocks)
            assert _device_answers(gt, case, case.reads) == exp, blocks
    finally:
        gpu_ctx.set_knob("recruit_blocks", -1)
        gt.close()
