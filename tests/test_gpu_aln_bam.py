"""lcty_bam_read_device + lcty_reads_append_bam: a locus's aln.bam read on the device must be the host reader's table,
word for word and error for error, on every design of tests/aln_bam_cases.py under both inflate routes; appended to a batch from the
device it must leave the batch as lcty_reads_append of the host view leaves it."""
import ctypes as C

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io as lio, synth
from tests import aln_bam_cases as AC
from tests import pyref_sample_bam as SB

pytestmark = pytest.mark.gpu

DESIGNS = AC.all_designs()


def _read(p, alleles, paired, **kw):
    try:
        return lio.BamTable(p, alleles, paired=bool(paired), **kw), None
    except _lib.LocityperError as e:
        return None, (e.code, str(e))


@pytest.mark.parametrize("inflate", [0, 1])
def test_device_table_is_the_host_readers_on_every_design(gpu_ctx, tmp_path, inflate):
    p = str(tmp_path / "aln.bam")
    gpu_ctx.set_knob("sample_bam_inflate", inflate)
    try:
        n_err = n_tab = 0
        for d in DESIGNS:
            AC.write(d, p)
            for paired in (0, 1):
                what = f"{d['name']} paired={paired} inflate={inflate}"
                H, eh = _read(p, d["alleles"], paired)
                D, ed = _read(p, d["alleles"], paired, ctx=gpu_ctx)
                assert eh == ed, what                                   # status and text
                if eh is not None:
                    n_err += 1
                    continue
                n_tab += 1
                AC.assert_same_table(AC.table_of(D), AC.table_of(H), what)
                assert D.sizes() == H.sizes() and D.stats["records"] == H.sizes()[2] and D.stats["pairs"] == H.n_pairs, what
                # without host_copy: the per-pair arrays and the names only; the view is refused
                N = lio.BamTable(p, d["alleles"], paired=bool(paired), ctx=gpu_ctx, host_copy=False)
                assert N.sizes() == H.sizes() and N.chunk is None, what
                view = cdefs.ReadsHost()
                rc = _lib.lib().lcty_bam_table_view(N._h, C.byref(view), None, None, None)
                assert rc == cdefs.ERR_INVALID_INPUT and b"host_copy" in _lib.lib().lcty_last_error(), what
                with pytest.raises(_lib.LocityperError) as e:
                    N.quals()
                assert e.value.code == cdefs.ERR_INVALID_INPUT, what
                for T in (H, D, N):
                    T.close()
        assert n_err > 120 and n_tab >= 20
    finally:
        gpu_ctx.set_knob("sample_bam_inflate", -1)


# ---- a synthetic locus as the mapper would have written it ------------------------------------------------------------------------------

N_ALLELES, N_PAIRS = 6, 300


def _unpack(chunk, mate):
    off, ln = int(chunk.mate_off[mate]), int(chunk.mate_len[mate])
    idx = off + np.arange(ln)
    codes = (chunk.bases2[idx >> 4] >> (2 * (idx & 15))) & 3
    isn = (chunk.nmask[idx >> 5] >> (idx & 31)) & 1
    return "".join("N" if n else "ACGT"[c] for c, n in zip(codes, isn))


@pytest.fixture(scope="module")
def locus_bam(gpu_ctx, tmp_path_factory):
    L = synth.SynthLocus(N_ALLELES, N_PAIRS, base_len=8000)
    ch = L.reads(0, N_PAIRS)
    names = [f"a{a}" for a in range(N_ALLELES)]
    lens = [int(L.seq_off[a + 1] - L.seq_off[a]) for a in range(N_ALLELES)]
    recs = []
    for r in range(ch.n_pairs):
        lo, hi = int(ch.aln_off[r]), int(ch.aln_off[r + 1])
        cbase, end = int(ch.cigar_off[r]), 0
        for t in range(lo, hi):
            rec = ch.recs[t]
            primary = (int(rec["flags"]) & (cdefs.FLAG_SECONDARY | cdefs.FLAG_SUPPL)) == 0
            if primary and t > lo:
                end = 1
            words = ch.cigar[cbase + int(rec["cigar_rel"]): cbase + int(rec["cigar_rel"]) + int(rec["n_cigar"])].tolist()
            recs.append(SB.rec(int(rec["contig"]), int(rec["pos"]), f"read{r}", int(rec["flags"]), [(SB.OPS[w & 15], w >> 4) for w in words],
                               _unpack(ch, 2 * r + end) if primary else ""))
    p = str(tmp_path_factory.mktemp("aln") / "aln.bam")
    SB.write_bam(p, list(zip(names, lens)), recs, block_size=0xff00, index=False)
    prm = api.resolve_params(api.default_params(), L.bg)
    loc = api.Locus(gpu_ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, prm)
    H = lio.BamTable(p, names, paired=True)
    D = lio.BamTable(p, names, paired=True, ctx=gpu_ctx, host_copy=False)
    assert H.n_pairs == N_PAIRS == D.n_pairs
    return L, loc, p, names, H, D


def _products(aa):
    aln_off, recs, cig_off, cigar = aa.records()
    status, weight, unm, uniq = aa.status()
    off, pa = aa.pair_alns()
    return [aln_off, recs.tobytes(), cig_off, cigar, status, weight, unm, uniq, aa.best_aln_matrix(), off, pa.tobytes()]


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x == y) if isinstance(x, bytes) else (np.array_equal(x, y) and x.tobytes() == y.tobytes()), f"{what}: product {i}"


@pytest.mark.parametrize("cuts", [(0, N_PAIRS), (0, 100, 101, N_PAIRS), (0, 1, N_PAIRS), (0, 299, N_PAIRS)])
def test_append_bam_leaves_the_batch_as_append_of_the_host_chunk(locus_bam, cuts):
    L, loc, p, names, H, D = locus_bam
    n, nb, nr, nc, _ = D.sizes()
    want = api.AllAlignments(loc, n, nb, nr, nc)
    got = api.AllAlignments(loc, n, nb, nr, nc)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        want.append(H.chunk.slice(lo, hi))
        got.append_bam(D, lo, hi - lo)
    got_recs, want_recs = got.records(), want.records()
    for x, y in zip(got_recs, want_recs):
        assert x.tobytes() == y.tobytes(), f"records before scoring, cuts {cuts}"
    want.score(); got.score()
    _same(_products(got), _products(want), f"cuts {cuts}")


def test_append_bam_into_a_streaming_batch(locus_bam):
    L, loc, p, names, H, D = locus_bam
    cuts = (0, 120, 121, N_PAIRS)
    chunks = [H.chunk.slice(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    want = api.AllAlignments.load_streaming(loc, chunks)
    got = api.AllAlignments(loc, N_PAIRS, (max(c.n_bases for c in chunks) + 31) // 32 * 32, max(len(c.recs) for c in chunks),
                            max(len(c.cigar) for c in chunks), streaming_chunk_pairs=max(c.n_pairs for c in chunks))
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got.append_bam(D, lo, hi - lo)
        got.score()
    for f in ("status", "best_aln_matrix", "pair_alns"):
        a, b = getattr(got, f)(), getattr(want, f)()
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), f


def test_append_bam_refuses_what_it_cannot_take(gpu_ctx, locus_bam):
    L, loc, p, names, H, D = locus_bam
    n, nb, nr, nc, _ = D.sizes()
    aa = api.AllAlignments(loc, n, nb, nr, nc)
    for T, first, cnt, word in ((H, 0, 1, "lcty_bam_read"), (D, n, 1, "outside"), (D, 0, n + 1, "outside"), (D, 2 ** 63, 2 ** 63, "outside")):
        with pytest.raises(_lib.LocityperError) as e:
            aa.append_bam(T, first, cnt)
        assert e.value.code == cdefs.ERR_INVALID_INPUT and word in str(e.value)
    # a handle used on another context. The three objects are destroyed here, batch first and context last: the caught exception
    # keeps them in a reference cycle, and the collector would take them later in any order — a batch after its context
    other = api.Context(0)
    loc2 = bb = None
    try:
        loc2 = api.Locus(other, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, api.resolve_params(api.default_params(), L.bg))
        bb = api.AllAlignments(loc2, n, nb, nr, nc)
        with pytest.raises(_lib.LocityperError) as e:
            bb.append_bam(D)
        assert e.value.code == cdefs.ERR_INVALID_INPUT and "context" in str(e.value)
    finally:
        for obj in (bb, loc2, other):
            if obj is not None:
                obj.close()
    aa.append_bam(D, n, 0)                                          # an empty range at the end is nothing
    assert aa.n_pairs == 0


def test_slice_knob_refuses_by_name(gpu_ctx, locus_bam):
    L, loc, p, names, H, D = locus_bam
    gpu_ctx.set_knob("aln_bam_max_slice_bytes", 4096)
    try:
        with pytest.raises(_lib.LocityperError) as e:
            lio.BamTable(p, names, paired=True, ctx=gpu_ctx)
        assert e.value.code == cdefs.ERR_UNSUPPORTED and "aln_bam_max_slice_bytes" in str(e.value)
    finally:
        gpu_ctx.set_knob("aln_bam_max_slice_bytes", -1)
    assert lio.BamTable(p, names, paired=True, ctx=gpu_ctx).n_pairs == N_PAIRS
