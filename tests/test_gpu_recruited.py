"""A resident set of recruited reads (lcty_recruited) on the device against tests/pyref_recruited.py, bit for bit: designed
mate lengths and N bases, every shape of answer, several adds with regrowth, adds beyond one tile of the scan and the sort, the three
sources, the names, every error status with the set unchanged behind it, and two runs giving the same bytes."""
import os
import re

import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from locityper_amd._lib import LocityperError
from tests import pyref_recruited as PR
from tests import pyref_sample_bam as PB
from tests import sample_bam_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    """the session's context: it outlives every batch and locus made on it here, whenever the collector gets to them"""
    return gpu_ctx


def make_targets(ctx, n_loci, finalize=True):
    """n_loci loci of one random allele of 200 bases: the set only needs their number"""
    rng = np.random.default_rng(n_loci)
    t = api.Targets(ctx, api.recruit_params(paired=True))
    for _ in range(n_loci):
        s = rng.choice(list(b"ACGT"), 200).astype(np.uint8)
        t.add_locus(s, np.array([0, 200], dtype=np.uint64), np.zeros(176, dtype=np.uint16), np.array([0, 176], dtype=np.uint64), 25)
    if finalize:
        t.finalize()
    return t


@pytest.fixture(scope="module")
def targets5(ctx):
    return make_targets(ctx, 5)


def chunk_of(pairs):
    mate_len, mate_off, bases2, nmask = PR.pack_reads(pairs)
    z = np.zeros(len(pairs) + 1, dtype=np.uint64)
    # as lcty_fastx_next hands a chunk out: room for one more word behind the last unit
    return cdefs.ReadsChunk(mate_len, mate_off, np.concatenate([bases2, [0, 0]]).astype(np.uint32), np.concatenate([nmask, [0]]).astype(np.uint32), z,
                            np.zeros(0, dtype=cdefs.ALN_REC_DTYPE), z, np.zeros(0, dtype=np.uint32))


def same_as(rset, E):
    """every locus of the set, bit for bit, against the restatement"""
    total = 0
    for l in range(E.n_loci):
        mate_len, mate_off, b2, nm, ordinal = E.locus(l)
        assert rset.sizes(l) == (len(ordinal), int(mate_off[-1])), l
        v, o = rset.view(l)
        assert v.n_pairs == len(ordinal)
        assert np.array_equal(v.mate_len, mate_len) and np.array_equal(v.mate_off, mate_off), l
        assert np.array_equal(v.bases2, b2) and np.array_equal(v.nmask, nm), l
        assert np.array_equal(o, ordinal), l
        total += len(ordinal)
    return total


def seq(rng, n, n_at=()):
    s = rng.choice(list(b"ACGT"), n).astype(np.uint8)
    for p in n_at:
        s[p] = ord("N")
    return bytes(s)


def designed_pairs(rng):
    pairs = [(seq(rng, n), seq(rng, n)) for n in (1, 31, 32, 33, 64, 150, 255, 256)]
    pairs += [(seq(rng, a), seq(rng, b)) for a, b in ((1, 256), (33, 31), (150, 1), (32, 64))]
    pairs += [(seq(rng, n), None) for n in (1, 32, 33, 150, 256, 257, 500, 5000)]                      # single-end: every odd mate absent
    # N at the first base, at the last base, across a unit boundary
    pairs += [(seq(rng, 150, (0,)), seq(rng, 150, (149,))), (seq(rng, 64, (31, 32)), seq(rng, 33, (31, 32))), (seq(rng, 32, (0, 31)), seq(rng, 1, (0,))),
              (seq(rng, 500, (0, 255, 256, 499)), None)]
    return pairs


def designed_answers(n, max_out=3):
    """pairs with 0, 1, 2 and max_out loci among loci 0..3, increasing as recruitment leaves them; locus 4 gets none"""
    cnt = np.array([(0, 1, 2, max_out)[i % 4] for i in range(n)], dtype=np.uint32)
    loci = np.full((n, max_out), 0xFFFFFFFF, dtype=np.uint32)                # beyond cnt: never read
    for i in range(n):
        a = (i // 4) % 4
        if cnt[i] == 1:
            loci[i, 0] = a
        elif cnt[i] == 2:
            loci[i, :2] = sorted((a, (a + 1 + (i // 16) % 3) % 4))
        elif cnt[i] == max_out:
            loci[i, :max_out] = [x for x in range(4) if x != a][:max_out]
    return cnt, loci


def test_designed_lengths_n_bases_and_answer_shapes(ctx, targets5):
    rng = np.random.default_rng(1)
    pairs = designed_pairs(rng)
    chunk = chunk_of(pairs)
    cnt, loci = designed_answers(len(pairs))
    assert set(cnt.tolist()) == {0, 1, 2, 3} and 4 not in loci[loci != 0xFFFFFFFF]
    rset, E = api.Recruited(targets5), PR.Expected(5)
    rset.add(chunk, cnt, loci)
    E.add(chunk, cnt, loci)
    assert same_as(rset, E) == int(cnt.sum())
    assert rset.sizes(4) == (0, 0) and rset.view(4)[0].n_pairs == 0           # a locus without reads
    # a second add: every read to locus 0, some to others as well; the reads of the first add stay where they were
    cnt2 = np.array([1 + (i % 3) for i in range(len(pairs))], dtype=np.uint32)
    loci2 = np.tile(np.array([0, 1, 4], dtype=np.uint32), (len(pairs), 1))
    rset.add(chunk, cnt2, loci2)
    E.add(chunk, cnt2, loci2)
    same_as(rset, E)
    assert rset.sizes(0)[0] == len(pairs) + sum(0 in loci[i, :cnt[i]] for i in range(len(pairs)))
    rset.close()


def test_three_adds_with_regrowth_and_running_ordinals(ctx, targets5):
    rng = np.random.default_rng(2)
    ctx.set_knob("recruited_init_units", 1)
    try:
        rset, E = api.Recruited(targets5), PR.Expected(5)
        for k, n in enumerate((40, 25, 90)):
            pairs = [(seq(rng, int(rng.integers(1, 257))), seq(rng, int(rng.integers(1, 257))) if i % 5 else None) for i in range(n)]
            chunk = chunk_of(pairs)
            cnt, loci = designed_answers(n)
            if k == 1:
                cnt[:] = 0                                                   # the middle add recruits nothing
            rset.add(chunk, cnt, loci)
            E.add(chunk, cnt, loci)
            same_as(rset, E)
        # from one unit every locus with reads has doubled several times; the ordinals of the third add start behind both earlier ones
        assert all(rset.sizes(l)[1] // 32 >= 16 for l in range(4))
        assert int(rset.view(0)[1].max()) >= 65 and E.n_seen == 155
        rset.close()
    finally:
        ctx.set_knob("recruited_init_units", -1)


def test_more_entries_than_one_tile_of_the_scan_and_the_sort(ctx):
    src = open(os.path.join(ROOT, "locityper_amd", "csrc", "lcty_sort.hip")).read()
    scan_chunk = int(re.search(r"constexpr uint32_t SCAN_CHUNK = (\d+);", src).group(1))
    sort_tile = int(re.search(r"constexpr uint32_t SORT_TILE = (\d+);", src).group(1))
    n_loci = 300                                                             # two bytes of locus index: two passes of the sort
    targets = make_targets(ctx, n_loci)
    rng = np.random.default_rng(3)
    n = 3000
    pairs = [(seq(rng, int(rng.integers(1, 152))), seq(rng, int(rng.integers(0, 152))) or None) for _ in range(n)]
    chunk = chunk_of(pairs)
    cnt = rng.integers(0, 4, n).astype(np.uint32)
    cnt[:max(scan_chunk, sort_tile) // 3 + 1] = 3                           # one past a tile whatever the draw
    loci = np.full((n, 3), 0xFFFFFFFF, dtype=np.uint32)
    for i in range(n):
        loci[i, :cnt[i]] = np.sort(rng.choice(n_loci, int(cnt[i]), replace=False))
    assert int(cnt.sum()) > max(scan_chunk, sort_tile) and n > 0 and int(loci[loci != 0xFFFFFFFF].max()) >= 256
    sets = []
    for _ in range(2):
        rset, E = api.Recruited(targets), PR.Expected(n_loci)
        rset.add(chunk, cnt, loci)
        rset.add(chunk, cnt[::-1].copy(), loci[::-1].copy())                 # and once more onto loci that hold reads
        E.add(chunk, cnt, loci)
        E.add(chunk, cnt[::-1], loci[::-1])
        assert same_as(rset, E) == 2 * int(cnt.sum())
        sets.append(rset)
    # two runs: the same bytes
    for l in (0, 17, 255, 256, 299):
        (a, oa), (b, ob) = sets[0].view(l), sets[1].view(l)
        assert a.bases2.tobytes() == b.bases2.tobytes() and a.nmask.tobytes() == b.nmask.tobytes() and a.mate_off.tobytes() == b.mate_off.tobytes()
        assert oa.tobytes() == ob.tobytes()
    for s in sets:
        s.close()
    targets.close()


# ---------------------------------------------------------------- the three sources, and the names
def _write_sources(tmp, pairs, names):
    r1, r2, bam = str(tmp / "r1.fq"), str(tmp / "r2.fq"), str(tmp / "reads.bam")
    with open(r1, "w") as a, open(r2, "w") as b:
        for (s1, s2), nm in zip(pairs, names):
            a.write(f"@{nm}/1 first mate\n{s1.decode()}\n+\n{'I' * len(s1)}\n")
            b.write(f"@{nm}/2\n{s2.decode()}\n+\n{'5' * len(s2)}\n")
    recs = []
    for k, ((s1, s2), nm) in enumerate(zip(pairs, names)):
        recs.append(PB.rec(0, 100 + k, nm, 0x41, [("M", len(s1))], s1.decode(), bytes([40]) * len(s1), 0, 5000 + k))
    for k, ((s1, s2), nm) in enumerate(zip(pairs, names)):
        recs.append(PB.rec(0, 5000 + k, nm, 0x81, [("M", len(s2))], s2.decode(), bytes([20]) * len(s2), 0, 100 + k))
    PB.write_bam(bam, SC.HAND_REFS, recs, block_size=2000)
    return r1, r2, bam


def _names_in(path):
    """the name of every pair of a reads.fq of paired FASTQ records: the header of every other record"""
    lines = open(path).read().splitlines()
    assert len(lines) % 8 == 0
    return [ln[1:] for ln in lines[0::8]]


def test_the_three_sources_give_the_same_set_and_the_writers_names(ctx, targets5, tmp_path):
    rng = np.random.default_rng(4)
    n = 60
    pairs = [(seq(rng, int(rng.integers(20, 152)), (0,) if i % 7 == 0 else ()), seq(rng, int(rng.integers(20, 152)), (3,) if i % 11 == 0 else ())) for i in range(n)]
    names = [f"pair{i}" for i in range(n)]
    r1, r2, bam = _write_sources(tmp_path, pairs, names)
    cnt, loci = designed_answers(n)
    E = PR.Expected(5)
    host_chunk = chunk_of(pairs)
    # host chunks, in two adds
    from_host = api.Recruited(targets5, keep_names=True)
    for lo, hi in ((0, 25), (25, n)):
        part = host_chunk.slice(lo, hi)
        from_host.add(part, cnt[lo:hi], loci[lo:hi])
        E.add(part, cnt[lo:hi], loci[lo:hi])
    # the FASTQ files on the device, in chunks of 25 records
    from_fastx = api.Recruited(targets5, keep_names=True)
    dev = lio.FastxDevice(ctx, r1, r2)
    paths_fx = [str(tmp_path / f"fx{l}.fq") for l in range(5)]
    w = lio.FastxWriters(paths_fx)
    at = 0
    while dev.next(25):
        k = dev.n
        v = dev.view()
        assert np.array_equal(v.mate_len, host_chunk.mate_len[2 * at:2 * (at + k)])
        dev.add_recruited(from_fastx, cnt[at:at + k], loci[at:at + k])
        dev.write_recruited(w, cnt[at:at + k], loci[at:at + k])
        at += k
    w.close(); dev.close()
    assert at == n
    # the BAM of the same reads
    from_bam = api.Recruited(targets5, keep_names=True)
    reads = lio.SampleBam(bam).fetch(ctx, [(0, 0, 10_000)], paired=True)
    v = reads.view()[0]
    assert v.n_pairs == n and np.array_equal(v.mate_len, host_chunk.mate_len)
    paths_bam = [str(tmp_path / f"bam{l}.fq") for l in range(5)]
    w = lio.FastxWriters(paths_bam)
    reads.add_recruited(from_bam, cnt, loci)
    reads.write_recruited(w, cnt, loci)
    w.close()
    for rset in (from_host, from_fastx, from_bam):
        assert same_as(rset, E) == int(cnt.sum())
    # names: what the writers wrote for the same calls
    for l in range(5):
        want = [names[i] for i in range(n) if l in loci[i, :cnt[i]]]
        assert from_fastx.names(l) == _names_in(paths_fx[l]) == [w + "/1" for w in want]
        assert from_bam.names(l) == _names_in(paths_bam[l]) == want
        off, blob = from_bam.names_raw(l)
        assert len(off) == len(want) + 1 and blob == b"".join(w.encode() for w in want)
    with pytest.raises(LocityperError) as e:                                 # lcty_recruited_add has no names
        from_host.names(0)
    assert e.value.code == cdefs.ERR_INVALID_INPUT
    for rset in (from_host, from_fastx, from_bam):
        rset.close()
    reads.close()


# ---------------------------------------------------------------- errors: the status, and the set as it was
def test_every_error_leaves_the_set_as_it_was(ctx, targets5, tmp_path):
    rng = np.random.default_rng(5)
    pairs = [(seq(rng, 100), seq(rng, 77)) for _ in range(20)]
    chunk = chunk_of(pairs)
    cnt, loci = designed_answers(20)
    rset, E = api.Recruited(targets5), PR.Expected(5)
    rset.add(chunk, cnt, loci)
    E.add(chunk, cnt, loci)
    same_as(rset, E)

    def refused(code, call, *words):
        with pytest.raises(LocityperError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value)
        same_as(rset, E)

    # out_cnt[i] > max_out; a locus beyond the targets'
    over = cnt.copy(); over[7] = 4
    refused(cdefs.ERR_INVALID_INPUT, lambda: rset.add(chunk, over, loci))
    far = loci.copy(); far[1, 0] = 5
    assert cnt[1] >= 1
    refused(cdefs.ERR_INVALID_INPUT, lambda: rset.add(chunk, cnt, far))
    # 2^32 entries in one add: decided from the counts, before a locus is read
    two = chunk_of([(None, None), (None, None)])                             # no bases: the entries alone are too many
    hs = two.host_struct()
    big_cnt = np.array([1 << 31, 1 << 31], dtype=np.uint32)
    few = np.zeros(8, dtype=np.uint32)
    from locityper_amd._lib import lib, check
    import ctypes as C
    refused(cdefs.ERR_UNSUPPORTED, lambda: check(lib().lcty_recruited_add(rset._h, C.byref(hs), 1, 1 << 31, big_cnt.ctypes.data, few.ctypes.data)), "2^32")
    # locus_ix beyond the targets' loci
    for call in (lambda: rset.sizes(5), lambda: rset.view(5), lambda: rset.names(5)):
        refused(cdefs.ERR_INVALID_INPUT, call)
    refused(cdefs.ERR_INVALID_INPUT, lambda: rset.names(0))                  # created without keep_names
    # the byte cap: one byte under the need is refused naming the knob, before anything is copied; the need itself fits
    need = PR.Expected(5)
    need.add(chunk, cnt, loci); need.add(chunk, cnt, loci)
    ctx.set_knob("recruited_max_bytes", need.bytes() - 1)
    try:
        refused(cdefs.ERR_UNSUPPORTED, lambda: rset.add(chunk, cnt, loci), "recruited_max_bytes")
        ctx.set_knob("recruited_max_bytes", need.bytes())
        rset.add(chunk, cnt, loci)
        E.add(chunk, cnt, loci)
        same_as(rset, E)
    finally:
        ctx.set_knob("recruited_max_bytes", -1)
    # another context: the source handle's, and targets that are not finalized
    other = api.Context(0)
    fq = str(tmp_path / "one.fq")
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    dev = lio.FastxDevice(other, fq)
    assert dev.next() == 1
    one = (np.ones(1, dtype=np.uint32), np.zeros((1, 1), dtype=np.uint32))
    refused(cdefs.ERR_INVALID_INPUT, lambda: dev.add_recruited(rset, *one), "context")
    dev.close()
    other.close()                                                            # behind what was made on it, not left to the collector
    open_targets = make_targets(ctx, 2, finalize=False)
    refused(cdefs.ERR_INVALID_INPUT, lambda: api.Recruited(open_targets))
    open_targets.close()
    rset.close()
