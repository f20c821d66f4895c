"""The chunk of reads resident on the device (ReadChunk) behind every source of a sample's reads: the same designed reads
as a host chunk, as FASTQ parsed on the device, as an indexed BAM and as a streamed BAM give the same arrays word for word, the same
answers of recruitment and the same recruited sets; a handle that is used again gives a smaller chunk with exactly its own sizes; single
reads of every route of the recruitment kernels; the empty chunk of every source."""
import ctypes as C

import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from locityper_amd._lib import check, lib
from tests import pyref_sample_bam as SB
from tests.test_gpu_bam_stream import knobs
from tests.test_gpu_recruited import chunk_of, seq

pytestmark = pytest.mark.gpu

REFS = [("chrA", 100_000)]
LENS = (1, 31, 32, 33, 63, 64, 65, 151, 256)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    return gpu_ctx


def make_targets(ctx, loci, paired, base_k=25):
    t = api.Targets(ctx, api.recruit_params(paired=paired))
    for a in loci:
        t.add_locus(np.frombuffer(a, dtype=np.uint8), np.array([0, len(a)], dtype=np.uint64), np.zeros(len(a) - base_k + 1, dtype=np.uint16),
                    np.array([0, len(a) - base_k + 1], dtype=np.uint64), base_k)
    t.finalize()
    return t


def same_words(v, h, lo=0, hi=None):
    """the view v of a device chunk against pairs lo .. hi of the host chunk h, word for word (h lays its mates out on consecutive units)"""
    hi = h.n_pairs if hi is None else hi
    assert v.n_pairs == hi - lo
    base = int(h.mate_off[2 * lo])
    nb = int(h.mate_off[2 * hi]) - base
    assert np.array_equal(v.mate_len, h.mate_len[2 * lo:2 * hi])
    assert np.array_equal(v.mate_off, h.mate_off[2 * lo:2 * hi + 1] - np.uint64(base))
    assert np.array_equal(v.bases2[:nb // 16], h.bases2[base // 16:(base + nb) // 16])
    assert np.array_equal(v.nmask[:nb // 32], h.nmask[base // 32:(base + nb) // 32])


def same_answers(a, b):
    (cnt, loci), (cnt2, loci2) = a, b
    answered = np.arange(loci.shape[1])[None, :] < cnt[:, None]
    assert np.array_equal(cnt, cnt2) and np.array_equal(loci[answered], loci2[answered])


def same_sets(sets, n_loci):
    first = sets[0]
    for s in sets[1:]:
        for l in range(n_loci):
            assert s.sizes(l) == first.sizes(l)
            (a, oa), (b, ob) = first.view(l), s.view(l)
            for x, y in ((a.mate_len, b.mate_len), (a.mate_off, b.mate_off), (a.bases2, b.bases2), (a.nmask, b.nmask), (oa, ob)):
                assert x.tobytes() == y.tobytes(), l


def write_fastq(path, reads, names):
    with open(path, "w") as f:
        for s, nm in zip(reads, names):
            f.write(f"@{nm}\n{s.decode()}\n+\n{'I' * len(s)}\n")


def write_paired(tmp, pairs, tag):
    """the pairs as two FASTQ files, as a coordinate-sorted indexed BAM and as a name-grouped BAM without an index"""
    names = [f"{tag}{i}" for i in range(len(pairs))]
    r1, r2, bam, grouped = (str(tmp / f"{tag}.{x}") for x in ("r1.fq", "r2.fq", "sorted.bam", "grouped.bam"))
    write_fastq(r1, [p[0] for p in pairs], names)
    write_fastq(r2, [p[1] for p in pairs], names)
    first = [SB.rec(0, 100 + k, nm, 0x41, [("M", len(p[0]))], p[0].decode(), bytes([40]) * len(p[0]), 0, 5000 + k) for k, (p, nm) in enumerate(zip(pairs, names))]
    second = [SB.rec(0, 5000 + k, nm, 0x81, [("M", len(p[1]))], p[1].decode(), bytes([20]) * len(p[1]), 0, 100 + k) for k, (p, nm) in enumerate(zip(pairs, names))]
    SB.write_bam(bam, REFS, first + second, block_size=2000)
    SB.write_bam(grouped, REFS, [r for ab in zip(first, second) for r in ab], block_size=700, index=False)
    return r1, r2, bam, grouped


def stream_chunks(ctx, path, interleaved, window, on_chunk):
    """on_chunk(reads, first pair of the chunk) for every chunk of the stream -> the number of chunks"""
    chunks = at = 0
    with knobs(ctx, bam_stream_window_bytes=window):
        st = lio.BamStream(ctx, path, interleaved)
        while True:
            reads, _ = st.next()
            n = reads.stats["n_pairs"]
            if n == 0:
                break
            on_chunk(reads, at)
            at += n
            chunks += 1
        st.close()
    return chunks


# ---------------------------------------------------------------- 1: four sources, one chunk
@pytest.fixture(scope="module")
def designed(tmp_path_factory):
    """45 pairs: every length of LENS as mate 1 and as mate 2, two pairs in three cut from a locus (mate 2 from the other strand), an N at
    the first and at the last base of mates of every length"""
    rng = np.random.default_rng(31)
    loci = [seq(rng, 3000) for _ in range(3)]
    pairs = []
    for i in range(45):
        l1, l2 = LENS[i % 9], LENS[(i + i // 9) % 9]
        if i % 3:
            a, p = loci[i % 2], int(rng.integers(0, 2000))
            s1, s2 = a[p:p + l1], a[p + 400:p + 400 + l2].translate(COMP)[::-1]
        else:
            s1, s2 = seq(rng, l1), seq(rng, l2)
        if i % 5 == 0:
            s1 = b"N" + s1[1:]
        if i % 5 == 1:
            s2 = s2[:-1] + b"N"
        pairs.append((s1, s2))
    assert {len(a) for a, b in pairs} == {len(b) for a, b in pairs} == set(LENS)
    assert any(a[0:1] == b"N" and len(a) == n for a, b in pairs for n in (1, 32, 256)) and any(b[-1:] == b"N" and len(b) > 32 for a, b in pairs)
    d = tmp_path_factory.mktemp("read_chunk")
    return dict(dir=d, loci=loci, pairs=pairs, host=chunk_of(pairs), files=write_paired(d, pairs, "d"))


def test_the_host_chunk_lays_mates_out_on_consecutive_units(designed):
    """no device: what same_words relies on"""
    h = designed["host"]
    units = (h.mate_len.astype(np.uint64) + np.uint64(31)) // np.uint64(32)
    assert np.array_equal(h.mate_off, np.concatenate([[0], np.cumsum(units) * np.uint64(32)]).astype(np.uint64))


def test_four_sources_one_chunk(ctx, designed):
    pairs, host, n = designed["pairs"], designed["host"], len(designed["pairs"])
    r1, r2, bam, grouped = designed["files"]
    gt = make_targets(ctx, designed["loci"], paired=True)
    want = gt.recruit(host, paired=True, max_out=3)
    # the 15 pairs of no locus recruit nothing; of the 30 cut from loci 0 and 1, those with two mates of 63 bases or more do
    assert (want[0] > 0).sum() >= 5 and (want[0] == 0).sum() >= 15 and set(want[1][want[0] > 0, 0].tolist()) == {0, 1}
    sets = [api.Recruited(gt)]
    sets[0].add(host, *want)

    def whole(recruit, add):
        got = recruit()
        same_answers(got, want)
        sets.append(api.Recruited(gt))
        add(sets[-1], *got)

    def in_chunks(add_all):
        sets.append(api.Recruited(gt))
        cnts, locis = add_all(sets[-1])
        same_answers((np.concatenate(cnts), np.concatenate(locis)), want)

    for step in (1, 25):
        def fastx(rset):
            dev, at, out = lio.FastxDevice(ctx, r1, r2), 0, ([], [])
            while dev.next(step):
                same_words(dev.view(), host, at, at + dev.n)
                cnt, lc = dev.recruit(gt, max_out=3)
                dev.add_recruited(rset, cnt, lc)
                out[0].append(cnt.copy()); out[1].append(lc.copy())
                at += dev.n
            dev.close()
            assert at == n
            return out
        in_chunks(fastx)

    reads = lio.SampleBam(bam).fetch(ctx, [(0, 0, 10_000)], paired=True)
    same_words(reads.view()[0], host)
    whole(lambda: reads.recruit(gt, max_out=3), reads.add_recruited)
    reads.close()

    def streamed(rset):
        out = ([], [])
        def on_chunk(reads, at):
            same_words(reads.view()[0], host, at, at + reads.stats["n_pairs"])
            cnt, lc = reads.recruit(gt, max_out=3)
            reads.add_recruited(rset, cnt, lc)
            out[0].append(cnt.copy()); out[1].append(lc.copy())
        assert stream_chunks(ctx, grouped, True, 1500, on_chunk) >= 3
        return out
    in_chunks(streamed)

    assert len(sets) == 5
    same_sets(sets, 3)
    for s in sets:
        s.close()
    gt.close()


# ---------------------------------------------------------------- 2: a handle used again, large then small
def test_a_smaller_chunk_behind_a_larger_one(ctx, designed, tmp_path):
    pairs, host = designed["pairs"], designed["host"]
    gt = make_targets(ctx, designed["loci"], paired=True)
    # pairs 0 .. 24 and 25 .. 27 to one handle; the last three alone to a fresh one. The three have fewer units than any 25
    big = write_paired(tmp_path, pairs[:28], "b")
    small = write_paired(tmp_path, pairs[25:28], "s")
    tail = chunk_of(pairs[25:28])
    want = gt.recruit(tail, paired=True, max_out=3)

    def fastx(paths, steps):
        dev = lio.FastxDevice(ctx, paths[0], paths[1])
        for k in steps:
            assert dev.next(k) == k
        v, got = dev.view(), dev.recruit(gt, max_out=3)
        assert dev.next(25) == 0
        dev.close()
        return v, got

    def streamed(path, sizes):
        seen = []
        def on_chunk(reads, at):
            seen.append((reads.stats["n_pairs"], reads.view()[0], reads.recruit(gt, max_out=3)))
        stream_chunks(ctx, path, True, None, on_chunk)
        assert [s[0] for s in seen] == sizes
        return seen[-1][1], (seen[-1][2][0].copy(), seen[-1][2][1].copy())

    for v, got in (fastx(big, (25, 3)), fastx(small, (3,))):
        same_words(v, tail)                                                      # its own sizes and words, nothing of the chunk before
        same_answers(got, want)
    # the stream: 25 pairs in one file and 3 in the next one, which a window does not cross
    names = [f"g{i}" for i in range(28)]
    recs = [[SB.rec(-1, -1, nm, (0x4D, 0x8D)[e], [], p[e].decode(), bytes([30]) * len(p[e])) for p, nm in zip(pairs[lo:hi], names[lo:hi]) for e in (0, 1)]
            for lo, hi in ((0, 25), (25, 28))]
    paths = []
    for k, r in enumerate(recs):
        paths.append(str(tmp_path / f"two.{k}.bam"))
        SB.write_bam(paths[-1], REFS, r, index=False)
    for v, got in (streamed(paths, [25, 3]), streamed(paths[1:], [3])):
        same_words(v, tail)
        same_answers(got, want)
    gt.close()


# ---------------------------------------------------------------- 3: single reads and the long route
def test_single_reads_of_every_route(ctx, tmp_path):
    rng = np.random.default_rng(33)
    loci = [seq(rng, 8000) for _ in range(2)]
    lens = (200, 256, 257, 600, 5000)
    reads = []
    for i, n in enumerate(lens * 2):
        a, p = loci[i % 2], int(rng.integers(0, 8000 - n))
        reads.append(a[p:p + n] if i < len(lens) else a[p:p + n].translate(COMP)[::-1])
    reads += [seq(rng, n) for n in lens]                                        # and reads of no locus
    names = [f"s{i}" for i in range(len(reads))]
    host = chunk_of([(s, None) for s in reads])
    gt = make_targets(ctx, loci, paired=False)
    want = gt.recruit(host, paired=False, max_out=2)
    assert want[0][:10].tolist() == [1] * 10 and want[0][10:].tolist() == [0] * 5
    fq, bam = str(tmp_path / "single.fq"), str(tmp_path / "single.bam")
    write_fastq(fq, reads, names)
    SB.write_bam(bam, REFS, [SB.rec(0, 100 + 10 * k, nm, 0, [("M", len(s))], s.decode(), bytes([30]) * len(s)) for k, (s, nm) in enumerate(zip(reads, names))],
                 block_size=3000)

    def checked(v, got):
        assert v.mate_len[1::2].tolist() == [0] * len(reads)                    # mate 2: no base ...
        assert np.array_equal(v.mate_off[1::2], v.mate_off[2::2])               # ... and no unit
        same_words(v, host)
        same_answers(got, want)

    dev = lio.FastxDevice(ctx, fq)
    assert not dev.paired and dev.next() == len(reads)
    checked(dev.view(), dev.recruit(gt, max_out=2))
    dev.close()
    fetched = lio.SampleBam(bam).fetch(ctx, whole_file=True, paired=False)
    chunk, _, paired = fetched.view()
    assert not paired
    checked(chunk, fetched.recruit(gt, max_out=2))
    fetched.close()
    def on_chunk(r, at):
        assert at == 0
        checked(r.view()[0], r.recruit(gt, max_out=2))
    assert stream_chunks(ctx, bam, False, None, on_chunk) == 1
    gt.close()


# ---------------------------------------------------------------- 4: the empty chunk
def test_the_empty_chunk_of_every_source(ctx, designed, tmp_path):
    gt = make_targets(ctx, designed["loci"], paired=True)
    rset = api.Recruited(gt, keep_names=True)
    out = [str(tmp_path / f"none{l}.fq") for l in range(3)]
    w = lio.FastxWriters(out)
    none = (np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.uint32))

    def no_ops(src, v):
        assert v.n_pairs == 0 and v.mate_len.size == 0 and v.mate_off.tolist() == [0]
        # the library's own arrays: three offset arrays of one element
        hs = cdefs.ReadsHost()
        if isinstance(src, lio.FastxDevice):
            check(lib().lcty_fastx_device_view(src._h, C.byref(hs)))
        else:
            check(lib().lcty_sample_reads_view(src._h, C.byref(hs), None, None))
        assert hs.n_pairs == 0 and hs.mate_off[0] == 0 and hs.aln_off[0] == 0 and hs.cigar_off[0] == 0
        cnt, loci = src.recruit(gt, max_out=3)
        assert cnt.size == 0 and loci.shape == (0, 3)
        assert src.write_recruited(w, *none) == 0
        src.add_recruited(rset, *none)

    fq = str(tmp_path / "empty.fq")
    open(fq, "w").close()
    dev = lio.FastxDevice(ctx, fq)
    assert dev.next() == 0 and dev.n == 0
    no_ops(dev, dev.view())
    dev.close()
    # a region without reads, beside the designed ones
    reads = lio.SampleBam(designed["files"][2]).fetch(ctx, [(0, 50_000, 60_000)], paired=True)
    assert reads.stats["n_pairs"] == 0
    no_ops(reads, reads.view()[0])
    reads.close()
    # a header and nothing else: fetched whole, and streamed
    bam = str(tmp_path / "header.bam")
    SB.write_bam(bam, REFS, [])
    reads = lio.SampleBam(bam).fetch(ctx, whole_file=True, paired=False)
    assert reads.stats["n_pairs"] == 0
    no_ops(reads, reads.view()[0])
    reads.close()
    st = lio.BamStream(ctx, bam, False)
    reads, _ = st.next()
    assert reads.stats["n_pairs"] == 0
    no_ops(reads, reads.view()[0])
    st.close()
    w.close()
    assert all(rset.sizes(l) == (0, 0) for l in range(3)) and all(open(p, "rb").read() == b"" for p in out)
    rset.close()
    gt.close()
