"""lcty_bam_stream_* on the device against the restatement tests/pyref_bam_stream.py: whole BAM files without an index read in windows,
single-end and interleaved, across files, at BGZF block sizes and window knobs that put a record boundary, a waiting first mate and a
file's end at every place of a window; every error status with what is handed out in front of it; and the consumers of the chunks
(recruitment, the writers, the resident set) against the FASTQ route over the same reads. The inputs are the smallest that reach every
turn (tests/bam_stream_cases.py)."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from locityper_amd._lib import LocityperError
from tests import bam_stream_cases as BC
from tests import pyref_bam_stream as PB
from tests import pyref_sample_bam as SB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    return gpu_ctx


class knobs:
    """context knobs for one block, restored behind it"""

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            if v is not None:
                self.ctx.set_knob(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_knob(k, -1)


def read_all(ctx, paths, interleaved, window=None, inflate=None, on_chunk=None):
    """every chunk of the stream concatenated -> dict(mate_len, mate_off, bases2, nmask, ordinal [2 n], chunks, stats, error)"""
    lens, offs, b2, nm, ords = [], [np.zeros(1, dtype=np.uint64)], [], [], []
    out = dict(chunks=0, error=None)
    with knobs(ctx, bam_stream_window_bytes=window, sample_bam_inflate=inflate):
        st = lio.BamStream(ctx, paths, interleaved)
        try:
            while True:
                reads, stats = st.next()
                n = reads.stats["n_pairs"]
                if n == 0:
                    break
                chunk, src, paired = reads.view()
                assert paired == interleaved and chunk.n_pairs == n
                base = int(offs[-1][-1])
                lens.append(chunk.mate_len); offs.append(chunk.mate_off[1:] + np.uint64(base))
                nb = int(chunk.mate_off[-1])
                b2.append(chunk.bases2[:nb // 16]); nm.append(chunk.nmask[:nb // 32])
                ords.append(np.where(src == 0xFFFFFFFF, -1, src.astype(np.int64) + stats["first_kept"]))
                out["chunks"] += 1
                if on_chunk:
                    on_chunk(reads, stats)
        except LocityperError as e:
            out["error"] = e
            with pytest.raises(LocityperError) as again:                      # and so does every call after it
                st.next()
            assert again.value.code == e.code and str(again.value) == str(e)
        out["stats"] = st.stats
        st.close()
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dtype=dt)
    out.update(mate_len=cat(lens, np.uint32), mate_off=np.concatenate(offs), bases2=cat(b2, np.uint32), nmask=cat(nm, np.uint32), ordinal=cat(ords, np.int64))
    return out


def assert_equals(got, s):
    """the concatenated chunks against the restatement s (a PB.Stream), word for word; the error, if it has one"""
    mate_len, mate_off, bases2, nmask = s.packed()
    nb = int(mate_off[-1])
    assert got["mate_len"].tolist() == mate_len.tolist() and got["mate_off"].tolist() == mate_off.tolist()
    assert np.array_equal(got["bases2"], bases2[:nb // 16]) and np.array_equal(got["nmask"], nmask[:nb // 32])
    assert got["ordinal"].tolist() == [-1 if k is None else k for u in s.units for k in u]
    st = got["stats"]
    assert (st["records_walked"], st["records_primary"], st["records_kept"], st["bases_kept"], st["reads"]) == s.totals()
    if s.refused is None:
        assert got["error"] is None
    else:
        assert got["error"] is not None and got["error"].code == s.refused.status and s.refused.what in str(got["error"])


# ---------------------------------------------------------------- single-end, by hand
@pytest.fixture(scope="module")
def single(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_stream_single")
    recs = BC.single_end_records()
    s = PB.Stream([recs], interleaved=False)
    assert s.refused is None and len(s.units) == 21 and any(r["flag"] & 0x100 for r in recs) and any(r["flag"] & 0x800 for r in recs)
    assert {len(r["seq"]) for r in s.kept} >= {1, 31, 32, 33, 63, 64, 65, 255, 300, 5000} and any(len(r["seq"]) & 1 for r in s.kept)
    assert any(r["flag"] & 0x10 for r in s.kept) and any(set(r["seq"]) - set("ACGT") for r in s.kept)
    return dict(dir=d, recs=recs, s=s)


@pytest.mark.parametrize("block_size", [64, 200, 0xff00])
def test_single_end_at_every_block_size_and_window(ctx, single, block_size):
    path = BC.write_files(single["dir"], f"single.b{block_size}", [single["recs"]], block_size)
    for window in (1, 256, 4096, None):
        got = read_all(ctx, path, False, window)
        assert_equals(got, single["s"])
        if window is not None and block_size < 0xff00:                         # a window is whole blocks: one of 0xff00 bytes holds the file
            assert got["stats"]["windows_enlarged"] > 0, (block_size, window)      # the record of 5 000 bases is larger than the window
        if window == 1 and block_size < 0xff00:
            assert got["chunks"] > 5 and got["stats"]["bytes_carried"] > 0
    assert got["stats"]["files"] == 1 and got["stats"]["windows"] >= 1


def test_single_end_equals_the_indexed_reader_on_an_indexed_copy(ctx, single):
    # the same records where an index can be written: placed, coordinate-sorted; what the stream keeps does not look at either
    recs = [dict(r, tid=0, pos=100 + 10 * i, flag=r["flag"] & ~4, cigar=[("M", len(r["seq"]))] if r["seq"] else []) for i, r in enumerate(single["recs"])]
    path = str(single["dir"] / "indexed.bam")
    SB.write_bam(path, BC.REFS, recs, block_size=200, index=True)
    got = read_all(ctx, path, False, 256)
    assert_equals(got, PB.Stream([recs], interleaved=False))
    reads = lio.SampleBam(path).fetch(ctx, whole_file=True, paired=False)
    chunk, src, paired = reads.view()
    nb = int(chunk.mate_off[-1])
    assert not paired and chunk.mate_len.tolist() == got["mate_len"].tolist() and chunk.mate_off.tolist() == got["mate_off"].tolist()
    assert np.array_equal(chunk.bases2[:nb // 16], got["bases2"]) and np.array_equal(chunk.nmask[:nb // 32], got["nmask"])
    assert np.where(src == 0xFFFFFFFF, -1, src.astype(np.int64)).tolist() == got["ordinal"].tolist()
    reads.close()


# ---------------------------------------------------------------- interleaved, seeded
@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_stream_pairs")
    recs = BC.interleaved_records(1000)
    s = PB.Stream([recs], interleaved=True)
    assert s.refused is None and len(s.units) == 1000 and len(s.kept) == 2000 and len(recs) == 2000 + 100 + 50
    path = BC.write_files(d, "pairs", [recs], 0xff00)
    return dict(dir=d, recs=recs, s=s, path=path)


@pytest.mark.parametrize("inflate", [0, 1])
def test_interleaved_pairs_at_every_window_and_inflate(ctx, seeded, inflate):
    totals = set()
    for window in (1, 777, 65536, None):
        got = read_all(ctx, seeded["path"], True, window, inflate)
        assert_equals(got, seeded["s"])
        st = got["stats"]
        totals.add((st["records_walked"], st["records_primary"], st["records_kept"], st["bases_kept"], st["reads"], st["bytes_inflated"], st["blocks_inflated"]))
        if window == 65536:
            assert got["chunks"] > 3 and st["bytes_carried"] > 0                # kept counts of the windows cross 64 and 256
    assert len(totals) == 1


def test_129_pairs_in_one_window(ctx, tmp_path):
    recs = BC.interleaved_records(129, between=0, behind=0)
    path = BC.write_files(tmp_path, "p129", [recs])
    got = read_all(ctx, path, True)
    assert got["chunks"] == 1 and got["stats"]["windows"] == 1 and got["stats"]["records_kept"] == 258    # the last pair: lanes 0 and 1 of a second block
    assert_equals(got, PB.Stream([recs], interleaved=True))
    again = read_all(ctx, path, True)                                          # two runs: the same bytes
    for k in ("mate_len", "mate_off", "bases2", "nmask", "ordinal"):
        assert got[k].tobytes() == again[k].tobytes()


# ---------------------------------------------------------------- several files
def test_a_pair_across_three_files(ctx, tmp_path):
    files = BC.three_files()
    s = PB.Stream(files, interleaved=True)
    assert s.refused is None and len(s.units) == 4 and files[1] == [] and files[0][-1]["flag"] & 0x800 and files[2][0]["flag"] & 0x100
    for block_size in (64, 0xff00):
        paths = BC.write_files(tmp_path, f"three.b{block_size}", files, block_size)
        for window in (1, 300, None):
            got = read_all(ctx, paths, True, window)
            assert_equals(got, s)
            assert got["stats"]["files"] == 3 and got["stats"]["bytes_carried"] > 0
    # single-end over the same files: every kept record, file after file
    assert_equals(read_all(ctx, paths, False, 300), PB.Stream(files, interleaved=False))


def test_a_file_cut_in_its_last_record_is_refused_by_name(ctx, tmp_path):
    files, interleaved = BC.error_cases()["cut"]
    paths = BC.write_files(tmp_path, "cut", files, 200)
    s = PB.Stream(files, interleaved, paths)
    assert s.refused is not None and paths[1] in s.refused.what and len(s.units) == 71
    for window in (1, None):
        got = read_all(ctx, paths, interleaved, window)
        assert_equals(got, s)
        assert "cut.1.bam" in str(got["error"]) and "leaves the end of its file" in str(got["error"])


# ---------------------------------------------------------------- names
def test_names_of_mates(ctx, tmp_path):
    files, _ = BC.error_cases()["names-pass"]
    got = read_all(ctx, BC.write_files(tmp_path, "names", files), True)
    assert got["error"] is None and len(got["mate_len"]) == 10                 # r/1 + r/2, abc + xyz, abcd + xbzz (and the shortest names)
    for a, b in (("abcd", "aXcd"), ("abcd", "abcde")):
        files = [BC.pair("r/1", "r/2") + BC.pair(a, b)]
        paths = BC.write_files(tmp_path, f"names-{b}", files)
        got = read_all(ctx, paths, True)
        assert_equals(got, PB.Stream(files, True, paths))
        assert got["error"].code == cdefs.ERR_INVALID_DATA and f"({a} and {b})" in str(got["error"]) and len(got["mate_len"]) == 2


# ---------------------------------------------------------------- errors
@pytest.mark.parametrize("case", ["odd", "odd-two-files", "noseq-first", "noseq-second", "noseq-single", "noseq-dropped", "short", "short-dropped",
                                  "mismatch-len", "mismatch-byte", "mismatch-then-noseq", "noseq-then-mismatch"])
def test_the_first_offending_record_decides(ctx, tmp_path, case):
    files, interleaved = BC.error_cases()[case]
    paths = BC.write_files(tmp_path, case, files, 200)
    s = PB.Stream(files, interleaved, paths)
    assert (s.refused is None) == (case == "noseq-dropped") and len(s.units) >= 70
    handed = []
    for window in (1, None):
        got = read_all(ctx, paths, interleaved, window)
        assert_equals(got, s)                                                 # the pairs in front, then the status and message, then the status again
        handed.append((got["mate_len"].tobytes(), got["bases2"].tobytes(), got["ordinal"].tobytes()))
    assert handed[0] == handed[1]
    if case == "mismatch-then-noseq":
        assert "non matching" in s.refused.what
    if case == "noseq-then-mismatch":
        assert "has no sequence" in s.refused.what
    if case.startswith("odd"):
        message = str(got["error"]).split("] ", 1)[1]                          # behind "[lcty error 2] "
        assert message.startswith("Odd number of records in an interleaved input file(s)") and all(p in message for p in paths)


def test_open_errors(ctx, tmp_path):
    import gzip
    def refused(code, paths, *words):
        with pytest.raises(LocityperError) as e:
            lio.BamStream(ctx, paths)
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value)
    good = BC.write_files(tmp_path, "good", [BC.pair("a/1", "a/2")])[0]
    cram, gz, empty, plain = (str(tmp_path / n) for n in ("x.cram", "x.gz", "empty.bam", "plain.bam"))
    open(cram, "wb").write(b"CRAM\x03\x00" + bytes(64))
    with gzip.open(gz, "wb") as f:
        f.write(b"BAM\1" + bytes(100))
    open(empty, "wb").close()
    data, _ = SB.bgzf_blocks(b"BAX\1" + bytes(50), 0xff00)
    open(plain, "wb").write(data)
    refused(cdefs.ERR_UNSUPPORTED, [cram], "CRAM")
    refused(cdefs.ERR_INVALID_DATA, [gz], "is not a BAM file")
    refused(cdefs.ERR_INVALID_DATA, [good, empty], "empty.bam is not a BAM file")
    refused(cdefs.ERR_INVALID_DATA, [plain], "is not a BAM file")
    refused(cdefs.ERR_INVALID_INPUT, [good, str(tmp_path / "nowhere.bam")], "cannot open")
    refused(cdefs.ERR_INVALID_INPUT, [])
    head = SB.header_bytes(BC.REFS)
    data, _ = SB.bgzf_blocks(head[:-3], 0xff00)
    open(plain, "wb").write(data)
    refused(cdefs.ERR_INVALID_DATA, [plain], "truncated BAM header")
    from locityper_amd._lib import lib, VP
    import ctypes as C
    out = VP()
    arr = (C.c_char_p * 1)(good.encode())
    assert lib().lcty_bam_stream_open(None, arr, 1, 0, C.byref(out)) == cdefs.ERR_INVALID_INPUT
    assert lib().lcty_bam_stream_open(ctx._h, None, 1, 0, C.byref(out)) == cdefs.ERR_INVALID_INPUT
    assert lib().lcty_bam_stream_open(ctx._h, arr, 1, 0, None) == cdefs.ERR_INVALID_INPUT
    assert lib().lcty_bam_stream_open(ctx._h, (C.c_char_p * 1)(None), 1, 0, C.byref(out)) == cdefs.ERR_INVALID_INPUT and not out.value
    st = lio.BamStream(ctx, good)
    assert lib().lcty_bam_stream_next(st._h, None, None, None) == cdefs.ERR_INVALID_INPUT
    with knobs(ctx, bam_stream_window_bytes=0):
        refused(cdefs.ERR_INVALID_INPUT, [good], "bam_stream_window_bytes")
    # the indexed reader is what it was: paired reads of a whole file stay refused there
    SB.write_bam(str(tmp_path / "ix.bam"), BC.REFS, [SB.rec(0, 10, "a", 0x41, [("M", 4)], "ACGT"), SB.rec(0, 20, "a", 0x81, [("M", 4)], "ACGT")])
    with pytest.raises(LocityperError) as e:
        lio.SampleBam(str(tmp_path / "ix.bam")).fetch(ctx, whole_file=True, paired=True)
    assert e.value.code == cdefs.ERR_UNSUPPORTED
    st.close()


# ---------------------------------------------------------------- downstream: the same reads as a name-grouped BAM and as interleaved FASTQ
def _two_loci():
    rng = np.random.default_rng(21)
    return [[bytes(rng.choice(list(b"ACGT"), 3000).astype(np.uint8)) for _ in range(2)] for _ in range(2)]


def _targets(ctx, loci, base_k=25):
    gt = api.Targets(ctx, api.recruit_params(paired=True))
    for alleles in loci:
        counts = [np.zeros(len(a) - base_k + 1, dtype=np.uint16) for a in alleles]
        seqs = np.frombuffer(b"".join(alleles), dtype=np.uint8)
        seq_off = np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64)
        cnt_off = np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64)
        gt.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, base_k)
    gt.finalize()
    return gt


def test_downstream_equals_the_fastq_route(ctx, tmp_path):
    rng = np.random.default_rng(8)
    loci = _two_loci()
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    recs, fq = [], []
    for i in range(400):
        if i % 3 == 0:
            a = loci[i % 2][(i // 2) % 2]
            p = int(rng.integers(0, 3000 - 400))
            s1, s2 = a[p:p + 120].decode(), a[p + 250:p + 370].translate(comp)[::-1].decode()
        else:
            s1, s2 = BC.seq_of(rng, 120), BC.seq_of(rng, 120)
        q1, q2 = bytes([30 + i % 10] * 120), bytes([20 + i % 7] * 120)
        # the file holds mate 2 of every fifth pair as it was aligned: reverse-complemented with flag 0x10, which the reader undoes
        rev = i % 5 == 0
        b_seq = s2.encode().translate(comp)[::-1].decode() if rev else s2
        recs.append(SB.rec(-1, -1, f"p{i}/1", 0x4D, [], s1, q1))
        if i % 6 == 0:
            recs.append(SB.rec(-1, -1, f"p{i}/1", 0x800 | 4, [], s1[:30], q1[:30]))
        recs.append(SB.rec(-1, -1, f"p{i}/2", 0x8D | (0x10 if rev else 0), [], b_seq, q2[::-1] if rev else q2))
        fq.append(f"@p{i}/1\n{s1}\n+\n{''.join(chr(q + 33) for q in q1)}\n@p{i}/2\n{s2}\n+\n{''.join(chr(q + 33) for q in q2)}\n")
    bam, fastq = str(tmp_path / "grouped.bam"), str(tmp_path / "reads.fq")
    SB.write_bam(bam, BC.REFS, recs, block_size=3000, index=False)
    open(fastq, "w").write("".join(fq))
    s = PB.Stream([recs], interleaved=True)
    assert s.refused is None and len(s.units) == 400
    gt = _targets(ctx, loci)

    def run(source):
        rset = api.Recruited(gt, keep_names=True)
        paths = [str(tmp_path / f"{source}{l}.fq") for l in range(2)]
        w = lio.FastxWriters(paths)
        cnts, locis = [], []
        if source == "bam":
            def on_chunk(reads, stats):
                cnt, lc = reads.recruit(gt)
                assert reads.write_recruited(w, cnt, lc) == int((cnt > 0).sum())
                reads.add_recruited(rset, cnt, lc)
                cnts.append(cnt.copy()); locis.append(lc.copy())
            got = read_all(ctx, bam, True, 20_000, on_chunk=on_chunk)
            assert got["chunks"] > 3 and got["error"] is None
        else:
            dev = lio.FastxDevice(ctx, fastq, interleaved=True)
            while dev.next(90):
                cnt, lc = dev.recruit(gt)
                dev.write_recruited(w, cnt, lc)
                dev.add_recruited(rset, cnt, lc)
                cnts.append(cnt.copy()); locis.append(lc.copy())
            dev.close()
        w.close()
        cnt, lc = np.concatenate(cnts), np.concatenate(locis)
        return rset, cnt, lc, [open(p, "rb").read() for p in paths]

    from_bam, cnt, lc, text = run("bam")
    from_fq, cnt2, lc2, text2 = run("fastq")
    answered = np.arange(lc.shape[1])[None, :] < cnt[:, None]
    assert np.array_equal(cnt, cnt2) and np.array_equal(lc[answered], lc2[answered])
    assert (cnt > 0).sum() > 50 and (cnt == 0).sum() > 200
    for l in range(2):
        mine = {i for i in range(400) if l in lc[i, :cnt[i]]}
        assert text[l] == s.text(which=mine) == text2[l]
        (a, oa), (b, ob) = from_bam.view(l), from_fq.view(l)
        assert a.n_pairs == len(mine) and np.array_equal(oa, ob)
        for x, y in ((a.mate_len, b.mate_len), (a.mate_off, b.mate_off), (a.bases2, b.bases2), (a.nmask, b.nmask)):
            assert np.array_equal(x, y)
        assert from_bam.names(l) == from_fq.names(l) == [f"p{i}/1" for i in sorted(mine)]
    from_bam.close(); from_fq.close(); gt.close()
