"""FASTA / FASTQ text parsed on the device (lcty_fastx_device_*) against the host route as it stands (lcty_fastx_next,
lcty_fastx_write_recruited, lcty_recruit) and tests/pyref_fastx.py, over the corpus of tests/fastx_cases.py: the same records in the
same layout, word for word; the same status and message; the same recruitment and the same per-locus files."""
import gzip
import os

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from locityper_amd import io as lio
from tests import fastx_cases as FC
from tests import pyref_fastx as PR

pytestmark = pytest.mark.gpu

WINDOWS = [64, 65, 127, 4096, -1]                     # -1: the default, 2^28
NO_LIMIT = 2 ** 62


@pytest.fixture(scope="module")
def gpu_ctx():
    return api.Context(0)


def open_pair(ctx, paths, interleaved, window=-1, inflate=-1, limit=-1):
    ctx.set_knob("fastx_window_bytes", window); ctx.set_knob("sample_bam_inflate", inflate); ctx.set_knob("fastx_window_limit", limit)
    try:
        dev = lio.FastxDevice(ctx, paths[0], paths[1] if len(paths) > 1 else None, interleaved=interleaved)
    finally:
        for k in ("fastx_window_bytes", "fastx_window_limit"):
            ctx.set_knob(k, -1)
    return dev, lio.Fastx(paths[0], paths[1] if len(paths) > 1 else None, interleaved=interleaved)


def same_chunk(v, h):
    nb = int(h.mate_off[-1])
    assert np.array_equal(v.mate_len, h.mate_len) and np.array_equal(v.mate_off, h.mate_off)
    # the layout of pack(): every mate at the running sum of the lengths rounded up to 32
    assert np.array_equal(v.mate_off, np.concatenate([[0], np.cumsum((v.mate_len.astype(np.uint64) + 31) // 32 * 32)]))
    assert np.array_equal(v.bases2[:nb // 16 + 1], h.bases2[:nb // 16 + 1]) and np.array_equal(v.nmask[:nb // 32 + 1], h.nmask[:nb // 32 + 1])


def both_routes(ctx, paths, interleaved, tmp, window=-1, max_records=NO_LIMIT, inflate=-1, limit=-1, keep=False):
    """The two routes in step: every chunk of the device route against lcty_fastx_next for as many records; every record written
    through both writers. -> (units read, error of the device route or None, error of the host route or None, the chunks when kept)"""
    dev, host = open_pair(ctx, paths, interleaved, window, inflate, limit)
    assert dev.paired == host.paired
    out = [os.path.join(tmp, "dev.txt"), os.path.join(tmp, "host.txt")]
    wd, wh = lio.FastxWriters([out[0]]), lio.FastxWriters([out[1]])
    n_units, derr, herr, chunks = 0, None, None, []
    ctx.set_knob("sample_bam_inflate", inflate)
    try:
        while True:
            try:
                n = dev.next(max_records)
            except _lib.LocityperError as e:
                derr = e
                break
            if n == 0:
                break
            assert n <= max_records
            v = dev.view()
            h = host.next(n)
            assert h is not None and h.n_pairs == n
            same_chunk(v, h)
            ones, zeros = np.ones(n, dtype=np.uint32), np.zeros((n, 1), dtype=np.uint32)
            assert dev.write_recruited(wd, ones, zeros) == n and host.write_recruited(wh, ones, zeros) == n
            n_units += n
            if keep:
                chunks.append(v)
        try:
            assert host.next(1) is None or derr is not None                  # the device route never ends early
        except _lib.LocityperError as e:
            herr = e
    finally:
        ctx.set_knob("sample_bam_inflate", -1)
        wd.close(); wh.close()
    assert open(out[0], "rb").read() == open(out[1], "rb").read()
    assert dev.stats["records"] == n_units * (2 if dev.paired else 1)
    stats = dev.stats
    dev.close(); host.close()
    return n_units, derr, herr, chunks, stats, open(out[0], "rb").read()


CASES = FC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_equals_the_host_route(gpu_ctx, case, tmp_path):
    paths = FC.write_case(case, str(tmp_path))
    units, err = PR.read_all(case["files"], case["interleaved"], " and ".join(paths))
    text = b"".join(PR.record_text(r) for u in units for r in u)
    for window in WINDOWS:
        for max_records in (1, NO_LIMIT):
            n, derr, herr, _, stats, written = both_routes(gpu_ctx, paths, case["interleaved"], str(tmp_path), window, max_records)
            where = (case["name"], window, max_records, derr, herr)
            if case["kind"] == "mixed":                                     # the host reader goes on; the device route refuses, naming the record
                assert n == 1 and herr is None and derr.code == cdefs.ERR_UNSUPPORTED and ("record s1" in str(derr) or "record r1" in str(derr)), where
                continue
            assert n == len(units) and written == text, where
            if case["kind"] == "valid":
                assert derr is None and herr is None, where
            else:                                                            # the same status and message, and the reference's
                assert derr is not None and herr is not None and derr.code == herr.code == err.code and str(derr) == str(herr), where
                assert str(derr).endswith(err.msg), where
            if case["name"] == "read-of-10000" and window != -1:
                assert stats["windows_enlarged"] > 0, where                   # a read longer than the window: the window grows


def test_a_record_beyond_the_window_limit_is_refused_naming_the_knob(gpu_ctx, tmp_path):
    p = str(tmp_path / "long.fq")
    open(p, "wb").write(b"@r1\nACGT\n+\nIIII\n@long\n" + b"A" * 3000 + b"\n+\n" + b"I" * 3000 + b"\n")
    n, derr, herr, _, stats, _ = both_routes(gpu_ctx, [p], False, str(tmp_path), window=64, limit=4096)
    assert n == 1 and herr is None and derr.code == cdefs.ERR_UNSUPPORTED and "fastx_window_bytes" in str(derr) and stats["windows_enlarged"] >= 5
    n, derr, herr, _, _, _ = both_routes(gpu_ctx, [p], False, str(tmp_path), window=64, limit=8192)
    assert n == 2 and derr is None and herr is None
    gpu_ctx.set_knob("fastx_window_bytes", 63)
    with pytest.raises(_lib.LocityperError) as e:
        lio.FastxDevice(gpu_ctx, p)
    gpu_ctx.set_knob("fastx_window_bytes", -1)
    assert e.value.code == cdefs.ERR_INVALID_INPUT and "fastx_window_bytes" in str(e.value)
    for bad in ("reads.fq.lz4", "reads.fq.br"):
        with pytest.raises(_lib.LocityperError) as e:
            lio.FastxDevice(gpu_ctx, tmp_path / bad)
        assert e.value.code == cdefs.ERR_UNSUPPORTED
    with pytest.raises(_lib.LocityperError) as e:
        lio.FastxDevice(gpu_ctx, tmp_path / "a.fq", tmp_path / "b.fq", interleaved=True)
    assert e.value.code == cdefs.ERR_INVALID_INPUT


@pytest.mark.parametrize("fasta", [False, True])
def test_seeded_records_equal_the_host_route_and_two_runs_are_identical(gpu_ctx, fasta, tmp_path):
    case = FC.property_case(fasta=fasta)
    paths = FC.write_case(case, str(tmp_path))
    runs = [both_routes(gpu_ctx, paths, False, str(tmp_path), window=1024, keep=True) for _ in range(2)]
    for n, derr, herr, chunks, stats, _ in runs:
        assert n == 2000 and derr is None and herr is None and stats["windows"] > 100
    assert len(runs[0][3]) == len(runs[1][3])
    for a, b in zip(runs[0][3], runs[1][3]):
        assert all(np.array_equal(x, y) for x, y in ((a.mate_len, b.mate_len), (a.mate_off, b.mate_off), (a.bases2, b.bases2), (a.nmask, b.nmask)))


def test_containers_and_both_inflates_give_identical_arrays(gpu_ctx, tmp_path):
    data = FC.property_case(seed=8, n=2000)["files"][0]
    plain, gz, bgzf = (str(tmp_path / n) for n in ("r.fq", "r.fq.gz", "r.bgzf.fq.gz"))
    open(plain, "wb").write(data)
    with gzip.open(gz, "wb") as f:
        f.write(data)
    lio.write_bgzf(bgzf, data)
    assert len(data) > 8 * 0xff00
    got = {}
    for path in (plain, gz, bgzf):
        for inflate in (0, 1):
            for window in (100_000, -1):
                n, derr, herr, chunks, stats, _ = both_routes(gpu_ctx, [path], False, str(tmp_path), window=window, inflate=inflate, keep=True)
                assert n == 2000 and derr is None and herr is None and stats["records"] == 2000
                assert stats["bytes_read"] == os.path.getsize(path) and stats["bytes_inflated"] == (0 if path == plain else len(data))
                got[path, inflate, window] = chunks
    first = got[plain, 0, -1]
    assert len(first) == 1
    for key, chunks in got.items():
        if key[2] == -1:                                                     # one window: one chunk, the same arrays
            assert len(chunks) == 1 and all(np.array_equal(getattr(chunks[0], f), getattr(first[0], f)) for f in ("mate_len", "mate_off", "bases2", "nmask")), key
        else:                                                                # the same windows whatever inflates them
            ref = got[key[0], 0, key[2]]
            assert len(chunks) == len(ref) > 1 and all(np.array_equal(a.bases2, b.bases2) and np.array_equal(a.mate_off, b.mate_off) for a, b in zip(chunks, ref)), key


def test_recruitment_and_the_per_locus_files_of_the_two_routes(gpu_ctx, tmp_path):
    """The small loci and seeded reads of tests/test_gpu_recruit.py (locus-drawn and foreign pairs): lcty_fastx_device_recruit equals
    lcty_recruit on the host view entry for entry, and the per-locus files are byte-equal, plain and .gz, from FASTQ and from FASTA."""
    from tests.test_gpu_recruit import _both, _reads
    from tests.test_oracle_recruit import _loci
    rng = np.random.default_rng(21)
    loci = _loci(rng, n_loci=3)
    gt, _ = _both(gpu_ctx, loci)
    pairs = _reads(rng, loci, 300)
    qual = lambda n: "".join(chr(33 + int(q)) for q in rng.integers(2, 40, n))
    with gzip.open(tmp_path / "r1.fq.gz", "wt") as a, open(tmp_path / "r2.fq", "w") as b, open(tmp_path / "r1.fa", "w") as fa, open(tmp_path / "r2.fa", "w") as fb:
        for i, p in enumerate(pairs):
            a.write(f"@pair{i}/1 some description\n{p['seq1']}\n+\n{qual(len(p['seq1']))}\n")
            b.write(f"@pair{i}/2\n{p['seq2']}\n+pair{i}/2\n{qual(len(p['seq2']))}\n")
            fa.write(f">pair{i}/1 d\n" + "".join(p["seq1"][k:k + 61] + "\n" for k in range(0, len(p["seq1"]), 61)))
            fb.write(f">pair{i}/2\n{p['seq2']}\n")
    for kind, files in (("fq", ("r1.fq.gz", "r2.fq")), ("fa", ("r1.fa", "r2.fa"))):
        paths = [str(tmp_path / f) for f in files]
        for window in (4096, -1):
            dev, host = open_pair(gpu_ctx, paths, False, window)
            names = [[str(tmp_path / f"{route}_{kind}_locus{l}.{kind}") + (".gz" if l == 1 else "") for l in range(len(loci))] for route in ("dev", "host")]
            wd, wh = lio.FastxWriters(names[0]), lio.FastxWriters(names[1])
            n_pairs = n_recruited = 0
            while True:
                n = dev.next(64)
                if n == 0:
                    break
                answer = lambda cnt, lc: (cnt, np.where(np.arange(lc.shape[1])[None, :] < cnt[:, None], lc, 0))    # the entries in front of cnt
                cnt, lc = answer(*dev.recruit(gt))
                h = host.next(n)
                hcnt, hlc = answer(*gt.recruit(h, paired=True))
                vcnt, vlc = answer(*gt.recruit(dev.view(), paired=True))
                assert np.array_equal(cnt, hcnt) and np.array_equal(lc, hlc) and np.array_equal(cnt, vcnt) and np.array_equal(lc, vlc)
                written = dev.write_recruited(wd, cnt, lc)
                assert written == host.write_recruited(wh, hcnt, hlc) == int((cnt > 0).sum())
                n_pairs += n; n_recruited += written
            wd.close(); wh.close()
            assert host.next(1) is None and n_pairs == 300 and n_recruited > 100
            sizes = [os.path.getsize(f) for f in names[0]]
            assert sum(1 for s in sizes if s > 100) >= 2                      # the sample recruits to several loci
            for d, h in zip(*names):
                assert open(d, "rb").read() == open(h, "rb").read(), (d, window)
            dev.close(); host.close()
    other = api.Context(0)                                                   # the handle's context must be the targets'
    dev = lio.FastxDevice(other, tmp_path / "r1.fq.gz", tmp_path / "r2.fq")
    assert dev.next(10) == 10
    with pytest.raises(_lib.LocityperError) as e:
        dev.recruit(gt)
    assert e.value.code == cdefs.ERR_INVALID_INPUT and "different contexts" in str(e.value)
    dev.close()
    gt.close()
