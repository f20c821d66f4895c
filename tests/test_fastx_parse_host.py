"""The record rules of locityper_amd/csrc/lcty_fastx_parse.hpp and the windows of lcty_fastx_window.hpp on the CPU, with the serial
executor of scripts/fastx_probe_host.cpp in place of the kernels, over the corpus of tests/fastx_cases.py: the records,
the status and the message against tests/pyref_fastx.py and against the host reader lcty_fastx_next as it stands, at windows of 64, 65,
127 and 4096 bytes and the default, one record a call and without a limit; the containers; the knob and its place in the header."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import pytest

from locityper_amd import _lib, cdefs
from locityper_amd import io as lio
from tests import fastx_cases as FC
from tests import pyref_fastx as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = [64, 65, 127, 4096, 1 << 28]
LIMIT = (1 << 31) - 64


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fastx_probe") / "libfastx_probe_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "locityper_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "fastx_probe_host.cpp"), "-lz", "-o", out], check=True)
    L = C.CDLL(out)
    L.fastx_probe_run.restype = C.c_int32
    L.fastx_probe_run.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                  C.c_char_p, C.POINTER(C.c_uint64)]
    L.fastx_probe_free.argtypes = [C.c_void_p]
    return L


def run_probe(L, paths, interleaved, window, max_records=2 ** 64 - 1, limit=LIMIT):
    """(status, message, [(name, seq, qual), ..], counters) of the windowed reader with the serial executor"""
    out, n, msg, cnt = C.c_void_p(), C.c_uint64(0), C.create_string_buffer(1024), (C.c_uint64 * 5)()
    rc = L.fastx_probe_run(paths[0].encode(), paths[1].encode() if len(paths) > 1 else None, int(interleaved), window, limit, max_records,
                           C.byref(out), C.byref(n), msg, cnt)
    raw = C.string_at(out, n.value)
    L.fastx_probe_free(out)
    recs, at = [], 0
    while at < len(raw):
        f = []
        for _ in range(3):
            (ln,) = struct.unpack_from("<I", raw, at)
            f.append(raw[at + 4:at + 4 + ln]); at += 4 + ln
        recs.append(tuple(f))
    return rc, msg.value.decode("latin-1"), recs, dict(zip(("bytes_read", "bytes_inflated", "windows", "windows_enlarged", "records"), cnt))


def what_of(paths):
    return " and ".join(paths)


def flat(units):
    return [(n, s, q or b"") for u in units for (n, s, q) in u]


def host_route(paths, interleaved, tmp, max_records=7):
    """lcty_fastx_next / lcty_fastx_write_recruited as they stand: every record written to one file -> (its bytes, error or None)"""
    out = os.path.join(tmp, "host_route.txt")
    w = lio.FastxWriters([out])
    err = None
    try:
        f = lio.Fastx(paths[0], paths[1] if len(paths) > 1 else None, interleaved=interleaved)
        while True:
            ch = f.next(max_records)
            if ch is None:
                break
            f.write_recruited(w, [1] * ch.n_pairs, [[0]] * ch.n_pairs)
    except _lib.LocityperError as e:
        err = e
    w.close()
    return open(out, "rb").read(), err


CASES = FC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_records_status_and_message_are_the_reference_readers(probe, case, tmp_path):
    paths = FC.write_case(case, str(tmp_path))
    units, err = PR.read_all(case["files"], case["interleaved"], what_of(paths))
    assert (err is None) == (case["kind"] != "error"), (case["name"], err)
    # the host reader as it stands agrees with the restated rules (a chunk that meets the error is lost as a whole: no limit of 7 then)
    text, herr = host_route(paths, case["interleaved"], str(tmp_path), max_records=1)
    assert text == b"".join(PR.record_text(r) for u in units for r in u), case["name"]
    assert (herr is None) == (err is None) and (err is None or (herr.code == err.code and str(herr).endswith(err.msg))), (case["name"], herr, err)
    for window in WINDOWS:
        for max_records in (1, 2 ** 64 - 1):
            rc, msg, recs, cnt = run_probe(probe, paths, case["interleaved"], window, max_records)
            if case["kind"] == "mixed":                                     # refused, naming the record, after the records in front of it
                assert rc == cdefs.ERR_UNSUPPORTED and ("record s1" in msg or "record r1" in msg), (case["name"], window, msg)
                assert recs == flat(units)[:len(recs)] and len(recs) == 1
                continue
            assert recs == flat(units), (case["name"], window, max_records)
            assert (rc, msg) == ((cdefs.OK, "") if err is None else (err.code, err.msg)), (case["name"], window, max_records, msg)
            total = sum(len(f) for f in case["files"])                     # small windows stop reading at the end of the input or the error
            assert cnt["records"] == len(recs) and (cnt["bytes_read"] == total if window == WINDOWS[-1] else cnt["bytes_read"] <= total)


@pytest.mark.parametrize("fasta", [False, True])
def test_seeded_records_at_small_windows(probe, fasta, tmp_path):
    case = FC.property_case(fasta=fasta)
    paths = FC.write_case(case, str(tmp_path))
    units, err = PR.read_all(case["files"], False, paths[0])
    assert err is None and len(units) == 2000
    for window in (64, 1024, 1 << 28):
        rc, msg, recs, cnt = run_probe(probe, paths, False, window)
        assert rc == 0 and recs == flat(units), (window, msg)
        assert window == 1024 or (cnt["windows_enlarged"] > 0) == (window == 64)   # records of up to 1.2 kb: a window of 64 bytes grows


def test_containers_give_the_same_records(probe, tmp_path):
    case = FC.property_case(seed=8, n=700)
    data = case["files"][0]
    plain, gz, multi, bgzf = (str(tmp_path / n) for n in ("r.fq", "r.fq.gz", "multi.fq.gz", "r.bgzf.fq.gz"))
    open(plain, "wb").write(data)
    with gzip.open(gz, "wb") as f:
        f.write(data)
    with open(multi, "wb") as f:                                             # several gzip members, as `cat a.gz b.gz` leaves them
        f.write(gzip.compress(data[:1000]) + gzip.compress(b"") + gzip.compress(data[1000:]))
    lio.write_bgzf(bgzf, data)
    assert len(data) > 3 * 0xff00                                            # several blocks
    want = flat(PR.read_all([data], False, plain)[0])
    for path in (plain, gz, multi, bgzf):
        for window in (64, 4096, 100_000, 1 << 28):
            rc, msg, recs, cnt = run_probe(probe, [path], False, window)
            assert rc == 0 and recs == want, (path, window, msg)
            assert cnt["bytes_read"] == os.path.getsize(path) and cnt["bytes_inflated"] == (0 if path == plain else len(data))
    for bad in ("reads.fq.lz4", "reads.fq.br"):
        open(tmp_path / bad, "wb").write(data)
        rc, msg, _, _ = run_probe(probe, [str(tmp_path / bad)], False, 4096)
        assert rc == cdefs.ERR_UNSUPPORTED and "plain or gzip-compressed" in msg
    rc, msg, _, _ = run_probe(probe, [str(tmp_path / "missing.fq")], False, 4096)
    assert rc == cdefs.ERR_INVALID_INPUT and "cannot open" in msg
    open(tmp_path / "cut.fq.gz", "wb").write(open(gz, "rb").read()[:-40])   # a gzip stream that ends early
    rc, msg, _, _ = run_probe(probe, [str(tmp_path / "cut.fq.gz")], False, 4096)
    assert rc == cdefs.ERR_INVALID_DATA


def test_a_record_beyond_the_window_limit_is_refused_naming_the_knob(probe, tmp_path):
    p = str(tmp_path / "long.fq")
    open(p, "wb").write(b"@r1\nACGT\n+\nIIII\n@long\n" + b"A" * 3000 + b"\n+\n" + b"I" * 3000 + b"\n")
    rc, msg, recs, cnt = run_probe(probe, [p], False, 64, limit=4096)
    assert rc == cdefs.ERR_UNSUPPORTED and "fastx_window_bytes" in msg and [r[0] for r in recs] == [b"r1"] and cnt["windows_enlarged"] >= 5
    rc, msg, recs, _ = run_probe(probe, [p], False, 64, limit=8192)          # 6 030 bytes fit
    assert rc == 0 and len(recs) == 2 and len(recs[1][1]) == 3000
    rc, msg, _, _ = run_probe(probe, [p], False, 63)
    assert rc == cdefs.ERR_INVALID_INPUT and "fastx_window_bytes" in msg


def test_window_knobs_are_in_the_list_and_in_the_header():
    """tests/test_host_api.py's rule for a knob: in the list lcty_ctx_set_knob accepts, with its words in the header's knob paragraph,
    and what the reader asks its context for"""
    import re
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    api_src, header, src = read("locityper_amd", "csrc", "lcty_api.hip"), read("include", "locityper_hip.h"), read("locityper_amd", "csrc", "lcty_fastx_device.hip")
    known = api_src[api_src.index("known[] = {"):api_src.index("nullptr};")]
    paragraph = header[:header.index("int32_t lcty_ctx_set_knob(")]
    asked = set(re.findall(r'knob\("(fastx_[a-z_]+)"', src))
    assert asked == {"fastx_window_bytes", "fastx_window_limit"}
    for name in asked:
        assert f'"{name}"' in known and f'"{name}"   ' in paragraph, name
    assert "2^28" in paragraph[paragraph.index('"fastx_window_bytes"'):][:200]
