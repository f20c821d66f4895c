"""The DEFLATE encoder of locityper_amd/csrc/lcty_deflate.hpp compiled for the host (scripts/deflate_probe_host.cpp) over the corpus of
tests/deflate_cases.py: every stream inflates to its input under Python's zlib, under gzip and under the host build of the project's own
decoder (scripts/inflate_probe_host.cpp, as it is); no stream is longer than n + 5 bytes; the match finder and the dynamic codes earn
their keep; the sizes DESIGN.md 5p tables are not exceeded; the code lengths are complete and limited; a block's bytes depend on the
block alone. The device build emits the same bytes (tests/test_gpu_bgzf_deflate.py), which is what makes these tests speak for the kernel."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORED, FIXED, DYNAMIC = 0, 1, 2
# stream bytes of the four payloads at 0xff00 (the encoder is deterministic: these are what it gives; a change may lower them)
TABLED = {"acgt": 20_813, "run": 80, "random": 65_285, "bam": 39_679}


def _compile(tmp, name):
    out = str(tmp / f"lib{name}.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "locityper_amd", "csrc"),
                    os.path.join(ROOT, "scripts", f"{name}.cpp"), "-o", out], check=True)
    return C.CDLL(out)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = _compile(tmp_path_factory.mktemp("deflate_probe"), "deflate_probe_host")
    L.deflate_probe_block.restype = C.c_uint32
    L.deflate_probe_block.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.deflate_probe_last_crc.restype = C.c_uint32
    L.deflate_probe_code_lengths.restype = None
    L.deflate_probe_code_lengths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.deflate_probe_state_bytes.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def inflate_lib(tmp_path_factory):
    L = _compile(tmp_path_factory.mktemp("inflate_probe"), "inflate_probe_host")
    L.inflate_probe_block.restype = C.c_uint32
    L.inflate_probe_block.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    return L


def encode(lib, data, n=None):
    """(stream, form, crc) of the first n bytes of data; a guard band behind the n + 5 bytes of room must stay as it was"""
    n = len(data) if n is None else n
    src = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)                  # never an empty array
    out = np.full(n + 5 + 64, 0xA5, dtype=np.uint8)
    form = C.c_uint32(9)
    m = lib.deflate_probe_block(src.ctypes.data, n, out.ctypes.data, n + 5, C.byref(form))
    assert m != 0xFFFFFFFF and (out[n + 5:] == 0xA5).all()
    return bytes(out[:m]), form.value, lib.deflate_probe_last_crc()


@pytest.fixture(scope="module")
def encoded(lib):
    """every case of the corpus encoded once: name -> (data, stream, form, crc)"""
    return {name: (data,) + encode(lib, data) for name, data in DC.cases()}


def test_every_stream_inflates_to_its_input(encoded, inflate_lib):
    assert len(encoded) == 4 * 17 + 9
    for name, (data, stream, form, crc) in encoded.items():
        d = zlib.decompressobj(-15)
        assert d.decompress(stream) == data and d.eof and d.unused_data == b"", name
        assert crc == zlib.crc32(data) & 0xFFFFFFFF, name
        payload = stream + DC.trailer(data)
        assert gzip.decompress(DC.block(payload)) == data, name
        out = np.full(len(data) + 64, 0xA5, dtype=np.uint8)
        end = C.c_uint32(0xFFFFFFFF)
        rc = inflate_lib.inflate_probe_block(payload, len(payload), out.ctypes.data, len(data), 1, C.byref(end))
        assert rc == 0 and end.value == len(stream) and bytes(out[:len(data)]) == data and (out[len(data):] == 0xA5).all(), (name, rc)


def test_no_stream_is_longer_than_a_stored_block(encoded):
    for name, (data, stream, form, _) in encoded.items():
        assert len(stream) <= len(data) + 5 and form in (STORED, FIXED, DYNAMIC), name
    data, stream, form, _ = encoded[f"random-{DC.MAX_IN}"]
    assert len(stream) == DC.MAX_IN + 5 and form == STORED
    assert stream[:5] == b"\x01\x00\xff\xff\x00" and stream[5:] == data
    # one byte too far is no match: nothing but literals to gain from
    assert encoded["one-too-far"][2] == STORED


def test_matches_and_dynamic_codes_earn_their_keep(encoded):
    for kind in ("run", "bam"):
        data, stream, form, _ = encoded[f"{kind}-{DC.MAX_IN}"]
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        huffman_only = len(c.compress(data) + c.flush())
        print(kind, len(stream), "against Z_HUFFMAN_ONLY", huffman_only)
        assert len(stream) < huffman_only, kind
    assert encoded[f"bam-{DC.MAX_IN}"][2] == DYNAMIC


def test_sizes_stay_within_the_table_of_the_design(encoded):
    for kind, most in TABLED.items():
        n = len(encoded[f"{kind}-{DC.MAX_IN}"][1])
        print(kind, n, "tabled", most)
        assert n <= most, kind


def _lengths(lib, freq, limit):
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    lens = np.full(len(f) + 8, 0xA5, dtype=np.uint8)
    lib.deflate_probe_code_lengths(f.ctypes.data, len(f), limit, lens.ctypes.data)
    assert (lens[len(f):] == 0xA5).all()
    return lens[:len(f)].astype(np.int64)


def _check_lengths(lib, freq, limit):
    freq = np.asarray(freq)
    lens = _lengths(lib, freq, limit)
    used = int((freq > 0).sum())
    assert ((freq > 0) == (lens > 0)).all()
    assert lens.max(initial=0) <= limit
    kraft = int((1 << (limit - lens[lens > 0])).sum())                       # in units of 2^-limit: exact
    if used >= 2:
        assert kraft == 1 << limit, (used, limit, kraft)
    elif used == 1:
        assert lens.max() == 1
    return lens


def test_code_lengths_are_complete_and_limited(lib):
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for limit in (15, 7):
        lens = _check_lengths(lib, fib, limit)
        assert lens.max() == limit                                            # the unlimited tree is 39 deep
        assert (np.diff(lens) <= 0).all()                                     # rarer symbols never get shorter codes
    assert sorted(_check_lengths(lib, [5] * 286, 15)) == [8] * 226 + [9] * 60
    one = np.zeros(30, dtype=np.uint32); one[17] = 9
    assert _check_lengths(lib, one, 15)[17] == 1
    two = np.zeros(286, dtype=np.uint32); two[3] = 1; two[256] = 70_000
    assert _check_lengths(lib, two, 15).sum() == 2
    rng = np.random.default_rng(41)
    for k in range(2000):
        n_sym = (286, 30, 19)[k % 3]
        limit = 7 if n_sym == 19 else 15
        shape = k % 5
        f = rng.integers(0, (2, 10, 1000, 65_000, 3)[shape], n_sym)
        if shape == 4:
            f = f * rng.integers(0, 2, n_sym) * (1 << rng.integers(0, 16, n_sym))   # sparse, powers of two apart: deep trees
        _check_lengths(lib, f, limit)


def test_fibonacci_block_round_trips_with_limited_codes(encoded):
    data, stream, form, _ = encoded["fibonacci"]
    assert form == DYNAMIC and zlib.decompress(stream, -15) == data


def test_a_block_depends_on_its_own_bytes_alone(lib):
    a = DC.payload("bam")
    b, c = DC.payload("acgt", 5000), DC.payload("random", 5000)
    first = encode(lib, a + b, DC.MAX_IN)
    assert first == encode(lib, a + c, DC.MAX_IN) == encode(lib, a)
    assert first == encode(lib, a + b, DC.MAX_IN)                             # and the same twice: no state survives a block


def test_state_fits_six_blocks_in_a_compute_unit(lib):
    assert lib.deflate_probe_state_bytes() <= 160 * 1024
    assert 160 * 1024 // lib.deflate_probe_state_bytes() == 6                 # DESIGN.md 5p, lcty_deflate.hip
