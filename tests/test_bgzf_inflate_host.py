"""The DEFLATE decoder of locityper_amd/csrc/lcty_inflate.hpp compiled for the host (scripts/inflate_probe_host.cpp) against Python's
zlib over the corpus of tests/inflate_cases.py: the bytes and the end of every stream zlib accepts, zlib's verdict on every invalid and
every mutated stream, the class of error of the invalid ones, and the CRC helper against zlib.crc32."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import inflate_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inflate_probe") / "libinflate_probe_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "locityper_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "inflate_probe_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.inflate_probe_block.restype = C.c_uint32
    L.inflate_probe_block.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    L.inflate_probe_crc.restype = C.c_uint32
    L.inflate_probe_crc.argtypes = [C.c_char_p, C.c_uint64]
    L.inflate_probe_class.restype = C.c_char_p
    L.inflate_probe_class.argtypes = [C.c_uint32]
    L.inflate_probe_state_bytes.restype = C.c_uint32
    return L


def run(lib, case, raw=False):
    """(status, output, end) of the decoder on a case; a guard band behind the output must stay as it was"""
    out = np.full(case["isize"] + 64, 0xA5, dtype=np.uint8)
    end = C.c_uint32(0xFFFFFFFF)
    rc = lib.inflate_probe_block(case["payload"], len(case["payload"]), out.ctypes.data, case["isize"], 0 if raw else 1, C.byref(end))
    assert (out[case["isize"]:] == 0xA5).all(), case["name"]
    return rc, bytes(out[:case["isize"]]), end.value


def test_every_valid_stream_inflates_to_zlibs_bytes(lib):
    cases = IC.valid_cases()
    assert len(cases) > 100
    for c in cases:
        rc, out, end = run(lib, c)
        assert rc == 0, (c["name"], lib.inflate_probe_class(rc))
        assert out == c["out"] and end == c["end"], c["name"]
        rc, out, end = run(lib, c, raw=True)                                  # the stream alone
        assert rc == 0 and out == c["out"] and end == c["end"], c["name"]


# the class each invalid stream must end in (lcty_inflate.hpp: the enum)
CLASS_OF = {"bad-before-start": 12, "bad-distance-30": 11, "bad-literal-286": 10, "bad-btype-3": 2, "bad-stored-nlen": 3, "bad-over-subscribed": 8,
            "bad-incomplete": 8, "bad-no-end-of-block": 7, "bad-repeat-without-previous": 6, "bad-repeat-past-the-end": 6, "bad-hlit-287": 4,
            "bad-code-length-code-incomplete": 5, "bad-one-over-isize": 13, "bad-one-under-isize": 14, "bad-truncated-no-trailer": 1, "bad-crc": 15,
            "bad-trailer-isize": 16}


def test_every_invalid_stream_is_refused_with_its_class(lib):
    cases = IC.invalid_cases()
    assert {c["name"] for c in cases} == set(CLASS_OF) | {"bad-truncated"}
    for c in cases:
        rc, _, _ = run(lib, c)
        assert rc != 0, c["name"]
        if c["name"] in CLASS_OF:                                             # a stream cut in the middle ends in whatever its trailer decodes to
            assert rc == CLASS_OF[c["name"]], (c["name"], rc, lib.inflate_probe_class(rc))
    assert len({lib.inflate_probe_class(k) for k in range(18)}) == 18


def test_every_mutated_stream_gets_zlibs_verdict(lib):
    cases = IC.mutated_cases()
    assert len(cases) == 2000
    accepted = 0
    for c in cases:
        rc, out, end = run(lib, c, raw=c["raw"])
        assert (rc == 0) == (c["out"] is not None), (c["name"], rc, lib.inflate_probe_class(rc))
        if rc == 0:
            assert out == c["out"] and end == c["end"], c["name"]
            accepted += 1
    assert accepted > 10


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 65_536])
def test_crc_helper(lib, n):
    data = bytes(np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8))
    assert lib.inflate_probe_crc(data, n) == zlib.crc32(data) & 0xFFFFFFFF
    assert lib.inflate_probe_state_bytes() <= 40 * 1024                      # four wavefronts' worth fit the 160 KiB of a compute unit
