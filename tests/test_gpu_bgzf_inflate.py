"""lcty_bgzf_inflate on the device against Python's zlib, over the corpus of tests/inflate_cases.py: the valid blocks in one call, many
tiny blocks (the grid stride), every invalid stream with its status and offset, the first refused block of several, the context after a
refusal, sizing, the capacity check, and the host route of blocks with more in their gzip header. The mutated streams stay on the CPU
(tests/test_bgzf_inflate_host.py)."""
import struct
import zlib

import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from locityper_amd._lib import LocityperError
from tests import inflate_cases as IC
from tests import pyref_sample_bam as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def good():
    """a small valid block and its bytes"""
    data = b"ACGTTGCA" * 40 + b"the quick brown fox"
    return IC.block(IC._deflate(data, 6) + IC.trailer(data)), data


def _refused(ctx, comp, status, *words):
    with pytest.raises(LocityperError) as err:
        lio.bgzf_inflate(ctx, comp)
    assert err.value.code == status, str(err.value)
    for w in words:
        assert w in str(err.value), str(err.value)


def test_valid_corpus_in_one_call(ctx):
    cases = IC.valid_cases()
    comp = b"".join(IC.block(c["payload"]) for c in cases)
    want = b"".join(c["out"] for c in cases)
    out, st = lio.bgzf_inflate(ctx, comp)
    assert out.tobytes() == want
    assert st["n_blocks"] == len(cases) and st["bytes_in"] == len(comp) and st["bytes_out"] == len(want) and st["ms_kernel"] > 0
    again, _ = lio.bgzf_inflate(ctx, comp)
    assert np.array_equal(out, again)


def test_three_thousand_tiny_blocks(ctx):
    rng = np.random.default_rng(4)
    src = IC._payload("bam")
    comp, want = [], []
    for k in range(3000):
        n = int(rng.integers(0, 48))
        at = int(rng.integers(0, len(src) - 64))
        data = src[at:at + n]
        comp.append(IC.block(IC._deflate(data, (0, 1, 6)[k % 3]) + IC.trailer(data)) if k % 50 else P.EOF_BLOCK)
        want.append(data if k % 50 else b"")
    out, st = lio.bgzf_inflate(ctx, b"".join(comp))
    assert out.tobytes() == b"".join(want) and st["n_blocks"] == 3000


def test_every_invalid_stream_is_refused_and_the_context_goes_on(ctx, good):
    for c in IC.invalid_cases():
        blk = IC.block(c["payload"])
        said = struct.unpack("<I", blk[-4:])[0]
        _refused(ctx, blk, cdefs.ERR_INVALID_DATA, "offset 0", "corrupt BGZF block" if said <= 65_536 else "a BGZF block of")
        _refused(ctx, good[0] + blk, cdefs.ERR_INVALID_DATA, f"offset {len(good[0])}")
        out, _ = lio.bgzf_inflate(ctx, good[0])
        assert out.tobytes() == good[1], c["name"]


def test_the_first_refused_block_is_named(ctx, good):
    bad = {c["name"]: IC.block(c["payload"]) for c in IC.invalid_cases()}
    a, b = bad["bad-crc"], bad["bad-before-start"]
    _refused(ctx, good[0] + a + good[0] + b, cdefs.ERR_INVALID_DATA, f"corrupt BGZF block at offset {len(good[0])} (CRC32 mismatch)")
    _refused(ctx, good[0] + b + good[0] + a, cdefs.ERR_INVALID_DATA, f"corrupt BGZF block at offset {len(good[0])} (distance before the start")
    out, _ = lio.bgzf_inflate(ctx, good[0] + good[0])
    assert out.tobytes() == good[1] * 2


def test_sizing_capacity_and_bytes_that_are_no_block(ctx, good):
    comp = good[0] * 3 + P.EOF_BLOCK
    assert lio.bgzf_inflate(ctx, comp, size_only=True) == 3 * len(good[1])
    assert lio.bgzf_inflate(ctx, b"", size_only=True) == 0 and len(lio.bgzf_inflate(ctx, P.EOF_BLOCK)[0]) == 0
    with pytest.raises(LocityperError) as err:
        lio.bgzf_inflate(ctx, comp, out=np.zeros(3 * len(good[1]) - 1, dtype=np.uint8))
    assert err.value.code == cdefs.ERR_INVALID_INPUT
    out, _ = lio.bgzf_inflate(ctx, comp, out=np.zeros(3 * len(good[1]) + 5, dtype=np.uint8))
    assert out.tobytes() == good[1] * 3
    _refused(ctx, good[0] + b"\x1f\x8b\x08\x00 not BGZF" * 4, cdefs.ERR_INVALID_DATA, f"not a BGZF block at offset {len(good[0])}")
    _refused(ctx, good[0] + good[0][:-3], cdefs.ERR_INVALID_DATA, f"not a BGZF block at offset {len(good[0])}")


def test_a_block_with_a_file_name_takes_the_host_route(ctx, good):
    data = IC._payload("acgt")[:3000]
    named = IC.block(IC._deflate(data, 6) + IC.trailer(data), flg=12, name=b"reads.bam")
    assert zlib.decompress(named, 31) == data
    out, st = lio.bgzf_inflate(ctx, good[0] + named + good[0])
    assert out.tobytes() == good[1] + data + good[1]
    assert st["ms_kernel"] == 0 and st["n_blocks"] == 3
    bad = bytearray(named)
    bad[len(bad) // 2] ^= 0x55
    _refused(ctx, good[0] + bytes(bad), cdefs.ERR_INVALID_DATA, "corrupt BGZF block")
