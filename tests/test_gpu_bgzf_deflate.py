"""lcty_bgzf_deflate on the device over the corpus of tests/deflate_cases.py: what any inflater and the project's own make of the whole
corpus in one call, the block offsets, the statistics; every case's stream against the host build of the same text (scripts/
deflate_probe_host.cpp), byte for byte; tiny inputs and the grid stride; the slice seam; capacity and arguments, and the context after
each refusal."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from locityper_amd._lib import LocityperError, lib
from tests import deflate_cases as DC
from tests import pyref_sample_bam as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_IN = DC.MAX_IN


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("deflate_probe") / "libdeflate_probe_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "locityper_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "deflate_probe_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.deflate_probe_block.restype = C.c_uint32
    L.deflate_probe_block.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


def blocks_of(out):
    """[(offset, size)] of the BGZF blocks of a file's bytes, each checked to start with the header the host writer gives"""
    res, at = [], 0
    while at < len(out):
        assert out[at:at + 16] == b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00", at
        size = struct.unpack_from("<H", out, at + 16)[0] + 1
        res.append((at, size))
        at += size
    assert at == len(out)
    return res


def _refused(call, *words):
    with pytest.raises(LocityperError) as err:
        call()
    assert err.value.code == cdefs.ERR_INVALID_INPUT, str(err.value)
    for w in words:
        assert w in str(err.value), str(err.value)


def test_the_whole_corpus_in_one_call(ctx):
    data = b"".join(d for _, d in DC.cases())
    out, off, st = lio.bgzf_deflate(ctx, data)
    raw = out.tobytes()
    assert gzip.decompress(raw) == data
    assert raw.endswith(P.EOF_BLOCK)
    n_blocks = (len(data) + MAX_IN - 1) // MAX_IN
    assert len(off) == n_blocks + 1 and (np.diff(off.astype(np.int64)) > 0).all() and off[0] == 0
    blocks = blocks_of(raw)
    assert [b[0] for b in blocks] == off.tolist() and blocks[-1][1] == 28     # every offset a header whose BSIZE reaches the next; the marker last
    for i, (at, size) in enumerate(blocks[:-1]):
        want = data[i * MAX_IN:(i + 1) * MAX_IN]
        assert struct.unpack_from("<I", raw, at + size - 4)[0] == len(want)
    back, _ = lio.bgzf_inflate(ctx, raw)
    assert back.tobytes() == data
    assert st["n_blocks"] == n_blocks and st["bytes_in"] == len(data) and st["bytes_out"] == len(raw)
    assert st["n_stored"] + st["n_fixed"] + st["n_dynamic"] == n_blocks and st["n_dynamic"] > 0 and st["ms_kernel"] > 0
    again, off2, _ = lio.bgzf_deflate(ctx, data)
    assert np.array_equal(out, again) and np.array_equal(off, off2)


def test_the_device_emits_the_bytes_of_the_host_build(ctx, host):
    forms = set()
    for name, data in DC.cases():
        buf = C.create_string_buffer(len(data) + 5)
        form = C.c_uint32(9)
        n = host.deflate_probe_block(data, len(data), buf, len(data) + 5, C.byref(form))
        out, off, st = lio.bgzf_deflate(ctx, data, with_eof=False)
        raw = out.tobytes()
        if not data:
            assert raw == b"" and off.tolist() == [0], name
            continue
        assert len(raw) == 18 + n + 8 and raw[18:18 + n] == buf.raw[:n], name
        assert raw[18 + n:] == DC.trailer(data), name
        assert (st["n_stored"], st["n_fixed"], st["n_dynamic"]) == tuple(int(form.value == k) for k in range(3)), name
        forms.add(form.value)
    assert forms == {0, 1, 2}


def test_tiny_inputs_and_the_grid_stride(ctx):
    rng = np.random.default_rng(4)
    src = DC.payload("bam")
    for k in range(3000):
        n = int(rng.integers(0, 48))
        at = int(rng.integers(0, len(src) - 64))
        data = src[at:at + n]
        out, off, st = lio.bgzf_deflate(ctx, data, with_eof=bool(k & 1))
        raw = out.tobytes()
        assert gzip.decompress(raw) == data if raw else (n == 0 and not k & 1), k
        assert len(raw) <= int(lib().lcty_bgzf_deflate_bound(n, k & 1)) and st["n_blocks"] == (1 if n else 0)
    data = (DC.payload("acgt") + DC.payload("bam") + DC.payload("run") + DC.payload("random"))[:3 * MAX_IN + 1]
    out, off, st = lio.bgzf_deflate(ctx, data)
    assert st["n_blocks"] == 4 and gzip.decompress(out.tobytes()) == data
    assert int(off[4]) - int(off[3]) == 18 + 3 + 8                            # one byte: a fixed block of 3 bytes


def test_more_blocks_than_workgroups_in_flight(ctx):
    """1 700 blocks (the grid is at most six workgroups per compute unit, 1 536 on 256): a workgroup takes a second block with the state the
    first left behind. The input repeats every four blocks, so the sizes must too."""
    unit = DC.payload("bam") + DC.payload("acgt") + DC.payload("random") + DC.payload("run", MAX_IN)
    assert len(unit) == 4 * MAX_IN
    data = np.tile(np.frombuffer(unit, dtype=np.uint8), 425)
    out, off, st = lio.bgzf_deflate(ctx, data)
    sizes = np.diff(off.astype(np.int64))
    assert st["n_blocks"] == 1700 and len(sizes) == 1700 and (sizes.reshape(425, 4) == sizes[:4]).all()
    first, _, _ = lio.bgzf_deflate(ctx, unit, with_eof=False)
    assert np.array_equal(out[:len(first)], first) and np.array_equal(out[int(off[1696]):int(off[1700])], first)
    back, _ = lio.bgzf_inflate(ctx, out)
    assert np.array_equal(back, data)


def test_the_slice_seam_changes_no_byte(ctx):
    data = (DC.payload("bam") + DC.payload("acgt") + DC.payload("random") + DC.payload("run") + DC.payload("bam"))[:4 * MAX_IN + 777]
    want, off, _ = lio.bgzf_deflate(ctx, data)
    assert len(off) == 6
    try:
        for knob in (MAX_IN, 2 * MAX_IN):
            ctx.set_knob("bgzf_deflate_max_bytes", knob)
            out, off2, st = lio.bgzf_deflate(ctx, data)
            assert np.array_equal(out, want) and np.array_equal(off, off2) and st["n_blocks"] == 5, knob
        ctx.set_knob("bgzf_deflate_max_bytes", MAX_IN - 1)
        _refused(lambda: lio.bgzf_deflate(ctx, data), "bgzf_deflate_max_bytes")
    finally:
        ctx.set_knob("bgzf_deflate_max_bytes", -1)
    out, _, _ = lio.bgzf_deflate(ctx, data)
    assert np.array_equal(out, want)


def test_capacity_and_arguments(ctx):
    data = DC.payload("bam", 70_000)
    bound = int(lib().lcty_bgzf_deflate_bound(len(data), 1))
    assert bound == len(data) + 31 * 2 + 28 and int(lib().lcty_bgzf_deflate_bound(len(data), 0)) == bound - 28
    assert int(lib().lcty_bgzf_deflate_bound(0, 1)) == 28 and int(lib().lcty_bgzf_deflate_bound(MAX_IN, 0)) == MAX_IN + 31
    _refused(lambda: lio.bgzf_deflate(ctx, data, out_cap=bound - 1), str(bound))
    out, _, _ = lio.bgzf_deflate(ctx, data, out_cap=bound)
    assert gzip.decompress(out.tobytes()) == data
    n = C.c_uint64(0)
    buf = np.frombuffer(data, dtype=np.uint8)
    room = np.empty(bound, dtype=np.uint8)
    L = lib()
    assert L.lcty_bgzf_deflate(None, buf.ctypes.data, len(buf), 1, room.ctypes.data, bound, C.byref(n), None, None) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_bgzf_deflate(ctx._h, None, len(buf), 1, room.ctypes.data, bound, C.byref(n), None, None) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_bgzf_deflate(ctx._h, buf.ctypes.data, len(buf), 1, None, bound, C.byref(n), None, None) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_bgzf_deflate(ctx._h, buf.ctypes.data, len(buf), 1, room.ctypes.data, bound, None, None, None) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_bgzf_deflate(ctx._h, buf.ctypes.data, len(buf), 1, room.ctypes.data, bound, C.byref(n), None, None) == 0   # block_off and stats may be null
    assert room[:n.value].tobytes() == out.tobytes()
    out, off, st = lio.bgzf_deflate(ctx, b"")
    assert out.tobytes() == P.EOF_BLOCK and off.tolist() == [0] and st["n_blocks"] == 0 and st["bytes_out"] == 28
    out, off, st = lio.bgzf_deflate(ctx, b"", with_eof=False)
    assert len(out) == 0 and off.tolist() == [0] and st["bytes_out"] == 0
