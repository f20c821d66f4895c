"""The corpus of the BGZF inflate tests (locityper_amd/csrc/lcty_inflate.hpp, lcty_bgzf_inflate): every case is one BGZF block of at
most 65 536 bytes, and the oracle is Python's zlib. A case is a dict: name, payload (the bytes behind the 18-byte BGZF header: deflate
stream and trailer), isize (what sizes the output: the last four bytes of the block), out (the inflated bytes, None = zlib refuses), end
(offset in payload of the first byte behind the deflate stream, when accepted), raw (mutations only: judged without the trailer).
  valid_cases()    zlib-made streams (levels 0, 1, 6, 9; Z_FIXED, Z_RLE, Z_HUFFMAN_ONLY; memLevel 1) and hand-assembled ones
  invalid_cases()  one per class of error of the decoder
  mutated_cases()  2 000 seeded byte flips, bit flips and truncations of the valid ones"""
import functools
import struct
import zlib

import numpy as np

from tests import pyref_sample_bam as P
from tests import sample_bam_cases as S

LENGTHS = [0, 1, 2, 63, 64, 65, 257, 258, 259, 32_767, 32_768, 32_769, 65_279, 0xff00, 65_536]
GZIP_HEAD = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"


def block(payload, flg=4, name=b""):
    """the BGZF block of a payload; flg 12 puts `name` (FNAME, 0-terminated) behind the extra field"""
    extra = name + b"\0" if flg & 8 else b""
    total = 18 + len(extra) + len(payload)
    assert total <= 65_536, total
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, flg, 0, 0, 255, 6, 66, 67, 2, total - 1) + extra + payload


def zlib_verdict(payload, isize, raw=False):
    """(out, end) when zlib takes the payload as a gzip member (raw: as a raw deflate stream) that inflates to exactly isize bytes, else None"""
    d = zlib.decompressobj(-15 if raw else 31)
    try:
        out = d.decompress(payload if raw else GZIP_HEAD + payload, isize + 1)
    except zlib.error:
        return None
    if not d.eof or len(out) != isize:
        return None
    return out, len(payload) - len(d.unused_data) - (0 if raw else 8)


def trailer(data):
    return struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def _case(name, stream, data, isize=None, tail=None):
    payload = stream + (trailer(data) if tail is None else tail)
    isize = len(data) if isize is None else isize
    v = zlib_verdict(payload, isize)
    return dict(name=name, payload=payload, isize=isize, out=None if v is None else v[0], end=None if v is None else v[1])


# ---- payloads ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _payload(kind):
    rng = np.random.default_rng(17)
    if kind == "acgt":
        unit = bytes(rng.choice(list(b"ACGT"), 9000).astype(np.uint8))
        return (unit * 8)[:65_536]                                            # repeats 9 000 bytes back: long distances
    if kind == "run":
        return b"G" * 65_536
    if kind == "random":
        return bytes(rng.integers(0, 256, 0xff00, dtype=np.uint8))
    recs = S.seeded_records()
    data = b"".join(P.record_bytes(r) for r in recs)
    assert len(data) >= 65_536
    return data[:65_536]


def _deflate(data, level, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


def zlib_made():
    cases = []
    plans = []
    for kind in ("acgt", "run", "random", "bam"):
        for n in LENGTHS:
            plans.append((kind, n, 6, 8, zlib.Z_DEFAULT_STRATEGY))
    few = [0, 1, 258, 32_768, 0xff00]
    for level in (0, 1, 9):
        for kind in ("acgt", "random", "bam"):
            for n in few:
                plans.append((kind, n, level, 8, zlib.Z_DEFAULT_STRATEGY))
    for strategy in (zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY):
        for kind in ("acgt", "run", "bam"):
            for n in (1, 259, 32_769, 0xff00):
                plans.append((kind, n, 6, 8, strategy))
    for kind in ("acgt", "bam"):
        for n in (32_768, 0xff00, 65_536):
            plans.append((kind, n, 6, 1, zlib.Z_DEFAULT_STRATEGY))
    for kind, n, level, mem, strategy in plans:
        src = _payload(kind)
        if n > len(src):
            continue                                                          # 65 536 random bytes do not fit a block
        data = src[:n]
        stream = _deflate(data, level, mem, strategy)
        if 18 + len(stream) + 8 > 65_536:
            assert level == 0 or strategy != zlib.Z_DEFAULT_STRATEGY, (kind, n, level)
            continue
        c = _case(f"zlib-{kind}-{n}-l{level}-m{mem}-s{strategy}", stream, data)
        assert c["out"] == data and c["end"] == len(stream)
        cases.append(c)
    # the forms the list must hold
    firsts = {(c["name"].split("-")[3], (c["payload"][0] >> 1) & 3) for c in cases}
    assert ("l0", 0) in firsts and ("l6", 2) in firsts and ("l6", 1) in firsts
    several = [c for c in cases if "-m1-" in c["name"]]
    assert several and all(c["payload"][0] & 1 == 0 for c in several)         # memLevel 1: the first deflate block is not the last
    return cases


# ---- hand-assembled streams ------------------------------------------------------------------------------------------------------------

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical(lengths):
    """{symbol: (code, length)} of RFC 1951 3.2.2"""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, ls in enumerate(lengths):
            if ls == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = {s: (s, 5) for s in range(32)}


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):                                                 # least significant bit first
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, pair):                                                     # a Huffman code: most significant bit first
        c, n = pair
        self.bits(int(format(c, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


class Coder:
    """symbols of one block under a literal/length and a distance code, and what they inflate to"""

    def __init__(self, w, lit, dist, data):
        self.w, self.lit, self.dist, self.data = w, lit, dist, data

    def literal(self, b):
        self.w.code(self.lit[b])
        self.data.append(b)

    def match(self, length, distance, check=True):
        ls = max(i for i in range(29) if LEN_BASE[i] <= length)
        self.w.code(self.lit[257 + ls])
        self.w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(i for i in range(30) if DIST_BASE[i] <= distance)
        self.w.code(self.dist[ds])
        self.w.bits(distance - DIST_BASE[ds], DIST_EXTRA[ds])
        if check:
            for _ in range(length):
                self.data.append(self.data[-distance])

    def end(self):
        self.w.code(self.lit[256])


def fixed_block(w, data, final=1):
    w.bits(final, 1)
    w.bits(1, 2)
    return Coder(w, FIXED_LIT, FIXED_DIST, data)


CL_PLAIN = [4] * 16 + [0, 0, 0]                                               # lengths 0 .. 15 written as they are
CL_REPEATS = [4] * 14 + [5, 0, 5, 5, 5]                                       # 0 .. 13, and 14, 16, 17, 18 with five bits


def dynamic_header(w, lit_lens, dist_lens, final=1, cl_lens=CL_PLAIN, symbols=None, hlit=None):
    """BTYPE 2 and its code lengths; symbols: the code-length symbols [(symbol, extra value)] when they are not lit_lens + dist_lens as they are"""
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits((len(lit_lens) if hlit is None else hlit) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    if symbols is None:
        symbols = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    for s, extra in symbols:
        w.code(cl[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])


def _lit_lens(assign, n=257):
    lens = [0] * n
    for s, l in assign.items():
        lens[s] = l
    return lens


def hand_made():
    rng = np.random.default_rng(5)
    cases = []

    def close(name, w, data):
        stream = w.done()
        assert zlib.decompress(stream, -15) == bytes(data), name
        c = _case("hand-" + name, stream, bytes(data))
        assert c["out"] == bytes(data), name
        cases.append(c)

    # length 258 at distance 32 768, the farthest one: zlib's compressor stops at 32 506
    w, data = BitWriter(), bytearray()
    c = fixed_block(w, data)
    for b in rng.choice(list(b"ACGT"), 32_768).tolist():
        c.literal(b)
    c.match(258, 32_768)
    c.match(258, 32_768)
    c.match(3, 32_768 - 100)
    c.end()
    close("far", w, data)
    # length 258 at distance 1; length 5 at distance 2
    w, data = BitWriter(), bytearray()
    c = fixed_block(w, data)
    c.literal(65); c.match(258, 1); c.end()
    close("run", w, data)
    w, data = BitWriter(), bytearray()
    c = fixed_block(w, data)
    c.literal(65); c.literal(66); c.match(5, 2); c.end()
    close("overlap", w, data)
    # every length once, at distances around it (shorter: the copy wraps; longer: it does not), over two blocks, the first not final
    w, data = BitWriter(), bytearray()
    c = fixed_block(w, data, final=0)
    for b in rng.integers(0, 256, 300).tolist():
        c.literal(b)
    for length in range(3, 131):
        c.match(length, [1, 2, 3, length - 1, length, length + 1, 64, 65, 299][length % 9] or 1)
    c.end()
    c = fixed_block(w, data)
    for length in range(131, 259):
        c.match(length, [1, 2, 63, length - 1, length, length + 1, 64, 65, 300][length % 9])
    c.end()
    close("all-lengths", w, data)
    # a dynamic block whose only distance code has one bit (an incomplete set that is legal)
    w, data = BitWriter(), bytearray()
    lit = _lit_lens({65: 1, 256: 2, 257: 2}, 258)
    dynamic_header(w, lit, [1])
    c = Coder(w, canonical(lit), canonical([1]), data)
    c.literal(65); c.literal(65); c.match(3, 1); c.literal(65); c.end()
    close("one-distance", w, data)
    # a dynamic block without any distance code, literals only
    w, data = BitWriter(), bytearray()
    lit = _lit_lens({65: 1, 66: 2, 256: 2})
    dynamic_header(w, lit, [0])
    c = Coder(w, canonical(lit), {}, data)
    for b in b"ABBABAAB":
        c.literal(b)
    c.end()
    close("no-distance", w, data)
    # lengths written with the repeat codes 16, 17, 18; a stored block of no bytes between two others
    w, data = BitWriter(), bytearray()
    lit = _lit_lens({65: 3, 66: 3, 67: 3, 68: 3, 256: 1})
    symbols = [(18, 65 - 11), (3, 0), (16, 3 - 3), (18, 138 - 11), (18, 39 - 11), (17, 10 - 3), (1, 0), (0, 0)]
    assert 65 + 1 + 3 + 138 + 39 + 10 + 1 + 1 == 258
    dynamic_header(w, lit, [0], final=0, cl_lens=CL_REPEATS, symbols=symbols)
    c = Coder(w, canonical(lit), {}, data)
    for b in b"ABCDDCBA":
        c.literal(b)
    c.end()
    w.bits(0, 1); w.bits(0, 2); w.align(); w.bits(0, 16); w.bits(0xFFFF, 16)
    w.bits(1, 1); w.bits(0, 2); w.align(); w.bits(3, 16); w.bits(0xFFFC, 16)
    for b in b"xyz":
        w.bits(b, 8); data.append(b)
    close("repeats-and-stored", w, data)
    # a trailer that is not at the block's end: zlib reads it behind the stream and leaves the rest
    stream = _deflate(b"trailing bytes behind the trailer", 6)
    data = b"trailing bytes behind the trailer"
    c = _case("hand-trailing", stream, data, tail=trailer(data) + b"\0\0\0\0" + struct.pack("<I", len(data)))
    assert c["out"] == data
    cases.append(c)
    return cases


@functools.lru_cache(maxsize=None)
def valid_cases():
    cases = zlib_made() + hand_made()
    assert all(c["out"] is not None for c in cases)
    return cases


# ---- invalid streams -------------------------------------------------------------------------------------------------------------------

def _raw_refused(stream):
    try:
        d = zlib.decompressobj(-15)
        d.decompress(stream)
        return not d.eof
    except zlib.error:
        return True


@functools.lru_cache(maxsize=None)
def invalid_cases():
    cases = []

    def raw(name, w_or_stream, isize=16):
        stream = w_or_stream if isinstance(w_or_stream, bytes) else w_or_stream.done()
        assert _raw_refused(stream), name
        c = _case("bad-" + name, stream, b"", isize=isize, tail=struct.pack("<II", 0, isize))
        assert c["out"] is None, name
        cases.append(c)

    def member(name, stream, data, isize, tail):
        c = _case("bad-" + name, stream, data, isize=isize, tail=tail)
        assert c["out"] is None, name
        try:
            d = zlib.decompressobj(31)
            d.decompress(GZIP_HEAD + c["payload"])
            assert not d.eof, name
        except zlib.error:
            pass
        cases.append(c)

    w = BitWriter(); c = fixed_block(w, bytearray()); c.literal(65); c.match(3, 2, check=False); c.end()
    raw("before-start", w)
    w = BitWriter(); c = fixed_block(w, bytearray()); c.literal(65); w.code(FIXED_LIT[257]); w.code((30, 5)); c.end()
    raw("distance-30", w)
    w = BitWriter(); c = fixed_block(w, bytearray()); c.literal(65); w.code(FIXED_LIT[286]); c.end()
    raw("literal-286", w)
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2); w.bits(0, 29)
    raw("btype-3", w)
    w = BitWriter(); w.bits(1, 1); w.bits(0, 2); w.align(); w.bits(4, 16); w.bits(0xFFFA, 16); w.bits(0x64636261, 32)
    raw("stored-nlen", w)
    for name, assign in (("over-subscribed", {65: 1, 66: 1, 256: 1}), ("incomplete", {65: 1, 256: 2}), ("no-end-of-block", {65: 1, 66: 1})):
        w = BitWriter(); lit = _lit_lens(assign); dynamic_header(w, lit, [0]); w.bits(0, 32)
        raw(name, w)
    w = BitWriter(); dynamic_header(w, [0] * 257, [0], cl_lens=CL_REPEATS, symbols=[(16, 0), (1, 0)]); w.bits(0, 32)
    raw("repeat-without-previous", w)
    w = BitWriter(); dynamic_header(w, [0] * 257, [0], cl_lens=CL_REPEATS, symbols=[(18, 127), (18, 127)]); w.bits(0, 32)
    raw("repeat-past-the-end", w)
    w = BitWriter(); dynamic_header(w, [0] * 257, [0], hlit=287, symbols=[]); w.bits(0, 64)
    raw("hlit-287", w)
    w = BitWriter(); dynamic_header(w, _lit_lens({65: 1, 256: 1}), [0], cl_lens=[0] * 16 + [1, 0, 0], symbols=[]); w.bits(0, 64)
    raw("code-length-code-incomplete", w)
    data = _payload("bam")[:5000]
    stream = _deflate(data, 6)
    member("one-over-isize", stream, data, len(data) - 1, struct.pack("<II", zlib.crc32(data), len(data) - 1))
    member("one-under-isize", stream, data, len(data) + 1, struct.pack("<II", zlib.crc32(data), len(data) + 1))
    member("truncated", stream[:len(stream) // 2], data, len(data), trailer(data))
    member("truncated-no-trailer", stream, data, len(data), b"")
    stored = bytearray(_deflate(_payload("random")[:1000], 0))
    stored[5 + 400] ^= 0x10
    member("crc", bytes(stored), _payload("random")[:1000], 1000, trailer(_payload("random")[:1000]))
    member("trailer-isize", stream, data, len(data), struct.pack("<III", zlib.crc32(data), len(data) + 7, len(data)))
    return cases


# ---- seeded mutations ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mutated_cases(n=2000, seed=99):
    rng = np.random.default_rng(seed)
    valid = [c for c in valid_cases() if len(c["payload"]) > 8]
    small = [c for c in valid if len(c["payload"]) <= 8192]
    cases = []
    for k in range(n):
        pool = small if k % 4 else valid
        base = pool[int(rng.integers(len(pool)))]
        p = bytearray(base["payload"])
        kind = k % 3
        for _ in range(int(rng.integers(1, 4)) if kind < 2 else 1):
            # early bytes hold the block headers and code lengths: half of the changes go there
            at = int(rng.integers(min(len(p), 96))) if rng.random() < 0.5 else int(rng.integers(len(p)))
            if kind == 0:
                p[at] = int(rng.integers(256))
            elif kind == 1:
                p[at] ^= 1 << int(rng.integers(8))
            else:
                del p[int(rng.integers(len(p))):]
        raw = k % 2 == 1                                                      # every other one is judged as a stream without trailer
        v = zlib_verdict(bytes(p), base["isize"], raw)
        cases.append(dict(name=f"mut-{k}-{base['name']}", payload=bytes(p), isize=base["isize"], out=None if v is None else v[0],
                          end=None if v is None else v[1], raw=raw))
    assert sum(c["out"] is None for c in cases) > n // 2 and sum(c["out"] is not None for c in cases) > 10
    return cases


def write_corpus(path, cases):
    """the corpus as scripts/inflate_probe_host.cpp reads it"""
    with open(path, "wb") as f:
        for c in cases:
            ok = c["out"] is not None
            f.write(struct.pack("<IIII", len(c["payload"]), c["isize"], int(ok) | (2 if c.get("raw") else 0), c["end"] if ok else 0))
            f.write(c["payload"])
            if ok:
                f.write(c["out"])
