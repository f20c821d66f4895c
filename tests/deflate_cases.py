"""The corpus of the BGZF deflate tests (locityper_amd/csrc/lcty_deflate.hpp, lcty_bgzf_deflate): every case is (name, bytes) with at
most 0xff00 bytes, the input of one BGZF block. The four payloads of tests/inflate_cases.py at the lengths where a rule of the format
or a path of the encoder changes, and designed blocks: the smallest inputs at which each rule of the encoder can go wrong."""
import functools
import struct

import numpy as np

from tests.inflate_cases import _payload, block, trailer  # noqa: F401  (block and trailer: for the tests that build a BGZF block)

MAX_IN = 0xff00
KINDS = ("acgt", "run", "random", "bam")
LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 260, 32_767, 32_768, 32_769, 65_279, MAX_IN]


def payload(kind, n=MAX_IN):
    return _payload(kind)[:n]


def fibonacci_block():
    """46 367 bytes: byte value k occurs fib(k) times for 22 values (1, 1, 2, 3, ..), seeded-shuffled: a Huffman tree deeper than 15"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, k, dtype=np.uint8) for k, f in enumerate(fib)])
    np.random.default_rng(5).shuffle(data)
    assert len(data) == 46_367
    return bytes(data)


@functools.lru_cache(maxsize=None)
def designed():
    rng = np.random.default_rng(29)
    far = bytes(rng.integers(0, 256, 32_768, dtype=np.uint8))
    too_far = bytes(rng.integers(0, 256, 32_769, dtype=np.uint8))
    return [
        ("farthest-distance", far + far[:MAX_IN - 32_768]),                   # a legal match 32 768 back
        ("one-too-far", too_far + too_far[:MAX_IN - 32_769]),                 # the only repeat is 32 769 back
        ("two-values", bytes(rng.choice([7, 201], 5000).astype(np.uint8))),
        ("run-then-other", b"T" * 999 + b"X"),                                # a match runs into the last byte
        ("run-300", b"A" * 300),                                              # 258 + 42
        ("run-remainder-1", b"C" * (1 + 258 * 3 + 1)),                        # a literal, three matches, 1 byte left
        ("run-remainder-2", b"C" * (1 + 258 * 3 + 2)),
        ("all-256-once", bytes(rng.permutation(256).astype(np.uint8))),       # no match: the distance set is empty
        ("fibonacci", fibonacci_block()),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    out = [(f"{kind}-{n}", payload(kind, n)) for kind in KINDS for n in LENGTHS]
    out += designed()
    assert all(len(d) <= MAX_IN for _, d in out)
    return out


def write_corpus(path):
    """the corpus as scripts/deflate_probe_host.cpp reads it: per case u32 n, n bytes"""
    with open(path, "wb") as f:
        for _, d in cases():
            f.write(struct.pack("<I", len(d)) + d)
    return len(cases())
