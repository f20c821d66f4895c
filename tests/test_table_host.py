"""The key table of locityper_amd/csrc/lcty_table.hpp compiled for the host (scripts/table_probe_host.cpp): claim and find under a
hash the test controls against a Python dict, on the shapes where linear probing goes wrong, and the sizing rule against the five
spellings it replaced."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDEF64 = (1 << 64) - 1
IDENTITY, CONSTANT = 0, 1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("table_probe") / "libtable_probe_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "locityper_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "table_probe_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.table_probe.restype = C.c_int
    L.table_probe.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.table_probe_set_home.argtypes = [C.c_uint64]
    L.table_probe_slots.restype = C.c_uint64
    L.table_probe_slots.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64]
    L.table_probe_slot_stride.restype = C.c_uint32
    return L


class Table:
    """`slots` keys at `stride` words, all free; what a Slot holds behind its key is a pattern nobody may touch"""

    def __init__(self, lib, slots, stride, free, policy, home=0):
        self.lib, self.slots, self.stride, self.free, self.policy, self.home = lib, slots, stride, free, policy, home
        self.words = np.full(slots * stride, 0xABCD_0000_1234_5678, dtype=np.uint64)
        self.words[::stride] = free
        self.where = {}                                                        # the dict: key -> slot

    def _call(self, take, key):
        self.lib.table_probe_set_home(self.home)
        slot = C.c_uint64(UNDEF64)
        found = self.lib.table_probe(take, self.policy, int(self.free == 0), self.stride, self.words.ctypes.data, self.slots - 1, key, C.byref(slot))
        return slot.value, bool(found)

    def claim(self, key):
        slot, found = self._call(1, key)
        assert found == (key in self.where)
        assert self.where.setdefault(key, slot) == slot
        self.check()
        return slot, found

    def find(self, key):
        return self._call(0, key)

    def check(self):
        keys = self.words[::self.stride]
        want = np.full(self.slots, self.free, dtype=np.uint64)
        for key, slot in self.where.items():
            want[slot] = key
        assert np.array_equal(keys, want)
        if self.stride > 1:
            assert (self.words.reshape(self.slots, self.stride)[:, 1:] == 0xABCD_0000_1234_5678).all()
        for key, slot in self.where.items():
            assert self.find(key) == (slot, True)


def _layouts(lib):
    return [(stride, free) for stride in (1, lib.table_probe_slot_stride()) for free in (UNDEF64, 0)]


def test_slot_stride_is_the_key_start_count_slot(lib):
    assert lib.table_probe_slot_stride() == 2                                  # {u64 key, u32 start, u32 count}


def test_a_chain_from_the_last_slot_wraps_to_slot_0(lib):
    for slots in (8, 16):
        for stride, free in _layouts(lib):
            t = Table(lib, slots, stride, free, IDENTITY)
            keys = [slots - 1 + slots * i for i in range(1, 5)]                 # home: the last slot, all of them
            assert [t.claim(k) for k in keys] == [(slots - 1, False), (0, False), (1, False), (2, False)]
            assert t.claim(slots * 3) == (3, False)                            # home 0, pushed on by the wrapped chain
            assert t.find(slots * 5) == (4, False)                             # absent, home 0: ends at the first free slot behind the chain
            assert t.find(slots * 9 - 1) == (4, False)                         # absent, home the last slot: wraps too
            assert t.find(slots + 5) == (5, False)                             # absent, its home is free


def test_every_key_homes_to_one_slot(lib):
    for slots in (8, 16):
        for home in (0, 5, slots - 1):
            for stride, free in _layouts(lib):
                t = Table(lib, slots, stride, free, CONSTANT, home)
                for i in range(slots - 1):
                    assert t.claim(1000 + i) == ((home + i) & (slots - 1), False)
                assert t.find(7) == ((home + slots - 1) & (slots - 1), False)


def test_one_free_slot_still_ends_a_find(lib):
    for slots in (8, 16):
        for stride, free in _layouts(lib):
            t = Table(lib, slots, stride, free, IDENTITY)
            for key in range(1, slots):                                        # every slot but slot 0
                assert t.claim(key) == (key, False)
            for absent in (slots + 1, 2 * slots - 1, 3 * slots + slots // 2):  # homes 1, the last slot, the middle: all end in slot 0
                assert t.find(absent) == (0, False)
            assert t.claim(2 * slots + 3) == (0, False)                        # and the claim of one takes it


def test_a_second_claim_returns_the_same_slot_and_was_there(lib):
    for stride, free in _layouts(lib):
        t = Table(lib, 8, stride, free, IDENTITY)
        assert t.claim(13) == (5, False) and t.claim(21) == (6, False)
        assert t.claim(13) == (5, True) and t.claim(21) == (6, True) and t.claim(13) == (5, True)
        assert len(t.where) == 2


@pytest.mark.parametrize("slots", [8, 16])
@pytest.mark.parametrize("policy", [IDENTITY, CONSTANT])
def test_random_keys_against_the_dict(lib, slots, policy):
    """claims in random order, repeats among them, up to one free slot; the expected slot is linear probing restated"""
    rng = np.random.default_rng(slots + policy)
    for stride, free in _layouts(lib):
        for trial in range(20):
            home = int(rng.integers(0, slots))
            t = Table(lib, slots, stride, free, policy, home)
            model = [free] * slots
            pool = [int(x) for x in rng.integers(1, 1 << 40, slots - 1)]
            for key in pool + [pool[int(i)] for i in rng.integers(0, len(pool), slots)]:
                slot = (key if policy == IDENTITY else home) & (slots - 1)
                while model[slot] not in (free, key):
                    slot = (slot + 1) & (slots - 1)
                was = model[slot] == key
                model[slot] = key
                assert t.claim(key) == (slot, was)
            assert len(t.where) == len(set(pool)) <= slots - 1
            for absent in (int(x) for x in rng.integers(1 << 41, 1 << 42, 8)):
                slot, found = t.find(absent)
                assert not found and model[slot] == free


# ---- the sizing rule against the spellings it replaced ----
def _next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def _from(floor, bound):
    cap = floor
    while cap < bound:
        cap <<= 1
    return cap


OLD = [
    # what the call site passes as (n_keys, load_shift, floor), and what it computed before
    ("k-mer set, first table", lambda n: (n, 1, 1024), lambda n: _next_pow2(max(2 * n, 1024))),
    ("k-mer set", lambda n: (n, 2, 1024), lambda n: _next_pow2(max(4 * n, 1024))),
    ("genome table", lambda n: (n, 1, 64), lambda n: _from(64, 2 * n)),
    ("database tables", lambda n: (n, 1, 1024), lambda n: _from(1024, 2 * max(n, 1))),
    ("map index", lambda n: (n, 1, 1024), lambda n: _from(1024, 2 * n)),
    ("recruitment and transfer: 2 n + 2", lambda n: (n + 1, 1, 64), lambda n: _from(64, 2 * n + 2)),
]


@pytest.mark.parametrize("name,args,old", OLD, ids=[o[0] for o in OLD])
def test_table_slots_equals_the_old_spellings(lib, name, args, old):
    floor = args(0)[2]
    for n in (0, 1, floor // 2 - 1, floor // 2, floor // 2 + 1, floor, 4096, 4097, (1 << 20) - 1, 1 << 20, 3_000_001):
        got = lib.table_probe_slots(*args(n))
        assert got == old(n), (name, n)
        assert got & (got - 1) == 0 and got > n                                # a power of two with a free slot
