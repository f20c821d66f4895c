"""Host side of the locus-database build (`locityper target`): the writers of kmers.bin / distances.bin / haplotypes.fa, discard_identical
and the error statuses, against tests/pyref_db.py. Byte equality throughout; no device."""
import ctypes as C

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs, io
from tests import pyref_db as R


def _concat(arrs, dtype):
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrs])
    flat = np.concatenate([np.asarray(a, dtype=dtype) for a in arrs]) if len(arrs) and off[-1] else np.zeros(0, dtype=dtype)
    return flat, off


def _seqs(strs):
    return _concat([np.frombuffer(s.encode() if isinstance(s, str) else s, dtype=np.uint8) for s in strs], np.uint8)


def _parse_block(data):
    """The FIRST block of `data` through lcty_kmer_counts_parse: (k, [counts per contig], bytes consumed)."""
    k, off, counts, used = api.parse_kmer_counts(data)
    return k, [counts[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)], used


@pytest.mark.parametrize("counter_bytes", [1, 2])
def test_kmer_counts_write_equals_reference_and_parses_back(counter_bytes):
    rng = np.random.default_rng(3 + counter_bytes)
    maxv = R.max_value(counter_bytes)
    blocks = []
    for _ in range(2):
        arrs = [rng.integers(0, maxv + 1, n).astype(np.uint16) for n in (0, 1, 300, 77)]
        arrs[2][:3] = [maxv, 0, 128]                       # the maximum, zero, the first two-byte varint
        blocks.append(arrs)
    data = b""
    for arrs in blocks:
        flat, off = _concat(arrs, np.uint16)
        b = io.kmer_counts_write(25, counter_bytes, off, flat)
        assert b == R.kmer_counts_save(25, counter_bytes, arrs)
        data += b
    k, got, used = _parse_block(data)
    assert k == 25 and len(got) == 4 and all(np.array_equal(g, a) for g, a in zip(got, blocks[0]))
    k2, got2, used2 = _parse_block(data[used:])            # the second block through `consumed`
    assert k2 == 25 and all(np.array_equal(g, a) for g, a in zip(got2, blocks[1])) and used + used2 == len(data)


def test_kmer_counts_write_refuses_a_count_above_the_counters_maximum():
    with pytest.raises(_lib.LocityperError) as e:
        io.kmer_counts_write(25, 1, [0, 3], [1, 256, 2])
    assert e.value.code == cdefs.ERR_INVALID_DATA and "256" in str(e.value)
    assert io.kmer_counts_write(25, 2, [0, 3], [1, 256, 2]) == R.kmer_counts_save(25, 2, [[1, 256, 2]])


def test_distances_write_equals_reference_and_parses_back():
    rng = np.random.default_rng(5)
    for n in (2, 3, 17):
        uniq = rng.integers(0, 70000, n * (n - 1) // 2).astype(np.uint32)
        uniq[0] = 0
        uniq[-1] = 2 ** 32 - 2
        b = io.distances_write(15, 10, n, uniq)
        assert b == R.write_divergences(15, 10, n, uniq)
        k, w, dist = io.distances_parse(b, n)
        want = np.full((n, n), cdefs.NONE_U32, dtype=np.uint32)
        for (i, j), d in zip(R.triangle_indices(n), uniq):
            want[i, j] = want[j, i] = d
        assert (k, w) == (15, 10) and np.array_equal(dist, want)


DUP_CASES = {
    "first": (["a", "b", "c", "d"], ["ACGT", "TTTT", "ACGT", "GG"]),
    "middle": (["a", "b", "c", "d"], ["ACGT", "TTTT", "GG", "TTTT"]),
    "last": (["a", "b", "c", "d"], ["GG", "ACGT", "TTTT", "TTTT"]),
    "triple": (["h1", "h2", "h3", "h4", "h5", "h6"], ["ACGTA", "CC", "ACGTA", "CC", "ACGTA", "ACGTT"]),
    "none": (["a", "b", "c"], ["ACGT", "ACGA", "ACG"]),
    "long": (["x", "y", "z"], ["ACGT" * 5000, "ACGT" * 4999 + "ACGA", "ACGT" * 5000]),
}


@pytest.mark.parametrize("case", sorted(DUP_CASES))
def test_discard_identical_equals_reference(case):
    names, strs = DUP_CASES[case]
    seqs, off = _seqs(strs)
    kept, folded, text = api.db_discard_identical(names, seqs, off)
    rkept, rtext = R.discard_identical(names, [s.encode() for s in strs])
    assert list(kept) == rkept and text == rtext
    assert (text == b"") == (case == "none")
    for i in rkept:
        assert folded[i] == [names[j] for j in range(len(strs)) if j != i and strs[j] == strs[i] and j > i]


def test_discard_identical_text_of_the_triple():
    names, strs = DUP_CASES["triple"]
    seqs, off = _seqs(strs)
    assert api.db_discard_identical(names, seqs, off)[2] == b"h1 = h3, h5\nh2 = h4\n"


def test_fasta_text_equals_reference_and_reads_back(tmp_path):
    rng = np.random.default_rng(9)
    strs = ["".join(rng.choice(list("ACGT"), n)) for n in (1, 119, 120, 121, 240, 1000)] + [""]
    names = [f"hap{i}" for i in range(len(strs))]
    seqs, off = _seqs(strs)
    text = io.fasta_text(names, seqs, off)
    assert text == R.multiline_fasta(names, [s.encode() for s in strs])
    path = tmp_path / "haplotypes.fa.gz"
    io.write_gz(path, text)
    n2, s2, o2 = io.fasta_read(path)
    assert n2 == names and np.array_equal(s2, seqs) and np.array_equal(o2, off)


def _raises(code, fn):
    with pytest.raises(_lib.LocityperError) as e:
        fn()
    assert e.value.code == code
    assert _lib.lib().lcty_last_error() != b""


def test_error_statuses_of_the_host_entries():
    L = _lib.lib()
    need = C.c_uint64()
    off2 = np.array([0, 2], dtype=np.uint64)
    two = np.array([1, 2], dtype=np.uint16)
    _raises(cdefs.ERR_INVALID_INPUT, lambda: io.kmer_counts_write(25, 0, off2, two))                # counter length
    _raises(cdefs.ERR_INVALID_INPUT, lambda: io.kmer_counts_write(25, 9, off2, two))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: io.kmer_counts_write(256, 2, off2, two))               # k in one byte
    _raises(cdefs.ERR_INVALID_INPUT, lambda: io.kmer_counts_write(25, 2, [2, 0], two))              # offsets descend
    _raises(cdefs.ERR_INVALID_DATA, lambda: io.kmer_counts_write(25, 1, off2, [1, 300]))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_kmer_counts_write(25, 2, 1, off2.ctypes.data, two.ctypes.data, None, 0, None)))
    small = np.zeros(2, dtype=np.uint8)
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_kmer_counts_write(25, 2, 1, off2.ctypes.data, two.ctypes.data, small.ctypes.data, 2,
                                                                                 C.byref(need))))   # buffer too small
    _raises(cdefs.ERR_INVALID_INPUT, lambda: io.distances_write(300, 15, 2, [1]))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_distances_write(15, 15, 3, None, None, 0, C.byref(need))))
    seqs, off = _seqs(["ACGT", "ACGA"])
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_fasta_write_text(2, None, seqs.ctypes.data, off.ctypes.data, None, 0, C.byref(need))))
    bad_off = np.array([0, 4, 2], dtype=np.uint64)
    _raises(cdefs.ERR_INVALID_INPUT, lambda: io.fasta_text(["a", "b"], seqs, bad_off))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: api.db_discard_identical(["a", "b"], seqs, bad_off))
    nk = C.c_uint32()
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_db_discard_identical(2, seqs.ctypes.data, off.ctypes.data, None, None, C.byref(nk), None, None,
                                                                                    0, C.byref(need))))
    # the device entries refuse a missing context before anything else
    moff = np.zeros(3, dtype=np.uint64)
    h = C.c_void_p()
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_db_minimizers(None, 2, seqs.ctypes.data, off.ctypes.data, 15, 15, moff.ctypes.data, C.byref(h), None)))
    u = np.zeros(1, dtype=np.uint32)
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_db_divergences(None, 2, seqs.ctypes.data, off.ctypes.data, 15, 15, u.ctypes.data, None, None, None)))
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_db_off_target(None, 2, seqs.ctypes.data, off.ctypes.data, None, None, 25, 2, None, 0, None, 0,
                                                                             None, None, None)))
    p = api.db_params()
    f = cdefs.DbFiles()
    _raises(cdefs.ERR_INVALID_INPUT, lambda: _lib.check(L.lcty_db_build_locus(None, 2, b"a\0b\0", seqs.ctypes.data, off.ctypes.data, None, 0, None, None, 25, 2,
                                                                              C.byref(p), C.byref(f))))


def test_db_params_default():
    p = api.db_params()
    assert (p.div_k, p.div_w, p.calc_div, p.only_seqs) == (15, 15, 0, 0)       # add.rs:76-78
    assert api.db_params(calc_div=1, div_w=10).div_w == 10
