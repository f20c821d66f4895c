"""Genome k-mer counts without a device: the Python restatement (tests/pyref_kmer_count.py) against answers written out by hand, and
the argument checks of the C ABI that are made before a device is needed."""
import ctypes as C

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from tests import pyref_kmer_count as R


def _counts(contigs, seqs, k, cb=2):
    return [list(map(int, v)) for v in R.kmer_counts(contigs, seqs, k, cb)]


def test_twelve_bases_at_k3_every_count_written_out():
    # ACGTACGTTTAA: ACG x2 (= CGT rc) and CGT x2 -> 4; GTA x1 and TAC x1 (= rc GTA) -> 2; GTT 1 + AAC 0; TTT 1; TTA 1 (= TAA rc) + TAA 1 -> 2
    g = [("c", b"ACGTACGTTTAA")]
    want = [4, 4, 2, 2, 4, 4, 1, 1, 2, 2]
    assert _counts(g, [b"ACGTACGTTTAA"], 3) == [want]
    assert _counts(g, [b"AAC", b"AAA", b"CCC"], 3) == [[1], [1], [1]]            # GTT's reverse complement; TTT's; absent: the floor


def test_kmer_and_reverse_complement_count_together():
    g = [("c", b"AAGAACTT")]          # AAG, AGA, GAA, AAC, ACT, CTT; CTT = rc(AAG), so both count 2
    assert _counts(g, [b"AAG", b"CTT", b"AGA", b"TCT"], 3) == [[2], [2], [1], [1]]


def test_contig_junction_is_not_counted():
    g = [("a", b"AAC"), ("b", b"GGG")]
    # ACG and CGG would span the junction; GGG = CCC
    assert _counts(g, [b"AACGGG"], 3) == [[1, 1, 1, 1]]
    assert R.genome_table(g, 3) == {0b000001: 1, 0b010101: 1}                     # AAC, CCC (= rc GGG)
    assert _counts([("ab", b"AACGGG")], [b"AACGGG"], 3) == [[1, 1, 1, 1]]
    assert R.genome_table([("ab", b"AACGGG")], 3)[0b000110] == 1                  # ACG is there once the contigs are one


def test_lower_case_is_counted():
    assert R.genome_table([("c", b"acgTAcgt")], 3) == R.genome_table([("c", b"ACGTACGT")], 3)
    assert _counts([("c", b"acgtacgt")], [b"ACG"], 3) == [[4]]


def test_n_and_iupac_letters_split():
    for x in (b"N", b"R", b"n", b"y"):
        t = R.genome_table([("c", b"ACG" + x + b"ACG")], 3)
        assert t == {0b000110: 2}, x                                              # ACG twice, nothing across the letter
    assert R.genome_table([("c", b"ACNNAC")], 3) == {}
    with pytest.raises(R.GenomeByteError) as e:
        R.genome_table([("chrZ", b"ACG-ACG")], 3)
    assert (e.value.contig, e.value.pos, e.value.byte) == ("chrZ", 3, ord("-"))
    assert R.standardize(b"acgtNrX"[:6]) == b"ACGTNN"


def test_floor_and_clamps():
    g = [("a", b"A" * 70_000), ("t", b"C" * 300)]
    assert _counts(g, [b"AAA"], 3, 2) == [[65535]] and _counts(g, [b"AAA"], 3, 1) == [[255]] and _counts(g, [b"AAA"], 3, 4) == [[65535]]
    assert _counts(g, [b"GGG"], 3, 2) == [[298]] and _counts(g, [b"GGG"], 3, 1) == [[255]]
    assert _counts(g, [b"ACA", b"AC", b""], 3) == [[1], [], []]
    with pytest.raises(RuntimeError, match="Cannot count k-mers for sequence with Ns"):
        R.query({}, [b"ACNT"], 3)
    with pytest.raises(ValueError):
        R.query({}, [b"ACgT"], 3)


# ---- the C ABI, before any device ----
def _call(genome, k, cb, cnt_off=True):
    off = np.zeros(2, dtype=np.uint64)
    cnt = np.zeros(2, dtype=np.uint64)
    st = cdefs.GenomeCountStats()
    rc = _lib.lib().lcty_genome_kmer_counts(genome, k, cb, 1, None, off.ctypes.data, None, cnt.ctypes.data if cnt_off else None, C.byref(st))
    return rc, _lib.lib().lcty_last_error().decode()


def test_k_and_counter_checks_need_no_device():
    rc, msg = _call(None, 24, 2)
    assert rc == cdefs.ERR_INVALID_DATA and msg == "Jellyfish counts are calculated for an even k size (24), odd k is required"
    rc, msg = _call(None, 0, 2)
    assert rc == cdefs.ERR_INVALID_DATA and "even k size (0)" in msg
    rc, msg = _call(None, 33, 2)
    assert rc == cdefs.ERR_UNSUPPORTED and "k = 33" in msg and "k <= 31" in msg
    assert _call(None, 63, 2)[0] == cdefs.ERR_UNSUPPORTED
    assert _call(None, 65, 2)[0] == cdefs.ERR_INVALID_DATA
    for cb in (0, 9):
        rc, msg = _call(None, 25, cb)
        assert rc == cdefs.ERR_INVALID_INPUT and f"{cb}-byte counters" in msg
    rc, msg = _call(None, 25, 2)
    assert rc == cdefs.ERR_INVALID_INPUT and msg == "null argument"
    assert _call(None, 25, 2, cnt_off=False)[0] == cdefs.ERR_INVALID_INPUT


def test_null_handles_are_refused():
    L = _lib.lib()
    n, nb, ln = C.c_uint32(), C.c_uint64(), C.c_uint64()
    out = np.zeros(4, dtype=np.uint8)
    assert L.lcty_genome_append(None, b"c", out.ctypes.data, 4, 0) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_genome_info(None, C.byref(n), C.byref(nb)) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_genome_contig(None, 0, None, 0, C.byref(ln)) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_genome_fetch(None, b"c", 0, 1, out.ctypes.data) == cdefs.ERR_INVALID_INPUT
    assert L.lcty_genome_create(None, None) == cdefs.ERR_INVALID_INPUT
    h = C.c_void_p()
    assert L.lcty_genome_load_fasta(None, None, C.byref(h)) == cdefs.ERR_INVALID_INPUT and not h.value
    assert L.lcty_genome_load_fasta(None, b"x.fa", None) == cdefs.ERR_INVALID_INPUT
    L.lcty_genome_destroy(None)                                                    # a no-op
    assert C.sizeof(cdefs.GenomeCountStats) == 5 * 8 + 2 * 4 + 4 * 8


def test_genome_create_fails_loudly_without_a_device():
    """No context can exist without a device, so a NULL one is what a caller has: the message is the one lcty_ctx_create gives."""
    h = C.c_void_p()
    rc = _lib.lib().lcty_genome_create(None, C.byref(h))
    msg = _lib.lib().lcty_last_error().decode()
    assert not h.value
    if api.device_count() > 0:
        assert rc == cdefs.ERR_INVALID_INPUT
    else:
        assert rc == cdefs.ERR_RUNTIME and "no CPU fallback" in msg
        rc = _lib.lib().lcty_genome_load_fasta(None, b"genome.fa", C.byref(h))
        assert rc == cdefs.ERR_RUNTIME and "no CPU fallback" in _lib.lib().lcty_last_error().decode()
