"""lcty_bg_reads_fetch: the alignments of a background region through the BAI index of a whole BAM file, records on the device.
The definition is lcty_bg_reads_load on a file of the same records (and pyref_bg.load_alns behind it): the view field for field and
word for word, the status and the read of every error, and the estimate that follows, bit for bit."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, io
from locityper_amd._lib import LocityperError
from tests import bg_fetch_cases as K, bg_synth, pyref_bg as R

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
ARRAYS = ("pos", "end", "qlen", "flags", "mate", "cigar_off", "cigar", "seq_off", "bases2", "nmask")
SCALARS = ("n_records", "n_ignored", "n_wo_cigar", "paired", "read_len")
CTX = []


def ctx():
    if not CTX:
        CTX.append(api.Context(0))
    return CTX[0]


def fetch(path, contig, start, end, padded_start, padded_len, params=None, context=None):
    bam = io.SampleBam(path)
    try:
        return api.BgReads.fetch(context or ctx(), bam, contig, start, end, padded_start, padded_len, params or api.bg_params())
    finally:
        bam.close()


def assert_same_view(a, b):
    for f in SCALARS:
        assert getattr(a, f) == getattr(b, f), f
    for f in ARRAYS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f


def assert_view_is_pyref(v, L):
    recs = L["recs"]
    assert (v.n_records, v.n_ignored, v.n_wo_cigar, v.paired, v.read_len) == (len(recs), L["ignored"], L["wo_cigar"], L["paired"], L["read_len"])
    assert v.pos.tolist() == [r["pos"] for r in recs] and v.end.tolist() == [r["end"] for r in recs]
    assert v.qlen.tolist() == [len(r["seq"]) for r in recs]
    assert v.flags.tolist() == [int(r["reverse"]) | (2 * int(r["second"])) for r in recs]
    assert v.mate.tolist() == [NONE if m is None else m for m in L["mate"]]
    words = [(n << 4) | R.OPS.index(o) for r in recs for o, n in r["cigar"]]
    assert v.cigar.tolist() == words
    assert v.cigar_off.tolist() == np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in recs])]).tolist()
    assert v.seq_off.tolist() == np.concatenate([[0], np.cumsum([(len(r["seq"]) + 31) // 32 * 32 for r in recs])]).tolist()
    nb = int(v.seq_off[-1])
    assert len(v.bases2) == nb // 16 + 2 and len(v.nmask) == nb // 32 + 1
    b2 = np.zeros(len(v.bases2), dtype=np.uint32); nm = np.zeros(len(v.nmask), dtype=np.uint32)
    for r, o in zip(recs, v.seq_off.tolist()):
        for k, c in enumerate(r["seq"]):                         # as stored: neither reversed nor complemented
            e = "ACGT".find(c)
            if e >= 0:
                b2[(o + k) >> 4] |= np.uint32(e << (2 * ((o + k) & 15)))
            else:
                nm[(o + k) >> 5] |= np.uint32(1 << ((o + k) & 31))
    assert np.array_equal(v.bases2, b2) and np.array_equal(v.nmask, nm)


# ---- 1. the hand file ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    H = K.Hand()
    d = tmp_path_factory.mktemp("bgfetch_hand")
    H.plain = K.write_plain(d / "plain.bam", H.refs, H.records)
    H.pyref = {c: R.load_alns(H.plain, c, H.S, H.E, H.padded_seq, H.P) for c in ("chrA", "chrB")}
    H.dir = d
    return H


@pytest.mark.parametrize("block_size", [0xff00, 4096, 257])
def test_hand_file_equals_load_and_pyref(hand, block_size):
    H = hand
    path = K.write_indexed(H.dir / f"hand{block_size}.bam", H.refs, H.records, block_size=block_size)
    for contig in ("chrA", "chrB"):
        v = fetch(path, contig, H.S, H.E, H.P, H.PLEN)
        assert_same_view(v, api.BgReads(path, contig, H.S, H.E, H.P, H.PLEN, api.bg_params()))
        assert_view_is_pyref(v, H.pyref[contig])
        assert v.stats["records_kept"] == v.n_records and v.stats["n_discarded"] == 0
        assert v.stats["n_pairs"] == sum(m is not None for m in H.pyref[contig]["mate"]) // 2
    names = [r["name"] for r in H.pyref["chrA"]["recs"]]
    for kept in ("mapq30", "clip3", "lead_ins", "edge_keep_end", "edge_eqx", "pos_last", "end_past_start", "ops200", "len1", "len65", "len151",
                 "rev151", "codes", "n", "n" * 254, "full", "mate_mapq", "mate_outside"):
        assert kept in names, kept
    for gone in ("mapq29", "clip4", "all_soft", "edge_drop_end", "edge_drop_start", "pos_end", "end_at_start", "noref_before", "noref_at",
                 "dropped_with_n", "filtered_with_h", "ops130_cross", "flag4", "flag100", "flag200", "flag400", "flag800"):
        assert gone not in names, gone


# ---- 2. / 3. seeded samples ------------------------------------------------------------------------------------------------------
class Routes:
    def __init__(self, s, d, params):
        self.s, self.params = s, params
        self.refs = K.wide_refs(s)
        self.all_records = K.with_foreign(s)
        self.path = K.write_indexed(d / "whole.bam", self.refs, self.all_records)
        self.plain = K.write_plain(d / "slice.bam", self.refs, s.records)
        self.args = (s.contig, s.start, s.end, s.padded_start, s.padded_len())
        self.fetched = fetch(self.path, *self.args, params)
        self.loaded = api.BgReads(self.plain, *self.args, params)

    def estimate(self, reads):
        s = self.s
        return api.estimate_bg(ctx(), reads, s.padded_seq, s.padded_start, s.kmer_counts, s.k, s.start, s.end, self.params)


def assert_same_estimate(a, b):
    (bg1, rl1, d1), (bg2, rl2, d2) = a, b
    assert bytes(bg1) == bytes(bg2) and rl1 == rl2
    assert io.bg_to_json(bg1, rl1) == io.bg_to_json(bg2, rl2)
    for k, v in d1.items():
        x, y = np.asarray(v), np.asarray(d2[k])
        if x.dtype.kind in "ui":
            assert x.tobytes() == y.tobytes(), k


@pytest.fixture(scope="module")
def pe(tmp_path_factory):
    return Routes(bg_synth.Sample(region_len=100_000), tmp_path_factory.mktemp("bgfetch_pe"), api.bg_params())


@pytest.fixture(scope="module")
def ont(tmp_path_factory):
    return Routes(bg_synth.ont_sample(region_len=100_000, depth=10.0), tmp_path_factory.mktemp("bgfetch_ont"), api.bg_params(cdefs.TECH_NANOPORE))


def test_paired_sample_view_and_index_use(pe):
    assert_same_view(pe.fetched, pe.loaded)
    assert pe.fetched.paired and pe.fetched.n_records > 10_000 and (pe.fetched.mate != NONE).sum() > 10_000
    st = pe.fetched.stats
    assert st["bytes_read"] < st["file_bytes"]
    assert pe.fetched.n_records <= st["records_walked"] < len(pe.s.records) < len(pe.all_records)
    assert st["records_kept"] == pe.fetched.n_records


def test_paired_sample_estimate_is_bit_identical(pe):
    assert_same_estimate(pe.estimate(pe.fetched), pe.estimate(pe.loaded))


def test_two_fetches_are_bit_identical(pe):
    assert_same_view(fetch(pe.path, *pe.args, pe.params), pe.fetched)


def test_long_read_sample_view_and_estimate(ont):
    """At the default window (5 000 bases for 10 kb reads) the planted repeats of this 100 kb sample leave fewer than two windows, so
    lcty_bg_estimate ends with "Too few windows" after all of its kernels, whichever route made the handle: the two routes must
    agree on that too. With windows of 500 bases the estimate completes, and is compared bit for bit."""
    assert_same_view(ont.fetched, ont.loaded)
    assert not ont.fetched.paired and np.diff(ont.fetched.cigar_off.astype(np.int64)).max() > 64       # the wavefront's path
    assert (ont.fetched.mate == NONE).all()

    def outcome(reads):
        try:
            return ("ok",) + ont.estimate(reads)
        except LocityperError as e:
            return "refused", e.code, str(e)
    a, b = outcome(ont.fetched), outcome(ont.loaded)
    assert a[0] == b[0]
    if a[0] == "ok":
        assert_same_estimate(a[1:], b[1:])
    else:
        assert a == b
    ont.params = api.bg_params(cdefs.TECH_NANOPORE, window_size=500)
    assert_same_estimate(ont.estimate(ont.fetched), ont.estimate(ont.loaded))


# ---- 4. knobs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,value", [("sample_bam_hash_bits", 4), ("sample_bam_hash_bits", 0), ("sample_bam_inflate", 1)])
def test_knobs_leave_the_view_alone(pe, hand, knob, value):
    c = ctx()
    c.set_knob(knob, value)
    try:
        assert_same_view(fetch(pe.path, *pe.args, pe.params), pe.loaded)
        path = K.write_indexed(hand.dir / "hand_knob.bam", hand.refs, hand.records, block_size=4096)
        assert_view_is_pyref(fetch(path, "chrA", hand.S, hand.E, hand.P, hand.PLEN), hand.pyref["chrA"])
    finally:
        c.set_knob(knob, -1)


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def refused(fn):
    with pytest.raises(LocityperError) as e:
        fn()
    return e.value.code, str(e.value)


def both_refuse(hand, d, name, records, read=None, params=None, contig="chrA"):
    """load on the plain file and fetch on the indexed one: the same status, and the read's name in both messages"""
    params = params or api.bg_params()
    plain = K.write_plain(d / f"{name}_plain.bam", hand.refs, records)
    indexed = K.write_indexed(d / f"{name}.bam", hand.refs, records, block_size=4096)
    args = (contig, hand.S, hand.E, hand.P, hand.PLEN)
    c1, m1 = refused(lambda: api.BgReads(plain, *args, params))
    c2, m2 = refused(lambda: fetch(indexed, *args, params))
    assert c1 == c2, (m1, m2)
    if read is not None:
        assert read in m2, m2
    return c2, m1, m2


def test_errors_equal_loads(hand, tmp_path):
    H, d = hand, tmp_path
    good = H.good_pairs()
    at = H.S + 600
    m150 = [("M", 150)]
    q = K.seq_of(150, 9)

    def one(name, cigar, seq=q, flag=H.F1, mapq=60, pos=at):
        return (0, pos, name, mapq, flag, cigar, seq)
    for op in "HNP":
        cig = [("M", 100), (op, 2), ("M", 50)] if op != "H" else [("H", 2), ("M", 150)]
        code, m1, m2 = both_refuse(H, d, f"op{op}", K.by_coordinate(good + [one(f"bad_{op}", cig)]), read=f"bad_{op}")
        assert code == cdefs.ERR_INVALID_DATA and f"operation {op}" in m2 and m1 == m2
    code, m1, m2 = both_refuse(H, d, "qlen", K.by_coordinate(good + [one("short_seq", m150, seq=q[:149])]), read="short_seq")
    assert code == cdefs.ERR_INVALID_DATA and m1 == m2
    code, _, m2 = both_refuse(H, d, "nocigar", K.by_coordinate(good + [one("bare", [])]), read="bare")
    assert code == cdefs.ERR_INVALID_DATA and "without a CIGAR" in m2
    code, m1, m2 = both_refuse(H, d, "mixed", K.by_coordinate(good + [one("single", m150, flag=0)]))
    assert code == cdefs.ERR_INVALID_DATA and "both paired and unpaired" in m2 and m1 == m2
    code, m1, m2 = both_refuse(H, d, "none", K.by_coordinate([one("lowq", m150, mapq=3), one("far", m150, pos=H.E + 5000)]))
    assert code == cdefs.ERR_INVALID_DATA and "no reads in the target region" in m2 and m1 == m2
    for flag, word in ((H.F1, "first"), (H.F2, "second")):
        recs = K.by_coordinate(good + [one("twice", m150, flag=flag, pos=at), one("twice", m150, flag=flag, pos=at + 50),
                                       one("thrice", m150, flag=flag, pos=at + 60), one("thrice", m150, flag=flag, pos=at + 70)])
        code, m1, m2 = both_refuse(H, d, f"two_{word}", recs, read="twice")
        assert code == cdefs.ERR_INVALID_DATA and f"several {word} mates" in m2 and m1 == m2
    code, m1, m2 = both_refuse(H, d, "tech", K.by_coordinate(good), params=api.bg_params(cdefs.TECH_NANOPORE))
    assert code == cdefs.ERR_INVALID_INPUT and m1 == m2
    code, _, m2 = both_refuse(H, d, "contig", K.by_coordinate(good), contig="chrZ", read="chrZ")
    assert code == cdefs.ERR_INVALID_INPUT
    # an interval outside the padded sequence
    path = K.write_indexed(d / "good.bam", H.refs, K.by_coordinate(good), block_size=4096)
    for args in (("chrA", H.P - 1, H.E, H.P, H.PLEN), ("chrA", H.S, H.P + H.PLEN + 1, H.P, H.PLEN), ("chrA", H.E, H.S, H.P, H.PLEN)):
        c1, m1 = refused(lambda: api.BgReads(path, *args, api.bg_params()))
        c2, m2 = refused(lambda: fetch(path, *args))
        assert c1 == c2 == cdefs.ERR_INVALID_INPUT and m1 == m2
    # two offences: the earlier record in file order is the one named, whichever its class
    first_h = K.by_coordinate(good + [one("early_h", [("H", 2), ("M", 150)], pos=at), one("late_len", m150, seq=q[:140], pos=at + 20)])
    code, m1, m2 = both_refuse(H, d, "two_a", first_h, read="early_h")
    assert m1 == m2 and "late_len" not in m2
    first_len = K.by_coordinate(good + [one("early_len", m150, seq=q[:140], pos=at), one("late_h", [("H", 2), ("M", 150)], pos=at + 20)])
    code, m1, m2 = both_refuse(H, d, "two_b", first_len, read="early_len")
    assert m1 == m2 and "late_h" not in m2
    # a record error goes before the errors of the whole set, as in load's loop
    code, m1, m2 = both_refuse(H, d, "two_c", K.by_coordinate(good + [one("single", m150, flag=0, pos=at), one("late_h", [("H", 2), ("M", 150)], flag=0, pos=at + 20)]),
                               read="late_h")
    assert m1 == m2
    # beyond load: coordinates running backwards inside the slice, a slice above the cap
    back = K.by_coordinate(good)
    back.insert(3, one("backwards", m150, pos=H.S + 400))
    path = K.write_indexed(d / "back.bam", H.refs, back, block_size=4096)
    code, msg = refused(lambda: fetch(path, "chrA", H.S, H.E, H.P, H.PLEN))
    assert code == cdefs.ERR_INVALID_DATA and "run backwards" in msg and "backwards" in msg.split("read ")[1]
    c = ctx()
    c.set_knob("sample_bam_max_slice_bytes", 100)
    try:
        code, msg = refused(lambda: fetch(d / "good.bam", "chrA", H.S, H.E, H.P, H.PLEN))
        assert code == cdefs.ERR_UNSUPPORTED and "sample_bam_max_slice_bytes" in msg
    finally:
        c.set_knob("sample_bam_max_slice_bytes", -1)
    # the context goes on
    v = fetch(d / "good.bam", "chrA", H.S, H.E, H.P, H.PLEN)
    assert v.n_records == len(good) and (v.mate != NONE).all()
