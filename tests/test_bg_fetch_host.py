"""lcty_bg_reads_fetch without a device: the symbol, its argument checks, and the indexed files the GPU tests read — the same records
as bg_synth's plain files, as pyref_bg.load_alns sees them."""
import ctypes as C

from locityper_amd import api, cdefs
from locityper_amd._lib import lib
from tests import bg_fetch_cases as K, pyref_bg as R


def test_symbol_exists():
    assert hasattr(lib(), "lcty_bg_reads_fetch")
    assert hasattr(api.BgReads, "fetch")


def test_null_arguments_leave_out_untouched(tmp_path):
    H = K.Hand()
    path = K.write_indexed(tmp_path / "hand.bam", H.refs, H.records)
    bam = C.c_void_p()
    assert lib().lcty_sample_bam_open(str(path).encode(), None, C.byref(bam)) == cdefs.OK
    params = api.bg_params()
    not_null = C.c_void_p(C.addressof(C.create_string_buffer(64)))            # checked against NULL only, never read
    sentinel = 0x5A5A5A5A

    def call(ctx, b, out_ref):
        return lib().lcty_bg_reads_fetch(ctx, b, b"chrA", H.S, H.E, H.P, H.PLEN, C.byref(params), out_ref, None)
    try:
        for ctx, b in ((None, bam), (not_null, None)):
            out = C.c_void_p(sentinel)
            assert call(ctx, b, C.byref(out)) == cdefs.ERR_INVALID_INPUT
            assert out.value == sentinel
        assert call(not_null, bam, None) == cdefs.ERR_INVALID_INPUT
    finally:
        lib().lcty_sample_bam_close(bam)


def test_indexed_file_holds_the_records_of_the_plain_one(tmp_path):
    H = K.Hand()
    plain = K.write_plain(tmp_path / "plain.bam", H.refs, H.records)
    for bs in (0xff00, 257):
        indexed = K.write_indexed(tmp_path / f"indexed{bs}.bam", H.refs, H.records, block_size=bs)
        for contig in ("chrA", "chrB"):
            a = R.load_alns(plain, contig, H.S, H.E, H.padded_seq, H.P)
            b = R.load_alns(indexed, contig, H.S, H.E, H.padded_seq, H.P)
            assert a == b
            assert len(a["recs"]) > 3 and a["paired"]
    a = R.load_alns(plain, "chrA", H.S, H.E, H.padded_seq, H.P)
    assert a["wo_cigar"] == 4 and a["ignored"] >= 10
    assert sum(m is not None for m in a["mate"]) == 6
