"""The designs of tests/aln_bam_cases.py held against the host reader (lcty_bam_read) and against the table built from the record
lists in Python: the designs and their expected errors are right before a GPU sees them (tests/test_gpu_aln_bam.py)."""
import numpy as np
import pytest

from locityper_amd import _lib, io as lio
from tests import aln_bam_cases as AC

DESIGNS = AC.all_designs()


def test_designs_cover_the_shapes_they_claim():
    by = {d["name"]: d for d in DESIGNS}
    assert len(by) == len(DESIGNS)
    # records start at every byte offset mod 4, and straddle the borders of 700-byte blocks
    d = by["shapes_700"]
    starts = np.cumsum([d["head_len"]] + d["blob_lens"])[:-1]
    assert set(int(s) % 4 for s in starts) == {0, 1, 2, 3}
    assert sum(int(s) // 700 != (int(s) + n - 1) // 700 for s, n in zip(starts, d["blob_lens"])) >= 10
    assert by["header_spans"]["head_len"] > 3 * 700
    # primaries at records 255, 256, 257 and at a workgroup border; groups of 0 .. 300 non-primary records
    prim = [i for i, r in enumerate(by["groups"]["recs"]) if not r["flag"] & 0x900]
    assert {255, 256, 257} <= set(prim) and any(i and i % 256 == 0 for i in prim) and len(prim) % 2 == 0
    assert {0, 1, 63, 64, 65, 255, 256, 257, 300} <= set(np.diff(prim + [len(by["groups"]["recs"])]) - 1)
    recs = by["shapes"]["recs"]
    assert {len(r["name"]) for r in recs} >= set(AC.NAME_LENS) and {len(r["seq"]) for r in recs} >= set(AC.SEQ_LENS)
    assert {len(r["cigar"]) for r in recs} >= set(AC.CIGAR_LENS) and max(len(r["cigar"]) for r in by["cigar_65535"]["recs"]) == 65535
    assert set("".join(r["seq"] for r in recs)) == set(AC.CODES)
    assert any(r["qual"] is None and r["seq"] for r in recs) and any(r["qual"] for r in recs)


@pytest.mark.parametrize("paired", [0, 1])
def test_host_reader_and_python_table_agree_on_every_design(tmp_path, paired):
    p = str(tmp_path / "aln.bam")
    n_err = 0
    for d in DESIGNS:
        AC.write(d, p)
        what = f"{d['name']} paired={paired}"
        try:
            want = AC.expected(d, paired)
        except AC.Refused as r:
            n_err += 1
            with pytest.raises(_lib.LocityperError) as e:
                lio.BamTable(p, d["alleles"], paired=bool(paired))
            assert e.value.code == r.status and str(e.value).endswith("] " + r.text.format(path=p)), f"{what}: {e.value} / {r.text}"
            continue
        T = lio.BamTable(p, d["alleles"], paired=bool(paired))
        AC.assert_same_table(AC.table_of(T), want, what)
        assert T.sizes() == (want["n_pairs"], int(want["mate_off"][-1]), len(want["recs"]), len(want["cigar"]), want["n_refs"]), what
        T.close()
    assert n_err > 60


def test_block_size_does_not_change_the_inflated_bytes():
    from tests import pyref_sample_bam as SB
    d = next(x for x in DESIGNS if x["name"] == "groups")
    for block in (700, 0xff00):
        raw = AC.file_bytes(d, block)
        import zlib
        out, at = b"", 0
        while at < len(raw):
            o = zlib.decompressobj(31)
            out += o.decompress(raw[at:])
            at = len(raw) - len(o.unused_data)
        assert out == d["data"]
