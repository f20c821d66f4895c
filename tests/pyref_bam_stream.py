"""The reads that whole BAM files without an index give to recruitment (`locityper genotype|recruit -a a.bam [-a b.bam] --no-index [-^]`),
restated on plain Python: process_readers! (src/seq/fastx.rs:1029-1043) -> DirectBamReader (692-729), under PairedEndInterleaved
(423-453) with -^; BamRecord::read_from (587-611) with min_start = i64::MIN; equal_names_fast (104-110).

Built on tests/pyref_sample_bam.py: its records (rec), its writer (write_bam(index=False, block_size=..., raw_records=...)), restored,
packed and record_text. A record may carry "bad": "short" (shorter than its fields) or "cut" (it leaves the end of its file); the
reference has no answer for either, the library refuses both."""
from tests import pyref_sample_bam as SB

Refused = SB.Refused


def equal_names_fast(a, b):
    n = len(a)
    return n == len(b) and (n <= 3 or a[n - 3] == b[n - 3])


def paths_text(paths):
    """ext::fmt::paths"""
    return ", ".join(str(p) for p in paths)


class Stream:
    """kept: the kept records of the whole input in order, up to the first refusal; units: [(k1, k2 or None)] ordinals into kept of the
    reads (pairs) completed in front of it; refused: the Refused (what: the whole message) or None; walked: records in front of it."""

    def __init__(self, files, interleaved=False, paths=None):
        paths = [f"file{i}" for i in range(len(files))] if paths is None else [str(p) for p in paths]
        what = paths_text(paths)
        self.kept, self.units, self.refused, self.walked = [], [], None, 0
        waiting = None
        try:
            for fi, recs in enumerate(files):                     # the records of file 0, then file 1, ...: a waiting mate crosses over
                for r in recs:
                    if r.get("bad") == "short":
                        raise Refused(SB.ERR_INVALID_DATA, r["name"], f"{paths[fi]}: record {self.walked} is shorter than its fields")
                    if r.get("bad") == "cut":
                        raise Refused(SB.ERR_INVALID_DATA, r["name"], f"{paths[fi]}: record {self.walked} leaves the end of its file")
                    if r["flag"] & 0x900:                          # read_from: nothing else of the record matters
                        self.walked += 1
                        continue
                    if len(r["seq"]) == 0:
                        raise Refused(SB.ERR_INVALID_DATA, r["name"], f"Primary alignment for read {r['name']} has no sequence")
                    k = len(self.kept)
                    if not interleaved:
                        self.units.append((k, None))
                    elif waiting is None:
                        waiting = k
                    else:
                        a, b = self.kept[waiting]["name"], r["name"]
                        if not equal_names_fast(a.encode(), b.encode()):
                            raise Refused(SB.ERR_INVALID_DATA, b, f"Interleaved input file(s) {what} contains non matching first and second mate ({a} and {b})")
                        self.units.append((waiting, k))
                        waiting = None
                    self.kept.append(r)
                    self.walked += 1
            if waiting is not None:
                raise Refused(SB.ERR_INVALID_DATA, "", f"Odd number of records in an interleaved input file(s) {what}")
        except Refused as e:
            self.refused = e

    def mates(self):
        return [[SB.restored(self.kept[k]) if k is not None else None for k in u] for u in self.units]

    def packed(self):
        """mate_len, mate_off, bases2, nmask of all units as one chunk"""
        return SB.packed(self.mates())

    def text(self, which=None):
        """record_text of the units (all, or those whose index is in `which`), the mates one after the other"""
        out = b""
        for i, u in enumerate(self.units):
            if which is None or i in which:
                out += b"".join(SB.record_text(self.kept[k]) for k in u if k is not None)
        return out

    def totals(self):
        """records_walked, records_primary, records_kept, bases_kept, reads as lcty_bam_stream_stats sums them"""
        bases = sum(len(self.kept[k]["seq"]) for u in self.units for k in u if k is not None)
        return self.walked, len(self.kept), len(self.kept), bases, len(self.units)
