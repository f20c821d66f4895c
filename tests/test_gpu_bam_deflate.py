"""lcty_write_bam with knob "bgzf_deflate": the batch of tests/test_gpu_bam.py::test_bam_of_one_genotype written with the blocks deflated on
the host (0) and on the device (1): the same BAM stream, the same index once every virtual offset is taken to an offset in that stream
through its own file's blocks, every chunk on a record; the knob's values; lcty_io_write_bgzf_device."""
import gzip
import struct

import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio, synth
from locityper_amd._lib import LocityperError
from tests import pyref_sample_bam as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """host.bam, device.bam, host2.bam (the knob set back to 0) of one batch, and what the knob's other values did"""
    ctx = api.Context(0)
    tmp = tmp_path_factory.mktemp("bam_deflate")
    n_alleles, n_pairs, attempts = 6, 1500, 8
    L = synth.SynthLocus(n_alleles, n_pairs, base_len=12_000, technology=cdefs.TECH_ILLUMINA, read_len=150)
    p = api.resolve_params(api.default_params(), L.bg)
    loc = api.Locus(ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    ch = L.reads(0, n_pairs)
    aa = api.AllAlignments.load(loc, ch)
    gt = np.array(L.true_genotype, dtype=np.uint16)
    read_off, counts = api.assignment_counts(aa, gt, api.default_solver(cdefs.SOLVER_ANNEAL), attempts, api.chain_seeds(9, attempts))
    names = [f"read{r}" for r in range(n_pairs)]
    allele_names = [f"hap{a}" for a in range(n_alleles)]
    quals = [bytes([(7 * m + k) % 40 for k in range(int(ch.mate_len[m]))]) for m in range(2 * n_pairs)]

    def write(name):
        lio.write_bam(tmp / name, aa, ch, names, allele_names, gt, attempts, read_off, counts, quals=quals)
        return tmp / name

    out = {"host": write("host.bam")}
    ctx.set_knob("bgzf_deflate", 1)
    out["device"] = write("device.bam")
    refusals = []
    for bad in (2, -1):
        with pytest.raises(LocityperError) as err:
            ctx.set_knob("bgzf_deflate", bad)
        refusals.append((err.value.code, str(err.value)))
    out["device2"] = write("device2.bam")                                    # a refused value leaves the knob where it was
    ctx.set_knob("bgzf_deflate", 0)
    out["host2"] = write("host2.bam")
    out["refusals"] = refusals
    out["ctx"] = ctx
    return out


def mapped_bai(path):
    """the .bai of a BAM with every virtual offset as an offset in the inflated stream: ([per reference (bins {bin: [(beg, end)]}, pseudo
    bin or None, linear [..])], n_no_coor), and the starts of all chunks"""
    data, blocks = P.read_bgzf(path)
    start_of = {c: u for u, c, _ in blocks}

    def m(v):
        assert v >> 16 in start_of, (v >> 16, v & 0xFFFF)
        return start_of[v >> 16] + (v & 0xFFFF)

    b = open(str(path) + ".bai", "rb").read()
    assert b[:4] == b"BAI\1"
    (n_ref,) = struct.unpack_from("<I", b, 4)
    at, refs, chunk_starts = 8, [], []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<I", b, at); at += 4
        bins, pseudo = {}, None
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<II", b, at); at += 8
            pairs = [struct.unpack_from("<QQ", b, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if bin_ == 37450:
                pseudo = (m(pairs[0][0]), m(pairs[0][1]), pairs[1])
            else:
                bins[bin_] = [(m(x), m(y)) for x, y in pairs]
                chunk_starts += [m(x) for x, _ in pairs]
        (n_intv,) = struct.unpack_from("<I", b, at); at += 4
        linear = [m(v) for v in struct.unpack_from(f"<{n_intv}Q", b, at)]
        at += 8 * n_intv
        refs.append((bins, pseudo, linear))
    (no_coor,) = struct.unpack_from("<Q", b, at)
    assert at + 8 == len(b)
    return (refs, no_coor), chunk_starts, data


def test_the_same_stream_and_the_same_index(files):
    host_bai, host_starts, host_data = mapped_bai(files["host"])
    dev_bai, dev_starts, dev_data = mapped_bai(files["device"])
    assert host_data == dev_data and len(host_data) > 3 * 0xff00             # several blocks: offsets beyond the first are translated
    assert open(files["host"], "rb").read().endswith(P.EOF_BLOCK) and open(files["device"], "rb").read().endswith(P.EOF_BLOCK)
    assert open(files["host"], "rb").read() != open(files["device"], "rb").read()     # the device's deflate bytes are its own
    assert host_bai == dev_bai and host_starts == dev_starts and max(host_starts) > 0xff00      # a chunk that starts beyond the first block
    _, records = P.read_bam(files["device"])
    record_at = {r["at"] for r in records}
    assert set(dev_starts) <= record_at
    # the same blocks of inflated bytes on both routes
    assert [u for u, _, _ in P.read_bgzf(files["host"])[1]] == [u for u, _, _ in P.read_bgzf(files["device"])[1]]


def test_the_knob_takes_0_and_1_only(files):
    for code, text in files["refusals"]:
        assert code == cdefs.ERR_INVALID_INPUT and "bgzf_deflate" in text
    assert open(files["device2"], "rb").read() == open(files["device"], "rb").read()
    assert open(files["host2"], "rb").read() == open(files["host"], "rb").read()
    assert open(str(files["host2"]) + ".bai", "rb").read() == open(str(files["host"]) + ".bai", "rb").read()


def test_write_bgzf_device(files, tmp_path):
    rng = np.random.default_rng(8)
    lines = [f"chr1\t{1000 + 37 * k}\t.\t{'ACGT'[k % 4]}\t{'ACGT'[(k + 1 + k // 7) % 4]}\t60\t.\t.\tGT\t" + "\t".join(f"{a}|{b}" for a, b in rng.integers(0, 2, (12, 2)))
             for k in range(3000)]
    text = ("##fileformat=VCFv4.2\n" + "\n".join(lines) + "\n").encode()[:200_000]
    assert len(text) == 200_000
    st = lio.write_bgzf_device(files["ctx"], tmp_path / "x.vcf.gz", text)
    raw = open(tmp_path / "x.vcf.gz", "rb").read()
    assert gzip.decompress(raw) == text and raw.endswith(P.EOF_BLOCK)
    assert st["n_blocks"] == 4 and st["bytes_out"] == len(raw) and len(raw) < len(text) // 3
