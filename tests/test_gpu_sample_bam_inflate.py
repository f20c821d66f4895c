"""lcty_sample_bam_fetch with knob "sample_bam_inflate" 1 (BGZF blocks inflated on the device) against the same fetch with knob 0 (zlib
on the host): the view, the counts, recruitment and the written files must not differ; a corrupt block and the slice limit are refused
alike. Files in blocks of 700 bytes (records straddle blocks, many blocks) and of 0xff00."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from locityper_amd._lib import LocityperError
from tests import pyref_sample_bam as P
from tests import sample_bam_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _two_loci():
    rng = np.random.default_rng(21)
    loci = []
    for _ in range(2):
        base = rng.choice(list(b"ACGT"), 3000).astype(np.uint8)
        alleles = []
        for _ in range(3):
            s = base.copy(); m = rng.random(3000) < 0.01
            s[m] = rng.choice(list(b"ACGT"), int(m.sum()))
            alleles.append(bytes(s))
        loci.append(alleles)
    return loci


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the hand-made and the seeded file at both block sizes: name -> (path, regions)"""
    d = tmp_path_factory.mktemp("gpu_sample_bam_inflate")
    loci = _two_loci()
    out = {"loci": loci, "dir": d}
    for name, refs, recs, regions in (("hand", S.HAND_REFS, S.hand_records(), S.HAND_REGIONS),
                                      ("seeded", S.SEEDED_REFS, S.seeded_records(loci=loci), S.SEEDED_REGIONS)):
        for bs in (700, 0xff00):
            path = str(d / f"{name}-{bs}.bam")
            P.write_bam(path, refs, recs, block_size=bs)
            out[f"{name}-{bs}"] = (path, regions)
    return out


@pytest.fixture(scope="module")
def targets(ctx, files):
    prm = api.recruit_params(paired=True)
    gt = api.Targets(ctx, prm)
    base_k = 25
    for alleles in files["loci"]:
        counts = [np.zeros(len(a) - base_k + 1, dtype=np.uint16) for a in alleles]
        seqs = np.frombuffer(b"".join(alleles), dtype=np.uint8)
        seq_off = np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64)
        cnt_off = np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64)
        gt.add_locus(seqs, seq_off, np.concatenate(counts), cnt_off, base_k)
    gt.finalize()
    return gt


def _fetch(ctx, path, knob, **kw):
    ctx.set_knob("sample_bam_inflate", knob)
    try:
        return lio.SampleBam(path).fetch(ctx, **kw)
    finally:
        ctx.set_knob("sample_bam_inflate", -1)


def _same(a, b):
    (ca, sa, pa), (cb, sb, pb) = a.view(), b.view()
    assert pa == pb and np.array_equal(sa, sb)
    for f in ("mate_len", "mate_off", "bases2", "nmask"):
        assert np.array_equal(getattr(ca, f), getattr(cb, f)), f
    counts = [k for k in a.stats if not k.startswith("ms_")]
    assert len(counts) == 11 and [a.stats[k] for k in counts] == [b.stats[k] for k in counts]


FETCHES = {"regions": dict(paired=True), "unmapped": dict(with_unmapped=True, paired=True), "single": dict(with_unmapped=True, paired=False),
           "whole": dict(whole_file=True, paired=False)}


@pytest.mark.parametrize("fetch", sorted(FETCHES))
@pytest.mark.parametrize("name", ["hand-700", "hand-65280", "seeded-700", "seeded-65280"])
def test_both_routes_fetch_the_same(ctx, files, name, fetch):
    path, regions = files[name]
    kw = dict(FETCHES[fetch])
    if not kw.get("whole_file"):
        kw["regions"] = regions
    host, dev = _fetch(ctx, path, 0, **kw), _fetch(ctx, path, 1, **kw)
    assert host.stats["blocks_inflated"] > (20 if name == "seeded-700" else 0) and host.stats["records_kept"] > 5
    _same(host, dev)


@pytest.mark.parametrize("bs", [700, 0xff00])
def test_recruitment_and_the_written_files_are_the_same(ctx, files, targets, bs):
    path, regions = files[f"seeded-{bs}"]
    written = []
    for knob in (0, 1):
        reads = _fetch(ctx, path, knob, regions=regions, with_unmapped=True)
        cnt, loci = reads.recruit(targets)
        paths = [str(files["dir"] / f"k{knob}-{bs}-locus{k}.fq") for k in range(2)]
        w = lio.FastxWriters(paths)
        n = reads.write_recruited(w, cnt, loci)
        w.close()
        answered = np.arange(loci.shape[1])[None, :] < cnt[:, None]
        written.append((cnt, loci[answered], n, [open(p, "rb").read() for p in paths]))
    (c0, l0, n0, f0), (c1, l1, n1, f1) = written
    assert np.array_equal(c0, c1) and np.array_equal(l0, l1) and n0 == n1 and f0 == f1
    assert (c0 > 0).sum() > 50 and len(f0[0]) > 1000


def test_a_corrupt_block_is_refused_by_both_routes(ctx, files, tmp_path):
    src, _ = files["seeded-700"]
    raw = bytearray(open(src, "rb").read())
    _, blocks = P.read_bgzf(src)
    _, at, bsize = blocks[len(blocks) // 2]
    raw[at + 18 + (bsize - 26) // 2] ^= 0x21
    path = str(tmp_path / "corrupt.bam")
    open(path, "wb").write(bytes(raw))
    open(path + ".bai", "wb").write(open(src + ".bai", "rb").read())
    for knob in (0, 1):
        with pytest.raises(LocityperError) as err:
            _fetch(ctx, path, knob, whole_file=True, paired=False)
        assert err.value.code == cdefs.ERR_INVALID_DATA and "corrupt BGZF block" in str(err.value), (knob, str(err.value))
    assert f"offset {at}" in str(err.value)
    _same(_fetch(ctx, src, 0, whole_file=True, paired=False), _fetch(ctx, src, 1, whole_file=True, paired=False))


def test_the_slice_limit_and_the_knob_values(ctx, files):
    path, regions = files["hand-700"]
    ctx.set_knob("sample_bam_max_slice_bytes", 100)
    try:
        with pytest.raises(LocityperError) as err:
            _fetch(ctx, path, 1, regions=regions)
        assert err.value.code == cdefs.ERR_UNSUPPORTED and "sample_bam_max_slice_bytes" in str(err.value)
    finally:
        ctx.set_knob("sample_bam_max_slice_bytes", -1)
    with pytest.raises(LocityperError) as err:
        _fetch(ctx, path, 2, regions=regions)
    assert err.value.code == cdefs.ERR_INVALID_INPUT and "sample_bam_inflate" in str(err.value)
