"""CPU tier of the background estimate (lcty_bg.hip / lcty_io.hip): the restatement in pyref_bg against hand-derived answers and
simulated samples, the region reader against the Python parse of the same BAM file, and the distr.gz text round trip. Host code only."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, io
from locityper_amd._lib import LocityperError
from tests import bg_synth, pyref_bg as R
from tests.helpers import make_bg


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    s = bg_synth.Sample()
    path = tmp_path_factory.mktemp("bg") / "bg.bam"
    s.write(path)
    return s, path


# ---- pyref against hand-derived answers ------------------------------------------------------------------------------------------
def test_pyref_loess_gives_a_line_back():
    x = np.sort(np.random.default_rng(1).uniform(10, 90, 400))
    y = 3.0 + 0.25 * x
    out = R.loess(x, y, None, 0.3)
    assert np.allclose(out, 3.0 + 0.25 * np.arange(101), rtol=1e-10, atol=1e-10)
    w = np.random.default_rng(2).uniform(0.1, 1.0, 400)
    assert np.allclose(R.loess(x, y, w, 1.0), 3.0 + 0.25 * np.arange(101), rtol=1e-10, atol=1e-10)


def test_pyref_interpol_quantile():
    a = np.array([5.0, 1.0, 3.0, 2.0, 4.0])
    assert R.interpol_quantile(a, 0.5) == 3.0
    assert R.interpol_quantile(a, 0.99) == pytest.approx(4.96)
    assert R.interpol_quantile(np.array([1.0, 2.0]), 0.0000001) == 1.0          # fraction < 1e-6: no interpolation


def test_pyref_nbinom_fits_recover_parameters():
    rng = np.random.default_rng(3)
    n, p = 12.0, 0.3
    x = rng.negative_binomial(n, p, 200_000).astype(np.float64)
    m, v = R.mean_variance(x)
    nc, pc = R.nbinom_corrected(m, v)
    assert nc == pytest.approx(n, rel=0.03) and pc == pytest.approx(p, rel=0.02)
    nr, pr = R.nb_regularized(m, v)
    mr, vr = R.nb_mean_var(nr, pr)
    assert mr == pytest.approx(m, rel=1e-4) and vr == pytest.approx(v, rel=1e-4)
    # the quantile restatement brackets the CDF
    q = R.nbinom_quantile(n, p, 0.9)
    assert R.nbinom_cdf(n, p, np.floor(q)) <= 0.9 <= R.nbinom_cdf(n, p, np.floor(q) + 1)


def test_pyref_betabinomial_fit_recovers_parameters():
    rng = np.random.default_rng(4)
    a, b, n = 2.0, 300.0, 150
    k = rng.binomial(n, rng.beta(a, b, 100_000))
    ks, cnt = np.unique(k, return_counts=True)
    triples = (ks.astype(float), np.full(len(ks), float(n)), cnt.astype(float))
    (fa, fb), _ = R.bb_fit(triples, 3.0 / 100_000)
    assert fa == pytest.approx(a, rel=0.05) and fb / fa == pytest.approx(b / a, rel=0.03)
    thr = R.bb_inv_cdf(fa, fb, n, 0.99)
    assert abs(np.mean(k <= thr) - 0.99) < 0.01


def test_pyref_pinned_quirks_of_count_region_operations():
    # =, X, D by overlap; I only when it starts inside; the first S up to the region start, any other S up to its end
    rs, re = 100, 200
    assert R.count_region_operations(90, [("=", 20), ("X", 5), ("D", 3), ("=", 10)], rs, re) == (20, 5, 0, 3, 0)
    assert R.count_region_operations(95, [("I", 4), ("=", 20)], rs, re) == (15, 0, 0, 0, 0)
    assert R.count_region_operations(100, [("I", 4), ("=", 20)], rs, re) == (20, 0, 4, 0, 0)
    assert R.count_region_operations(103, [("S", 10), ("=", 20), ("S", 7)], rs, re) == (20, 0, 0, 0, 3 + 7)
    assert R.count_region_operations(190, [("=", 5), ("S", 10)], rs, re) == (5, 0, 0, 0, 5)
    with pytest.raises(R.PyrefError):
        R.count_region_operations(100, [("H", 5), ("=", 20)], rs, re)
    # raw_clipping: a leading I counts, a one-op CIGAR twice, H is not in the divisor
    assert R.clipping_rate(dict(cigar=[("I", 3), ("M", 97)], seq="A" * 100)) == 0.03
    assert R.clipping_rate(dict(cigar=[("S", 50)], seq="A" * 50)) == 2.0
    assert R.clipping_rate(dict(cigar=[("H", 5), ("M", 50)], seq="A" * 50)) == 0.1


def test_pyref_infer_ext_cigar_drops_at_the_padded_end():
    ref = "ACGT" * 25                                    # 100 bases from 1000
    rec = dict(pos=1090, cigar=[("M", 10)], seq=ref[90:100], name="r")
    assert R.infer_ext_cigar(rec, ref, 1000) is None     # ends at the end: dropped (>=)
    rec = dict(pos=1089, cigar=[("M", 10)], seq=ref[89:98] + "N", name="r")
    assert R.infer_ext_cigar(rec, ref, 1000) == [("=", 9), ("X", 1)]
    rec = dict(pos=999, cigar=[("M", 10)], seq=ref[:10], name="r")
    assert R.infer_ext_cigar(rec, ref, 1000) is None
    rec = dict(pos=5000, cigar=[("=", 10)], seq=ref[:10], name="r")
    assert R.infer_ext_cigar(rec, ref, 1000) == [("=", 10)]


# ---- the region reader (host code) -----------------------------------------------------------------------------------------------
def test_region_reader_matches_the_python_parse(sample):
    s, path = sample
    r = api.read_bg_bam(path, s.contig, s.start, s.end, s.padded_start, s.padded_len(), api.bg_params())
    L = R.load_alns(path, s.contig, s.start, s.end, s.padded_seq, s.padded_start)
    assert (r.n_records, r.n_ignored, r.n_wo_cigar, r.paired) == (len(L["recs"]), L["ignored"], L["wo_cigar"], True)
    assert r.n_wo_cigar == 2 and r.n_ignored > 1000
    assert r.read_len == L["read_len"]
    assert np.array_equal(r.pos, [x["pos"] for x in L["recs"]])
    assert np.array_equal(r.end, [x["end"] for x in L["recs"]])
    assert np.array_equal(r.qlen, [len(x["seq"]) for x in L["recs"]])
    assert np.array_equal(r.flags, [int(x["reverse"]) | 2 * int(x["second"]) for x in L["recs"]])
    assert np.array_equal(r.mate, [0xFFFFFFFF if m is None else m for m in L["mate"]])
    for i in range(0, len(L["recs"]), 997):
        x = L["recs"][i]
        words = r.cigar[int(r.cigar_off[i]):int(r.cigar_off[i + 1])]
        assert [(R.OPS[w & 15], int(w >> 4)) for w in words] == x["cigar"]
        o = int(r.seq_off[i])
        dec = "".join("N" if (r.nmask[(o + t) >> 5] >> ((o + t) & 31)) & 1 else "ACGT"[(r.bases2[(o + t) >> 4] >> (2 * ((o + t) & 15))) & 3]
                      for t in range(len(x["seq"])))
        assert dec == x["seq"]
    names = [x["name"] for x in L["recs"]]
    assert "edge_keep_end" in names and "edge_drop_end" not in names and "edge_drop_start" not in names and "edge_eqx" in names


def _bam(tmp_path, s, recs, name="x.bam"):
    return s.write(tmp_path / name, recs)


def test_region_reader_errors(sample, tmp_path):
    s, _ = sample
    ref = s.padded_seq
    P = s.padded_start
    rs = s.start - P
    p = api.bg_params()
    rd = lambda path: api.read_bg_bam(path, s.contig, s.start, s.end, s.padded_start, s.padded_len(), p)
    mixed = [(0, P + rs + 10, "a", 60, 0x1 | 0x40, [("M", 150)], ref[rs + 10:rs + 160]),
             (0, P + rs + 20, "b", 60, 0, [("M", 150)], ref[rs + 20:rs + 170])]
    with pytest.raises(LocityperError) as e:
        rd(_bam(tmp_path, s, mixed))
    assert e.value.code == cdefs.ERR_INVALID_DATA and "both paired and unpaired" in str(e.value)
    with pytest.raises(LocityperError) as e:
        rd(_bam(tmp_path, s, [(0, P + rs + 10, "a", 5, 0, [("M", 150)], ref[rs + 10:rs + 160])]))
    assert e.value.code == cdefs.ERR_INVALID_DATA and "no reads" in str(e.value)
    two = [(0, P + rs + 10, "a", 60, 0x1 | 0x40, [("M", 150)], ref[rs + 10:rs + 160]),
           (0, P + rs + 30, "a", 60, 0x1 | 0x40, [("M", 150)], ref[rs + 30:rs + 180])]
    with pytest.raises(LocityperError) as e:
        rd(_bam(tmp_path, s, two))
    assert e.value.code == cdefs.ERR_INVALID_DATA and "several first mates" in str(e.value)
    hard = [(0, P + rs + 10, "a", 60, 0, [("H", 2), ("M", 150)], ref[rs + 10:rs + 160])]
    with pytest.raises(LocityperError) as e:
        rd(_bam(tmp_path, s, hard))
    assert e.value.code == cdefs.ERR_INVALID_DATA and "unsupported CIGAR operation H" in str(e.value)
    bad_len = [(0, P + rs + 10, "a", 60, 0, [("M", 150)], ref[rs + 10:rs + 159])]
    with pytest.raises(LocityperError) as e:
        rd(_bam(tmp_path, s, bad_len))
    assert e.value.code == cdefs.ERR_INVALID_DATA
    # the process goes on: a good file still reads
    ok = [(0, P + rs + 10, "a", 60, 0, [("M", 150)], ref[rs + 10:rs + 160])]
    assert rd(_bam(tmp_path, s, ok)).n_records == 1


# ---- distr.gz text ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tech,paired", [(cdefs.TECH_ILLUMINA, True), (cdefs.TECH_NANOPORE, False)])
def test_bg_to_json_round_trip_is_bit_exact(tech, paired):
    bg = make_bg(technology=tech, paired=paired, window=100 if paired else 6667, neighb=300 if paired else 6667)
    rng = np.random.default_rng(5)
    for i in range(cdefs.GC_BINS):
        bg.depth_n[i], bg.depth_p[i] = rng.uniform(0.5, 40.0), rng.uniform(0.01, 0.99)
    bg.edit_alpha, bg.edit_beta = float(rng.uniform(0.1, 3)), float(rng.uniform(10, 3000))
    if not paired:
        bg.ins_n = bg.ins_p = 0.0
    rl = 150.0007 if paired else 9997.877207062601
    text = io.bg_to_json(bg, rl, ploidy=2)
    assert ('"insert_distr":{}' in text) == (not paired)
    back, rl2 = io.bg_from_json(text)
    assert bytes(back) == bytes(bg) and rl2 == rl
