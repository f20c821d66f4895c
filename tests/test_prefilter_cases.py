"""The case builder of the prefilter tests (tests/prefilter_cases.py) on the oracle's matrix: every design must yield the level
histogram per row, the column totals per block of 128 rows and the residues of R and of the column total that it names. The GPU tests
(tests/test_gpu_prefilter.py) assert the same on the device's own matrix before they use it."""
import numpy as np
import pytest

from locityper_amd import api, cdefs, synth
from tests import oracle_ffi as O
from tests import prefilter_cases as PC


@pytest.fixture(scope="module")
def small():
    A = 70
    L = synth.SynthLocus(A, 100, seed=5, base_len=3000)
    p = api.resolve_params(api.default_params(), L.bg)
    ol = O.OracleLocus(L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    return A, L, ol


def load(small, design, insert0=None):
    A, L, ol = small
    ch = PC.build_chunk(design, L.seqs, L.seq_off, PC.mean_insert(L.bg) if insert0 is None else insert0)
    oa = ol.load(ch)
    assert oa.n_good == len(design) and (oa.status == cdefs.READ_GOOD).all()          # every designed pair is a row
    return oa.best_aln_matrix(), oa.status


def test_levels_design(small):
    design, counts = PC.levels_1_2_16_17(small[0], 300)
    M, status = load(small, design)
    assert np.array_equal(PC.row_levels(M), counts)
    for b in range(0, 300, 128):                                                       # every block of 128 rows mixes all of them
        assert set(counts[b:b + 128].tolist()) == {1, 2, 15, 16, 17, 22}
    geo = PC.gram_geometry(M, status)
    assert geo["n_res"] == int((counts > 16).sum()) == 100 and geo["n_cols"] == int(np.where(counts > 16, 0, counts - 1).sum())
    # equal level ids of a row are bit-equal entries, different ids different entries
    for r in (1, 3, 5, 17):
        ids, inv = np.unique(design[r], return_inverse=True)
        vals = np.array([M[np.nonzero(inv == t)[0][0], r] for t in range(len(ids))])
        assert np.array_equal(M[:, r], vals[inv]) and len(set(vals.tolist())) == len(ids)


@pytest.mark.parametrize("totals,tail,residue", [([0, 31, 32, 33, 5], 1, 32), ([32, 31, 0], 127, 64), ([33, 0, 31, 32, 33, 31], 127, 96)])
def test_block_edges_design(small, totals, tail, residue):
    design, counts = PC.block_edges(small[0], totals, tail)
    R = 128 * (len(totals) - 1) + tail
    assert design.shape[0] == R and R % 128 == tail
    M, status = load(small, design)
    geo = PC.gram_geometry(M, status)
    assert np.array_equal(geo["levels"], counts)
    assert geo["block_cols"].tolist() == totals
    assert geo["n_cols_padded"] % 128 == residue
    assert geo["n_res"] == len(totals) - (1 if tail == 1 else 0)                       # a 17-level row in every block that has room
    assert counts.max() == 17 and (counts == 16).any()


def test_tile_edges_design(small):
    A = small[0]
    design, counts = PC.tile_edges(A, 120)
    M, status = load(small, design)
    assert np.array_equal(PC.row_levels(M), counts) and (counts == 2).all()
    for e in PC.edge_alleles(A):                                                       # e differs from each neighbour in some row
        for nb in (e - 1, e + 1):
            if 0 <= nb < A:
                assert (M[e] != M[nb]).any(), (e, nb)
    assert PC.edge_alleles(200) == [0, 31, 32, 63, 64, 127, 128, 199] and PC.edge_alleles(A) == [0, 31, 32, 63, 64, 69]


def test_wide_range_design(small):
    A, L, ol = small
    insert0 = PC.mean_insert(L.bg) - 150
    near = PC.closest_insert_shifts(ol.insert_lnprob, insert0)
    design, counts = PC.wide_range(A, 200, near)
    M, status = load(small, design, insert0)
    geo = PC.gram_geometry(M, status)
    assert np.array_equal(geo["levels"], counts)
    ratio = geo["dmax"] / geo["dmin"]
    print(f"wide_range: largest level difference {geo['dmax']:.3f}, smallest {geo['dmin']:.3e}, ratio {ratio:.3e}")
    # reached with this background: 2.7e6 (a perfect pair against no alignment, 46 ln-units; two insert sizes 1.7e-5 apart)
    assert ratio > 1e5 and geo["dmin"] * 2.0 ** 35 / geo["dmax"] > 1.0                 # and the small weight is still more than one unit


def test_mostly_many_valued_design(small):
    design, counts = PC.mostly_many_valued(small[0], 200)
    M, status = load(small, design)
    geo = PC.gram_geometry(M, status)
    assert np.array_equal(geo["levels"], counts) and geo["n_res"] * 4 > len(design)


def test_rows_around_the_level_limit_design(small):
    for design, counts, n_res in (PC.many_sixteens(small[0], 200) + (0,), PC.mostly_many_valued(small[0], 200, many=17, few=2) + (80,)):
        M, status = load(small, design)
        geo = PC.gram_geometry(M, status)
        assert np.array_equal(geo["levels"], counts) and geo["n_res"] == n_res
        assert int((counts >= 16).sum()) * 4 > len(design) and geo["n_cols_padded"] <= 6 * len(design)


def test_appended_to_synthetic_reads_and_the_sums(small):
    """The designed chunk behind SynthLocus reads: rows in order, zero rows for pairs that are not good; the higher-precision sum and the
    bounds on a case the oracle's own f64 sum can be held against."""
    A, L, ol = small
    syn = L.reads(0, 100)
    design, counts = PC.levels_1_2_16_17(A, 60)
    both = PC.concat_chunks([syn, PC.build_chunk(design, L.seqs, L.seq_off, PC.mean_insert(L.bg))])
    oa = ol.load(both)
    M = oa.best_aln_matrix()
    assert np.array_equal(oa.status[100:], np.zeros(60)) and np.array_equal(PC.row_levels(M)[-60:], counts)
    geo = PC.gram_geometry(M, oa.status)
    assert geo["n_rows"] == 160 and (geo["levels"][:100][oa.status[:100] != cdefs.READ_GOOD] == 1).all()
    i, j = PC.sample_genotypes(A, 500)
    assert len(set(zip(i.tolist(), j.tolist()))) == len(i) >= A + 21
    want, want_abs = PC.long_sum(M, i, j)
    so = O.run_filter(M, O.generate_genotypes(A, 2))[PC.gt_index(i, j, A)]
    err = np.abs(so - want).astype(np.float64)
    assert (err <= PC.tile_bound(M.shape[1], want_abs.astype(np.float64))).all()
    assert PC.gram_bound(geo, float(want_abs.max()), float(np.abs(want).max())) < 1e-9 * float(np.abs(want).max())
    assert [PC.level_kernel_width(a) for a in (256, 257, 512, 513, 1025, 2048, 2049, 4095, 4096)] == [4, 8, 8, 16, 32, 32, 64, 64, 64]
