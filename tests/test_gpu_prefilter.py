"""run_filter on the device — the f64 tile kernel (lcty_prefilter.hip) and the integer Gram contraction on the matrix cores
(lcty_gram.hip) — at every allele-count class up to 4 096 and on designed rows (tests/prefilter_cases.py).

Every case is checked twice: against the oracle's serial f64 sum at the project's tolerance (1e-9 x max |score|), and, on
a sample of genotypes, against the same sum made in np.longdouble from the DEVICE's matrix, with bounds that follow from the kernels
(prefilter_cases.gram_bound / tile_bound). The sample is a limit on cost, not a tolerance: N_SAMPLE genotypes drawn with a fixed seed, plus every
pair among the edge alleles (0, 31, 32, 63, 64, 127, 128, A - 1 and their neighbours) and the whole diagonal {i, i}.

Every case prints one line ("prefilter case ...", shown by pytest -rA / -s): A, R, the Gram columns, the residual rows, the instantiation
of the level kernel and which kernel the default took, the worst error against the longdouble sum and its bound. The library has no counter
for these: they are derived from the device's matrix the way lcty_gram.hip defines them (prefilter_cases.gram_geometry).

Left out: non-finite matrix entries (the level kernel guards against them), which no loaded read pair produces — every entry is a finite
sum of finite ln-probabilities or the pair's finite no-alignment value — and the C ABI has no entry point that takes a matrix.
"""
import contextlib
import json

import numpy as np
import pytest

from locityper_amd import api, synth
from tests import oracle_ffi as O
from tests import prefilter_cases as PC
from tests.helpers import compare_gpu_to_oracle

pytestmark = pytest.mark.gpu

N_SAMPLE = 20_000
KNOBS = ("prefilter_gram", "prefilter_gram_levels", "prefilter_gram_cols")
VANISHED = "the case this test is about has vanished"


@contextlib.contextmanager
def knobs(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_knob(k, v)
        yield
    finally:
        for k in KNOBS:
            ctx.set_knob(k, -1)


def make_locus(ctx, A, seed=None, base_len=3000):
    L = synth.SynthLocus(A, 4000, seed=(700 + A) if seed is None else seed, base_len=base_len)
    p = api.resolve_params(api.default_params(), L.bg)
    loc = api.Locus(ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    ol = O.OracleLocus(L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, p)
    return L, loc, ol, p


def designed(L, design, insert0=None):
    return PC.build_chunk(design, L.seqs, L.seq_off, PC.mean_insert(L.bg) if insert0 is None else insert0)


def column_room(R, cols_per_row=6):
    """k_cap of launch_prefilter_gram: the columns the buffers take before the batch goes to the tile kernel."""
    return (R * cols_per_row + (R + 127) // 128 * 32 + 127) // 128 * 128


def tile_splits(A, R, cus=256):
    """The read splits launch_prefilter_tile picks (for the log; at the sizes used here the CU count does not matter: R / 256 is smaller)."""
    n_t = (A + 127) // 128
    n_tp = n_t * (n_t + 1) // 2
    splits = min(max(1, (2 * cus + n_tp - 1) // n_tp), max(1, (R + 255) // 256))
    per = ((R + splits - 1) // splits + 31) // 32 * 32
    return max(1, (R + per - 1) // per), per


class Case:
    """A loaded batch, its matrix (compared with the oracle's), the oracle's scores of every genotype and the longdouble sample."""

    def __init__(self, ctx, name, L, loc, ol, p, chunks, aa=None):
        self.ctx, self.name, self.p = ctx, name, p
        chunks = chunks if isinstance(chunks, (list, tuple)) else [chunks]
        self.aa = api.AllAlignments.load(loc, list(chunks)) if aa is None else aa
        oa = ol.load(PC.concat_chunks(chunks))
        self.M, _ = compare_gpu_to_oracle(self.aa, oa)
        self.status = self.aa.status()[0]
        self.A, self.R = self.M.shape[0], len(self.status)
        self.geo = PC.gram_geometry(self.M, self.status)
        self.gts = O.generate_genotypes(self.A, 2)
        self.want = O.run_filter(self.M, self.gts)                     # the oracle's sum over the device's matrix: only the prefilter is under test
        self.scale = max(float(np.abs(self.want).max()), 1.0)
        self.i, self.j = PC.sample_genotypes(self.A, N_SAMPLE)
        self.g = PC.gt_index(self.i, self.j, self.A)
        assert np.array_equal(self.gts[self.g], np.stack([self.i, self.j], axis=1))
        self.exact, self.exact_abs = PC.long_sum(self.M, self.i, self.j)
        self.log = dict(case=name, A=self.A, R=self.R, good=int(self.M.shape[1]), cols=self.geo["n_cols"], cols_padded=self.geo["n_cols_padded"],
                        residual_rows=self.geo["n_res"], level_kernel_vpl=PC.level_kernel_width(self.A), dmax=self.geo["dmax"], dmin=self.geo["dmin"])

    def run(self, **kw):
        with knobs(self.ctx, **kw):
            return self.aa.run_filter()

    def against_oracle(self, sc, what):
        err = float(np.abs(sc - self.want).max())
        assert err <= 1e-9 * self.scale, (self.name, what, err / self.scale)            # 1e-9 relative on sums
        assert int(np.argmax(sc)) == int(np.argmax(self.want)), (self.name, what)
        ix = np.arange(len(sc))
        for min_size in (1, 500):
            keep_g = api.truncate_ixs(sc, ix, self.p.filt_diff, min_size, 1)
            keep_w = O.truncate(self.want, ix, self.p.filt_diff, min_size, 1)
            assert set(keep_g.tolist()) == set(keep_w.tolist()), (self.name, what, min_size)

    def tile_exact(self, sc, what="tile"):
        err = np.abs(sc[self.g].astype(np.longdouble) - self.exact).astype(np.float64)
        bound = PC.tile_bound(self.R, self.exact_abs.astype(np.float64)) + PC.U * np.abs(sc[self.g])   # + the rounding of the longdouble difference to f64
        self.log[what + "_err"], self.log[what + "_bound"] = float(err.max()), float(bound.max())
        w = int(np.argmax(err - bound))
        assert (err <= bound).all(), (self.name, what, int(self.i[w]), int(self.j[w]), float(err[w]), float(bound[w]))

    def gram_exact(self, sc, what="gram", lmax=PC.GR_LMAX):
        geo = self.geo if lmax == PC.GR_LMAX else PC.gram_geometry(self.M, self.status, lmax)
        err = np.abs(sc[self.g].astype(np.longdouble) - self.exact).astype(np.float64)
        bound = PC.gram_bound(geo, float(self.exact_abs.max()), float(np.abs(self.exact).max())) + PC.U * float(np.abs(sc[self.g]).max())
        self.log[what + "_err"], self.log[what + "_bound"] = float(err.max()), float(bound)
        w = int(np.argmax(err))
        assert err.max() <= bound, (self.name, what, "alleles", int(self.i[w]), int(self.j[w]), "tiles", int(self.i[w]) // 128, int(self.j[w]) // 128,
                                    float(err[w]), bound, geo["n_cols"], geo["n_res"])

    def both_forms(self):
        """(a) and (b): tile, Gram (twice) and the default."""
        tile = self.run(prefilter_gram=0)
        gram = self.run(prefilter_gram=1)
        again = self.run(prefilter_gram=1)
        default = self.run()
        fits = self.geo["n_cols_padded"] <= column_room(self.R) and self.A <= 4096 and self.R > 0
        assert fits, (VANISHED, self.name, "no room for the columns: the forced Gram form would have fallen back")
        self.against_oracle(tile, "tile"); self.against_oracle(gram, "gram")
        assert np.array_equal(gram, again), self.name                                    # integer sums: reproducible whatever the column order
        self.tile_exact(tile); self.gram_exact(gram)
        takes_gram = self.A >= 512 and self.geo["n_res"] * 4 <= self.R
        assert np.array_equal(default, gram if takes_gram else tile), (self.name, "default", takes_gram)
        self.log["default_kernel"] = "gram" if takes_gram else "tile"
        return tile, gram

    def mixed_forms(self, tile, gram):
        """(c): the contraction told to take fewer levels (mixed Gram / residual rows) and given too little room."""
        for lmax in (3, 15):
            mixed = self.run(prefilter_gram=1, prefilter_gram_levels=lmax)
            self.against_oracle(mixed, f"levels<={lmax}")
            self.gram_exact(mixed, f"gram_l{lmax}", lmax)
        narrow = self.run(prefilter_gram=1, prefilter_gram_cols=1)
        if self.geo["n_cols_padded"] <= column_room(self.R, 1):                          # still room: the same integers in another layout
            assert np.array_equal(narrow, gram), self.name
            self.log["cols_1"] = "gram"
        else:
            assert np.array_equal(narrow, tile), self.name
            self.log["cols_1"] = "tile"

    def report(self):
        print("prefilter case " + json.dumps(self.log))


# ------------------------------------------------------------------ (a) + (b): every allele-count class
@pytest.mark.parametrize("A,n_synth,n_edges,n_levels", [(257, 1500, 96, 120), (512, 1200, 96, 120), (1025, 600, 96, 90), (2048, 300, 96, 60),
                                                        (2049, 300, 96, 60), (4095, 150, 72, 48), (4096, 150, 72, 48)])
def test_allele_count_classes(gpu_ctx, A, n_synth, n_edges, n_levels):
    """One allele count per instantiation of gram_levels_kernel that no other test launches (8, 32, 64 values per lane) and both sides of the
    boundaries: 257 and 512 (8), 1 025 and 2 048 (32), 2 049, 4 095 and 4 096 (64; 4 096 is 32 full tiles of 128, 528 tile pairs).
    Synthetic reads, then tile_edges rows, then levels_1_2_16_17 rows, appended as three chunks."""
    L, loc, ol, p = make_locus(gpu_ctx, A)
    d_edges, c_edges = PC.tile_edges(A, n_edges, seed=A)
    d_lv, c_lv = PC.levels_1_2_16_17(A, n_levels, seed=A + 1)
    c = Case(gpu_ctx, f"classes A={A}", L, loc, ol, p, [L.reads(0, n_synth), designed(L, d_edges), designed(L, d_lv)])
    lv = c.geo["levels"]
    assert np.array_equal(lv[n_synth:], np.concatenate([c_edges, c_lv])), VANISHED
    assert (lv == 16).any() and (lv == 17).any() and c.geo["n_res"] * 4 <= c.R and c.geo["n_cols"] > 0, VANISHED
    for e in PC.edge_alleles(A):
        for nb in (e - 1, e + 1):
            if 0 <= nb < A:
                assert (c.M[e, -(n_edges + n_levels):] != c.M[nb, -(n_edges + n_levels):]).any(), (VANISHED, e, nb)
    assert PC.level_kernel_width(A) == {257: 8, 512: 8, 1025: 32, 2048: 32, 2049: 64, 4095: 64, 4096: 64}[A]
    c.both_forms()
    c.report()


# ------------------------------------------------------------------ (c): designed rows
def _designs(A, ol, L):
    insert_low = PC.mean_insert(L.bg) - 150
    near = PC.closest_insert_shifts(ol.insert_lnprob, insert_low)
    return {
        "levels_1_2_16_17": (PC.levels_1_2_16_17(A, 300), None),
        "block_edges_r1": (PC.block_edges(A, [0, 31, 32, 33, 5], 1), None),              # R = 513, columns = 32 mod 128
        "block_edges_r127a": (PC.block_edges(A, [32, 31, 0], 127), None),                # R = 383, columns = 64 mod 128
        "block_edges_r127b": (PC.block_edges(A, [33, 0, 31, 32, 33, 31], 127), None),    # R = 767, columns = 96 mod 128
        "wide_range": (PC.wide_range(A, 400, near), insert_low),
    }


@pytest.mark.parametrize("A", [200, 520])
@pytest.mark.parametrize("name", ["levels_1_2_16_17", "block_edges_r1", "block_edges_r127a", "block_edges_r127b", "wide_range"])
def test_designed_rows(gpu_ctx, A, name):
    """Rows made to sit where the decomposition has its edges (see prefilter_cases): 1 / 2 / 15 / 16 / 17 / 22 levels; blocks of 128 rows
    with 0, 31, 32 and 33 columns, a column total that is 32, 64 or 96 modulo 128 and a last block of 1 or 127 rows; a largest level
    difference more than six orders of magnitude above the smallest (the 35-bit fixed point is scaled by the largest)."""
    L, loc, ol, p = make_locus(gpu_ctx, A)
    (design, counts), insert0 = _designs(A, ol, L)[name]
    c = Case(gpu_ctx, f"{name} A={A}", L, loc, ol, p, designed(L, design, insert0))
    assert c.M.shape[1] == len(design) and np.array_equal(c.geo["levels"], counts), VANISHED
    if name.startswith("block_edges"):
        totals, residue = {"block_edges_r1": ([0, 31, 32, 33, 5], 32), "block_edges_r127a": ([32, 31, 0], 64),
                           "block_edges_r127b": ([33, 0, 31, 32, 33, 31], 96)}[name]
        assert c.geo["block_cols"].tolist() == totals and c.geo["n_cols_padded"] % 128 == residue and c.R % 128 in (1, 127), VANISHED
    if name == "wide_range":
        c.log["ratio"] = c.geo["dmax"] / c.geo["dmin"]
        assert c.log["ratio"] > 1e5, VANISHED
    tile, gram = c.both_forms()
    c.mixed_forms(tile, gram)
    c.report()


# ------------------------------------------------------------------ (d): the automatic choice, on its refusing side
def test_mostly_many_valued_rows_fall_back_by_themselves(gpu_ctx):
    """More than a quarter of the rows with more than 16 levels at 520 alleles: with every knob at its default the batch goes to the tile
    kernel (bit for bit its scores); forced, the Gram form (40 % of the rows through the residual path) still holds."""
    A = 520
    L, loc, ol, p = make_locus(gpu_ctx, A)
    design, counts = PC.mostly_many_valued(A, 300)
    c = Case(gpu_ctx, f"mostly_many_valued A={A}", L, loc, ol, p, designed(L, design))
    assert np.array_equal(c.geo["levels"], counts) and c.geo["n_res"] * 4 > c.R, VANISHED
    tile, gram = c.both_forms()                                    # asserts default == tile here
    assert c.log["default_kernel"] == "tile"
    c.report()


@pytest.mark.parametrize("levels", [16, 17])
def test_automatic_choice_at_the_level_limit(gpu_ctx, levels):
    """Where the automatic choice turns: with three rows in ten at exactly 16 levels no row is residual and the default is the Gram form;
    with two rows in five at 17 levels more than a quarter is and the default is the tile kernel."""
    A = 520
    L, loc, ol, p = make_locus(gpu_ctx, A)
    design, counts = PC.many_sixteens(A, 300) if levels == 16 else PC.mostly_many_valued(A, 300, many=17, few=2)
    c = Case(gpu_ctx, f"level limit {levels} A={A}", L, loc, ol, p, designed(L, design))
    assert np.array_equal(c.geo["levels"], counts) and c.geo["n_res"] == (0 if levels == 16 else 120), VANISHED
    tile, gram = c.both_forms()
    assert c.log["default_kernel"] == ("gram" if levels == 16 else "tile")
    assert not np.array_equal(tile, gram), (VANISHED, "the two forms agree bit for bit: the default's choice cannot be seen")
    c.report()


# ------------------------------------------------------------------ (e): buffers that are grown and not cleared
def test_gram_buffers_reused_across_batches_of_other_sizes(gpu_ctx):
    """The Gram buffers of a batch object are grown, never cleared. One object: a large batch; a second object with a smaller batch on the
    same context; the first again after a further chunk was appended (larger) and after a reset to a small batch whose column total is not
    a multiple of 128 (smaller: bits and digits of the earlier batches lie behind its end). Each result equals bit for bit that of a fresh
    context and a fresh load of the same reads."""
    A = 520
    Ls = synth.SynthLocus(A, 4000, seed=700 + A, base_len=3000)
    p = api.resolve_params(api.default_params(), Ls.bg)
    big = [Ls.reads(0, 900), designed(Ls, PC.levels_1_2_16_17(A, 300, seed=8)[0])]
    more = designed(Ls, PC.block_edges(A, [33, 31, 32], 127, seed=9)[0])
    small = designed(Ls, PC.block_edges(A, [31, 5], 1, seed=10)[0])
    small2 = designed(Ls, PC.block_edges(A, [33, 31, 32, 0, 17], 127, seed=11)[0])

    def fresh(chunks):
        ctx = api.Context(0)
        loc = aa = None
        try:
            ctx.set_knob("prefilter_gram", 1)
            loc = api.Locus(ctx, Ls.seqs, Ls.seq_off, Ls.counts, Ls.cnt_off, Ls.k, Ls.bg, p)
            aa = api.AllAlignments.load(loc, chunks)
            return aa.run_filter(), aa.best_aln_matrix(), aa.status()[0]
        finally:                                                   # the batch and the locus go before their context
            if aa is not None: aa.close()
            if loc is not None: loc.close()
            ctx.close()

    want = {k: fresh(v) for k, v in (("big", big), ("small", [small]), ("grown", big + [more]), ("shrunk", [small2]))}
    for k in ("small", "shrunk"):
        geo = PC.gram_geometry(want[k][1], want[k][2])
        assert geo["n_cols_padded"] % 128 != 0 and geo["n_cols"] % 32 != 0, VANISHED
        print(f"prefilter case stale buffers {k}: R={geo['n_rows']} cols={geo['n_cols']} padded={geo['n_cols_padded']} residual={geo['n_res']}")
    loc = api.Locus(gpu_ctx, Ls.seqs, Ls.seq_off, Ls.counts, Ls.cnt_off, Ls.k, Ls.bg, p)
    n = lambda f: sum(f(c) for c in big + [more])
    with knobs(gpu_ctx, prefilter_gram=1):
        a1 = api.AllAlignments(loc, n(lambda c: c.n_pairs), n(lambda c: c.n_bases), n(lambda c: len(c.recs)), n(lambda c: len(c.cigar)))
        for ch in big: a1.append(ch)
        a1.score()
        assert np.array_equal(a1.run_filter(), want["big"][0])
        a2 = api.AllAlignments.load(loc, small)
        assert np.array_equal(a2.run_filter(), want["small"][0])
        a1.append(more); a1.score()
        assert np.array_equal(a1.best_aln_matrix(), want["grown"][1])
        assert np.array_equal(a1.run_filter(), want["grown"][0])
        a1.reset(loc); a1.append(small2); a1.score()
        assert np.array_equal(a1.best_aln_matrix(), want["shrunk"][1])
        assert np.array_equal(a1.run_filter(), want["shrunk"][0])
        assert np.array_equal(a2.run_filter(), want["small"][0])


# ------------------------------------------------------------------ (f): the tile kernel's own edges
@pytest.mark.parametrize("A", [128, 129, 1151, 1152])
def test_tile_kernel_edges(gpu_ctx, A):
    """prefilter_gram = 0 at allele counts that fill the 128-wide tiles exactly, exceed them by one and fall one short (one tile / two
    tiles / nine tiles: the diagonal-tile path at many tiles), with 1, 31, 32 and 33 rows (around the 32-row stage) and 767 and 769 rows:
    the launch splits the rows in runs of at least 8 stages (256 rows), so these are three splits with a last stage of 31 rows and four
    splits of 224 rows of which the last is partial."""
    L, loc, ol, p = make_locus(gpu_ctx, A)
    assert tile_splits(A, 767) == (3, 256) and tile_splits(A, 769) == (4, 224)
    for R in (1, 31, 32, 33, 767, 769):
        n_edges = min(R, 60)
        chunks = [designed(L, PC.tile_edges(A, n_edges, seed=R)[0])]
        if R > n_edges:
            chunks.append(designed(L, PC.levels_1_2_16_17(A, R - n_edges, seed=R + 1)[0]))
        c = Case(gpu_ctx, f"tile_edges A={A} R={R}", L, loc, ol, p, chunks)
        assert c.R == R == c.M.shape[1], VANISHED
        tile = c.run(prefilter_gram=0)
        c.against_oracle(tile, "tile")
        c.tile_exact(tile)
        assert np.array_equal(tile, c.run(prefilter_gram=0))
        c.log["tile_splits"] = tile_splits(A, R)
        c.report()
