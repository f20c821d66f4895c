"""CPU-side checks of the product library: it loads, exports every symbol the header declares,
host-only entry points agree with the oracle, and compute entry points fail loudly without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from locityper_amd import _lib, api, cdefs
from tests import oracle_ffi as O
from tests.helpers import make_bg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "locityper_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lcty_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    syms = header_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/locityper_hip.h but not exported"
    assert set(_lib.SIGNATURES) == set(syms), set(_lib.SIGNATURES) ^ set(syms)
    assert b"gfx950" in L.lcty_version()


def test_struct_layouts_match_header():
    # sizes implied by the C declarations (natural alignment)
    assert C.sizeof(cdefs.AlnRec) == 16 and C.sizeof(cdefs.PairAln) == 32
    assert C.sizeof(cdefs.Bg) == 8 * (5 + 2 + 2 + 2 * cdefs.GC_BINS + 2) + 4 * 6
    assert C.sizeof(cdefs.Params) == 8 + 12 * 8 + 15 * 8 + 4 + 2 + 2 + 4 + 4


def test_params_default_and_resolve_match_oracle():
    p, q = api.default_params(), O.default_params()
    assert bytes(p) == bytes(q) or all(
        (getattr(p, f) == getattr(q, f)) or (getattr(p, f) != getattr(p, f) and getattr(q, f) != getattr(q, f))
        for f, _ in cdefs.Params._fields_ if f not in ("alt_cn", "_pad0"))
    for tech in (cdefs.TECH_ILLUMINA, cdefs.TECH_NANOPORE):
        bg = make_bg(technology=tech, window=100 if tech == 0 else 3333)
        p, q = api.resolve_params(api.default_params(), bg), O.resolve_params(O.default_params(), bg)
        assert (p.tweak, p.unmapped_penalty, p.prob_diff) == (q.tweak, q.unmapped_penalty, q.prob_diff)
    bad = api.default_params()
    bad.tweak = 300
    with pytest.raises(_lib.LocityperError) as e:
        api.resolve_params(bad, make_bg())
    assert e.value.code == cdefs.ERR_INVALID_INPUT


def test_genotypes_and_truncate_match_oracle():
    for n, pl in [(1, 2), (5, 1), (7, 2), (4, 3), (3, 4), (256, 2)]:
        assert np.array_equal(api.generate_genotypes(n, pl), O.generate_genotypes(n, pl))
        assert api.count_genotypes(n, pl) == len(O.generate_genotypes(n, pl))
    rng = np.random.default_rng(1)
    for _ in range(30):
        n = int(rng.integers(1, 400))
        s = np.round(rng.normal(-5000, 300, n), 0)       # rounding creates ties
        fd, ms, th = float(rng.integers(1, 900)), int(rng.integers(1, 450)), int(rng.integers(1, 16))
        a = api.truncate_ixs(s, np.arange(n), fd, ms, th)
        b = O.truncate(s, np.arange(n), fd, ms, th)
        assert np.array_equal(a, b)


def test_compute_entry_points_fail_loudly_without_gpu():
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.LocityperError) as e:
        api.Context(0)
    assert e.value.code == cdefs.ERR_RUNTIME and "no CPU fallback" in str(e.value)


def test_product_package_never_imports_the_oracle():
    """No file of the product includes, imports, links or loads anything under oracle/ (comments may cite it)."""
    pkg = os.path.join(ROOT, "locityper_amd")
    bad = re.compile(r"(^\s*#\s*include[^\n]*oracle)|(^\s*(from|import)\s+[^\n]*oracle)|(CDLL[^\n]*oracle)|(dlopen[^\n]*oracle)|"
                     r"(liblcty_oracle)|(\borc_[a-z_]+\s*\()", re.M)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h", ".c")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not bad.search(txt), os.path.join(dirpath, f)


def test_final_comparison_host_entry_points_match_oracle():
    # lcty_chain_seeds, lcty_solver_default, lcty_discard_improbable, lcty_produce_result are host-only
    r = O.rng_from_seed(123)
    assert api.chain_seeds(123, 7).tolist() == [O.lib().orc_rng_next(C.byref(r)) for _ in range(7)]
    g, a = api.default_solver(cdefs.SOLVER_GREEDY), api.default_solver(cdefs.SOLVER_ANNEAL)
    assert (g.best_start, g.sample_size, g.plato_size) == (1, 10, 100)             # stoch.rs:45-53
    assert (a.anneal_steps, a.plato_size) == (20000, 10000) and a.init_prob == 0.5   # stoch.rs:161-169
    rng = np.random.default_rng(5)
    for n, spread in ((3, 1.0), (40, 30.0), (500, 400.0)):
        mean = -1e5 - spread * rng.random(n) ** 2 * 10
        att = rng.integers(1, 6, n).astype(np.uint32)
        var = np.where(att > 1, rng.random(n) * 4.0, np.nan)
        ixs = rng.permutation(n)[: max(2, n - n // 5)]
        for out_size in (1, 5, n):
            k1 = api.discard_improbable(mean, var, att, ixs, -4.0 * np.log(10), out_size, 2)
            k2 = O.discard_improbable(mean, var, att, ixs, -4.0 * np.log(10), out_size, 2)
            assert np.array_equal(k1, k2)
        i1, lp1, q1 = api.produce_result(mean, var, att, ixs, -4.0 * np.log(10))
        i2, lp2, q2 = O.produce_result(mean, var, att, ixs, -4.0 * np.log(10))
        assert np.array_equal(i1, i2) and np.allclose(lp1, lp2, rtol=1e-10, atol=1e-10)
        assert abs(q1 - q2) <= 1e-7 * max(1.0, abs(q2))


def test_call_checks_match_oracle_and_hand_values():
    # find_weighted_dist / check_first_prob / check_num_of_reads (solve.rs:621-675)
    rng = np.random.default_rng(9)
    A = 7
    dm = rng.integers(1, 500, (A, A)).astype(np.uint32)
    dm = np.minimum(dm, dm.T); np.fill_diagonal(dm, 0)
    for ploidy in (1, 2, 3, 4):
        gts = api.generate_genotypes(A, ploidy)
        pick = gts[rng.permutation(len(gts))[:12]]
        lp = np.sort(rng.random(12) * -8.0)[::-1].copy()
        lp -= np.logaddexp.reduce(lp)
        for d in (dm, None):
            g = api.call_checks(pick, lp, 1000, d)
            o = O.call_checks(pick, lp, 1000, d)
            assert np.array_equal(g[0], o[0]) and g[2] == o[2] == 0
            assert (np.isnan(g[1]) and np.isnan(o[1])) or abs(g[1] - o[1]) <= 1e-12 * max(1.0, abs(o[1]))
    # diploid by hand: min over the two pairings, identical alleles cost nothing
    g2 = np.array([[0, 1], [1, 0], [0, 2], [3, 4]], dtype=np.uint16)
    d, wdist, warn = api.call_checks(g2, np.log([0.7, 0.1, 0.1, 0.1]), 500, dm)
    assert d.tolist() == [0, 0, int(dm[1, 2]), int(min(dm[0, 3] + dm[1, 4], dm[1, 3] + dm[0, 4]))]
    assert abs(wdist - (0.1 * d[2] + 0.1 * d[3])) < 1e-9
    # an unknown distance poisons the weighted distance, not the other entries
    dm2 = dm.copy(); dm2[0, 3] = dm2[3, 0] = dm2[1, 3] = dm2[3, 1] = 0xFFFFFFFF
    d2, w2, _ = api.call_checks(g2, np.log([0.7, 0.1, 0.1, 0.1]), 500, dm2)
    o2 = O.call_checks(g2, np.log([0.7, 0.1, 0.1, 0.1]), 500, dm2)
    assert d2[3] == 0xFFFFFFFF and np.isnan(w2) and np.array_equal(d2, o2[0]) and np.isnan(o2[1])
    # warnings: improbable call; too few reads (ploidy 2: 1 read, 5 reads -> (1/2)^4 = 0.0625 <= 0.1 is fine, 3 reads -> 0.25)
    assert api.call_checks(g2[:1], [np.log(0.005)], 500)[2] == cdefs.WARN_NO_PROBABLE_GENOTYPE == O.call_checks(g2[:1], [np.log(0.005)], 500)[2]
    for n_reads, want in ((1, 2), (3, 2), (5, 0), (19, 0), (20, 0)):
        assert api.call_checks(g2[:1], [0.0], n_reads)[2] == want == O.call_checks(g2[:1], [0.0], n_reads)[2]


def test_counts_to_posteriors():
    """count_to_prob (model/bam.rs:56-67): the per-read posteriors the output BAMs carry (probability, MAPQ)."""
    import math
    prob, mapq = api.counts_to_posteriors([0, 20, 19, 10, 1, 2], 20)
    assert list(mapq) == [0, 60, 13, 3, 0, 0] and prob[0] == 0.0 and prob[1] == 1.0
    for c, p, q in zip([19, 10, 1, 2], prob[2:], mapq[2:]):
        pf = np.float32(c) / np.float32(20)
        assert p == pf and q == min(60, int(round(-10.0 * math.log10(1.0 - float(pf)))))
    prob, mapq = api.counts_to_posteriors([999], 1000)
    assert mapq[0] == 30
    with pytest.raises(_lib.LocityperError):
        api.counts_to_posteriors([21], 20)


# ---------------------------------------------------------------- KmerCounts::load (seq/counts.rs:108-150)
def _varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _save_kmer_counts(k, counter_bytes, contigs):
    """KmerCounts::save (counts.rs:108-124): u8 k, u8 counter bytes, u32 varint contigs, per contig u32 varint + u64 varints."""
    out = bytearray([k, counter_bytes]) + _varint(len(contigs))
    for c in contigs:
        out += _varint(len(c))
        for v in c:
            out += _varint(int(v))
    return bytes(out)


def test_kmer_counts_parse_known_answers_and_errors():
    from locityper_amd import api, _lib
    assert _varint(0) == b"\x00" and _varint(127) == b"\x7f" and _varint(128) == b"\x80\x01" and _varint(300) == b"\xac\x02"
    rng = np.random.default_rng(3)
    off_target = [rng.choice([0, 0, 0, 1, 5, 127, 128, 200, 16383, 16384, 65535, 70000, 2 ** 40], n) for n in (976, 0, 1, 3000)]
    regular = [np.ones(len(c), dtype=np.int64) for c in off_target]
    blob = _save_kmer_counts(25, 2, off_target) + _save_kmer_counts(25, 2, regular)      # add.rs:647-650: two blocks, the first is read
    k, off, counts, used = api.parse_kmer_counts(blob)
    assert k == 25 and used == len(_save_kmer_counts(25, 2, off_target))
    assert off.tolist() == [0, 976, 976, 977, 3977]
    want = np.concatenate([np.minimum(c, 65535) for c in off_target]).astype(np.uint16)                # clamped to KmerCount::MAX
    assert np.array_equal(counts, want)
    k2, off2, counts2, used2 = api.parse_kmer_counts(blob[used:])                                      # the second block parses too
    assert used2 == len(blob) - used and np.all(counts2 == 1) and off2.tolist() == off.tolist()
    # one counter byte: max_value = 255 (counts.rs:134)
    k3, off3, c3, _ = api.parse_kmer_counts(_save_kmer_counts(31, 1, [[0, 254, 255, 256, 65535]]))
    assert k3 == 31 and c3.tolist() == [0, 254, 255, 255, 255]
    # eight counter bytes: u64::MAX, i.e. the u16 clamp alone
    assert api.parse_kmer_counts(_save_kmer_counts(15, 8, [[1, 2 ** 63]]))[2].tolist() == [1, 65535]
    assert api.parse_kmer_counts(_save_kmer_counts(15, 2, []))[1].tolist() == [0]                        # no contigs
    for bad in (blob[:used - 1], blob[:1], b"", _save_kmer_counts(25, 9, [[1]]), bytes([25, 2]) + b"\xff" * 6,
                bytes([25, 2, 1, 1]) + b"\x80" * 10 + b"\x01"):
        with pytest.raises((_lib.LocityperError, ValueError)) as e:
            api.parse_kmer_counts(bad)
        assert not isinstance(e.value, _lib.LocityperError) or e.value.code in (cdefs.ERR_INVALID_DATA, cdefs.ERR_INVALID_INPUT)


def test_truncate_refuses_nan_and_orders_infinities():
    """`>` is not a strict weak order with a NaN (undefined behaviour in std::sort / nth_element). The reference sorts with
    f64::total_cmp (solve.rs:60) and never sees a NaN (priors are checked finite, genotype.rs:1116) -> refused up front; +-inf sort."""
    ixs = np.arange(6, dtype=np.uint64)
    s = np.array([0.0, -1.0, np.nan, -3.0, -2.0, -5.0])
    with pytest.raises(_lib.LocityperError) as e:
        api.truncate_ixs(s, ixs, 2.5, 2, 1)
    assert e.value.code == cdefs.ERR_INVALID_INPUT
    s = np.array([0.0, -np.inf, -1.0, np.inf, -np.inf, -2.0])
    keep = api.truncate_ixs(s, ixs, 1.5, 2, 1)
    assert keep.tolist() == O.truncate(s, ixs, 1.5, 2, 1).tolist() == [3, 0]
    keep = api.truncate_ixs(s, ixs, 1.5, 5, 1)              # min_size reaches into the -inf tie: both stay (partition_point)
    assert keep.tolist() == O.truncate(s, ixs, 1.5, 5, 1).tolist() == [3, 0, 2, 5, 1, 4]


def test_truncate_keeps_at_least_threads_genotypes():
    """run_filter passes data.threads to truncate_ixs (solve.rs:945, 80-81): with the default 8 threads at least 8 genotypes stay."""
    s = -np.arange(20, dtype=np.float64) * 100.0
    ixs = np.arange(20, dtype=np.uint64)
    assert len(api.truncate_ixs(s, ixs, 150.0, 1, 1)) == 2
    assert api.truncate_ixs(s, ixs, 150.0, 1, 8).tolist() == O.truncate(s, ixs, 150.0, 1, 8).tolist() == list(range(8))
    assert api.default_params().threads == 8


def test_knobs_are_named_and_checked():
    L = _lib.lib()
    assert L.lcty_ctx_set_knob(None, b"solve_budget_mb", 1) == cdefs.ERR_INVALID_INPUT


def test_align_knobs_are_in_the_list_and_in_the_header():
    """the knobs of lcty_align_haplotypes: each is in the list lcty_ctx_set_knob accepts (lcty_api.hip), has its words in the knob
    paragraph of the header, and is what lcty_align.hip asks its context for"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    read = lambda *p: open(os.path.join(root, *p)).read()
    api_src, header, align_src = read("locityper_amd", "csrc", "lcty_api.hip"), read("include", "locityper_hip.h"), read("locityper_amd", "csrc", "lcty_align.hip")
    known = api_src[api_src.index("known[] = {"):api_src.index("nullptr};")]
    paragraph = header[:header.index("int32_t lcty_ctx_set_knob(")]
    asked = set(re.findall(r'knob\("(align_[a-z_]+)"', align_src))
    assert asked == {"align_batch_pairs", "align_hash_bits", "align_dp_cells", "align_match_budget"}
    for name in asked:
        assert f'"{name}"' in known and f'"{name}"   ' in paragraph, name


def test_mapper_and_solver_defaults():
    """lcty_map_params_default / _default_long (host only): strobealign's and minimap2's scores, the long route's chaining limits; the struct is
    the header's (15 four-byte fields). lcty_solver_default for the exact solver: HiGHS' default relative gap of 1e-4, which the reference
    leaves alone (highs.rs:103-110); a proof of optimality is gap 0. lcty_ctx_set_path knows its names."""
    assert C.sizeof(cdefs.MapParams) == 15 * 4
    short, long_ = api.map_params(), api.map_params(long_reads=True)
    assert (short.k, short.stride, short.match, short.mismatch, short.gap_open, short.gap_extend, short.min_score, short.band) == (15, 5, 2, 8, 12, 1, 50, 16)
    assert (long_.k, long_.stride, long_.match, long_.mismatch, long_.gap_open, long_.gap_extend, long_.min_votes) == (15, 16, 2, 4, 6, 2, 3)
    assert long_.min_score == -(1 << 31) and long_.gap_open > long_.gap_extend
    for mp in (short, long_):
        assert (mp.route, mp.chain_gap, mp.chain_skew, mp.chain_back) == (cdefs.MAP_ROUTE_AUTO, 2000, 500, 32)
    assert _lib.lib().lcty_map_params_default_long(None) == cdefs.ERR_INVALID_INPUT
    ex = api.default_solver(cdefs.SOLVER_EXACT)
    assert ex.kind == cdefs.SOLVER_EXACT and ex.init_prob == 1e-4 and ex.node_limit == 20_000_000
    assert _lib.lib().lcty_ctx_set_path(None, b"exact_dump", b"/tmp/x") == cdefs.ERR_INVALID_INPUT
    assert api.default_solver(cdefs.SOLVER_ANNEAL).init_prob == 0.5


def test_rust_shim_declares_what_the_header_declares():
    """shim/src/hip/sys.rs is hand-written (no bindgen, no rustc in this image): every function it declares must be a symbol of the
    header with the same number of arguments, and its #[repr(C)] structs must list the header's fields in the header's order."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locityper_hip.h")).read(), flags=re.S)
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "shim", "src", "hip", "sys.rs")).read())
    L = _lib.lib()
    fns = re.findall(r"pub fn (lcty_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->\s*[^;]+)?;", rust, flags=re.S)
    assert len(fns) >= 10
    for name, args in fns:
        assert hasattr(L, name), f"{name} is not exported"
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in the header"
        c_args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        r_args = [a for a in args.split(",") if a.strip()]
        assert len(c_args) == len(r_args), f"{name}: {len(c_args)} arguments in the header, {len(r_args)} in sys.rs"
        assert len(_lib.SIGNATURES[name][1]) == len(c_args)
    for struct in ("lcty_solver", "lcty_gt_alns_view", "lcty_depth_tables"):
        m = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", header, flags=re.S)
        c_fields = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if decl:
                c_fields += [re.sub(r"[\s\*]", "", f).split("[")[0] for f in re.sub(r"^(const\s+)?\w+\s*\**", "", decl, count=1).split(",")]
        r = re.search(r"pub struct " + struct + r"\s*\{(.*?)\}", rust, flags=re.S)
        r_fields = re.findall(r"pub (\w+)\s*:", r.group(1))
        assert c_fields == r_fields, (struct, c_fields, r_fields)
    # the C sizes the Rust structs must have (natural alignment on both sides)
    assert C.sizeof(cdefs.Solver) == 32 and C.sizeof(cdefs.GtAlnsView) == 80 and C.sizeof(cdefs.DepthTables) == 24
