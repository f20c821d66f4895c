"""Thin Python binding of the C ABI (include/locityper_hip.h), used by tests/ and bench.py.

Class and method names follow the reference interface of the path:
  Locus        ~ ContigSet + KmerCounts + ContigInfos + UniqueKmers (src/model/locs.rs:930-963, windows.rs:584-615)
  AllAlignments ~ model::locs::AllAlignments (load 1085-1185, best_aln_matrix 1203-1212)
  run_filter / truncate_ixs ~ src/solvers/solve.rs:52-122
Everything is computed by liblocityper_hip.so on the GPU; nothing here falls back to the CPU.
"""
import ctypes as C

import numpy as np

from . import cdefs
from ._lib import lib, check, VP, U32, U64, D
from .cdefs import Bg, Params, Solver, PAIR_ALN_DTYPE


def device_count():
    return int(lib().lcty_device_count())


def default_params():
    p = Params()
    lib().lcty_params_default(C.byref(p))
    return p


def resolve_params(p, bg):
    check(lib().lcty_params_resolve(C.byref(p), C.byref(bg)))
    return p


class _PinnedBlock:
    def __init__(self, addr):
        self.addr = addr

    def __del__(self):
        try:
            lib().lcty_host_free(self.addr)
        except Exception:
            pass


class Context:
    def __init__(self, device=0):
        self._h = VP()
        check(lib().lcty_ctx_create(device, C.byref(self._h)))

    def synchronize(self):
        check(lib().lcty_ctx_synchronize(self._h))

    def set_knob(self, name, value):
        """lcty_ctx_set_knob: a limit of the retry / batching machinery (tests lower them); value < 0 = default."""
        check(lib().lcty_ctx_set_knob(self._h, name.encode(), int(value)))

    def set_path(self, name, path):
        """lcty_ctx_set_path: a file the library is asked to write ("exact_dump"); None switches it off."""
        check(lib().lcty_ctx_set_path(self._h, name.encode(), None if path is None else str(path).encode()))

    def trim(self):
        """lcty_ctx_trim: release the solver workspaces kept between stages."""
        check(lib().lcty_ctx_trim(self._h))

    def pinned_like(self, arr):
        """A copy of `arr` in page-locked host memory (lcty_host_alloc): chunks built from such arrays upload at PCIe link rate.
        The memory is released when the returned array (and every view of it) is gone."""
        arr = np.ascontiguousarray(arr)
        p = VP()
        check(lib().lcty_host_alloc(self._h, max(arr.nbytes, 1), C.byref(p)))
        holder = _PinnedBlock(p.value)
        buf = (C.c_uint8 * max(arr.nbytes, 1)).from_address(p.value)
        out = np.frombuffer(buf, dtype=arr.dtype, count=arr.size).reshape(arr.shape)
        out[...] = arr
        buf._lcty_block = holder                  # the block lives as long as the buffer object the array is a view of
        return out

    def pinned_chunk(self, ch):
        """A ReadsChunk whose arrays lie in page-locked memory."""
        from .cdefs import ReadsChunk
        return ReadsChunk(*(self.pinned_like(a) for a in (ch.mate_len, ch.mate_off, ch.bases2, ch.nmask, ch.aln_off, ch.recs,
                                                          ch.cigar_off, ch.cigar)))

    def timing_reset(self):
        """Switches the HIP-event timing of this context on (it is off until the first call) and zeroes the totals."""
        check(lib().lcty_timing_reset(self._h))

    def timing(self, kernel):
        n, ms = U64(), D()
        check(lib().lcty_timing_get(self._h, kernel, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def close(self):
        if self._h:
            lib().lcty_ctx_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


K_SCORE, K_PREFILTER, K_SOLVE, K_SOLVE_INIT, K_SOLVE_TABLE = 0, 1, 2, 3, 4
K_TRANSFER, K_ANNEAL = 5, 7
K_SOLVE_INIT_ANNEAL = 9          # the initialisation of an annealing stage's chains (K_SOLVE_INIT: a greedy or exact stage's)


class Locus:
    def __init__(self, ctx, seqs, seq_off, counts, cnt_off, k, bg, params):
        self.ctx = ctx
        self.seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        self.seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        self.counts = np.ascontiguousarray(counts, dtype=np.uint16)
        self.cnt_off = np.ascontiguousarray(cnt_off, dtype=np.uint64)
        self.n_alleles = len(self.seq_off) - 1
        self.allele_len = np.diff(self.seq_off.astype(np.int64))
        self.k, self.bg, self.params = k, bg, params
        self._h = VP()
        check(lib().lcty_locus_create(ctx._h, self.n_alleles, self.seqs.ctypes.data, self.seq_off.ctypes.data,
                                      self.counts.ctypes.data, self.cnt_off.ctypes.data, k,
                                      C.byref(bg), C.byref(params), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().lcty_locus_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_hap_alns(self, entries, transfer_fails=3, max_div=0.05):
        """HapAlns (seq/transfer.rs:21-67): entries = [(id1 query, id2 target, raw CIGAR words, n_matches, aln_len)]."""
        n = len(entries)
        id1 = np.array([e[0] for e in entries], dtype=np.uint32)
        id2 = np.array([e[1] for e in entries], dtype=np.uint32)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(e[2]) for e in entries], out=off[1:])
        words = np.concatenate([np.asarray(e[2], dtype=np.uint32) for e in entries]) if n else np.zeros(1, dtype=np.uint32)
        nm = np.array([e[3] for e in entries], dtype=np.uint32)
        ln = np.array([e[4] for e in entries], dtype=np.uint32)
        import time
        t0 = time.perf_counter()
        check(lib().lcty_locus_set_hap_alns(self._h, n, id1.ctypes.data, id2.ctypes.data, off.ctypes.data, words.ctypes.data, nm.ctypes.data,
                                            ln.ctypes.data, transfer_fails, max_div))
        self.set_hap_alns_call_s = time.perf_counter() - t0                   # the library call alone (bench reports it)

    def n_unique_kmers(self):
        n = U64()
        check(lib().lcty_locus_n_unique_kmers(self._h, C.byref(n)))
        return int(n.value)

    def contig_info(self, a):
        ln = int(self.seq_off[a + 1] - self.seq_off[a])
        npos = ln - self.bg.neighb + 1
        gc = np.zeros(npos, dtype=np.uint8)
        uniq = np.zeros(npos, dtype=np.uint32)
        cc = np.zeros(npos, dtype=np.uint16)
        nw, rs = U32(), U32()
        check(lib().lcty_locus_contig_info(self._h, a, gc.ctypes.data, uniq.ctypes.data, cc.ctypes.data,
                                           C.byref(nw), C.byref(rs)))
        return gc, uniq, cc, nw.value, rs.value

    def edit_thresholds(self, read_len):
        g, p = U32(), U32()
        check(lib().lcty_locus_edit_thresholds(self._h, read_len, C.byref(g), C.byref(p)))
        return g.value, p.value

    def insert_lnprob(self, sizes):
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        out = np.zeros(len(sizes), dtype=np.float64)
        pen = D()
        check(lib().lcty_locus_insert_lnprob(self._h, len(sizes), sizes.ctypes.data, out.ctypes.data, C.byref(pen)))
        return out, pen.value

    def set_explicit_weights(self, allele, start, end, value):
        """Explicit region weights (--reg-weights; load_explicit_weights, windows.rs:257-317) as parsed BED lines in file order."""
        al = np.ascontiguousarray(allele, dtype=np.uint32); st = np.ascontiguousarray(start, dtype=np.uint32)
        en = np.ascontiguousarray(end, dtype=np.uint32); va = np.ascontiguousarray(value, dtype=np.float64)
        if not (len(al) == len(st) == len(en) == len(va)):
            raise ValueError("explicit weights: columns of different lengths")
        check(lib().lcty_locus_set_explicit_weights(self._h, len(al), al.ctypes.data, st.ctypes.data, en.ctypes.data, va.ctypes.data))

    def window_weights(self):
        """ContigInfo::neighb_info weights of every moving-window position (alleles concatenated)."""
        n = sum(int(self.seq_off[a + 1] - self.seq_off[a]) - self.bg.neighb + 1 for a in range(self.n_alleles))
        out = np.zeros(n, dtype=np.float64)
        check(lib().lcty_locus_window_weights(self._h, out.ctypes.data))
        return out

    def depth_table(self, width):
        """lcty_locus_depth_table: the extended depth table of the solver stages, [101][width rounded up to a power of two]."""
        w = U32(width)
        check(lib().lcty_locus_depth_table(self._h, C.byref(w), None))
        out = np.zeros((cdefs.GC_BINS, int(w.value)), dtype=np.float64)
        check(lib().lcty_locus_depth_table(self._h, C.byref(w), out.ctypes.data))
        return out

    def depth_lut(self):
        out = np.zeros((cdefs.GC_BINS, cdefs.DEPTH_CACHE), dtype=np.float64)
        check(lib().lcty_locus_depth_lut(self._h, out.ctypes.data))
        return out


class AllAlignments:
    """Device-resident batch of read pairs and the products of AllAlignments::load."""

    def __init__(self, locus, cap_pairs, cap_bases, cap_recs, cap_cigar, streaming_chunk_pairs=None, cap_pair_alns=0):
        """streaming_chunk_pairs: a streaming batch (lcty_reads_create_streaming) — cap_bases / cap_recs / cap_cigar are then the
        capacities of ONE chunk, cap_pairs that of the whole batch; append + score chunk after chunk."""
        self.locus = locus
        self._h = VP()
        if streaming_chunk_pairs is None:
            check(lib().lcty_reads_create(locus._h, cap_pairs, cap_bases, cap_recs, cap_cigar, C.byref(self._h)))
        else:
            check(lib().lcty_reads_create_streaming(locus._h, cap_pairs, streaming_chunk_pairs, cap_bases, cap_recs, cap_cigar,
                                                    cap_pair_alns, C.byref(self._h)))
        self._scored = False

    @classmethod
    def load_streaming(cls, locus, chunks, cap_pair_alns=0):
        """AllAlignments::load of a batch whose records do not have to fit the device together: one chunk resident at a time."""
        chunks = list(chunks)
        self = cls(locus, sum(c.n_pairs for c in chunks), (max(c.n_bases for c in chunks) + 31) // 32 * 32,
                   max(len(c.recs) for c in chunks), max(len(c.cigar) for c in chunks),
                   streaming_chunk_pairs=max(c.n_pairs for c in chunks), cap_pair_alns=cap_pair_alns)
        for c in chunks:
            self.append(c)
            self.score()
        return self

    @classmethod
    def load(cls, locus, chunks, counted=False):
        """AllAlignments::load: upload `chunks` (ReadsChunk or list of them) and score them. counted: hand the records over as
        lcty_aln_counted entries (operations counted here, on the host, as the caller of lcty_reads_append_counted would)."""
        if not isinstance(chunks, (list, tuple)):
            chunks = [chunks]
        self = cls(locus, sum(c.n_pairs for c in chunks), sum(c.n_bases for c in chunks),
                   sum(len(c.recs) for c in chunks), 0 if counted else sum(len(c.cigar) for c in chunks))
        for c in chunks:
            self.append(c, counted=counted)
        self.score()
        return self

    def reset(self, locus):
        """lcty_reads_reset: an empty batch again, bound to `locus` (buffers stay)."""
        check(lib().lcty_reads_reset(self._h, locus._h))
        self.locus = locus
        self._scored = False

    def append(self, chunk, counted=False):
        """counted: True (the operations of the chunk's records are counted here, on the host) or the (n_records, 4) u32 array of
        lcty_aln_counted entries made earlier (ReadsChunk.counted), e.g. in page-locked memory"""
        hs = chunk.host_struct()
        if counted is not False and counted is not None:
            alns = np.ascontiguousarray(chunk.counted(self.locus.allele_len) if counted is True else counted, dtype=np.uint32)
            check(lib().lcty_reads_append_counted(self._h, C.byref(hs), alns.ctypes.data))
        else:
            check(lib().lcty_reads_append(self._h, C.byref(hs)))
        self._scored = False

    def append_bam(self, table, first=0, n=None):
        """lcty_reads_append_bam: pairs [first, first + n) of an io.BamTable read on this batch's context (BamTable(.., ctx=ctx)),
        device to device; n None: up to the table's last pair."""
        if n is None:
            n = table.n_pairs - first
        check(lib().lcty_reads_append_bam(self._h, table._h, first, n))
        self._scored = False

    def score(self):
        check(lib().lcty_score_reads(self._h))
        self._scored = True

    def recover(self):
        """Alignment recovery (transfer.rs:70-140) between two scoring passes; returns the number of transferred alignments."""
        n = U64()
        check(lib().lcty_recover_alignments(self._h, C.byref(n)))
        if n.value: self.score()                 # nothing transferred: the batch is as it was scored
        return int(n.value)

    def recover_dp_cells(self):
        """Cells of the aligner's matrices filled by the last recover()."""
        n = U64()
        check(lib().lcty_recover_dp_cells(self._h, C.byref(n)))
        return int(n.value)

    def recover_stats(self):
        """Read pairs the last recover() took at each of the three lane-scratch levels."""
        out = (C.c_uint64 * 3)()
        check(lib().lcty_recover_stats(self._h, out))
        return [int(x) for x in out]

    def close(self):
        if self._h:
            lib().lcty_reads_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_pairs(self):
        n = U64()
        check(lib().lcty_reads_n_pairs(self._h, C.byref(n)))
        return int(n.value)

    def n_good(self):
        n = U64()
        check(lib().lcty_reads_n_good(self._h, C.byref(n)))
        return int(n.value)

    def score_routes(self):
        """lcty_reads_score_routes: which scoring kernel took which pair in the last scoring launch. A dict of n_pairs, n_lean, n_two,
        n_general (they sum to n_pairs), lean_form (cdefs.LEAN_FORM_*), two_ran and route, one cdefs.ROUTE_* per pair of that launch."""
        route = np.full(self.n_pairs, 0xFF, dtype=np.uint8)
        r = cdefs.ScoreRoutes()
        r.route = route.ctypes.data if len(route) else None
        check(lib().lcty_reads_score_routes(self._h, C.byref(r)))
        out = {n: int(getattr(r, n)) for n in ("n_pairs", "n_lean", "n_two", "n_general", "lean_form")}
        out["two_ran"] = bool(r.two_ran)
        out["route"] = route[:out["n_pairs"]]
        return out

    def status(self):
        n = self.n_pairs
        status = np.zeros(n, dtype=np.uint8)
        weight = np.zeros(n, dtype=np.float64)
        unm = np.zeros(n, dtype=np.float64)
        uniq = np.zeros(2 * n, dtype=np.uint16)
        check(lib().lcty_reads_get_status(self._h, status.ctypes.data, weight.ctypes.data, unm.ctypes.data, uniq.ctypes.data))
        return status, weight, unm, uniq

    def best_aln_matrix(self):
        """[A][n_good] f64 (locs.rs:1203-1212)."""
        ng = self.n_good()
        out = np.zeros((self.locus.n_alleles, ng), dtype=np.float64)
        check(lib().lcty_best_aln_matrix(self._h, out.ctypes.data))
        return out

    def pair_alns(self):
        n = self.n_pairs
        off = np.zeros(n + 1, dtype=np.uint64)
        check(lib().lcty_reads_get_pair_alns(self._h, off.ctypes.data, None, 0))
        out = np.zeros(int(off[-1]), dtype=PAIR_ALN_DTYPE)
        check(lib().lcty_reads_get_pair_alns(self._h, off.ctypes.data, out.ctypes.data, len(out)))
        return off, out

    # ---- prefilter ----
    def run_filter(self, genotypes=None, priors=None, ploidy=2):
        """run_filter scores (solve.rs:101-119). genotypes None = all multisets of `ploidy`."""
        A = self.locus.n_alleles
        if genotypes is None:
            n = count_genotypes(A, ploidy)
            gptr = None
        else:
            genotypes = np.ascontiguousarray(genotypes, dtype=np.uint16)
            n, ploidy = genotypes.shape
            gptr = genotypes.ctypes.data
        scores = np.zeros(n, dtype=np.float64)
        pr = None if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
        check(lib().lcty_prefilter(self._h, gptr, n, ploidy, None if pr is None else pr.ctypes.data, scores.ctypes.data))
        return scores

    def records(self):
        """lcty_reads_get_records: (aln_off, recs, cigar_off, cigar) as the batch holds them now (after recover(): with the transferred
        alignments)."""
        n = self.n_pairs
        aln_off = np.zeros(n + 1, dtype=np.uint64); cig_off = np.zeros(n + 1, dtype=np.uint64)
        check(lib().lcty_reads_get_records(self._h, aln_off.ctypes.data, None, 0, cig_off.ctypes.data, None, 0))
        recs = np.zeros(max(int(aln_off[-1]), 1), dtype=cdefs.ALN_REC_DTYPE); cigar = np.zeros(max(int(cig_off[-1]), 1), dtype=np.uint32)
        check(lib().lcty_reads_get_records(self._h, aln_off.ctypes.data, recs.ctypes.data, len(recs), cig_off.ctypes.data, cigar.ctypes.data, len(cigar)))
        return aln_off, recs[:int(aln_off[-1])], cig_off, cigar[:int(cig_off[-1])]

    def prefilter_async(self, ploidy=2):
        check(lib().lcty_prefilter_async(self._h, ploidy))

    def prefilter_scores(self):
        n = count_genotypes(self.locus.n_alleles, 2)
        scores = np.zeros(n, dtype=np.float64)
        check(lib().lcty_prefilter_scores(self._h, scores.ctypes.data, n))
        return scores

    def prefilter_add_priors(self, priors):
        priors = np.ascontiguousarray(priors, dtype=np.float64)
        check(lib().lcty_prefilter_add_priors(self._h, priors.ctypes.data, len(priors)))

    def prefilter_truncate(self, filt_diff, min_size, threads):
        """lcty_prefilter_truncate: truncate_ixs on the scores the last prefilter call left on the device; the kept genotype indices
        sorted by (score desc, index asc)."""
        keep = U64()
        ixs = np.empty(count_genotypes(self.locus.n_alleles, 2), dtype=np.uint64)      # room for all of them: one call, one sort
        check(lib().lcty_prefilter_truncate(self._h, filt_diff, min_size, threads, ixs.ctypes.data, len(ixs), C.byref(keep)))
        return ixs[:int(keep.value)].copy()


def default_solver(kind):
    s = Solver()
    check(lib().lcty_solver_default(C.byref(s), kind))
    return s


def chain_seeds(master_seed, n):
    out = np.zeros(n, dtype=np.uint64)
    check(lib().lcty_chain_seeds(master_seed, n, out.ctypes.data))
    return out


def solve_stage(aa, genotypes, solver, attempts, seeds, priors=None):
    """One solver stage (solve.rs:816-843) on the GPU: returns (lik_mean, lik_var, liks[n_gt][attempts])."""
    genotypes = np.ascontiguousarray(genotypes, dtype=np.uint16)
    n, ploidy = genotypes.shape
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    assert len(seeds) == n * attempts
    mean, var, liks = np.zeros(n), np.zeros(n), np.zeros((n, attempts))
    pri = None if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
    check(lib().lcty_solve_stage(aa._h, genotypes.ctypes.data, n, ploidy, None if pri is None else pri.ctypes.data,
                                 C.byref(solver), attempts, seeds.ctypes.data, mean.ctypes.data, var.ctypes.data,
                                 liks.ctypes.data))
    return mean, var, liks


def rng_seed_from_u64(seed):
    """The four words of XoshiroRng::seed_from_u64(seed) (ext/rand.rs:3-22)."""
    st = np.zeros(4, dtype=np.uint64)
    check(lib().lcty_rng_seed_from_u64(seed, st.ctypes.data))
    return st


def rng_next_u64(state):
    """next_u64 of the xoshiro256++ generator whose four words `state` holds (advanced in place)."""
    out = U64(0)
    check(lib().lcty_rng_next_u64(state.ctypes.data, C.byref(out)))
    return int(out.value)


def solve_given(locus, read_ixs, ln_prob, windows, window_gc, window_weight, depth_contrib, aln_contrib, solver, rng_state, wshifts=None,
                tables=None, tables_id=0, deepest_only=False):
    """`Solver::solve` (solvers/mod.rs:59-72) on a GenotypeAlignments handed over as arrays (lcty_solve_given): one chain on the device
    over exactly these locations and window distributions. Returns (likelihood, read_assgn u16[n_reads], (aln_lik, depth_lik));
    `rng_state` (four uint64 words, xoshiro256++) is advanced in place by the one draw the call takes. With `tables` (f64[n_rows][width])
    `locus` is a Context and window_gc names rows of the caller's own distributions (lcty_solve_given_tables)."""
    read_ixs = np.ascontiguousarray(read_ixs, dtype=np.uint64)
    ln_prob = np.ascontiguousarray(ln_prob, dtype=np.float64)
    windows = np.ascontiguousarray(windows, dtype=np.uint32).reshape(-1)
    window_gc = np.ascontiguousarray(window_gc, dtype=np.uint8)
    window_weight = np.ascontiguousarray(window_weight, dtype=np.float64)
    n_reads = len(read_ixs) - 1
    v = cdefs.GtAlnsView()
    v.n_reads = n_reads
    v.read_ixs, v.ln_prob, v.windows = read_ixs.ctypes.data, ln_prob.ctypes.data, windows.ctypes.data
    v.n_windows = len(window_weight)
    v.window_gc, v.window_weight = window_gc.ctypes.data, window_weight.ctypes.data
    ws = None
    if wshifts is not None:
        ws = np.ascontiguousarray(wshifts, dtype=np.uint32)
        v.n_contigs, v.wshifts = len(ws) - 1, ws.ctypes.data
    v.depth_contrib, v.aln_contrib = depth_contrib, aln_contrib
    assgn = np.zeros(max(n_reads, 1), dtype=np.uint16)
    parts = np.zeros(2, dtype=np.float64)
    lik = D(0.0)
    if deepest_only:
        d = U32(0)
        check(lib().lcty_gt_alns_deepest(C.byref(v), C.byref(d)))
        return int(d.value)
    rs = None if rng_state is None else rng_state.ctypes.data
    if tables is None:
        check(lib().lcty_solve_given(locus._h, C.byref(v), C.byref(solver), rs, assgn.ctypes.data, parts.ctypes.data, C.byref(lik)))
    else:
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        t = cdefs.DepthTables(tables.shape[0], tables.shape[1], tables.ctypes.data, tables_id)
        check(lib().lcty_solve_given_tables(locus._h, C.byref(v), C.byref(t), C.byref(solver), rs, assgn.ctypes.data, parts.ctypes.data,
                                            C.byref(lik)))
    return float(lik.value), assgn[:n_reads], parts


def solve_stage_from_shards(shards, genotypes, solver, attempts, seeds, priors=None):
    """One solver stage over the reads of several batches of one locus on one device (lcty_solve_stage_from_shards): `shards` in
    read order; equals solve_stage on the unsharded batch."""
    genotypes = np.ascontiguousarray(genotypes, dtype=np.uint16)
    n, ploidy = genotypes.shape
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    assert len(seeds) == n * attempts
    mean, var, liks = np.zeros(n), np.zeros(n), np.zeros((n, attempts))
    pri = None if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
    handles = (VP * len(shards))(*[s._h for s in shards])
    check(lib().lcty_solve_stage_from_shards(handles, len(shards), genotypes.ctypes.data, n, ploidy,
                                             None if pri is None else pri.ctypes.data, C.byref(solver), attempts, seeds.ctypes.data,
                                             mean.ctypes.data, var.ctypes.data, liks.ctypes.data))
    return mean, var, liks


def assignment_counts(aa, genotype, solver, attempts, seeds):
    """Per-read assignment counts of one genotype (update_counts, assgn.rs:374-378): (read_off[n_good+1], counts u16)."""
    genotype = np.ascontiguousarray(genotype, dtype=np.uint16).reshape(-1)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    assert len(seeds) == attempts
    n_good = aa.n_good()
    off = np.zeros(n_good + 1, dtype=np.uint64)
    n = U64()
    args = (aa._h, genotype.ctypes.data, len(genotype), C.byref(solver), attempts, seeds.ctypes.data, off.ctypes.data)
    check(lib().lcty_assignment_counts(*args, None, 0, C.byref(n)))
    counts = np.zeros(int(n.value), dtype=np.uint16)
    check(lib().lcty_assignment_counts(*args, counts.ctypes.data, len(counts), C.byref(n)))
    return off, counts


def count_unexplained(aa, genotype):
    """Genotyping::count_unexplained_reads (solve.rs:718-729)."""
    genotype = np.ascontiguousarray(genotype, dtype=np.uint16).reshape(-1)
    out = U32()
    check(lib().lcty_count_unexplained(aa._h, genotype.ctypes.data, len(genotype), C.byref(out)))
    return int(out.value)


def call_checks(genotypes, ln_probs, n_reads, dist=None, n_alleles=0):
    """find_weighted_dist / check_first_prob / check_num_of_reads (solve.rs:621-675): (distances, weighted_dist, warnings)."""
    genotypes = np.ascontiguousarray(genotypes, dtype=np.uint16)
    n, ploidy = genotypes.shape
    lp = np.ascontiguousarray(ln_probs, dtype=np.float64)
    dm = None if dist is None else np.ascontiguousarray(dist, dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint32)
    wd, warn = D(), U32()
    check(lib().lcty_call_checks(genotypes.ctypes.data, n, ploidy, lp.ctypes.data, n_reads, None if dm is None else dm.ctypes.data,
                                 n_alleles if dm is None else dm.shape[0], out.ctypes.data, C.byref(wd), C.byref(warn)))
    return out, float(wd.value), int(warn.value)


def solve_stats(aa):
    """(chains, iterations, accepted moves) of the last solve_stage on this batch."""
    c, i, a = U64(), U64(), U64()
    check(lib().lcty_solve_stats(aa._h, C.byref(c), C.byref(i), C.byref(a)))
    return int(c.value), int(i.value), int(a.value)


def discard_improbable(lik_mean, lik_var, attempts, ixs, prob_thresh, out_size, threads):
    lik_mean = np.ascontiguousarray(lik_mean, dtype=np.float64)
    lik_var = np.ascontiguousarray(lik_var, dtype=np.float64)
    attempts = np.ascontiguousarray(attempts, dtype=np.uint32)
    ixs = np.ascontiguousarray(ixs, dtype=np.uint64).copy()
    keep = U64()
    check(lib().lcty_discard_improbable(lik_mean.ctypes.data, lik_var.ctypes.data, attempts.ctypes.data, ixs.ctypes.data,
                                        len(ixs), prob_thresh, out_size, threads, C.byref(keep)))
    return ixs[:int(keep.value)]


def produce_result(lik_mean, lik_var, attempts, ixs, prob_thresh, out_bams=0):
    lik_mean = np.ascontiguousarray(lik_mean, dtype=np.float64)
    lik_var = np.ascontiguousarray(lik_var, dtype=np.float64)
    attempts = np.ascontiguousarray(attempts, dtype=np.uint32)
    ixs = np.ascontiguousarray(ixs, dtype=np.uint64)
    out_ixs, out_lp = np.zeros(50, dtype=np.uint64), np.zeros(50, dtype=np.float64)
    n, q = U64(), D()
    check(lib().lcty_produce_result(lik_mean.ctypes.data, lik_var.ctypes.data, attempts.ctypes.data, ixs.ctypes.data, len(ixs),
                                    prob_thresh, out_bams, out_ixs.ctypes.data, out_lp.ctypes.data, C.byref(n), C.byref(q)))
    return out_ixs[:int(n.value)], out_lp[:int(n.value)], q.value


def count_genotypes(n_alleles, ploidy):
    return int(lib().lcty_count_genotypes(n_alleles, ploidy))


def generate_genotypes(n_alleles, ploidy):
    n = count_genotypes(n_alleles, ploidy)
    out = np.zeros((n, ploidy), dtype=np.uint16)
    check(lib().lcty_generate_genotypes(n_alleles, ploidy, out.ctypes.data, n))
    return out


def parse_kmer_counts(data):
    """KmerCounts::load (counts.rs:127-150) of the decompressed `kmers.bin`: (k, cnt_off[n_contigs+1], counts u16, bytes consumed)
    of the first block (the off-target counts)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    k, n, used = U32(), U32(), U64()
    check(lib().lcty_kmer_counts_parse(buf.ctypes.data, len(buf), C.byref(k), C.byref(n), None, 0, None, 0, C.byref(used)))
    off = np.zeros(n.value + 1, dtype=np.uint64)
    counts = np.zeros(max(int(used.value), 1), dtype=np.uint16)
    check(lib().lcty_kmer_counts_parse(buf.ctypes.data, len(buf), C.byref(k), C.byref(n), off.ctypes.data, n.value, counts.ctypes.data,
                                       len(counts), C.byref(used)))
    return int(k.value), off, counts[:int(off[-1])], int(used.value)


def truncate_ixs(scores, ixs, filt_diff, min_size, threads):
    """truncate_ixs (solve.rs:52-84): returns the kept indices sorted by (score desc, index asc)."""
    scores = np.ascontiguousarray(scores, dtype=np.float64)
    ixs = np.ascontiguousarray(ixs, dtype=np.uint64).copy()
    keep = U64()
    check(lib().lcty_truncate(scores.ctypes.data, ixs.ctypes.data, len(ixs), filt_diff, min_size, threads, C.byref(keep)))
    return ixs[:int(keep.value)]


# ---------------------------------------------------------------- solve::solve (src/solvers/solve.rs:926-981)
DEFAULT_SCHEME = (("greedy", 5000, 1), ("anneal", 20, 20))      # "-S greedy:i=5k,a=1 -S anneal:i=20,a=20" (solve.rs:211-230)


def solve(aa, params, scheme=DEFAULT_SCHEME, master_seed=1, priors=None, ploidy=2, genotypes=None, solvers=None):
    """The genotyping of one locus after AllAlignments::load, following solve::solve + solve_single_thread:
    run_filter/truncate_ixs when there are more genotypes than the first stage takes, then every stage
    (skipped when the survivors already fit the next stage's input, solve.rs:805-809) with
    discard_improbable_genotypes in between, and produce_result at the end.

    Returns dict(genotypes, ln_probs, quality, lik_mean, lik_var, attempts, kept_per_stage)."""
    A = aa.locus.n_alleles
    gts = generate_genotypes(A, ploidy) if genotypes is None else np.ascontiguousarray(genotypes, dtype=np.uint16)
    n = len(gts)
    pri = np.zeros(n) if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
    ixs = np.arange(n, dtype=np.uint64)
    threads = max(1, int(params.threads))     # run_filter gets data.threads (solve.rs:945); discard gets it too unless it is 1 (797, 1087)
    kept = []
    if params.dont_skip or scheme[0][1] < n:
        if genotypes is None:
            scores = aa.run_filter(ploidy=ploidy)
            scores = scores + pri
        else:
            scores = aa.run_filter(gts, pri)
        ixs = truncate_ixs(scores, ixs, params.filt_diff, scheme[0][1], threads)
        kept.append(len(ixs))
    lik_mean = np.full(n, np.nan)
    lik_var = np.full(n, np.nan)
    att = np.zeros(n, dtype=np.uint32)
    seed_base = 0
    all_seeds = None
    for si, (name, in_size, attempts) in enumerate(scheme):
        out_size = scheme[si + 1][1] if si + 1 < len(scheme) else None
        if not (params.dont_skip or out_size is None or out_size < len(ixs)):
            continue                                               # "Skipping stage, not enough genotypes"
        solver = solvers[si] if solvers else default_solver(cdefs.SOLVER_GREEDY if name == "greedy" else cdefs.SOLVER_ANNEAL)
        seeds = chain_seeds(master_seed + 0x9E3779B97F4A7C15 * (si + 1) & 0xFFFFFFFFFFFFFFFF, len(ixs) * attempts)
        m, v, _ = solve_stage(aa, gts[ixs], solver, attempts, seeds, priors=pri[ixs])
        lik_mean[ixs], lik_var[ixs], att[ixs] = m, v, attempts
        if out_size is not None:
            ixs = discard_improbable(lik_mean, lik_var, att, ixs, params.prob_thresh, out_size, threads)
        kept.append(len(ixs))
    out_ixs, ln_probs, quality = produce_result(lik_mean, lik_var, att, ixs, params.prob_thresh)
    unexpl = count_unexplained(aa, gts[out_ixs[0]])
    return dict(unexpl_reads=unexpl, genotypes=gts[out_ixs], ixs=out_ixs, ln_probs=ln_probs, quality=quality, lik_mean=lik_mean, lik_var=lik_var,
                attempts=att, kept_per_stage=kept)


def default_stages():
    """Scheme::default (solve.rs:211-230) as an array of lcty_stage."""
    st = (cdefs.Stage * 2)()
    n = U32()
    check(lib().lcty_stages_default(st, C.byref(n)))
    return st


def solve_locus(aa, stages=None, master_seed=1, priors=None, ploidy=2):
    """lcty_solve: the library's own solve::solve (scheme loop in C++). Returns (Call, lik_mean, lik_var, attempts)."""
    stages = default_stages() if stages is None else stages
    G = count_genotypes(aa.locus.n_alleles, ploidy)
    pri = None if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
    mean, var, att = np.zeros(G), np.zeros(G), np.zeros(G, dtype=np.uint32)
    call = cdefs.Call()
    check(lib().lcty_solve(aa._h, ploidy, stages, len(stages), master_seed, None if pri is None else pri.ctypes.data, C.byref(call),
                           mean.ctypes.data, var.ctypes.data, att.ctypes.data))
    return call, mean, var, att


def solve_queue(batches, stages=None, master_seeds=None, priors=None, ploidy=2):
    """lcty_solve_queue: score + solve every batch of the list (loci of one context), the last stage of each overlapped with the
    next entry. Returns the list of Call structs, one per entry."""
    stages = default_stages() if stages is None else stages
    n = len(batches)
    handles = (VP * n)(*[b._h for b in batches])
    seeds = np.ascontiguousarray(np.arange(1, n + 1) if master_seeds is None else master_seeds, dtype=np.uint64)
    assert len(seeds) == n
    pri_ptr = None
    keep = []
    if priors is not None:
        arr = (VP * n)()
        for i, p in enumerate(priors):
            if p is not None:
                keep.append(np.ascontiguousarray(p, dtype=np.float64))
                arr[i] = keep[-1].ctypes.data
        pri_ptr = arr
    calls = (cdefs.Call * n)()
    check(lib().lcty_solve_queue(handles, n, ploidy, stages, len(stages), seeds.ctypes.data, pri_ptr, calls))
    return list(calls)


def solve_queue_fed(n_loci, acquire, release=None, stages=None, master_seeds=None, ploidy=2):
    """lcty_solve_queue_fed: the queue with its batches handed over one at a time. acquire(i) -> AllAlignments (filled; may block until a
    loader thread is done with it), release(i) is called when nothing of position i's batch is in use any more. The library call
    runs without the interpreter lock; the callbacks take it."""
    stages = default_stages() if stages is None else stages
    seeds = np.ascontiguousarray(np.arange(1, n_loci + 1) if master_seeds is None else master_seeds, dtype=np.uint64)
    assert len(seeds) == n_loci
    failure = []

    @C.CFUNCTYPE(VP, VP, U32)
    def _acquire(_user, i):
        try:
            b = acquire(int(i))
            return None if b is None else b._h.value
        except BaseException as e:               # an exception cannot cross the C frames: the queue ends, the exception is raised below
            failure.append(e)
            return None

    @C.CFUNCTYPE(None, VP, U32)
    def _release(_user, i):
        try:
            if release is not None:
                release(int(i))
        except BaseException as e:
            failure.append(e)

    calls = (cdefs.Call * n_loci)()
    rc = lib().lcty_solve_queue_fed(n_loci, C.cast(_acquire, VP), C.cast(_release, VP), None, ploidy, stages, len(stages), seeds.ctypes.data, None, calls)
    if failure:
        raise failure[0]
    check(rc)
    return list(calls)


K_RECRUIT = 6
K_MAP = 8


def map_params(long_reads=False, **over):
    """lcty_map_params_default (seed length 15, a seed every 5 bases, scores 2 / 8 / end bonus 10, secondary records from score 50) or,
    with long_reads, lcty_map_params_default_long (a seed every 16 bases, scores 2 / 4 / gaps 4 + 2 n, every record kept)."""
    p = cdefs.MapParams()
    check((lib().lcty_map_params_default_long if long_reads else lib().lcty_map_params_default)(C.byref(p)))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def build_map_index(locus, basis, k=15):
    """lcty_locus_build_map_index: the k-mers of the basis alleles of the locus."""
    basis = np.ascontiguousarray(basis, dtype=np.uint16)
    check(lib().lcty_locus_build_map_index(locus._h, basis.ctypes.data, len(basis), k))


def map_append(aa, chunk, params):
    """lcty_reads_map_append: the read ends of `chunk` mapped onto the basis alleles, the records straight into the batch `aa`."""
    h = chunk.host_struct()
    check(lib().lcty_reads_map_append(aa._h, C.byref(h), C.byref(params)))
    aa._scored = False


def map_append_recruited(aa, rset, locus_ix, params, first_pair=0, n_pairs=None):
    """lcty_reads_map_append_recruited: pairs [first_pair, first_pair + n_pairs) of locus `locus_ix` of the Recruited set, mapped from
    where they lie on the device, the records straight into the batch `aa` (n_pairs None: to the end)."""
    if n_pairs is None:
        n_pairs = rset.sizes(locus_ix)[0] - first_pair
    check(lib().lcty_reads_map_append_recruited(aa._h, rset._h, locus_ix, first_pair, n_pairs, C.byref(params)))
    aa._scored = False


def map_reads(locus, chunk, params):
    """lcty_map_reads: the read ends of `chunk` (its sequence fields) onto the basis alleles; returns a ReadsChunk with the found
    records, =/X/S CIGARs and the bases in BAM orientation — ready for AllAlignments.append."""
    h = chunk.host_struct()
    n = chunk.n_pairs
    aln_off = np.zeros(n + 1, dtype=np.uint64); cig_off = np.zeros(n + 1, dtype=np.uint64)
    check(lib().lcty_map_reads(locus._h, C.byref(h), C.byref(params), aln_off.ctypes.data, None, 0, cig_off.ctypes.data, None, 0, None, None))
    recs = np.zeros(int(aln_off[-1]), dtype=cdefs.ALN_REC_DTYPE)
    cigar = np.zeros(max(int(cig_off[-1]), 1), dtype=np.uint32)
    b2 = np.zeros_like(chunk.bases2); nm = np.zeros_like(chunk.nmask)
    check(lib().lcty_map_reads(locus._h, C.byref(h), C.byref(params), aln_off.ctypes.data, recs.ctypes.data, len(recs), cig_off.ctypes.data,
                               cigar.ctypes.data, len(cigar), b2.ctypes.data, nm.ctypes.data))
    return cdefs.ReadsChunk(chunk.mate_len, chunk.mate_off, b2, nm, aln_off, recs, cig_off, cigar[:int(cig_off[-1])])


def recruit_params(technology=cdefs.TECH_ILLUMINA, paired=True, **over):
    """recruit::Params defaults (DEFAULT_MINIM_KW, match length 2000, k-mer threshold 50, Technology::default_match_frac)."""
    p = cdefs.RecruitParams()
    check(lib().lcty_recruit_params_default(C.byref(p), technology, int(paired)))
    for k, v in over.items():
        setattr(p, k, v)
    return p


class Targets:
    """recruit::Targets (TargetBuilder::add per locus, then finalize) and Targets::recruit_* on the device."""

    def __init__(self, ctx, params):
        self.ctx = ctx
        self._h = VP()
        check(lib().lcty_targets_create(ctx._h, C.byref(params), C.byref(self._h)))
        self.n_loci = 0

    def add_locus(self, seqs, seq_off, counts, cnt_off, base_k):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8); seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint16); cnt_off = np.ascontiguousarray(cnt_off, dtype=np.uint64)
        ix = U32()
        check(lib().lcty_targets_add_locus(self._h, len(seq_off) - 1, seqs.ctypes.data, seq_off.ctypes.data, counts.ctypes.data,
                                           cnt_off.ctypes.data, base_k, C.byref(ix)))
        self.n_loci += 1
        return int(ix.value)

    def finalize(self):
        n = U64()
        check(lib().lcty_targets_finalize(self._h, C.byref(n)))
        return int(n.value)

    def recruit(self, chunk, paired=True, max_out=8):
        """Loci of every read pair (single read) of the chunk: list of sorted lists."""
        hs = chunk.host_struct()
        n = chunk.n_pairs
        cnt = np.zeros(max(n, 1), dtype=np.uint32); loci = np.zeros(max(n, 1) * max_out, dtype=np.uint32)
        check(lib().lcty_recruit(self._h, C.byref(hs), int(paired), max_out, cnt.ctypes.data, loci.ctypes.data))
        return cnt[:n], loci.reshape(-1, max_out)[:n]

    def close(self):
        if self._h:
            lib().lcty_targets_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Recruited:
    """lcty_recruited: the recruited reads of every locus of finalized Targets, resident on the device in the mapper's layout
    (DESIGN.md 5v). add() takes a host ReadsChunk, add_fastx() the current chunk of an io.FastxDevice, add_sample() an io.SampleReads;
    cnt / loci are the answers of the matching recruit()."""

    def __init__(self, targets, keep_names=False):
        self._h = VP()
        self._targets = targets                        # the targets outlive the set
        check(lib().lcty_recruited_create(targets._h, int(keep_names), C.byref(self._h)))

    @staticmethod
    def _answers(cnt, loci):
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        loci = np.ascontiguousarray(loci, dtype=np.uint32).reshape(len(cnt), -1) if len(cnt) else np.zeros((0, 1), dtype=np.uint32)
        return cnt, np.ascontiguousarray(loci), max(loci.shape[1], 1)

    def add(self, chunk, cnt, loci, paired=True):
        cnt, loci, max_out = self._answers(cnt, loci)
        assert len(cnt) == chunk.n_pairs
        hs = chunk.host_struct()
        check(lib().lcty_recruited_add(self._h, C.byref(hs), int(paired), max_out, cnt.ctypes.data, loci.ctypes.data))

    def add_fastx(self, fastx_device, cnt, loci):
        cnt, loci, max_out = self._answers(cnt, loci)
        assert len(cnt) == fastx_device.n
        check(lib().lcty_recruited_add_fastx(self._h, fastx_device._h, max_out, cnt.ctypes.data, loci.ctypes.data))

    def add_sample(self, sample_reads, cnt, loci):
        cnt, loci, max_out = self._answers(cnt, loci)
        assert len(cnt) == sample_reads.stats["n_pairs"]
        check(lib().lcty_recruited_add_sample(self._h, sample_reads._h, max_out, cnt.ctypes.data, loci.ctypes.data))

    def sizes(self, locus_ix):
        """(pairs, bases spanned by the units) of a locus."""
        n, nb = U64(0), U64(0)
        check(lib().lcty_recruited_sizes(self._h, locus_ix, C.byref(n), C.byref(nb)))
        return int(n.value), int(nb.value)

    def view(self, locus_ix):
        """(cdefs.ReadsChunk of sequence fields, src_ordinal [n] uint64) of a locus: copies."""
        hs, ordp = cdefs.ReadsHost(), VP()
        check(lib().lcty_recruited_view(self._h, locus_ix, C.byref(hs), C.byref(ordp)))
        n = int(hs.n_pairs)
        def arr(ptr, count, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(count,)).copy() if count else np.zeros(0, dtype=dt)
        mate_off = arr(hs.mate_off, 2 * n + 1, C.c_uint64)
        nb = int(mate_off[-1])
        z = np.zeros(n + 1, dtype=np.uint64)
        chunk = cdefs.ReadsChunk(arr(hs.mate_len, 2 * n, C.c_uint32), mate_off, arr(hs.bases2, nb // 16, C.c_uint32), arr(hs.nmask, nb // 32, C.c_uint32),
                                 z, np.zeros(0, dtype=cdefs.ALN_REC_DTYPE), z, np.zeros(0, dtype=np.uint32))
        return chunk, arr(ordp, n, C.c_uint64)

    def names(self, locus_ix):
        """The names of a locus's pairs, in its order (keep_names)."""
        offp, namesp = VP(), VP()
        check(lib().lcty_recruited_names(self._h, locus_ix, C.byref(offp), C.byref(namesp)))
        n = self.sizes(locus_ix)[0]
        off = np.ctypeslib.as_array(C.cast(offp, C.POINTER(C.c_uint64)), shape=(n + 1,))
        blob = C.string_at(namesp, int(off[n]))
        return [blob[int(off[i]):int(off[i + 1])].decode() for i in range(n)]

    def names_raw(self, locus_ix):
        """(name_off [n + 1] uint64, names bytes) as lcty_write_bam takes them: copies."""
        offp, namesp = VP(), VP()
        check(lib().lcty_recruited_names(self._h, locus_ix, C.byref(offp), C.byref(namesp)))
        n = self.sizes(locus_ix)[0]
        off = np.ctypeslib.as_array(C.cast(offp, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        return off, C.string_at(namesp, int(off[n]))

    def close(self):
        if self._h:
            lib().lcty_recruited_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


COMM_ID_BYTES = 128


def comm_unique_id():
    """ncclGetUniqueId (rank 0); hand the bytes to the other ranks (locityper_amd.dist.make_comm does that over torch.distributed)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(lib().lcty_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """RCCL communicator of one process per GPU (lcty_comm): the SUM all-reduce of read-sharded run_filter scores."""

    def __init__(self, ctx, n_ranks, rank, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        self.ctx = ctx
        self._h = VP()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(lib().lcty_comm_create(ctx._h, n_ranks, rank, buf, C.byref(self._h)))
        self.n_ranks, self.rank = n_ranks, rank

    def rccl_ranks(self):
        """(ranks, rank) as RCCL reports them for this communicator (ncclCommCount / ncclCommUserRank)."""
        n, r = C.c_int32(0), C.c_int32(0)
        check(lib().lcty_comm_ranks(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def prefilter_allreduce(self, aa):
        check(lib().lcty_prefilter_allreduce(aa._h, self._h))

    def solve_stage(self, aa, genotypes, solver, attempts, seeds, priors=None):
        """solve_stage with the chains dealt to the ranks (lcty_solve_stage_sharded): same arguments on every rank, the results
        of all genotypes on every rank."""
        genotypes = np.ascontiguousarray(genotypes, dtype=np.uint16)
        n, ploidy = genotypes.shape
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert len(seeds) == n * attempts
        mean, var, liks = np.zeros(n), np.zeros(n), np.zeros((n, attempts))
        pri = None if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
        check(lib().lcty_solve_stage_sharded(aa._h, self._h, genotypes.ctypes.data, n, ploidy, None if pri is None else pri.ctypes.data,
                                             C.byref(solver), attempts, seeds.ctypes.data, mean.ctypes.data, var.ctypes.data,
                                             liks.ctypes.data))
        return mean, var, liks

    def solve_stage_read_sharded(self, shard, genotypes, solver, attempts, seeds, priors=None):
        """One solver stage of a locus whose reads are sharded over the ranks (lcty_solve_stage_read_sharded): `shard` holds this
        rank's block of the read list; same stage arguments on every rank, the results of all genotypes on every rank."""
        genotypes = np.ascontiguousarray(genotypes, dtype=np.uint16)
        n, ploidy = genotypes.shape
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert len(seeds) == n * attempts
        mean, var, liks = np.zeros(n), np.zeros(n), np.zeros((n, attempts))
        pri = None if priors is None else np.ascontiguousarray(priors, dtype=np.float64)
        check(lib().lcty_solve_stage_read_sharded(shard._h, self._h, genotypes.ctypes.data, n, ploidy,
                                                  None if pri is None else pri.ctypes.data, C.byref(solver), attempts,
                                                  seeds.ctypes.data, mean.ctypes.data, var.ctypes.data, liks.ctypes.data))
        return mean, var, liks

    def close(self):
        if self._h:
            lib().lcty_comm_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def counts_to_posteriors(counts, attempts):
    """count_to_prob (model/bam.rs:56-67) for every entry of an assignment-count array: (probability f32, MAPQ u8)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint16)
    prob = np.zeros(len(counts), dtype=np.float32); mapq = np.zeros(len(counts), dtype=np.uint8)
    check(lib().lcty_counts_to_posteriors(counts.ctypes.data, len(counts), attempts, prob.ctypes.data, mapq.ctypes.data))
    return prob, mapq


# ---- background distributions of a sample (lcty_bg.hip) ------------------------------------------------------------------------
def bg_params(technology=cdefs.TECH_ILLUMINA, **kw):
    """lcty_bg_params_default with the technology and any field given by name."""
    p = cdefs.BgParams()
    lib().lcty_bg_params_default(C.byref(p))
    p.technology = technology
    for k, val in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, val)
    return p


class BgReads:
    """lcty_bg_reads_load: the records of the background interval [start, end) of `contig` that load_alns keeps, as numpy arrays.
    BgReads.fetch: the same from the sample's indexed BAM file (lcty_bg_reads_fetch), with the stage times in `stats`."""

    def __init__(self, path, contig, start, end, padded_start, padded_len, params):
        self._h = VP()
        self.stats = None
        check(lib().lcty_bg_reads_load(str(path).encode(), contig.encode(), start, end, padded_start, padded_len, C.byref(params), C.byref(self._h)))
        self._take_view()

    @classmethod
    def fetch(cls, ctx, sample_bam, contig, start, end, padded_start, padded_len, params):
        """sample_bam: io.SampleBam. The handle keeps its arrays on the device of ctx: estimate_bg on that context reads them there.
        Close it before the context."""
        self = cls.__new__(cls)
        self._h = VP()
        st = cdefs.SampleBamStats()
        check(lib().lcty_bg_reads_fetch(ctx._h, sample_bam._h, contig.encode(), start, end, padded_start, padded_len, C.byref(params),
                                        C.byref(self._h), C.byref(st)))
        self.stats = st.as_dict()
        self._ctx = ctx
        self._take_view()
        return self

    def _take_view(self):
        v = cdefs.BgReadsView()
        check(lib().lcty_bg_reads_view_get(self._h, C.byref(v)))
        n = int(v.n_records)
        self.n_records, self.n_ignored, self.n_wo_cigar = n, int(v.n_ignored), int(v.n_wo_cigar)
        self.paired, self.read_len = bool(v.paired), float(v.read_len)

        def arr(p, count, dt):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (count,)).copy() if count else np.zeros(0, dtype=dt)
        self.pos, self.end, self.qlen = arr(v.pos, n, C.c_uint32), arr(v.end, n, C.c_uint32), arr(v.qlen, n, C.c_uint32)
        self.flags, self.mate = arr(v.flags, n, C.c_uint8), arr(v.mate, n, C.c_uint32)
        self.cigar_off = arr(v.cigar_off, n + 1, C.c_uint64)
        self.cigar = arr(v.cigar, int(self.cigar_off[-1]), C.c_uint32)
        self.seq_off = arr(v.seq_off, n + 1, C.c_uint64)
        nb = int(self.seq_off[-1])
        self.bases2, self.nmask = arr(v.bases2, nb // 16 + 2, C.c_uint32), arr(v.nmask, nb // 32 + 1, C.c_uint32)

    def close(self):
        if self._h:
            lib().lcty_bg_reads_free(self._h)
            self._h = VP()

    def __del__(self):
        self.close()


def read_bg_bam(path, contig, start, end, padded_start, padded_len, params):
    return BgReads(path, contig, start, end, padded_start, padded_len, params)


def estimate_bg(ctx, reads, padded_seq, padded_start, kmer_counts, k, region_start, region_end, params, with_diag=True):
    """lcty_bg_estimate -> (Bg, mean read length, diag dict or None). padded_seq: bytes (upper-case ACGT); kmer_counts: u16 of every
    k-mer of padded_seq."""
    seq = np.frombuffer(bytes(padded_seq), dtype=np.uint8)
    cnt = np.ascontiguousarray(kmer_counts, dtype=np.uint16)
    bg, rl = Bg(), D()
    dg, keep = None, {}
    if with_diag:
        nw, nr, npairs = U64(), U64(), U64()
        check(lib().lcty_bg_diag_sizes(reads._h, region_start, region_end, C.byref(params), C.byref(nw), C.byref(nr), C.byref(npairs)))
        nw, nr, npairs = int(nw.value), int(nr.value), int(npairs.value)
        dg = cdefs.BgDiag()
        dg.n_windows, dg.n_records, dg.n_pairs = nw, nr, npairs
        shapes = {"win_start": (nw, np.uint32), "win_gc": (nw, np.float64), "win_kmer_frac": (nw, np.float64), "win_keep": (nw, np.uint8),
                  "win_depth": (2 * nw, np.uint32), "rec_counts": (5 * nr, np.uint32), "rec_edit": (nr, np.uint32),
                  "rec_read_len": (nr, np.uint32), "rec_middle": (nr, np.uint32), "rec_window": (nr, np.uint32),
                  "pair_first": (npairs, np.uint32), "pair_second": (npairs, np.uint32), "pair_insert": (npairs, np.uint32),
                  "pair_same_strand": (npairs, np.uint8), "hist_size": (npairs, np.uint32), "hist_count": (npairs, np.uint32),
                  "edit_edit": (nr, np.uint32), "edit_len": (nr, np.uint32), "edit_count": (nr, np.uint64)}
        for name, (cnt_, dt) in shapes.items():
            keep[name] = np.zeros(max(cnt_, 1), dtype=dt)
            setattr(dg, name, keep[name].ctypes.data)
    check(lib().lcty_bg_estimate(ctx._h, reads._h, seq.ctypes.data, padded_start, len(seq), cnt.ctypes.data, k, region_start, region_end,
                                 C.byref(params), C.byref(bg), C.byref(rl), C.byref(dg) if dg is not None else None))
    if dg is None:
        return bg, float(rl.value), None
    nw, nr, npairs, nh, ne = int(dg.n_windows), int(dg.n_records), int(dg.n_pairs), int(dg.n_hist), int(dg.n_edit)
    sizes = {"win": nw, "rec": nr, "pair": npairs, "hist": nh, "edit": ne}
    out = {}
    for name, a in keep.items():
        m = sizes[name.split("_")[0]]
        m = 2 * m if name == "win_depth" else 5 * m if name == "rec_counts" else m
        out[name] = a[:m].copy()
    out["win_depth"] = out["win_depth"].reshape(-1, 2)
    out["rec_counts"] = out["rec_counts"].reshape(-1, 5)
    for f in ("orient", "op_totals", "n_stage", "gc_nwin", "loess_mean", "loess_var", "blur_mean", "blur_var", "nb_n", "nb_p"):
        out[f] = np.array(getattr(dg, f)[:])
    out["kernel_ms"] = np.array(dg.kernel_ms[:])
    for f in ("ins_limit", "ins_mean", "ins_var", "ci_low", "ci_high", "unif_coef", "depth_mean", "depth_var", "fit_ms", "total_ms"):
        out[f] = getattr(dg, f)
    return bg, float(rl.value), out


# ---- locus database build (locityper target; lcty_db.hip) ------------------------------------------------------------------------
def db_params(**kw):
    """lcty_db_params_default (div_k = div_w = 15, no divergences, counts wanted) with overrides."""
    p = cdefs.DbParams()
    lib().lcty_db_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _haps(seqs, seq_off):
    """A haplotype set as the C interface takes it: the bases back to back and the offsets, seq_off[0] = 0."""
    return np.ascontiguousarray(seqs, dtype=np.uint8), np.ascontiguousarray(seq_off, dtype=np.uint64)


def _take(ptr, n, dtype):
    """A copy of the n values at ptr (none for a null pointer)."""
    return np.frombuffer(C.string_at(ptr, n * np.dtype(dtype).itemsize), dtype=dtype).copy() if n and ptr else np.zeros(0, dtype=dtype)


def db_minimizers(ctx, seqs, seq_off, k=15, w=15):
    """lcty_db_minimizers: (min_off[n + 1], sorted minimizer hashes of every sequence concatenated, stats dict)."""
    sq, off = _haps(seqs, seq_off)
    n = len(off) - 1
    moff = np.zeros(n + 1, dtype=np.uint64)
    h, st = VP(), cdefs.DbStats()
    check(lib().lcty_db_minimizers(ctx._h, n, sq.ctypes.data, off.ctypes.data, k, w, moff.ctypes.data, C.byref(h), C.byref(st)))
    try:
        total = int(moff[-1])
        hashes = np.frombuffer(C.string_at(h, 8 * total), dtype=np.uint64).copy() if total else np.zeros(0, dtype=np.uint64)
    finally:
        lib().lcty_io_free(h)
    return moff, hashes, st.as_dict()


def db_divergences(ctx, seqs, seq_off, k=15, w=15, with_f64=True):
    """lcty_db_divergences: (uniq u32 triangle, diverg f64 triangle or None, check dict, stats dict), pairs in the order rows i, then j > i."""
    sq, off = _haps(seqs, seq_off)
    n = len(off) - 1
    npairs = max(n * (n - 1) // 2, 0)
    uniq = np.zeros(max(npairs, 1), dtype=np.uint32)
    div = np.zeros(max(npairs, 1), dtype=np.float64) if with_f64 else None
    ck, st = cdefs.DbCheck(), cdefs.DbStats()
    check(lib().lcty_db_divergences(ctx._h, n, sq.ctypes.data, off.ctypes.data, k, w, uniq.ctypes.data, div.ctypes.data if with_f64 else None,
                                    C.byref(ck), C.byref(st)))
    chk = {"n_high": int(ck.n_high), "highest": float(ck.highest), "pair": (int(ck.highest_i), int(ck.highest_j))}
    return uniq[:npairs], (div[:npairs] if with_f64 else None), chk, st.as_dict()


def db_off_target(ctx, seqs, seq_off, counts, cnt_off, k, counter_bytes, ref_seq, ref_counts):
    """lcty_db_off_target: (off-target counts u16 laid out as `counts`, warn bits, stats dict)."""
    sq, off = _haps(seqs, seq_off)
    cnt = np.ascontiguousarray(counts, dtype=np.uint16)
    coff = np.ascontiguousarray(cnt_off, dtype=np.uint64)
    ref = np.ascontiguousarray(ref_seq, dtype=np.uint8)
    rc = np.ascontiguousarray(ref_counts, dtype=np.uint16)
    out = np.zeros(max(len(cnt), 1), dtype=np.uint16)
    warn, st = U32(), cdefs.DbStats()
    check(lib().lcty_db_off_target(ctx._h, len(off) - 1, sq.ctypes.data, off.ctypes.data, cnt.ctypes.data, coff.ctypes.data, k, counter_bytes,
                                   ref.ctypes.data, len(ref), rc.ctypes.data, len(rc), out.ctypes.data, C.byref(warn), C.byref(st)))
    return out[:len(cnt)], int(warn.value), st.as_dict()


def db_discard_identical(names, seqs, seq_off):
    """lcty_db_discard_identical: (kept input indices, {kept index: [names folded into it]}, text of discarded_haplotypes.txt — b"" = no file)."""
    from .io import _names_blob
    sq, off = _haps(seqs, seq_off)
    n = len(off) - 1
    blob = _names_blob(names)
    kept = np.zeros(max(n, 1), dtype=np.uint32); owner = np.zeros(max(n, 1), dtype=np.uint32)
    nk, need = U32(), U64()
    check(lib().lcty_db_discard_identical(n, sq.ctypes.data, off.ctypes.data, blob, kept.ctypes.data, C.byref(nk), owner.ctypes.data, None, 0, C.byref(need)))
    text = np.zeros(max(int(need.value), 1), dtype=np.uint8)
    check(lib().lcty_db_discard_identical(n, sq.ctypes.data, off.ctypes.data, blob, None, C.byref(nk), None, text.ctypes.data, len(text), C.byref(need)))
    folded = {int(i): [] for i in kept[:nk.value]}
    for i in range(n):
        if int(owner[i]) != i:
            folded[int(owner[i])].append(names[i])
    return kept[:nk.value].copy(), folded, text[:int(need.value)].tobytes()


def db_build_locus(ctx, names, seqs, seq_off, ref_seq=None, counts=None, cnt_off=None, k=25, counter_bytes=2, params=None):
    """lcty_db_build_locus: process_alleles on buffers. counts / cnt_off: one block of n + 1 contigs, the reference sequence last.
    Returns a dict: fasta, kmers, distances, discarded (bytes, uncompressed), kept, warn_bits, check, stats."""
    from .io import _names_blob
    sq, off = _haps(seqs, seq_off)
    p = params if params is not None else db_params()
    ref = np.ascontiguousarray(ref_seq, dtype=np.uint8) if ref_seq is not None else None
    cnt = np.ascontiguousarray(counts, dtype=np.uint16) if counts is not None else None
    coff = np.ascontiguousarray(cnt_off, dtype=np.uint64) if cnt_off is not None else None
    f = cdefs.DbFiles()
    check(lib().lcty_db_build_locus(ctx._h, len(off) - 1, _names_blob(names), sq.ctypes.data, off.ctypes.data,
                                    None if ref is None else ref.ctypes.data, 0 if ref is None else len(ref),
                                    None if cnt is None else cnt.ctypes.data, None if coff is None else coff.ctypes.data, k, counter_bytes,
                                    C.byref(p), C.byref(f)))
    try:
        return {
            "fasta": C.string_at(f.fasta, f.fasta_len), "kmers": C.string_at(f.kmers, f.kmers_len),
            "distances": C.string_at(f.distances, f.distances_len), "discarded": C.string_at(f.discarded, f.discarded_len),
            "kept": np.frombuffer(C.string_at(f.kept, 4 * f.n_kept), dtype=np.uint32).copy(), "warn_bits": int(f.warn_bits),
            "check": {"n_high": int(f.check.n_high), "highest": float(f.check.highest), "pair": (int(f.check.highest_i), int(f.check.highest_j))},
            "stats": f.stats.as_dict(),
        }
    finally:
        lib().lcty_db_files_free(C.byref(f))


# ---- a locus from a pangenome VCF (locityper target -v; lcty_panvcf.hip) -------------------------------------------------------------
def panvcf_names(samples, ploidy, ref_name, leave_out=()):
    """lcty_panvcf_names (HaplotypeNames::new): (names of the retained columns, col_sample — NONE_U32 for the reference —, col_hap, haplotypes left out)."""
    from .io import _names_blob
    pl = np.ascontiguousarray(ploidy, dtype=np.uint32)
    sb, lb = _names_blob(samples), _names_blob(leave_out)
    n, nl, left = U32(), U64(), U32()
    args = (len(samples), sb, pl.ctypes.data, ref_name.encode(), len(leave_out), lb)
    check(lib().lcty_panvcf_names(*args, 0, C.byref(n), None, None, None, 0, C.byref(nl), C.byref(left)))
    cs = np.zeros(max(n.value, 1), dtype=np.uint32); ch = np.zeros(max(n.value, 1), dtype=np.uint32)
    names = np.zeros(max(int(nl.value), 1), dtype=np.uint8)
    check(lib().lcty_panvcf_names(*args, len(cs), C.byref(n), cs.ctypes.data, ch.ctypes.data, names.ctypes.data, len(names), C.byref(nl), C.byref(left)))
    return [x.decode() for x in names[:int(nl.value)].tobytes().split(b"\0")[:-1]], cs[:n.value].copy(), ch[:n.value].copy(), int(left.value)


def panvcf_columns(gt, hap_off, col_sample, col_hap):
    """The genotype matrix restricted to the retained columns of panvcf_names: a kept reference is a column of zeros."""
    gt = np.asarray(gt, dtype=np.int16)
    out = np.zeros((gt.shape[0], len(col_sample)), dtype=np.int16)
    for c, (s, h) in enumerate(zip(col_sample, col_hap)):
        if int(s) != cdefs.NONE_U32:
            out[:, c] = gt[:, int(hap_off[int(s)]) + int(h)]
    return out


def panvcf_filter(ctx, gt):
    """lcty_panvcf_filter: kept[v] = some column of gt[v] has allele >= 1."""
    g = np.ascontiguousarray(gt, dtype=np.int16)
    kept = np.zeros(max(g.shape[0], 1), dtype=np.uint8)
    n = U64()
    check(lib().lcty_panvcf_filter(ctx._h, g.shape[0], g.shape[1], g.ctypes.data, kept.ctypes.data, C.byref(n)))
    return kept[:g.shape[0]].astype(bool)


def _rec_arrays(recs):
    return (np.ascontiguousarray(recs["pos"], dtype=np.uint32), np.ascontiguousarray(recs["ref_len"], dtype=np.uint32),
            np.ascontiguousarray(recs["rec_allele"], dtype=np.uint32), np.ascontiguousarray(recs["allele_off"], dtype=np.uint64),
            np.ascontiguousarray(recs["allele_bytes"], dtype=np.uint8))


def panvcf_reconstruct(ctx, contig, ref_start, ref_end, ref_seq, recs, gt, names, unknown_frac=0.0001, overlaps_allowed=False):
    """lcty_panvcf_reconstruct: recs = the dict of io.Vcf.region (pos, ref_len, rec_allele, allele_off, allele_bytes), gt [n_recs][n_cols] the
    matrix of the retained columns (panvcf_columns). Returns a dict: names, seqs, seq_off, kept_cols, col_unknown, col_len, col_reason,
    total_overlaps, n_kept_records, stats."""
    from .io import _names_blob
    pos, rl, ra, ao, ab = _rec_arrays(recs)
    g = np.ascontiguousarray(gt, dtype=np.int16)
    if g.ndim != 2 or g.shape[0] != len(pos) or g.shape[1] != len(names):
        raise ValueError("gt must be [n_recs][n_cols]")
    ref = np.ascontiguousarray(ref_seq, dtype=np.uint8)
    if len(ref) != ref_end - ref_start:
        raise ValueError("ref_seq must hold ref_end - ref_start bytes")
    o = cdefs.PanvcfOut()
    check(lib().lcty_panvcf_reconstruct(ctx._h, contig.encode(), ref_start, ref_end, ref.ctypes.data, len(pos), pos.ctypes.data, rl.ctypes.data, ra.ctypes.data,
                                        ao.ctypes.data, ab.ctypes.data, g.shape[1], g.ctypes.data, _names_blob(names), unknown_frac, int(overlaps_allowed),
                                        C.byref(o)))
    try:
        arr = _take
        off = arr(o.seq_off, o.n_seqs + 1, np.uint64)
        return {"names": [x.decode() for x in C.string_at(o.names, o.names_len).split(b"\0")[:-1]], "seqs": arr(o.seqs, int(off[-1]), np.uint8),
                "seq_off": off, "kept_cols": arr(o.kept_cols, o.n_seqs, np.uint32), "col_unknown": arr(o.col_unknown, o.n_cols, np.uint32),
                "col_len": arr(o.col_len, o.n_cols, np.uint32), "col_reason": arr(o.col_reason, o.n_cols, np.uint8),
                "total_overlaps": int(o.total_overlaps), "n_kept_records": int(o.n_kept_records), "stats": o.stats.as_dict()}
    finally:
        lib().lcty_panvcf_out_free(C.byref(o))


def db_find_boundary(ctx, start, end, pos, ref_len, k, counts, allowed_expansion, moving_window, left, with_weights=True):
    """lcty_db_find_boundary: (position or None, the final weights [end - start] or None)."""
    p = np.ascontiguousarray(pos, dtype=np.uint32); rl = np.ascontiguousarray(ref_len, dtype=np.uint32)
    cnt = np.ascontiguousarray(counts, dtype=np.uint16)
    w = np.zeros(max(end - start, 1), dtype=np.float64) if with_weights and end > start else None
    found, at = C.c_int32(), U32()
    check(lib().lcty_db_find_boundary(ctx._h, start, end, len(p), p.ctypes.data, rl.ctypes.data, k, cnt.ctypes.data, len(cnt), allowed_expansion, moving_window,
                                      int(left), C.byref(found), C.byref(at), None if w is None else w.ctypes.data))
    return (int(at.value) if found.value else None), (None if w is None else w[:end - start])


DEFAULT_EXPANSIONS = (20_000, 50_000, 200_000)        # add.rs:72


def db_expand_locus(ctx, locus, inner_start, inner_end, contig_len, win_start, win_seq, k, win_counts, pos, ref_len, expansions=DEFAULT_EXPANSIONS,
                    moving_window=500):
    """lcty_db_expand_locus: pos / ref_len = the kept records of the window. Returns the ExpandOut fields as a dict."""
    ws = np.ascontiguousarray(win_seq, dtype=np.uint8); wc = np.ascontiguousarray(win_counts, dtype=np.uint16)
    p = np.ascontiguousarray(pos, dtype=np.uint32); rl = np.ascontiguousarray(ref_len, dtype=np.uint32)
    ex = np.ascontiguousarray(expansions, dtype=np.uint32)
    o = cdefs.ExpandOut()
    check(lib().lcty_db_expand_locus(ctx._h, locus.encode(), inner_start, inner_end, contig_len, win_start, ws.ctypes.data, len(ws), k, wc.ctypes.data, len(wc),
                                     len(p), p.ctypes.data, rl.ctypes.data, len(ex), ex.ctypes.data, moving_window, C.byref(o)))
    return o.as_dict()


def db_locus_from_vcf(ctx, locus, contig, inner_start, inner_end, contig_len, win_start, win_seq, recs, gt, names, k=25, win_counts=None,
                      expansions=DEFAULT_EXPANSIONS, moving_window=500, unknown_frac=0.0001, overlaps_allowed=False, hap_counts=None, hap_cnt_off=None,
                      counter_bytes=2, params=None):
    """lcty_db_locus_from_vcf: expansion, reconstruction, check_sequences, lcty_db_build_locus. recs / gt / names as panvcf_reconstruct, over the
    window. Returns the dict of db_build_locus plus ref_bed (bytes), hap_cols and the stats of the whole step under "locus_stats"."""
    from .io import _names_blob
    pos, rl, ra, ao, ab = _rec_arrays(recs)
    g = np.ascontiguousarray(gt, dtype=np.int16)
    if g.ndim != 2 or g.shape[0] != len(pos) or g.shape[1] != len(names):
        raise ValueError("gt must be [n_recs][n_cols]")
    ws = np.ascontiguousarray(win_seq, dtype=np.uint8)
    wc = None if win_counts is None else np.ascontiguousarray(win_counts, dtype=np.uint16)
    ex = np.ascontiguousarray(expansions, dtype=np.uint32)
    hc = None if hap_counts is None else np.ascontiguousarray(hap_counts, dtype=np.uint16)
    hco = None if hap_cnt_off is None else np.ascontiguousarray(hap_cnt_off, dtype=np.uint64)
    p = params if params is not None else db_params(only_seqs=int(hc is None))
    i = cdefs.LocusVcfIn()
    i.locus, i.contig, i.names = locus.encode(), contig.encode(), _names_blob(names)
    i.inner_start, i.inner_end, i.contig_len, i.win_start = inner_start, inner_end, contig_len, win_start
    i.win_seq, i.win_len = ws.ctypes.data, len(ws)
    i.win_counts, i.n_win_counts = (None, 0) if wc is None else (wc.ctypes.data, len(wc))
    i.k, i.counter_bytes, i.n_recs, i.n_cols = k, counter_bytes, len(pos), g.shape[1]
    i.pos, i.ref_len, i.rec_allele, i.allele_off, i.allele_bytes, i.gt = pos.ctypes.data, rl.ctypes.data, ra.ctypes.data, ao.ctypes.data, ab.ctypes.data, g.ctypes.data
    i.expansions, i.n_expansions, i.moving_window = ex.ctypes.data, len(ex), moving_window
    i.unknown_frac, i.overlaps_allowed = unknown_frac, int(overlaps_allowed)
    i.hap_counts, i.hap_cnt_off = (None if hc is None else hc.ctypes.data), (None if hco is None else hco.ctypes.data)
    o = cdefs.LocusVcfOut()
    check(lib().lcty_db_locus_from_vcf(ctx._h, C.byref(i), C.byref(p), C.byref(o)))
    try:
        f = o.files
        return {
            "fasta": C.string_at(f.fasta, f.fasta_len), "kmers": C.string_at(f.kmers, f.kmers_len),
            "distances": C.string_at(f.distances, f.distances_len), "discarded": C.string_at(f.discarded, f.discarded_len),
            "kept": np.frombuffer(C.string_at(f.kept, 4 * f.n_kept), dtype=np.uint32).copy(), "warn_bits": int(f.warn_bits),
            "stats": f.stats.as_dict(), "ref_bed": C.string_at(o.ref_bed, o.ref_bed_len),
            "hap_cols": np.frombuffer(C.string_at(o.hap_cols, 4 * o.n_hap_cols), dtype=np.uint32).copy(), "locus_stats": o.stats.as_dict(),
        }
    finally:
        lib().lcty_locus_vcf_out_free(C.byref(o))


# ---- basis haplotypes (the basis step of `locityper augment`) ----------------------------------------------------------------------------
def basis_params(**kw):
    """lcty_basis_params_default (divergence 0.01, window 250, step 0 = window / 2, minimal rows, 2 M nodes) with overrides."""
    p = cdefs.BasisParams()
    lib().lcty_basis_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _basis_entries(entries):
    """[(id1 query, id2 target, raw CIGAR words, n_matches, aln_len)] (io.paf_read, SynthLocus.hap_alns) -> the arrays of the C ABI"""
    n = len(entries)
    id1 = np.array([e[0] for e in entries], dtype=np.uint32)
    id2 = np.array([e[1] for e in entries], dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(e[2]) for e in entries], out=off[1:])
    words = np.concatenate([np.asarray(e[2], dtype=np.uint32) for e in entries] + [np.zeros(1, dtype=np.uint32)])
    nm = np.array([e[3] for e in entries], dtype=np.uint32)
    ln = np.array([e[4] for e in entries], dtype=np.uint32)
    return n, id1, id2, nm, ln, off, words


# ---- a locus's haplotypes as a VCF (locityper paf-vcf; lcty_pafvcf.hip) -------------------------------------------------------------
def pafvcf_samples(names, ref_hap, discarded=None):
    """lcty_pafvcf_samples (group_haplotypes): ([(sample, [contig index or None])] sorted by name, ref_id, warning bits). discarded: the
    text of discarded_haplotypes.txt (bytes) or None."""
    from .io import _names_blob
    nb = _names_blob(names)
    disc = None if discarded is None else bytes(discarded)
    ref = ref_hap.encode() if isinstance(ref_hap, str) else bytes(ref_hap)
    ns, nl, nslots, ref_id, warn = U32(), U64(), U32(), U32(), U32()
    args = (len(names), nb, disc, 0 if disc is None else len(disc), ref)
    check(lib().lcty_pafvcf_samples(*args, 0, C.byref(ns), None, 0, C.byref(nl), None, 0, C.byref(nslots), None, C.byref(ref_id), C.byref(warn)))
    blob = np.zeros(max(int(nl.value), 1), dtype=np.uint8)
    off = np.zeros(ns.value + 1, dtype=np.uint32); hap = np.zeros(max(nslots.value, 1), dtype=np.uint32)
    check(lib().lcty_pafvcf_samples(*args, ns.value, C.byref(ns), blob.ctypes.data, len(blob), C.byref(nl), off.ctypes.data, len(hap), C.byref(nslots),
                                    hap.ctypes.data, C.byref(ref_id), C.byref(warn)))
    sn = blob[:int(nl.value)].tobytes().split(b"\0")[:-1]
    groups = [(sn[i], [None if int(h) == cdefs.NONE_U32 else int(h) for h in hap[off[i]:off[i + 1]]]) for i in range(ns.value)]
    return groups, int(ref_id.value), int(warn.value)


def pafvcf_variants(ctx, seqs, seq_off, ref_id, entries):
    """lcty_pafvcf_variants: entries = [(id1 query, id2 target, raw CIGAR words, ...)] (io.paf_read). Returns a dict: var_off, ref_start,
    ref_end, hap_start, hap_end (after the left shift), has_aln, n_missing, n_bad_len, n_shifted."""
    sq, so = _haps(seqs, seq_off)
    n, id1, id2, _nm, _ln, off, words = _basis_entries([(e[0], e[1], e[2], 0, 0) for e in entries]) if entries else \
        (0, np.zeros(1, np.uint32), np.zeros(1, np.uint32), None, None, np.zeros(1, np.uint64), np.zeros(1, np.uint32))
    o = cdefs.PafvcfOut()
    check(lib().lcty_pafvcf_variants(ctx._h, len(so) - 1, sq.ctypes.data, so.ctypes.data, ref_id, n, id1.ctypes.data, id2.ctypes.data, off.ctypes.data,
                                     words.ctypes.data, C.byref(o)))
    try:
        nv = int(o.n_variants)
        out = {k: _take(getattr(o, k), nv, np.uint32) for k in ("ref_start", "ref_end", "hap_start", "hap_end")}
        out.update(var_off=_take(o.var_off, o.n_seqs + 1, np.uint64), has_aln=_take(o.has_aln, o.n_seqs, np.uint8),
                   n_missing=int(o.stats.n_missing), n_bad_len=int(o.stats.n_bad_len), n_shifted=int(o.stats.n_shifted))
        return out
    finally:
        lib().lcty_pafvcf_out_free(C.byref(o))


def pafvcf_ranges(ctx, ref_start, ref_end):
    """lcty_pafvcf_ranges: (unique ranges [n][2], merged ranges [m][2])."""
    rs = np.ascontiguousarray(ref_start, dtype=np.uint32); re_ = np.ascontiguousarray(ref_end, dtype=np.uint32)
    o = cdefs.PafvcfOut()
    check(lib().lcty_pafvcf_ranges(ctx._h, len(rs), rs.ctypes.data, re_.ctypes.data, C.byref(o)))
    try:
        nu, nm = int(o.n_unique), int(o.n_merged)
        return (np.stack([_take(o.unique_start, nu, np.uint32), _take(o.unique_end, nu, np.uint32)], axis=1),
                np.stack([_take(o.merged_start, nm, np.uint32), _take(o.merged_end, nm, np.uint32)], axis=1))
    finally:
        lib().lcty_pafvcf_out_free(C.byref(o))


def pafvcf_table(ctx, seqs, seq_off, ref_id, variants, ranges):
    """lcty_pafvcf_table: variants = the dict of pafvcf_variants, ranges [n][2]. Returns a dict: allele_ix [n_ranges][n_seqs] (-1 = None),
    n_alleles, allele_off, allele_hap, allele_start, allele_len."""
    sq, so = _haps(seqs, seq_off)
    v = {k: np.ascontiguousarray(variants[k], dtype=np.uint32) for k in ("ref_start", "ref_end", "hap_start", "hap_end")}
    vo = np.ascontiguousarray(variants["var_off"], dtype=np.uint64); has = np.ascontiguousarray(variants["has_aln"], dtype=np.uint8)
    rg = np.ascontiguousarray(ranges, dtype=np.uint32).reshape(-1, 2)
    r0, r1 = np.ascontiguousarray(rg[:, 0]), np.ascontiguousarray(rg[:, 1])
    o = cdefs.PafvcfOut()
    check(lib().lcty_pafvcf_table(ctx._h, len(so) - 1, sq.ctypes.data, so.ctypes.data, ref_id, vo.ctypes.data, v["ref_start"].ctypes.data, v["ref_end"].ctypes.data,
                                  v["hap_start"].ctypes.data, v["hap_end"].ctypes.data, has.ctypes.data, len(rg), r0.ctypes.data, r1.ctypes.data, C.byref(o)))
    try:
        nr, ns = int(o.n_ranges), int(o.n_seqs)
        aoff = _take(o.allele_off, nr + 1, np.uint64)
        na = int(aoff[-1]) if nr else 0
        return {"allele_ix": _take(o.allele_ix, nr * ns, np.int32).reshape(nr, ns), "n_alleles": _take(o.n_alleles, nr, np.uint32),
                "allele_off": aoff if nr else np.zeros(1, np.uint64), "allele_hap": _take(o.allele_hap, na, np.uint32),
                "allele_start": _take(o.allele_start, na, np.uint32), "allele_len": _take(o.allele_len, na, np.uint32)}
    finally:
        lib().lcty_pafvcf_out_free(C.byref(o))


def pafvcf_text(ctx, seqs, seq_off, ref_id, ranges, table, groups, chrom, shift=0):
    """lcty_pafvcf_text: the record lines (bytes, no header) of a table (the dict of pafvcf_table) for the samples of pafvcf_samples."""
    sq, so = _haps(seqs, seq_off)
    rg = np.ascontiguousarray(ranges, dtype=np.uint32).reshape(-1, 2)
    r0, r1 = np.ascontiguousarray(rg[:, 0]), np.ascontiguousarray(rg[:, 1])
    ix = np.ascontiguousarray(table["allele_ix"], dtype=np.int32); na = np.ascontiguousarray(table["n_alleles"], dtype=np.uint32)
    ao = np.ascontiguousarray(table["allele_off"], dtype=np.uint64)
    ah, as_, al = (np.ascontiguousarray(table[k], dtype=np.uint32) for k in ("allele_hap", "allele_start", "allele_len"))
    slot_off = np.zeros(len(groups) + 1, dtype=np.uint32)
    np.cumsum([len(g[1]) for g in groups], out=slot_off[1:])
    slot_hap = np.array([cdefs.NONE_U32 if h is None else h for g in groups for h in g[1]] + [0], dtype=np.uint32)
    c = chrom.encode() if isinstance(chrom, str) else bytes(chrom)
    o = cdefs.PafvcfOut()
    check(lib().lcty_pafvcf_text(ctx._h, len(so) - 1, sq.ctypes.data, so.ctypes.data, ref_id, len(rg), r0.ctypes.data, r1.ctypes.data, ix.ctypes.data, na.ctypes.data,
                                 ao.ctypes.data, ah.ctypes.data, as_.ctypes.data, al.ctypes.data, len(groups), slot_off.ctypes.data, slot_hap.ctypes.data, c, shift,
                                 C.byref(o)))
    try:
        return C.string_at(o.merged, o.merged_len) if o.merged_len else b""
    finally:
        lib().lcty_pafvcf_out_free(C.byref(o))


def paf_to_vcf(ctx, names, seqs, seq_off, entries, ref_hap, discarded=None, region=None, with_separate=True):
    """lcty_paf_to_vcf: (merged text, separate text or None, stats dict). region: None or (chrom, start, end)."""
    from .io import _names_blob
    sq, so = _haps(seqs, seq_off)
    n, id1, id2, _nm, _ln, off, words = _basis_entries([(e[0], e[1], e[2], 0, 0) for e in entries]) if entries else \
        (0, np.zeros(1, np.uint32), np.zeros(1, np.uint32), None, None, np.zeros(1, np.uint64), np.zeros(1, np.uint32))
    disc = None if discarded is None else bytes(discarded)
    ref = ref_hap.encode() if isinstance(ref_hap, str) else bytes(ref_hap)
    chrom, start, end = (None, 0, 0) if region is None else region
    if chrom is not None and isinstance(chrom, str):
        chrom = chrom.encode()
    o = cdefs.PafvcfOut()
    check(lib().lcty_paf_to_vcf(ctx._h, len(names), _names_blob(names), sq.ctypes.data, so.ctypes.data, disc, 0 if disc is None else len(disc), ref, n,
                                id1.ctypes.data, id2.ctypes.data, off.ctypes.data, words.ctypes.data, chrom, start, end, int(with_separate), C.byref(o)))
    try:
        return C.string_at(o.merged, o.merged_len), (C.string_at(o.separate, o.separate_len) if with_separate else None), o.stats.as_dict()
    finally:
        lib().lcty_pafvcf_out_free(C.byref(o))


# ---- a cohort's genotypes as a phased VCF (extra/into_vcf.py; lcty_gtvcf.hip) --------------------------------------------------------
def gtvcf_columns(samples, ploidy, genome_name, alleles):
    """lcty_gtvcf_columns (copy_genotype's rule): the column of the GT matrix every predicted allele reads (cdefs.GTVCF_REF: the genome).
    samples, ploidy: the variants file's (Vcf.view)."""
    from .io import _names_blob
    sb = _names_blob(samples)
    pl = np.ascontiguousarray(ploidy, dtype=np.uint32)
    off = np.zeros(len(pl) + 1, dtype=np.uint32)
    np.cumsum(pl, out=off[1:])
    buf = C.create_string_buffer(sb, len(sb) + 1)
    view = cdefs.VcfView(len(pl), int(off[-1]), 0, C.cast(buf, C.c_void_p), len(sb), pl.ctypes.data, off.ctypes.data)
    cols = np.zeros(max(len(alleles), 1), dtype=np.uint32)
    g = genome_name.encode() if isinstance(genome_name, str) else bytes(genome_name)
    check(lib().lcty_gtvcf_columns(C.byref(view), g, len(alleles), _names_blob(alleles), cols.ctypes.data))
    return cols[:len(alleles)]


def gtvcf_fixed_print(value, decimals, pad=False):
    """lcty_gtvcf_fixed_print: a fixed-point value (cdefs.GTVCF_ABSENT: absent) as bytes."""
    n = U64()
    buf = C.create_string_buffer(64)
    check(lib().lcty_gtvcf_fixed_print(int(value), decimals, int(pad), C.cast(buf, C.c_void_p), 64, C.byref(n)))
    return buf.raw[:n.value]


def gtvcf_fixed_parse(text, decimals):
    """lcty_gtvcf_fixed_parse: decimal text -> value x 10^decimals (cdefs.GTVCF_ABSENT for nan / NA)."""
    v = C.c_int64()
    check(lib().lcty_gtvcf_fixed_parse(text.encode() if isinstance(text, str) else bytes(text), decimals, C.byref(v)))
    return int(v.value)


def gtvcf_header(contigs, samples):
    """lcty_gtvcf_header: contigs = [(name, length or None)] -> the header's bytes."""
    from .io import _names_blob
    ln = np.array([0 if l is None else l for _, l in contigs] + [0], dtype=np.uint64)
    cb, sb = _names_blob([c for c, _ in contigs]), _names_blob(samples)
    n = U64()
    check(lib().lcty_gtvcf_header(len(contigs), cb, ln.ctypes.data, len(samples), sb, None, 0, C.byref(n)))
    buf = C.create_string_buffer(int(n.value) + 1)
    check(lib().lcty_gtvcf_header(len(contigs), cb, ln.ctypes.data, len(samples), sb, C.cast(buf, C.c_void_p), n.value, C.byref(n)))
    return buf.raw[:n.value]


def tbi_write(path, contigs, contig_ix, pos, ref_len, line_off, block_off):
    """lcty_tbi_write: the tabix index of a BGZF VCF whose text was cut every 0xff00 bytes (io.bgzf_deflate's block_off)."""
    from .io import _names_blob
    ci, ps, rl = (np.ascontiguousarray(a, dtype=np.uint32) for a in (contig_ix, pos, ref_len))
    lo, bo = np.ascontiguousarray(line_off, dtype=np.uint64), np.ascontiguousarray(block_off, dtype=np.uint64)
    if len(lo) != len(ps) + 1 or len(bo) < 1:
        raise ValueError("line_off has one entry more than the records, block_off at least one")
    check(lib().lcty_tbi_write(str(path).encode(), len(contigs), _names_blob(contigs), len(ps), ci.ctypes.data, ps.ctypes.data, rl.ctypes.data, lo.ctypes.data,
                               bo.ctypes.data, len(bo) - 1))


def res_summary_read(path):
    """lcty_res_summary_read: the top level of a res.json.gz as into_csv.py reads it. A dict: state (cdefs.RES_CALLED / RES_NO_GENOTYPE /
    RES_MISSING), genotype and warnings (bytes or None), qual10, reads, unexpl, wdist5 (int, None when absent)."""
    o = cdefs.ResSummary()
    check(lib().lcty_res_summary_read(str(path).encode(), C.byref(o)))
    try:
        num = {k: (None if getattr(o, k) == cdefs.GTVCF_ABSENT else int(getattr(o, k))) for k in ("qual10", "reads", "unexpl", "wdist5")}
        return dict(state=int(o.state), genotype=C.string_at(o.genotype) if o.genotype else None,
                    warnings=C.string_at(o.warnings) if o.warnings else None, **num)
    finally:
        lib().lcty_res_summary_free(C.byref(o))


def predictions_csv_write(path, rows):
    """lcty_predictions_csv_write: rows = [(sample, locus, summary)], summary a dict of res_summary_read."""
    def b(x):
        return x.encode() if isinstance(x, str) else bytes(x)
    n = len(rows)
    samples = (C.c_char_p * max(n, 1))(*[b(r[0]) for r in rows])
    loci = (C.c_char_p * max(n, 1))(*[b(r[1]) for r in rows])
    arr = (cdefs.ResSummary * max(n, 1))()
    keep = []
    for a, (_, _, s) in zip(arr, rows):
        a.state = s["state"]
        for k in ("qual10", "reads", "unexpl", "wdist5"):
            setattr(a, k, cdefs.GTVCF_ABSENT if s.get(k) is None else s[k])
        for k in ("genotype", "warnings"):
            if s.get(k) is not None:
                keep.append(C.create_string_buffer(b(s[k])))
                setattr(a, k, C.cast(keep[-1], C.c_void_p))
    check(lib().lcty_predictions_csv_write(str(path).encode(), n, C.cast(samples, C.c_void_p), C.cast(loci, C.c_void_p), C.cast(arr, C.c_void_p)))


def predictions_csv_read(path):
    """lcty_predictions_csv_read (load_predictions): a dict of samples (sorted bytewise) and rows = [dict(sample, locus, genotype, warnings,
    qual10, reads, unexpl, wdist5)] in file order; genotype b"*" / b"?" = no prediction."""
    o = cdefs.Predictions()
    check(lib().lcty_predictions_csv_read(str(path).encode(), C.byref(o)))
    try:
        n = int(o.n_rows)
        text = C.string_at(o.text, o.text_len)

        def at(off):
            return text[off:text.index(b"\0", off)]
        cols = {k: _take(getattr(o, k), n, np.uint64) for k in ("sample_off", "locus_off", "genotype_off", "warn_off")}
        nums = {k: _take(getattr(o, k), n, np.int64) for k in ("qual10", "reads", "unexpl", "wdist5")}
        rows = []
        for i in range(n):
            r = dict(sample=at(int(cols["sample_off"][i])), locus=at(int(cols["locus_off"][i])), genotype=at(int(cols["genotype_off"][i])),
                     warnings=at(int(cols["warn_off"][i])))
            r.update({k: (None if int(v[i]) == cdefs.GTVCF_ABSENT else int(v[i])) for k, v in nums.items()})
            rows.append(r)
        return dict(samples=[at(int(x)) for x in _take(o.samples_off, int(o.n_samples), np.uint64)], rows=rows)
    finally:
        lib().lcty_predictions_free(C.byref(o))


class GenotypeVcf:
    """lcty_gtvcf_create / _add_locus / _destroy: the VCF files of a cohort's loci, samples in the order given."""

    def __init__(self, ctx, samples, field_mask=cdefs.GTVCF_ALL):
        from .io import _names_blob
        self._h = C.c_void_p()
        self.ctx, self.n_samples = ctx, len(samples)
        check(lib().lcty_gtvcf_create(ctx._h, _names_blob(samples), len(samples), field_mask, C.byref(self._h)))

    def add_locus(self, chrom, contig_len, recs, gt, preds, ids=None, feats=None, warns=None, want_calls=False, locus=None, contig_ix=0, start=0, end=0):
        """recs: the dict of Vcf.region / VcfIndexed.fetch (pos, ref_len, rec_allele, allele_off, allele_bytes); gt [n_recs][n_haps] int16;
        preds: per sample the columns of gtvcf_columns ([] = no prediction); ids: per record bytes or None; feats: {"qual10" | "reads" |
        "unexpl" | "wdist5": per sample int or None}; warns: per sample bytes; locus (default: a running number), contig_ix, start, end:
        the locus's name and place, for merge(). Returns a dict: text, line_off, calls (want_calls), stats."""
        i = cdefs.GtvcfLocusIn()
        keep = []
        name = ("locus%d" % (getattr(self, "_n_added", 0) + 1)) if locus is None else locus
        i.locus = name.encode() if isinstance(name, str) else bytes(name)
        i.contig_ix, i.start, i.end = contig_ix, start, end

        def arr(a, dtype, pad=1):
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            a = np.concatenate([a, np.zeros(pad, dtype=dtype)]) if pad else a
            keep.append(a)
            return a.ctypes.data

        def csr(items):
            off = np.zeros(len(items) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in items], out=off[1:])
            return off, np.frombuffer(b"".join(bytes(x) for x in items), dtype=np.uint8)

        i.chrom = chrom.encode() if isinstance(chrom, str) else bytes(chrom)
        i.contig_len = int(contig_len or 0)
        pos = np.ascontiguousarray(recs["pos"], dtype=np.uint32)
        g = np.ascontiguousarray(gt, dtype=np.int16)
        if g.ndim != 2:
            g = g.reshape(len(pos), -1) if len(pos) else g.reshape(0, 0)
        if g.shape[0] != len(pos):
            raise ValueError("gt has one row per record")
        i.n_recs, i.n_haps = len(pos), g.shape[1]
        i.pos, i.gt, i.ref_len = arr(pos, np.uint32), arr(g, np.int16), arr(recs["ref_len"], np.uint32)
        i.rec_allele, i.allele_off = arr(recs["rec_allele"], np.uint32, 0), arr(recs["allele_off"], np.uint64, 0)
        i.allele_bytes = arr(recs["allele_bytes"], np.uint8)
        if ids is not None:
            off, b = csr([x or b"" for x in ids])
            i.id_off, i.id_bytes = arr(off, np.uint64, 0), arr(b, np.uint8)
        if len(preds) != self.n_samples:
            raise ValueError("one prediction per sample")
        poff = np.zeros(self.n_samples + 1, dtype=np.uint32)
        np.cumsum([len(p) for p in preds], out=poff[1:])
        i.pred_off = arr(poff, np.uint32, 0)
        i.pred_col = arr([c for p in preds for c in p], np.uint32)
        for key, vals in (feats or {}).items():
            setattr(i, key, arr([cdefs.GTVCF_ABSENT if v is None else v for v in vals], np.int64, 0))
        if warns is not None:
            off, b = csr(warns)
            i.warn_off, i.warn = arr(off, np.uint64, 0), arr(b, np.uint8)
        i.want_calls = int(want_calls)
        o = cdefs.GtvcfOut()
        check(lib().lcty_gtvcf_add_locus(self._h, C.byref(i), C.byref(o)))
        self._n_added = getattr(self, "_n_added", 0) + 1
        try:
            out = {"text": C.string_at(o.text, o.text_len), "line_off": _take(o.line_off, int(o.n_lines) + 1, np.uint64), "stats": o.stats.as_dict()}
            if want_calls:
                out["calls"] = _take(o.calls, int(o.n_lines) * int(o.n_slots), np.int16).reshape(int(o.n_lines), int(o.n_slots))
            return out
        finally:
            lib().lcty_gtvcf_out_free(C.byref(o))

    def merge(self):
        """lcty_gtvcf_merge over the loci added so far: a dict of text, line_off, contigs (names of the header), line_contig (every line's
        place among `contigs`), line_pos, line_ref_len (what tbi_write takes), contig_ix (the variants file's index of every header contig),
        n_joined, stats."""
        o = cdefs.GtvcfOut()
        check(lib().lcty_gtvcf_merge(self._h, C.byref(o)))
        try:
            n = int(o.n_lines)
            return {"text": C.string_at(o.text, o.text_len), "line_off": _take(o.line_off, n + 1, np.uint64), "n_joined": int(o.n_joined),
                    "contigs": C.string_at(o.contigs, o.contigs_len).split(b"\0")[:-1] if o.contigs_len else [],
                    "line_contig": _take(o.line_contig, n, np.uint32), "line_pos": _take(o.line_pos, n, np.uint32),
                    "line_ref_len": _take(o.line_ref_len, n, np.uint32), "contig_ix": _take(o.contig_ix, int(o.n_contigs), np.uint32),
                    "stats": o.stats.as_dict()}
        finally:
            lib().lcty_gtvcf_out_free(C.byref(o))

    def close(self):
        if self._h:
            lib().lcty_gtvcf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


def _leave_out_mask(n_alleles, leave_out):
    if leave_out is None or len(leave_out) == 0:
        return None
    m = np.zeros(n_alleles, dtype=np.uint8)
    m[np.asarray(list(leave_out), dtype=np.int64)] = 1
    return m


def _rows_ints(rows):
    """[n][words] u32 -> Python ints (bit i = haplotype i)"""
    return [int.from_bytes(r.astype("<u4").tobytes(), "little") for r in rows]


def basis_rows_from_ints(n_alleles, ints):
    words = (n_alleles + 31) // 32
    out = np.zeros((len(ints), words), dtype=np.uint32)
    for i, v in enumerate(ints):
        out[i] = np.frombuffer(int(v).to_bytes(4 * words, "little"), dtype="<u4")
    return out


def basis_windows(ctx, lengths, entries, params=None, leave_out=None):
    """lcty_basis_windows: (win_off[n + 1], rows [sum n_windows][ceil(n / 32)] u32, stats dict). leave_out: ids without rows."""
    p = params if params is not None else basis_params()
    lens = np.ascontiguousarray(lengths, dtype=np.uint32)
    n, id1, id2, nm, ln, off, words = _basis_entries(entries)
    mask = _leave_out_mask(len(lens), leave_out)
    win_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    h, st = VP(), cdefs.BasisStats()
    check(lib().lcty_basis_windows(ctx._h, len(lens), lens.ctypes.data, n, id1.ctypes.data, id2.ctypes.data, nm.ctypes.data, ln.ctypes.data,
                                   off.ctypes.data, words.ctypes.data, None if mask is None else mask.ctypes.data, C.byref(p),
                                   win_off.ctypes.data, C.byref(h), C.byref(st)))
    try:
        nw = (len(lens) + 31) // 32
        total = int(win_off[-1]) * nw
        rows = np.frombuffer(C.string_at(h, 4 * total), dtype=np.uint32).copy().reshape(-1, nw) if total else np.zeros((0, nw), dtype=np.uint32)
    finally:
        lib().lcty_io_free(h)
    return win_off, rows, st.as_dict()


def basis_constraints(ctx, n_alleles, rows, minimal=False):
    """lcty_basis_constraints: (the distinct rows in a fixed order — with minimal only those that contain no other row —, stats dict)."""
    r = np.ascontiguousarray(rows, dtype=np.uint32)
    nw = (n_alleles + 31) // 32
    n_out, h, st = U64(), VP(), cdefs.BasisStats()
    check(lib().lcty_basis_constraints(ctx._h, n_alleles, r.size // nw, r.ctypes.data, int(bool(minimal)), C.byref(n_out), C.byref(h), C.byref(st)))
    try:
        total = int(n_out.value) * nw
        out = np.frombuffer(C.string_at(h, 4 * total), dtype=np.uint32).copy().reshape(-1, nw) if total else np.zeros((0, nw), dtype=np.uint32)
    finally:
        lib().lcty_io_free(h)
    return out, st.as_dict()


def basis_select(n_alleles, rows, node_limit=0):
    """lcty_basis_select (host only): (ids ascending, proven lower bound, optimal, nodes)."""
    r = np.ascontiguousarray(rows, dtype=np.uint32)
    nw = (n_alleles + 31) // 32
    ids = np.zeros(max(n_alleles, 1), dtype=np.uint32)
    n_ids, bound, opt, nodes = U32(), U32(), C.c_int32(), U64()
    check(lib().lcty_basis_select(n_alleles, r.size // nw, r.ctypes.data, node_limit, ids.ctypes.data, C.byref(n_ids), C.byref(bound), C.byref(opt),
                                  C.byref(nodes)))
    return ids[:n_ids.value].copy(), int(bound.value), bool(opt.value), int(nodes.value)


def basis_build(ctx, lengths, entries, params=None, leave_out=None):
    """lcty_basis_build: windows -> constraints -> search. (ids ascending, bound, optimal, stats dict)."""
    p = params if params is not None else basis_params()
    lens = np.ascontiguousarray(lengths, dtype=np.uint32)
    n, id1, id2, nm, ln, off, words = _basis_entries(entries)
    mask = _leave_out_mask(len(lens), leave_out)
    ids = np.zeros(len(lens), dtype=np.uint32)
    n_ids, bound, opt, st = U32(), U32(), C.c_int32(), cdefs.BasisStats()
    check(lib().lcty_basis_build(ctx._h, len(lens), lens.ctypes.data, n, id1.ctypes.data, id2.ctypes.data, nm.ctypes.data, ln.ctypes.data,
                                 off.ctypes.data, words.ctypes.data, None if mask is None else mask.ctypes.data, C.byref(p), ids.ctypes.data,
                                 C.byref(n_ids), C.byref(bound), C.byref(opt), C.byref(st)))
    return ids[:n_ids.value].copy(), int(bound.value), bool(opt.value), st.as_dict()


def basis_tag(params=None, leave_out_names=()):
    """lcty_basis_tag (construct_basis_tag): the TAG of haplotypes-basis.TAG.fa.gz."""
    from .io import _names_blob
    p = params if params is not None else basis_params()
    buf = C.create_string_buffer(160)
    check(lib().lcty_basis_tag(C.byref(p), _names_blob(leave_out_names) if leave_out_names else None, len(leave_out_names), buf, len(buf)))
    return buf.value.decode()


def basis_fasta(names, seqs, seq_off, ids):
    """The text of haplotypes-basis.TAG.fa (lcty_fasta_write_text over the chosen haplotypes, in id order; io.write_gz makes the .gz)."""
    from .io import fasta_text
    sq, off = _haps(seqs, seq_off)
    parts = [sq[int(off[i]):int(off[i + 1])] for i in ids]
    o = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in parts], out=o[1:])
    return fasta_text([names[i] for i in ids], np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8), o)


# ---- pairwise haplotype alignments (locityper align --transitive 0; lcty_align.hip) ------------------------------------------------------
def align_params(**kw):
    """lcty_align_params_default (minimizers 15 / 15, thresholds 1.0, backbone ks 25, 51, 101, max_gap 10 000) with overrides;
    backbone_ks takes a sequence."""
    p = cdefs.AlignParams()
    lib().lcty_align_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "backbone_ks":
            ks = list(v)
            if len(ks) > 8:
                raise ValueError("at most 8 backbone ks")
            for i in range(8):
                p.backbone_ks[i] = ks[i] if i < len(ks) else 0
            p.n_backbone_ks = len(ks)
        elif not hasattr(p, k):
            raise AttributeError(k)
        else:
            setattr(p, k, v)
    return p


def align_all_pairs(n_seqs):
    """lcty_align_all_pairs: (ref_id, query_id) in the order rows i, then j > i, with i as the reference (`--all`)."""
    n = max(n_seqs * (n_seqs - 1) // 2, 0)
    r = np.zeros(max(n, 1), dtype=np.uint32); q = np.zeros(max(n, 1), dtype=np.uint32)
    check(lib().lcty_align_all_pairs(n_seqs, r.ctypes.data, q.ctypes.data))
    return r[:n], q[:n]


def align_haplotypes(ctx, seqs, seq_off, ref_id, query_id, params=None, against=None):
    """lcty_align_haplotypes: (dict of per-pair arrays aligned, n_matches, aln_len, nerrs, score, best_k, um, md, cigar_off, cigar;
    stats dict). Pairs in input order; ref_id[i] is the reference and query_id[i] the query of pair i."""
    p = params if params is not None else align_params()
    sq, off = _haps(seqs, seq_off)
    r = np.ascontiguousarray(ref_id, dtype=np.uint32); q = np.ascontiguousarray(query_id, dtype=np.uint32)
    if len(r) != len(q):
        raise ValueError("ref_id and query_id differ in length")
    ag = None if against is None else np.ascontiguousarray(against, dtype=np.uint8)
    o, st = cdefs.AlignOut(), cdefs.AlignStats()
    check(lib().lcty_align_haplotypes(ctx._h, len(off) - 1, sq.ctypes.data, off.ctypes.data, len(r), r.ctypes.data, q.ctypes.data,
                                      None if ag is None else ag.ctypes.data, C.byref(p), C.byref(o), C.byref(st)))
    try:
        n = int(o.n_pairs)
        res = {"aligned": _take(o.aligned, n, np.uint8), "n_matches": _take(o.n_matches, n, np.uint32), "aln_len": _take(o.aln_len, n, np.uint32),
               "nerrs": _take(o.nerrs, n, np.uint32), "score": _take(o.score, n, np.int32), "best_k": _take(o.best_k, n, np.uint32),
               "um": _take(o.um, n, np.uint32), "md": _take(o.md, n, np.float64), "cigar_off": _take(o.cigar_off, n + 1, np.uint64)}
        res["cigar"] = _take(o.cigar, int(res["cigar_off"][-1]), np.uint32)
    finally:
        lib().lcty_align_out_free(C.byref(o))
    return res, st.as_dict()


def align_tr_params(**kw):
    """lcty_align_tr_params_default (transitive_div 0.01, transitive_anchor 101) with overrides."""
    p = cdefs.AlignTrParams()
    lib().lcty_align_tr_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def align_haplotypes_transitive(ctx, seqs, seq_off, ref_id, query_id, params=None, tr_params=None, against=None):
    """lcty_align_haplotypes_transitive (`locityper align --tr-div`): the dict of align_haplotypes plus route (0 skipped, 1 backbone,
    2 / 3 composed through `via` by the first / second clause) and via (2^32 - 1: none); stats dict with the fields of both stats structs."""
    p = params if params is not None else align_params()
    tp = tr_params if tr_params is not None else align_tr_params()
    sq, off = _haps(seqs, seq_off)
    r = np.ascontiguousarray(ref_id, dtype=np.uint32); q = np.ascontiguousarray(query_id, dtype=np.uint32)
    if len(r) != len(q):
        raise ValueError("ref_id and query_id differ in length")
    ag = None if against is None else np.ascontiguousarray(against, dtype=np.uint8)
    o, to, st, ts = cdefs.AlignOut(), cdefs.AlignTrOut(), cdefs.AlignStats(), cdefs.AlignTrStats()
    check(lib().lcty_align_haplotypes_transitive(ctx._h, len(off) - 1, sq.ctypes.data, off.ctypes.data, len(r), r.ctypes.data, q.ctypes.data,
                                                 None if ag is None else ag.ctypes.data, C.byref(p), C.byref(tp), C.byref(o), C.byref(to),
                                                 C.byref(st), C.byref(ts)))
    try:
        n = int(o.n_pairs)
        res = {"aligned": _take(o.aligned, n, np.uint8), "n_matches": _take(o.n_matches, n, np.uint32), "aln_len": _take(o.aln_len, n, np.uint32),
               "nerrs": _take(o.nerrs, n, np.uint32), "score": _take(o.score, n, np.int32), "best_k": _take(o.best_k, n, np.uint32),
               "um": _take(o.um, n, np.uint32), "md": _take(o.md, n, np.float64), "cigar_off": _take(o.cigar_off, n + 1, np.uint64),
               "route": _take(to.route, n, np.uint8), "via": _take(to.via, n, np.uint32)}
        res["cigar"] = _take(o.cigar, int(res["cigar_off"][-1]), np.uint32)
    finally:
        lib().lcty_align_out_free(C.byref(o))
        lib().lcty_align_tr_out_free(C.byref(to))
    return res, {**st.as_dict(), **ts.as_dict()}


def align_backbone(ctx, seqs, seq_off, ref, query, k, params=None):
    """lcty_align_backbone: one pair, one k, every stage: dict of matches [n][2] (pos1, pos2), chain_score, path (match indices),
    cigar (raw words), score, n_dropped; stats dict."""
    p = params if params is not None else align_params()
    sq, off = _haps(seqs, seq_off)
    o, st = cdefs.AlignBackboneOut(), cdefs.AlignStats()
    check(lib().lcty_align_backbone(ctx._h, len(off) - 1, sq.ctypes.data, off.ctypes.data, ref, query, k, C.byref(p), C.byref(o), C.byref(st)))
    try:
        res = {"matches": _take(o.matches, 2 * int(o.n_matches), np.uint32).reshape(-1, 2), "chain_score": int(o.chain_score),
               "path": _take(o.path, int(o.path_len), np.uint32), "cigar": _take(o.cigar, int(o.n_cigar), np.uint32), "score": int(o.score),
               "n_dropped": int(o.n_dropped)}
    finally:
        lib().lcty_align_backbone_out_free(C.byref(o))
    return res, st.as_dict()


# ---- pruning similar haplotypes (locityper prune; lcty_prune.hip) ------------------------------------------------------------------------
def prune_power(power):
    """`--power` as lcty_prune_params.power takes it: "min" / "max" (PowerMean::from_str's names) or an integer -128 .. 127."""
    if isinstance(power, str):
        low = power.lower()
        if low in ("min", "-inf", "neg-inf"):
            return cdefs.PRUNE_POWER_MIN
        if low in ("max", "inf"):
            return cdefs.PRUNE_POWER_MAX
        return 0 if low == "geom" else int(power)
    return int(power)


def prune_params(**kw):
    """lcty_prune_params_default (threshold 0.0002, no n_clusters, power 2) with overrides; power takes prune_power's forms."""
    p = cdefs.PruneParams()
    lib().lcty_prune_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, prune_power(v) if k == "power" else v)
    return p


def _name_array(names):
    return (C.c_char_p * len(names))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])


def paf_divergences(text, names, field=None, repl_missing=0.002):
    """lcty_paf_divergences: (triangle f64 in the order rows i, then j > i; dict n_missing, n_negative, n_conflicting, missing_i, missing_j)."""
    buf = bytes(text)
    n = len(names)
    tri = np.zeros(max(n * (n - 1) // 2, 1), dtype=np.float64)
    st = cdefs.PafDivStats()
    check(lib().lcty_paf_divergences(buf, len(buf), _name_array(names), n, None if field is None else field.encode(), float(repl_missing),
                                     tri.ctypes.data, C.byref(st)))
    return tri[:n * (n - 1) // 2], st.as_dict()


def prune_multiplicities(text, names):
    """lcty_prune_multiplicities: (mult u32[n] = 1 + names the old discarded_haplotypes.txt lists per contig, all_identical)."""
    buf = None if text is None else bytes(text)
    mult = np.zeros(max(len(names), 1), dtype=np.uint32)
    all_id = C.c_int32(1)
    check(lib().lcty_prune_multiplicities(buf, 0 if buf is None else len(buf), _name_array(names), len(names), mult.ctypes.data, C.byref(all_id)))
    return mult[:len(names)], bool(all_id.value)


def _tri(n, tri):
    t = np.ascontiguousarray(tri, dtype=np.float64)
    if len(t) != n * (n - 1) // 2:
        raise ValueError("tri must hold n (n - 1) / 2 values")
    return t if len(t) else np.zeros(1, dtype=np.float64)


def prune_linkage(ctx, n, tri):
    """lcty_prune_linkage: (steps as a structured array cluster1, cluster2, dissimilarity, size; stats dict)."""
    t = _tri(n, tri)
    steps = np.zeros(max(n - 1, 1), dtype=cdefs.PRUNE_STEP_DTYPE)
    st = cdefs.PruneStats()
    check(lib().lcty_prune_linkage(ctx._h, n, t.ctypes.data, steps.ctypes.data, C.byref(st)))
    return steps[:n - 1], st.as_dict()


def _prune_out_dict(o):
    n, nc = int(o.n), int(o.n_clusters)
    steps = np.frombuffer(C.string_at(o.steps, cdefs.PRUNE_STEP_DTYPE.itemsize * (n - 1)), dtype=cdefs.PRUNE_STEP_DTYPE).copy() if n > 1 \
        else np.zeros(0, dtype=cdefs.PRUNE_STEP_DTYPE)
    off = _take(o.cluster_off, nc + 1, np.uint32)
    members, acc = _take(o.members, n, np.uint32), _take(o.acc, n, np.float64)
    return {"steps": steps, "threshold": float(o.threshold), "epsilon": float(o.epsilon), "keep_ids": _take(o.keep_ids, nc, np.uint32),
            "clusters": [members[int(off[k]):int(off[k + 1])] for k in range(nc)], "acc": [acc[int(off[k]):int(off[k + 1])] for k in range(nc)],
            "repr": _take(o.repr, nc, np.uint32), "stats": o.stats.as_dict()}


def prune_cluster(ctx, n, tri, mult=None, params=None, names=None, old_discarded=None):
    """lcty_prune_cluster: dict of steps, threshold, epsilon, keep_ids (sorted), clusters (member arrays in the reference's order), acc
    (the accumulators beside them), repr, stats. With names also newick and discarded (lcty_prune_texts on the same result)."""
    p = params if params is not None else prune_params()
    t = _tri(n, tri)
    m = None if mult is None else np.ascontiguousarray(mult, dtype=np.uint32)
    o = cdefs.PruneOut()
    check(lib().lcty_prune_cluster(ctx._h, n, t.ctypes.data, None if m is None else m.ctypes.data, C.byref(p), C.byref(o)))
    try:
        res = _prune_out_dict(o)
        if names is not None:
            res["newick"], res["discarded"] = _prune_texts(names, old_discarded, o)
    finally:
        lib().lcty_prune_out_free(C.byref(o))
    return res


def _prune_texts(names, old_discarded, o):
    from .io import _names_blob
    old = None if old_discarded is None else bytes(old_discarded)
    a, al, b, bl = VP(), U64(), VP(), U64()
    check(lib().lcty_prune_texts(len(names), _names_blob(names), old, 0 if old is None else len(old), C.byref(o), C.byref(a), C.byref(al),
                                 C.byref(b), C.byref(bl)))
    try:
        return C.string_at(a, al.value), C.string_at(b, bl.value)
    finally:
        lib().lcty_io_free(a)
        lib().lcty_io_free(b)


def prune_texts(names, steps, clusters, reprs, old_discarded=None):
    """lcty_prune_texts (host only) on a result given as arrays: (Newick text, discarded_haplotypes.txt text)."""
    n = len(names)
    st = np.ascontiguousarray(steps, dtype=cdefs.PRUNE_STEP_DTYPE)
    off = np.zeros(len(clusters) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c) for c in clusters])
    mem = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint32) for c in clusters]), dtype=np.uint32)
    rp = np.ascontiguousarray(reprs, dtype=np.uint32)
    o = cdefs.PruneOut()
    o.n, o.n_clusters = n, len(clusters)
    o.steps, o.cluster_off, o.members, o.repr = st.ctypes.data if len(st) else None, off.ctypes.data, mem.ctypes.data, rp.ctypes.data
    return _prune_texts(names, old_discarded, o)


def db_prune_locus(ctx, names, seqs, seq_off, paf, kmers=None, distances=None, discarded=None, field=None, params=None):
    """lcty_db_prune_locus: process_locus + prune_files on the decompressed contents of a locus directory. Returns a dict: newick,
    discarded, fasta, kmers, distances, paf (bytes), keep, unchanged, warn_bits, threshold, div, stats."""
    from .io import _names_blob
    p = params if params is not None else prune_params()
    sq, off = _haps(seqs, seq_off)
    b = lambda x: None if x is None else bytes(x)
    paf, kmers, distances, discarded = b(paf), b(kmers), b(distances), b(discarded)
    ln = lambda x: 0 if x is None else len(x)
    f = cdefs.PruneFiles()
    check(lib().lcty_db_prune_locus(ctx._h, len(off) - 1, _names_blob(names), sq.ctypes.data, off.ctypes.data, paf, ln(paf), kmers, ln(kmers),
                                    distances, ln(distances), discarded, ln(discarded), None if field is None else field.encode(), C.byref(p),
                                    C.byref(f)))
    try:
        return _prune_files_dict(f)
    finally:
        lib().lcty_prune_files_free(C.byref(f))


def _bytes_at(p, n):
    return C.string_at(p, n) if p and n else b""


def _prune_files_dict(f):
    return {"newick": _bytes_at(f.newick, f.newick_len), "discarded": _bytes_at(f.discarded, f.discarded_len),
            "fasta": _bytes_at(f.fasta, f.fasta_len), "kmers": _bytes_at(f.kmers, f.kmers_len),
            "distances": _bytes_at(f.distances, f.distances_len), "paf": _bytes_at(f.paf, f.paf_len),
            "keep": _take(f.keep, int(f.n_keep), np.uint32), "unchanged": bool(f.unchanged), "warn_bits": int(f.warn_bits),
            "threshold": float(f.threshold), "div": f.div.as_dict(), "stats": f.stats.as_dict()}


def prune_thin(names, seqs, seq_off, paf, keep, kmers=None, distances=None):
    """lcty_prune_thin (host only): the files of the kept haplotypes; the dict of db_prune_locus with fasta, kmers, distances, paf filled."""
    from .io import _names_blob
    sq, off = _haps(seqs, seq_off)
    b = lambda x: None if x is None else bytes(x)
    paf, kmers, distances = b(paf), b(kmers), b(distances)
    ln = lambda x: 0 if x is None else len(x)
    kp = np.ascontiguousarray(keep, dtype=np.uint32)
    f = cdefs.PruneFiles()
    check(lib().lcty_prune_thin(len(off) - 1, _names_blob(names), sq.ctypes.data, off.ctypes.data, paf, ln(paf), kmers, ln(kmers), distances,
                                ln(distances), kp.ctypes.data, len(kp), C.byref(f)))
    try:
        return _prune_files_dict(f)
    finally:
        lib().lcty_prune_files_free(C.byref(f))


# ---- a resident genome: k-mer counts and reference windows (lcty_genome.hip) ---------------------------------------------------------
class Genome:
    """JfKmerGetter (src/seq/counts.rs:258-369) without a Jellyfish database, and seq::fetch_seq: the genome packed on the device."""

    def __init__(self, ctx):
        self._ctx = ctx
        self._h = VP()
        check(lib().lcty_genome_create(ctx._h, C.byref(self._h)))

    @classmethod
    def from_fasta(cls, ctx, path):
        g = cls.__new__(cls)
        g._ctx, g._h = ctx, VP()
        check(lib().lcty_genome_load_fasta(ctx._h, str(path).encode(), C.byref(g._h)))
        return g

    def append(self, name, bases, continues=False):
        """One contig, or (continues) the next piece of the contig that is open. bases: bytes or a u8 array of ASCII."""
        b = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, dtype=np.uint8)
        check(lib().lcty_genome_append(self._h, None if name is None else name.encode(), b.ctypes.data if len(b) else None, len(b), int(continues)))

    def contigs(self):
        """[(name, length)] in order."""
        n, nb = U32(), U64()
        check(lib().lcty_genome_info(self._h, C.byref(n), C.byref(nb)))
        out = []
        buf = C.create_string_buffer(1 << 16)
        for i in range(n.value):
            ln = U64()
            check(lib().lcty_genome_contig(self._h, i, buf, len(buf), C.byref(ln)))
            out.append((buf.value.decode(), int(ln.value)))
        return out

    def n_bases(self):
        nb = U64()
        check(lib().lcty_genome_info(self._h, None, C.byref(nb)))
        return int(nb.value)

    def fetch(self, contig, start, end):
        """The window [start, end) of a contig as bytes: capitals A C G T, N for everything else."""
        out = np.zeros(max(int(end) - int(start), 1), dtype=np.uint8)
        check(lib().lcty_genome_fetch(self._h, contig.encode(), int(start), int(end), out.ctypes.data))
        return out[:int(end) - int(start)].tobytes()

    def kmer_counts(self, seqs, off, k, counter_bytes=2):
        """JfKmerGetter::fetch: (counts u16, cnt_off u64[n + 1], stats dict) for the sequences seqs[off[i]:off[i + 1]]."""
        sq, so = _haps(seqs, off)
        n = len(so) - 1
        n_values = int(sum(max(int(so[i + 1] - so[i]) + 1 - int(k), 0) for i in range(n)))
        counts = np.zeros(max(n_values, 1), dtype=np.uint16)
        cnt_off = np.zeros(n + 1, dtype=np.uint64)
        st = cdefs.GenomeCountStats()
        check(lib().lcty_genome_kmer_counts(self._h, k, counter_bytes, n, sq.ctypes.data, so.ctypes.data, counts.ctypes.data, cnt_off.ctypes.data,
                                            C.byref(st)))
        return counts[:n_values], cnt_off, st.as_dict()

    def close(self):
        if self._h:
            lib().lcty_genome_destroy(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
