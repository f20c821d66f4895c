"""ctypes wrappers of the file-format entry points of liblocityper_hip.so (lcty_io.hip): harness code for tests, bench and examples."""
import ctypes as C
import os
import time

import numpy as np

from . import cdefs
from ._lib import lib, check, VP, U32, U64, D


def read_file(path):
    """lcty_io_read_file: the bytes of a file with its .gz / .lz4 / .br container removed."""
    data, n = VP(), U64()
    check(lib().lcty_io_read_file(str(path).encode(), C.byref(data), C.byref(n)))
    try:
        return C.string_at(data, n.value)
    finally:
        lib().lcty_io_free(data)


def write_gz(path, data):
    buf = bytes(data)
    check(lib().lcty_io_write_gz(str(path).encode(), buf, len(buf)))


def write_bgzf(path, data):
    """lcty_io_write_bgzf: `data` as a BGZF file (blocks of at most 0xff00 bytes and the end-of-file block)."""
    buf = bytes(data)
    check(lib().lcty_io_write_bgzf(str(path).encode(), buf, len(buf)))


def write_br(path, data, quality=5):
    """lcty_io_write_br: a brotli stream of `data` (the reference's `.csv.br` debug tables); returns True when the stream is STORED in
    uncompressed meta-blocks (no libbrotlienc on this system, or quality < 0)."""
    buf = bytes(data)
    stored = C.c_int32(0)
    check(lib().lcty_io_write_br(str(path).encode(), buf, len(buf), quality, C.byref(stored)))
    return bool(stored.value)


def distances_parse(data, n_alleles):
    """lcty_distances_parse: distances.bin -> (k, w, symmetric u32 matrix, NONE_U32 on the diagonal)."""
    buf = bytes(data)
    k, w = U32(), U32()
    dist = np.zeros((n_alleles, n_alleles), dtype=np.uint32)
    check(lib().lcty_distances_parse(buf, len(buf), n_alleles, C.byref(k), C.byref(w), dist.ctypes.data))
    return int(k.value), int(w.value), dist


def _sized(call):
    need = U64(0)
    check(call(None, 0, C.byref(need)))
    buf = np.zeros(max(int(need.value), 1), dtype=np.uint8)
    check(call(buf.ctypes.data, len(buf), C.byref(need)))
    return buf[:int(need.value)].tobytes()


def _names_blob(names):
    return b"".join((n.encode() if isinstance(n, str) else bytes(n)) + b"\0" for n in names)


def kmer_counts_write(k, counter_bytes, cnt_off, counts):
    """lcty_kmer_counts_write (KmerCounts::save): one block of `kmers.bin`."""
    off = np.ascontiguousarray(cnt_off, dtype=np.uint64)
    cnt = np.ascontiguousarray(counts, dtype=np.uint16)
    return _sized(lambda o, c, n: lib().lcty_kmer_counts_write(k, counter_bytes, len(off) - 1, off.ctypes.data, cnt.ctypes.data, o, c, n))


def distances_write(k, w, n_alleles, uniq):
    """lcty_distances_write (write_divergences): the bytes of `distances.bin` from the triangle of non-shared minimizers."""
    u = np.ascontiguousarray(uniq, dtype=np.uint32)
    if len(u) != n_alleles * (n_alleles - 1) // 2:
        raise ValueError("uniq must hold n (n - 1) / 2 values")
    return _sized(lambda o, c, n: lib().lcty_distances_write(k, w, n_alleles, u.ctypes.data, o, c, n))


def fasta_text(names, seqs, seq_off):
    """lcty_fasta_write_text (write_multiline_fasta): the text of `haplotypes.fa` (write_gz makes the .gz)."""
    sq = np.ascontiguousarray(seqs, dtype=np.uint8)
    off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    blob = _names_blob(names)
    return _sized(lambda o, c, n: lib().lcty_fasta_write_text(len(off) - 1, blob, sq.ctypes.data, off.ctypes.data, o, c, n))


def fasta_read(path):
    """lcty_fasta_read: (names, upper-cased sequences concatenated as u8, seq_off[n + 1])."""
    n, nl, sl = U32(), U64(), U64()
    check(lib().lcty_fasta_read(str(path).encode(), C.byref(n), None, C.byref(nl), None, C.byref(sl), None))
    names = np.zeros(max(int(nl.value), 1), dtype=np.uint8)
    seqs = np.zeros(max(int(sl.value), 1), dtype=np.uint8)
    off = np.zeros(n.value + 1, dtype=np.uint64)
    check(lib().lcty_fasta_read(str(path).encode(), C.byref(n), names.ctypes.data, C.byref(nl), seqs.ctypes.data, C.byref(sl), off.ctypes.data))
    return [x.decode() for x in names[:int(nl.value)].tobytes().split(b"\0")[:n.value]], seqs[:int(sl.value)], off


def paf_read(path, names, with_distances=False):
    """lcty_paf_read: haplotypes.paf[.gz|.br|.lz4] -> [(id1 query, id2 target, raw CIGAR words, n_matches, aln_len)] in file order,
    the list Locus.set_hap_alns takes. names: the contig names of the locus in id order."""
    arr = (C.c_char_p * len(names))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])
    ne, nc = U64(0), U64(0)
    check(lib().lcty_paf_read(str(path).encode(), arr, len(names), C.byref(ne), None, None, None, None, None, None, C.byref(nc), None))
    n, w = int(ne.value), int(nc.value)
    id1 = np.zeros(max(n, 1), dtype=np.uint32); id2 = np.zeros(max(n, 1), dtype=np.uint32)
    nm = np.zeros(max(n, 1), dtype=np.uint32); al = np.zeros(max(n, 1), dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64); words = np.zeros(max(w, 1), dtype=np.uint32)
    dist = np.zeros((len(names), len(names)), dtype=np.uint32)
    check(lib().lcty_paf_read(str(path).encode(), arr, len(names), C.byref(ne), id1.ctypes.data, id2.ctypes.data, nm.ctypes.data, al.ctypes.data,
                              off.ctypes.data, words.ctypes.data, C.byref(nc), dist.ctypes.data if with_distances else None))
    ents = [(int(id1[t]), int(id2[t]), words[int(off[t]):int(off[t + 1])].copy(), int(nm[t]), int(al[t])) for t in range(n)]
    return (ents, dist) if with_distances else ents


def paf_write(names, seq_off, ref_id, query_id, res, params=None):
    """lcty_paf_write_text: the text of `haplotypes.paf` from the result dict of api.align_haplotypes (write_gz makes the .gz)."""
    from . import api
    p = params if params is not None else api.align_params()
    off = np.ascontiguousarray(seq_off, dtype=np.uint64)
    r = np.ascontiguousarray(ref_id, dtype=np.uint32); q = np.ascontiguousarray(query_id, dtype=np.uint32)
    keep = {k: np.ascontiguousarray(res[k]) for k in ("aligned", "n_matches", "aln_len", "nerrs", "score", "best_k", "um", "md", "cigar_off")}
    keep["cigar"] = np.ascontiguousarray(np.concatenate([res["cigar"], np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)
    o = cdefs.AlignOut()
    o.n_pairs = len(r)
    for k, a in keep.items():
        setattr(o, k, a.ctypes.data)
    blob = _names_blob(names)
    return _sized(lambda b, c, n: lib().lcty_paf_write_text(C.byref(p), len(off) - 1, blob, off.ctypes.data, len(r), r.ctypes.data, q.ctypes.data,
                                                            C.byref(o), b, c, n))


def bg_from_json(text):
    """BgDistr::load -> (Bg, mean read length)."""
    if isinstance(text, str):
        text = text.encode()
    bg, rl = cdefs.Bg(), D()
    check(lib().lcty_bg_from_json(text, len(text), C.byref(bg), C.byref(rl)))
    return bg, float(rl.value)


def bg_to_json(bg, read_len, ploidy=2):
    """BgDistr::save as text (lcty_bg_to_json): the content of PREPROC/distr.gz."""
    need = U64()
    check(lib().lcty_bg_to_json(C.byref(bg), float(read_len), int(ploidy), None, 0, C.byref(need)))
    buf = C.create_string_buffer(int(need.value))
    check(lib().lcty_bg_to_json(C.byref(bg), float(read_len), int(ploidy), buf, need.value, C.byref(need)))
    return buf.value.decode()


def res_to_json(call, genotypes, names, lik_mean, lik_var, distances=None, true_edit=False, weighted_dist=float("nan")):
    """Genotyping::to_json as text. genotypes[n_out][ploidy], lik_mean / lik_var[n_out] (natural log), in call.ixs order."""
    gt = np.ascontiguousarray(genotypes, dtype=np.uint16)
    n_out, ploidy = gt.shape
    assert n_out == int(call.n_out)
    nm = (C.c_char_p * len(names))(*[s.encode() for s in names])
    lm = np.ascontiguousarray(lik_mean, dtype=np.float64); lv = np.ascontiguousarray(lik_var, dtype=np.float64)
    dist = None if distances is None else np.ascontiguousarray(distances, dtype=np.uint32)
    need = U64()
    args = (C.byref(call), gt.ctypes.data, ploidy, nm, len(names), lm.ctypes.data, lv.ctypes.data,
            None if dist is None else dist.ctypes.data, int(true_edit), float(weighted_dist))
    check(lib().lcty_res_to_json(*args, None, 0, C.byref(need)))
    buf = C.create_string_buffer(int(need.value))
    check(lib().lcty_res_to_json(*args, buf, need.value, C.byref(need)))
    return buf.value.decode()


def write_bam(path, aa, chunk, names, allele_names, genotype, attempts, read_off, counts, quals=None):
    """lcty_write_bam: the alignments of the batch `aa` (scored from `chunk`) to one genotype, with the assignment counts of
    api.assignment_counts for that genotype. names: one per read pair; quals: list of bytes per mate or None. Returns the records written."""
    hs = chunk.host_struct()
    blob = "".join(names).encode()
    noff = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(n.encode()) for n in names], out=noff[1:])
    qoff = qbuf = None
    if quals is not None:
        qoff = np.zeros(len(quals) + 1, dtype=np.uint64)
        np.cumsum([len(q) for q in quals], out=qoff[1:])
        qbuf = np.frombuffer(b"".join(quals), dtype=np.uint8).copy()
    an = (C.c_char_p * len(allele_names))(*[s.encode() for s in allele_names])
    gt = np.ascontiguousarray(genotype, dtype=np.uint16)
    ro = np.ascontiguousarray(read_off, dtype=np.uint64); cn = np.ascontiguousarray(counts, dtype=np.uint16)
    n = U64()
    check(lib().lcty_write_bam(str(path).encode(), aa._h, C.byref(hs), noff.ctypes.data, blob, None if qoff is None else qoff.ctypes.data,
                               None if qbuf is None else qbuf.ctypes.data, an, gt.ctypes.data, len(gt), attempts, ro.ctypes.data,
                               cn.ctypes.data, C.byref(n)))
    return int(n.value)


class BamTable:
    """lcty_bam_read: aln.bam as a ReadsChunk (+ read names). ctx: the device route (lcty_bam_read_device) — the arrays are also
    resident on the context's device, AllAlignments.append_bam appends them from there; with host_copy=False only the per-pair
    arrays come back: no chunk, no quals(), but sizes(), names and append_bam."""

    def __init__(self, path, names, paired=True, ctx=None, host_copy=True):
        self._h = VP()
        nm = (C.c_char_p * len(names))(*[s.encode() for s in names])
        self.ctx, self.host_copy, self.stats = ctx, bool(host_copy) or ctx is None, None
        t0 = time.perf_counter()
        if ctx is None:
            check(lib().lcty_bam_read(str(path).encode(), nm, len(names), int(paired), C.byref(self._h)))
        else:
            st = cdefs.AlnBamStats()
            check(lib().lcty_bam_read_device(ctx._h, str(path).encode(), nm, len(names), int(paired), int(bool(host_copy)), C.byref(self._h), C.byref(st)))
            self.stats = st.as_dict()
        self.ms_native = 1e3 * (time.perf_counter() - t0)           # the library call alone, without the copies into numpy arrays below
        self.n_pairs, self.n_bases, self.n_recs, self.n_cigar, self.n_refs = self.sizes()
        self.view = self.chunk = self.names = None
        if self.host_copy:
            self._load_view()

    def sizes(self):
        """lcty_bam_table_sizes: (pairs, bases, records, CIGAR words, references of the header) — what AllAlignments needs."""
        a, b, c, d, r = U64(), U64(), U64(), U64(), U32()
        check(lib().lcty_bam_table_sizes(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(r)))
        return int(a.value), int(b.value), int(c.value), int(d.value), int(r.value)

    def quals(self):
        """lcty_bam_table_quals: (qual_off[2 n_pairs + 1], quals as stored, MAPQ per record)."""
        qo, q, mq = VP(), VP(), VP()
        check(lib().lcty_bam_table_quals(self._h, C.byref(qo), C.byref(q), C.byref(mq)))
        n = self.n_pairs

        def arr(p, count, dt):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (count,)).copy() if count else np.zeros(0, dtype=dt)
        qual_off = arr(qo, 2 * n + 1, C.c_uint64)
        return qual_off, arr(q, int(qual_off[-1]), C.c_uint8), arr(mq, self.n_recs, C.c_uint8)

    def _load_view(self):
        view = cdefs.ReadsHost()
        noff, blob, nref = VP(), VP(), U32()
        check(lib().lcty_bam_table_view(self._h, C.byref(view), C.byref(noff), C.byref(blob), C.byref(nref)))
        self.view, self.n_refs = view, int(nref.value)
        n = int(view.n_pairs)
        self.n_pairs = n

        def arr(p, count, dt):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (count,)).copy() if count else np.zeros(0, dtype=dt)
        mate_off = arr(view.mate_off, 2 * n + 1, C.c_uint64)
        aln_off = arr(view.aln_off, n + 1, C.c_uint64)
        cigar_off = arr(view.cigar_off, n + 1, C.c_uint64)
        n_bases = int(mate_off[-1]) if n else 0
        recs = np.frombuffer(C.string_at(view.recs, 16 * int(aln_off[-1])), dtype=cdefs.ALN_REC_DTYPE).copy() if n else np.zeros(0, dtype=cdefs.ALN_REC_DTYPE)
        self.chunk = cdefs.ReadsChunk(arr(view.mate_len, 2 * n, C.c_uint32), mate_off, arr(view.bases2, max((n_bases + 15) // 16, 2), C.c_uint32),
                                      arr(view.nmask, max((n_bases + 31) // 32, 1), C.c_uint32), aln_off, recs, cigar_off,
                                      arr(view.cigar, int(cigar_off[-1]) if n else 0, C.c_uint32))
        no = arr(noff, n + 1, C.c_uint64)
        raw = C.string_at(blob, int(no[-1])) if n else b""
        self.names = [raw[int(no[i]):int(no[i + 1])].decode() for i in range(n)]

    def close(self):
        if self._h:
            lib().lcty_bam_table_free(self._h)
            self._h = VP()

    def __del__(self):
        self.close()


class Fastx:
    """lcty_fastx_*: FASTA / FASTQ input for recruitment (src/seq/fastx.rs readers) and the per-locus writers behind it."""

    def __init__(self, path1, path2=None, interleaved=False):
        self._h = VP()
        check(lib().lcty_fastx_open(str(path1).encode(), None if path2 is None else str(path2).encode(), int(interleaved), C.byref(self._h)))
        p = C.c_int32(0)
        check(lib().lcty_fastx_is_paired(self._h, C.byref(p)))
        self.paired = bool(p.value)

    def next(self, max_records):
        """The next chunk as a cdefs.ReadsChunk of sequence fields (views into the handle: valid until the next call), or None."""
        hs = cdefs.ReadsHost()
        n = U64(0)
        check(lib().lcty_fastx_next(self._h, max_records, C.byref(hs), C.byref(n)))
        n = int(n.value)
        if n == 0:
            return None
        def arr(ptr, count, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(count,))
        mate_off = arr(hs.mate_off, 2 * n + 1, C.c_uint64)
        nb = int(mate_off[-1])
        z = np.zeros(n + 1, dtype=np.uint64)
        return cdefs.ReadsChunk(arr(hs.mate_len, 2 * n, C.c_uint32), mate_off, arr(hs.bases2, nb // 16 + 1, C.c_uint32),
                                arr(hs.nmask, nb // 32 + 1, C.c_uint32), z, np.zeros(0, dtype=cdefs.ALN_REC_DTYPE), z, np.zeros(0, dtype=np.uint32))

    def write_recruited(self, writers, cnt, loci):
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        loci = np.ascontiguousarray(loci, dtype=np.uint32)
        n = U64(0)
        check(lib().lcty_fastx_write_recruited(self._h, writers._h, loci.shape[1], cnt.ctypes.data, loci.ctypes.data, C.byref(n)))
        return int(n.value)

    def close(self):
        if self._h:
            lib().lcty_fastx_close(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastxDevice:
    """lcty_fastx_device_*: the same input as Fastx, parsed and packed on the device. Windows of text follow the context's
    knob "fastx_window_bytes"; stats holds the sums of lcty_fastx_device_stats after every call of next()."""

    def __init__(self, ctx, path1, path2=None, interleaved=False):
        self._h = VP()
        self._ctx = ctx
        self.stats = cdefs.FastxDeviceStats().as_dict()
        self.n = 0
        check(lib().lcty_fastx_device_open(ctx._h, str(path1).encode(), None if path2 is None else str(path2).encode(), int(interleaved), C.byref(self._h)))
        p = C.c_int32(0)
        check(lib().lcty_fastx_device_is_paired(self._h, C.byref(p)))
        self.paired = bool(p.value)

    def next(self, max_records=2 ** 62):
        """The next chunk stays on the device: -> its number of records (pairs, when paired), 0 at the end of the input."""
        n, st = U64(0), cdefs.FastxDeviceStats()
        self.n = 0
        try:
            check(lib().lcty_fastx_device_next(self._h, max_records, C.byref(n), C.byref(st)))
        finally:
            self.stats = st.as_dict()
        self.n = int(n.value)
        return self.n

    def view(self):
        """The current chunk as a cdefs.ReadsChunk of sequence fields, as Fastx.next gives it: copies."""
        hs = cdefs.ReadsHost()
        check(lib().lcty_fastx_device_view(self._h, C.byref(hs)))
        n = int(hs.n_pairs)
        def arr(ptr, count, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(count,)).copy()
        mate_off = arr(hs.mate_off, 2 * n + 1, C.c_uint64)
        nb = int(mate_off[-1])
        z = np.zeros(n + 1, dtype=np.uint64)
        return cdefs.ReadsChunk(arr(hs.mate_len, 2 * n, C.c_uint32) if n else np.zeros(0, dtype=np.uint32), mate_off, arr(hs.bases2, nb // 16 + 1, C.c_uint32),
                                arr(hs.nmask, nb // 32 + 1, C.c_uint32), z, np.zeros(0, dtype=cdefs.ALN_REC_DTYPE), z, np.zeros(0, dtype=np.uint32))

    def recruit(self, targets, max_out=8):
        n = self.n
        cnt = np.zeros(max(n, 1), dtype=np.uint32); loci = np.zeros(max(n, 1) * max_out, dtype=np.uint32)
        check(lib().lcty_fastx_device_recruit(targets._h, self._h, max_out, cnt.ctypes.data, loci.ctypes.data))
        return cnt[:n], loci.reshape(-1, max_out)[:n]

    def write_recruited(self, writers, cnt, loci):
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        loci = np.ascontiguousarray(loci, dtype=np.uint32)
        n = U64(0)
        check(lib().lcty_fastx_device_write_recruited(self._h, writers._h, loci.shape[1], cnt.ctypes.data, loci.ctypes.data, C.byref(n)))
        return int(n.value)

    def add_recruited(self, rset, cnt, loci):
        """lcty_recruited_add_fastx: the current chunk into an api.Recruited set, device to device."""
        rset.add_fastx(self, cnt, loci)

    def close(self):
        if self._h:
            lib().lcty_fastx_device_close(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fetch_regions(tid, start, end, contig_len, padding, alt_contig_len=10_000_000, merge_distance=1000):
    """lcty_recruit_fetch_regions (postprocess_targets): padded, short contigs added, sorted, merged -> (tid, start, end) arrays."""
    tid, start, end = (np.ascontiguousarray(a, dtype=np.uint32) for a in (tid, start, end))
    contig_len = np.ascontiguousarray(contig_len, dtype=np.uint32)
    cap = len(tid) + len(contig_len)
    out = [np.zeros(max(cap, 1), dtype=np.uint32) for _ in range(3)]
    n = U32(0)
    check(lib().lcty_recruit_fetch_regions(len(tid), tid.ctypes.data, start.ctypes.data, end.ctypes.data, len(contig_len), contig_len.ctypes.data,
                                           padding, alt_contig_len, merge_distance, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, C.byref(n)))
    return tuple(a[:n.value].copy() for a in out)


def _regions(regions):
    r = np.asarray(list(regions), dtype=np.uint32).reshape(-1, 3)
    return tuple(np.ascontiguousarray(r[:, j]) for j in range(3))


def bgzf_inflate(ctx, comp, out=None, size_only=False):
    """lcty_bgzf_inflate: whole BGZF blocks back to back (bytes or a uint8 array) -> (the inflated bytes as a uint8 array, stats).
    size_only: -> the inflated size, nothing is inflated. out: a uint8 array to inflate into (its size is the capacity given)."""
    buf = np.frombuffer(comp, dtype=np.uint8) if isinstance(comp, (bytes, bytearray, memoryview)) else np.ascontiguousarray(comp, dtype=np.uint8)
    n = U64(0)
    check(lib().lcty_bgzf_inflate(ctx._h, buf.ctypes.data if len(buf) else None, len(buf), None, 0, C.byref(n), None))
    if size_only:
        return int(n.value)
    if out is None:
        out = np.empty(int(n.value), dtype=np.uint8)
    st = cdefs.BgzfStats()
    check(lib().lcty_bgzf_inflate(ctx._h, buf.ctypes.data if len(buf) else None, len(buf), out.ctypes.data if len(out) else None, len(out), C.byref(n), C.byref(st)))
    return out[:int(n.value)], st.as_dict()


def bgzf_deflate(ctx, data, with_eof=True, out_cap=None):
    """lcty_bgzf_deflate: bytes or a uint8 array -> (the BGZF file's bytes as a uint8 array, block_off: the offset of every data block and
    the end of the last, stats). out_cap: the capacity given instead of lcty_bgzf_deflate_bound."""
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    cap = int(lib().lcty_bgzf_deflate_bound(len(buf), 1 if with_eof else 0)) if out_cap is None else int(out_cap)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    off = np.zeros((len(buf) + 0xff00 - 1) // 0xff00 + 1, dtype=np.uint64)
    n = U64(0)
    st = cdefs.BgzfDeflateStats()
    check(lib().lcty_bgzf_deflate(ctx._h, buf.ctypes.data if len(buf) else None, len(buf), 1 if with_eof else 0, out.ctypes.data, cap, C.byref(n),
                                  off.ctypes.data, C.byref(st)))
    return out[:int(n.value)], off, st.as_dict()


def write_bgzf_device(ctx, path, data):
    """lcty_io_write_bgzf_device: write_bgzf with the blocks deflated on the device -> stats"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    st = cdefs.BgzfDeflateStats()
    check(lib().lcty_io_write_bgzf_device(ctx._h, str(path).encode(), buf.ctypes.data if len(buf) else None, len(buf), C.byref(st)))
    return st.as_dict()


class SampleReads:
    """lcty_sample_reads: the reads of one lcty_sample_bam_fetch, resident on the device; owned=False: the current chunk of a
    BamStream, which belongs to the stream and is valid until its next next() or close()."""

    def __init__(self, handle, stats, owned=True):
        self._h, self.stats, self._owned = handle, stats, owned

    def view(self):
        """(cdefs.ReadsChunk of sequence fields, src_record [2 n] uint32, paired): copies."""
        hs, src, paired = cdefs.ReadsHost(), VP(), C.c_int32(0)
        check(lib().lcty_sample_reads_view(self._h, C.byref(hs), C.byref(src), C.byref(paired)))
        n = int(hs.n_pairs)
        def arr(ptr, count, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(dt)), shape=(count,)).copy() if count else np.zeros(0, dtype=dt)
        mate_off = arr(hs.mate_off, 2 * n + 1, C.c_uint64)
        nb = int(mate_off[-1])
        z = np.zeros(n + 1, dtype=np.uint64)
        chunk = cdefs.ReadsChunk(arr(hs.mate_len, 2 * n, C.c_uint32), mate_off, arr(hs.bases2, max(nb // 16, 2), C.c_uint32),
                                 arr(hs.nmask, max(nb // 32, 1), C.c_uint32), z, np.zeros(0, dtype=cdefs.ALN_REC_DTYPE), z, np.zeros(0, dtype=np.uint32))
        return chunk, arr(src, 2 * n, C.c_uint32), bool(paired.value)

    def recruit(self, targets, max_out=8):
        n = self.stats["n_pairs"]
        cnt = np.zeros(max(n, 1), dtype=np.uint32); loci = np.zeros(max(n, 1) * max_out, dtype=np.uint32)
        check(lib().lcty_sample_reads_recruit(targets._h, self._h, max_out, cnt.ctypes.data, loci.ctypes.data))
        return cnt[:n], loci.reshape(-1, max_out)[:n]

    def write_recruited(self, writers, cnt, loci):
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        loci = np.ascontiguousarray(loci, dtype=np.uint32)
        n = U64(0)
        check(lib().lcty_sample_reads_write_recruited(self._h, writers._h, loci.shape[1], cnt.ctypes.data, loci.ctypes.data, C.byref(n)))
        return int(n.value)

    def add_recruited(self, rset, cnt, loci):
        """lcty_recruited_add_sample: the fetched reads into an api.Recruited set, device to device."""
        rset.add_sample(self, cnt, loci)

    def close(self):
        if self._h and self._owned:
            lib().lcty_sample_reads_free(self._h)
        self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BamStream:
    """lcty_bam_stream_*: whole BAM files without an index, read front to back in windows (`locityper genotype -a a.bam [-a b.bam]
    --no-index [-^]`). Windows follow the context's knob "bam_stream_window_bytes"."""

    def __init__(self, ctx, paths, interleaved=False):
        self._h = VP()
        self._ctx = ctx
        self.interleaved = bool(interleaved)
        self.stats = cdefs.BamStreamStats().as_dict()
        paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        check(lib().lcty_bam_stream_open(ctx._h, arr, len(paths), int(self.interleaved), C.byref(self._h)))

    def next(self):
        """-> (a SampleReads that belongs to the stream: the reads, or pairs, of the next window that completes any; stats, the sums of
        lcty_bam_stream_stats). The reads' stats["n_pairs"] is 0 at the end of the last file."""
        h, n, st = VP(), U64(0), cdefs.BamStreamStats()
        try:
            check(lib().lcty_bam_stream_next(self._h, C.byref(h), C.byref(n), C.byref(st)))
        finally:
            self.stats = st.as_dict()
        return SampleReads(h, dict(self.stats, n_pairs=int(n.value)), owned=False), self.stats

    def close(self):
        if self._h:
            lib().lcty_bam_stream_close(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SampleBam:
    """lcty_sample_bam_*: a coordinate-sorted BAM file with its BAI index (`locityper genotype -a`)."""

    def __init__(self, path, index_path=None):
        self._h = VP()
        check(lib().lcty_sample_bam_open(str(path).encode(), None if index_path is None else str(index_path).encode(), C.byref(self._h)))
        n, names, noff, lens = U32(0), VP(), VP(), VP()
        check(lib().lcty_sample_bam_contigs(self._h, C.byref(n), C.byref(names), C.byref(noff), C.byref(lens)))
        n = n.value
        off = np.ctypeslib.as_array(C.cast(noff, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        blob = C.string_at(names, int(off[-1])) if n else b""
        self.contigs = [blob[int(off[i]):int(off[i + 1]) - 1].decode() for i in range(n)]
        self.lengths = np.ctypeslib.as_array(C.cast(lens, C.POINTER(C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)

    def is_paired(self):
        p = C.c_int32(0)
        check(lib().lcty_sample_bam_is_paired(self._h, C.byref(p)))
        return bool(p.value)

    def plan(self, regions, with_unmapped=False):
        """-> (chunks [n][2] uint64 of virtual offsets, BGZF blocks they span)"""
        t, s, e = _regions(regions)
        n, blocks = U64(0), U64(0)
        check(lib().lcty_sample_bam_plan(self._h, len(t), t.ctypes.data, s.ctypes.data, e.ctypes.data, int(with_unmapped), 0, C.byref(n), None, None, None))
        beg = np.zeros(max(n.value, 1), dtype=np.uint64); end = np.zeros(max(n.value, 1), dtype=np.uint64)
        check(lib().lcty_sample_bam_plan(self._h, len(t), t.ctypes.data, s.ctypes.data, e.ctypes.data, int(with_unmapped), len(beg), C.byref(n),
                                         beg.ctypes.data, end.ctypes.data, C.byref(blocks)))
        return np.stack([beg, end], axis=1)[:n.value], int(blocks.value)

    def fetch(self, ctx, regions=(), with_unmapped=False, whole_file=False, paired=None):
        t, s, e = _regions(regions)
        h, st = VP(), cdefs.SampleBamStats()
        check(lib().lcty_sample_bam_fetch(ctx._h, self._h, len(t), t.ctypes.data, s.ctypes.data, e.ctypes.data, int(with_unmapped), int(whole_file),
                                          -1 if paired is None else int(paired), C.byref(h), C.byref(st)))
        return SampleReads(h, st.as_dict())

    def close(self):
        if self._h:
            lib().lcty_sample_bam_close(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastxWriters:
    def __init__(self, paths):
        self._keep = [str(p).encode() for p in paths]
        arr = (C.c_char_p * len(self._keep))(*self._keep)
        self._h = VP()
        check(lib().lcty_fastx_writers_open(arr, len(self._keep), C.byref(self._h)))

    def close(self):
        if self._h:
            h, self._h = self._h, VP()
            check(lib().lcty_fastx_writers_close(h))


class Vcf:
    """lcty_vcf_open: a text VCF (plain, gzip, BGZF). samples, ploidy (of the first record), hap_off (columns of gt)."""

    def __init__(self, path):
        self._h = VP()
        check(lib().lcty_vcf_open(str(path).encode(), C.byref(self._h)))
        v = cdefs.VcfView()
        check(lib().lcty_vcf_view_get(self._h, C.byref(v)))
        blob = C.string_at(v.samples, v.samples_len) if v.samples_len else b""
        self.samples = [s.decode() for s in blob.split(b"\0")[:-1]]
        self.ploidy = np.frombuffer(C.string_at(v.ploidy, 4 * v.n_samples), dtype=np.uint32).copy() if v.n_samples else np.zeros(0, np.uint32)
        self.hap_off = np.frombuffer(C.string_at(v.hap_off, 4 * (v.n_samples + 1)), dtype=np.uint32).copy()
        self.n_haps, self.n_records = int(v.n_haps), int(v.n_records)

    def region(self, contig, start, end, sample_used=None):
        """lcty_vcf_region: the records fetch(start, end) returns, as a dict of flat arrays: pos, ref_len, rec_allele, allele_off,
        allele_bytes, gt [n_recs][n_haps] (int16, -1 = missing), phased [n_recs][n_samples]."""
        used = None if sample_used is None else np.ascontiguousarray(sample_used, dtype=np.uint8)
        if used is not None and len(used) != len(self.samples):
            raise ValueError("sample_used must have one entry per sample")
        r = cdefs.VcfRecords()
        check(lib().lcty_vcf_region(self._h, contig.encode(), start, end, None if used is None else used.ctypes.data, C.byref(r)))
        try:
            return _records_dict(r)
        finally:
            lib().lcty_vcf_records_free(C.byref(r))

    def close(self):
        if self._h:
            lib().lcty_vcf_free(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _records_dict(r):
    """The arrays of a lcty_vcf_records as a dict (the caller frees the struct)."""
    def arr(p, n, dt):
        return np.frombuffer(C.string_at(p, n * np.dtype(dt).itemsize), dtype=dt).copy() if n else np.zeros(0, dtype=dt)
    n = int(r.n_recs)
    return {"pos": arr(r.pos, n, np.uint32), "ref_len": arr(r.ref_len, n, np.uint32), "rec_allele": arr(r.rec_allele, n + 1, np.uint32),
            "allele_off": arr(r.allele_off, int(r.n_alleles) + 1, np.uint64), "allele_bytes": arr(r.allele_bytes, int(r.pool_len), np.uint8),
            "gt": arr(r.gt, n * int(r.n_haps), np.int16).reshape(n, int(r.n_haps)),
            "phased": arr(r.phased, n * int(r.n_samples), np.uint8).reshape(n, int(r.n_samples))}


class VcfIndexed:
    """lcty_vcf_indexed_*: a BGZF VCF with its tabix index (`locityper target -v`): only the chunks of a window are read, inflated and
    parsed, on the device. samples, ploidy (of the first record of the file), hap_off as Vcf; stats: those of the last region()."""

    def __init__(self, path, index_path=None, ctx=None):
        self._h = VP()
        self.ctx = ctx                               # the context of region(); open and plan are host work
        check(lib().lcty_vcf_indexed_open(str(path).encode(), None if index_path is None else str(index_path).encode(), C.byref(self._h)))
        v = cdefs.VcfView()
        check(lib().lcty_vcf_indexed_view_get(self._h, C.byref(v)))
        blob = C.string_at(v.samples, v.samples_len) if v.samples_len else b""
        self.samples = [s.decode() for s in blob.split(b"\0")[:-1]]
        self.ploidy = np.frombuffer(C.string_at(v.ploidy, 4 * v.n_samples), dtype=np.uint32).copy() if v.n_samples else np.zeros(0, np.uint32)
        self.hap_off = np.frombuffer(C.string_at(v.hap_off, 4 * (v.n_samples + 1)), dtype=np.uint32).copy()
        self.n_haps, self.n_records = int(v.n_haps), int(v.n_records)
        self.stats = None

    def contigs(self):
        """lcty_vcf_indexed_contigs: [(name, length or 0)] in the order of the file's contig indices."""
        c = cdefs.VcfContigs()
        check(lib().lcty_vcf_indexed_contigs(self._h, C.byref(c)))
        names = C.string_at(c.names, c.names_len).split(b"\0")[:-1] if c.names_len else []
        lens = np.frombuffer(C.string_at(c.length, 8 * c.n_contigs), dtype=np.uint64) if c.n_contigs else []
        return [(n.decode(), int(l)) for n, l in zip(names, lens)]

    def plan(self, contig, start, end):
        """-> (chunks [n][2] uint64 of virtual offsets, BGZF blocks they span)"""
        n, blocks = U64(0), U64(0)
        check(lib().lcty_vcf_indexed_plan(self._h, contig.encode(), start, end, 0, C.byref(n), None, None, None))
        beg = np.zeros(max(n.value, 1), dtype=np.uint64); end_ = np.zeros(max(n.value, 1), dtype=np.uint64)
        check(lib().lcty_vcf_indexed_plan(self._h, contig.encode(), start, end, len(beg), C.byref(n), beg.ctypes.data, end_.ctypes.data, C.byref(blocks)))
        return np.stack([beg, end_], axis=1)[:n.value], int(blocks.value)

    def region(self, contig, start, end, sample_used=None, ctx=None):
        """lcty_vcf_indexed_fetch: the dict of Vcf.region for the same file and arguments, on the context given here or at construction."""
        ctx = self.ctx if ctx is None else ctx
        used = None if sample_used is None else np.ascontiguousarray(sample_used, dtype=np.uint8)
        if used is not None and len(used) != len(self.samples):
            raise ValueError("sample_used must have one entry per sample")
        r, st = cdefs.VcfRecords(), cdefs.VcfFetchStats()
        check(lib().lcty_vcf_indexed_fetch(None if ctx is None else ctx._h, self._h, contig.encode(), start, end, None if used is None else used.ctypes.data,
                                           C.byref(r), C.byref(st)))
        try:
            self.stats = st.as_dict()
            return _records_dict(r)
        finally:
            lib().lcty_vcf_records_free(C.byref(r))

    def close(self):
        if self._h:
            lib().lcty_vcf_indexed_close(self._h)
            self._h = VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vcf_region(path, contig, start, end, sample_used=None):
    """Open, lcty_vcf_region, close: (Vcf fields as a dict, records dict)."""
    v = Vcf(path)
    try:
        return {"samples": v.samples, "ploidy": v.ploidy, "hap_off": v.hap_off}, v.region(contig, start, end, sample_used)
    finally:
        v.close()
