// lcty_recruited.hip — a resident set of recruited reads: for every locus of a finalized lcty_targets the reads recruited
// to it so far, on the device, as the sequence fields of one chunk — what the in-locus mapper reads (lcty_map.hip) — plus a source
// ordinal per pair. An add scatters a chunk of reads resident on the device (ReadChunk, lcty_read_chunk.hpp: a host chunk uploaded, or
// the chunk of a lcty_fastx_device / lcty_sample_reads where it lies) by the answers of recruitment:
//   entries   (locus, pair) for every locus of every pair, in input order (entry_kernel behind an exclusive_scan of out_cnt),
//             brought into locus order by the stable radix sort of lcty_sort.hpp on the bytes of the locus;
//   places    exclusive_scan (lcty_scan.hpp) of the entries' unit counts: a locus's entries are one run, so entry e of locus l goes to
//             unit  units(l) + unit_at[e] - unit_at[first(l)]  and pair  pairs(l) + e - first(l);
//   copy      scatter_kernel: a thread per unit (a 64-bit word of bases and a 32-bit word of mask: consecutive threads write
//             consecutive words of a locus and read consecutive words of a mate) and a thread per entry for the rebased
//             mate_len / mate_off and the ordinal.
// The result is a function of the chunks and the answers: no atomics, nothing depends on the grid. The host's half — what it keeps per
// locus, the plan of an add, the checks made before anything is copied — is lcty_recruited_host.hpp.
#include <functional>

#include "lcty_map_internal.hpp"
#include "lcty_read_chunk.hpp"
#include "lcty_recruited_host.hpp"
#include "lcty_sample_bam.hpp"
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"

using namespace lcty;
using recruited::LocusBook;

namespace {

// the arrays of one locus on the device; the capacities are LocusBook's
struct LocusDev {
    DevBuf<uint64_t> bases, off, ord;         // [cap_units + CHUNK_PAD_UNITS] (zeros follow the last unit, as in a ReadChunk), [2 cap_pairs + 1], [cap_pairs]
    DevBuf<uint32_t> nm, len;                 // [cap_units + CHUNK_PAD_UNITS], [2 cap_pairs]
};

// where a locus's share of an add goes
struct LocusDst {
    uint64_t* bases; uint32_t* nm; uint32_t* len; uint64_t* off; uint64_t* ord;
    uint64_t pair0, unit0;                    // pairs and units the locus holds already
    uint32_t first;                           // its first entry in locus order
};

struct ScatterView {
    // the source chunk
    const uint32_t* mate_len; const uint64_t* mate_off; const uint64_t* bases; const uint32_t* nmask;
    // the entries in locus order: key = locus, val = pair; unit_at[e] = units of the entries before e
    const uint64_t* key; const uint64_t* val; const uint32_t* unit_at;
    uint32_t n_entries, n_units;
    const LocusDst* dst;
    uint64_t ordinal0;                        // the ordinal of the chunk's pair 0
};

__device__ __forceinline__ uint32_t dev_units_of(uint32_t len) { return (len + 31u) >> 5; }

// out_cnt -> the (locus, pair) entries of pair i at entry_at[i] .., in input order
__global__ __launch_bounds__(256) void entry_kernel(uint64_t n, uint32_t max_out, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ loci,
                                                     const uint32_t* __restrict__ entry_at, uint64_t* __restrict__ key, uint64_t* __restrict__ val) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cnt[i], at = entry_at[i];
    for (uint32_t j = 0; j < c; j++) { key[at + j] = loci[i * max_out + j]; val[at + j] = i; }
}

// the units of every entry in locus order
__global__ __launch_bounds__(256) void entry_units_kernel(uint32_t n_entries, const uint64_t* __restrict__ val, const uint32_t* __restrict__ mate_len,
                                                           uint32_t* __restrict__ units) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    const uint64_t i = val[e];
    units[e] = dev_units_of(mate_len[2 * i]) + dev_units_of(mate_len[2 * i + 1]);
}

__global__ __launch_bounds__(256) void scatter_kernel(const ScatterView V) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t < V.n_units) {
        // the entry of unit t: the last one whose first unit is <= t (entries without units share a place with the next one)
        uint32_t lo = 0, hi = V.n_entries;
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (V.unit_at[mid] <= t) lo = mid; else hi = mid; }
        const uint32_t e = lo;
        const LocusDst D = V.dst[V.key[e]];
        const uint64_t i = V.val[e];
        const uint32_t within = t - V.unit_at[e], u1 = dev_units_of(V.mate_len[2 * i]);
        const uint64_t src = within < u1 ? (V.mate_off[2 * i] >> 5) + within : (V.mate_off[2 * i + 1] >> 5) + (within - u1);
        const uint64_t to = D.unit0 + (t - V.unit_at[D.first]);
        D.bases[to] = V.bases[src];
        D.nm[to] = V.nmask[src];
    }
    if (t < V.n_entries) {
        const uint32_t e = t;
        const LocusDst D = V.dst[V.key[e]];
        const uint64_t i = V.val[e], p = D.pair0 + (e - D.first);
        const uint32_t l1 = V.mate_len[2 * i], l2 = V.mate_len[2 * i + 1];
        const uint64_t at = 32ull * (D.unit0 + (V.unit_at[e] - V.unit_at[D.first]));
        D.len[2 * p] = l1; D.len[2 * p + 1] = l2;
        D.off[2 * p + 1] = at + 32ull * dev_units_of(l1);
        D.off[2 * p + 2] = at + 32ull * (dev_units_of(l1) + dev_units_of(l2));      // off[0] = 0 since the arrays were made
        D.ord[p] = V.ordinal0 + i;
    }
}

using NameFn = std::function<std::string(uint64_t)>;      // the name of pair i of a chunk; empty: the source has no names

}  // namespace

struct lcty_recruited {
    lcty_ctx* ctx = nullptr;
    lcty_targets* targets = nullptr;
    bool keep_names = false, any_unnamed = false;
    uint64_t n_seen = 0;                      // pairs of every add so far: the ordinal of the next chunk's pair 0
    std::vector<LocusBook> books;
    std::vector<LocusDev> dev;
    // the downloaded view of a locus, made on first use and dropped when the locus gains reads
    struct HostView { bool valid = false; std::vector<uint32_t> bases2, nmask; std::vector<uint64_t> ord, zero_off; };
    std::vector<HostView> views;
    // scratch of an add, grow-only
    RadixSort sorter;
    DevBuf<uint64_t> key_a, key_b, val_a, val_b;
    DevBuf<uint32_t> d_cnt, d_loci, entry_at, units, unit_at, scan_tmp;
    DevBuf<uint8_t> d_dst;
};

namespace {

// makes room for `pairs` pairs and `units` units in locus l, device to device; the contents stay
void reserve(lcty_recruited* S, size_t l, uint64_t pairs, uint64_t units, uint64_t init_units) {
    LocusBook& b = S->books[l];
    LocusDev& d = S->dev[l];
    hipStream_t s = S->ctx->stream;
    const uint64_t cap_units = recruited::grown(b.cap_units, units, init_units);
    const uint64_t cap_pairs = recruited::grown(b.cap_pairs, pairs, std::max<uint64_t>(init_units / 8, 1));
    if (cap_units != b.cap_units || !d.bases.p) {
        DevBuf<uint64_t> bases; DevBuf<uint32_t> nm;
        bases.alloc(cap_units + CHUNK_PAD_UNITS); nm.alloc(cap_units + CHUNK_PAD_UNITS);
        bases.zero(s); nm.zero(s);
        if (b.n_units) {
            LCTY_HIP(hipMemcpyAsync(bases.p, d.bases.p, b.n_units * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
            LCTY_HIP(hipMemcpyAsync(nm.p, d.nm.p, b.n_units * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        }
        LCTY_HIP(hipStreamSynchronize(s));
        d.bases = std::move(bases); d.nm = std::move(nm);
        b.cap_units = cap_units;
    }
    if (cap_pairs != b.cap_pairs || !d.len.p) {
        DevBuf<uint32_t> len; DevBuf<uint64_t> off, ord;
        len.alloc(2 * cap_pairs); off.alloc(2 * cap_pairs + 1); ord.alloc(cap_pairs);
        LCTY_HIP(hipMemsetAsync(off.p, 0, sizeof(uint64_t), s));
        if (b.n_pairs) {
            LCTY_HIP(hipMemcpyAsync(len.p, d.len.p, 2 * b.n_pairs * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            LCTY_HIP(hipMemcpyAsync(off.p, d.off.p, (2 * b.n_pairs + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
            LCTY_HIP(hipMemcpyAsync(ord.p, d.ord.p, b.n_pairs * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
        }
        LCTY_HIP(hipStreamSynchronize(s));
        d.len = std::move(len); d.off = std::move(off); d.ord = std::move(ord);
        b.cap_pairs = cap_pairs;
    }
}

void add_chunk(lcty_recruited* S, const ReadChunk& src, const NameFn& name, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci) {
    lcty_ctx* ctx = S->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = src.n;
    if (n == 0) return;
    if (n >= recruited::MAX_ENTRIES) fail(LCTY_ERR_UNSUPPORTED, "2^32 or more reads in one add: add the reads in smaller chunks");
    const uint64_t max_bytes = static_cast<uint64_t>(ctx->knob("recruited_max_bytes", static_cast<int64_t>(recruited::MAX_BYTES_DEFAULT)));
    const uint64_t init_units = static_cast<uint64_t>(std::max<int64_t>(1, ctx->knob("recruited_init_units", static_cast<int64_t>(recruited::INIT_UNITS_DEFAULT))));
    // ---- the plan: every check is made here, before anything is copied
    const uint32_t* h_len = src.h_len;
    const recruited::Plan P = recruited::plan_add(S->books, n, h_len, max_out, out_cnt, out_loci, max_bytes);
    const size_t n_loci = S->books.size();
    if (P.n_entries) {
        const uint32_t n_entries = static_cast<uint32_t>(P.n_entries), n_units = static_cast<uint32_t>(P.n_units);
        // ---- room (the contents of a locus stay what they were) and the table of destinations: O(loci)
        std::vector<LocusDst> dst(n_loci);
        uint64_t first = 0;
        for (size_t l = 0; l < n_loci; l++) {
            const LocusBook& b = S->books[l];
            if (P.add_pairs[l]) reserve(S, l, b.n_pairs + P.add_pairs[l], b.n_units + P.add_units[l], init_units);
            const LocusDev& d = S->dev[l];
            dst[l] = LocusDst{d.bases.p, d.nm.p, d.len.p, d.off.p, d.ord.p, b.n_pairs, b.n_units, static_cast<uint32_t>(first)};
            first += P.add_pairs[l];
        }
        S->d_dst.ensure_slack(n_loci * sizeof(LocusDst));
        LCTY_HIP(hipMemcpyAsync(S->d_dst.p, dst.data(), n_loci * sizeof(LocusDst), hipMemcpyHostToDevice, s));
        // ---- entries in input order
        S->d_cnt.ensure_slack(n); S->d_loci.ensure_slack(n * max_out); S->entry_at.ensure_slack(n);
        S->d_cnt.upload(out_cnt, n, s); S->d_loci.upload(out_loci, n * max_out, s);
        S->scan_tmp.ensure(scan_scratch_words(std::max<uint64_t>(n, n_entries)));
        exclusive_scan(S->d_cnt.p, S->entry_at.p, n, S->scan_tmp.p, s);
        S->key_a.ensure_slack(n_entries); S->key_b.ensure_slack(n_entries); S->val_a.ensure_slack(n_entries); S->val_b.ensure_slack(n_entries);
        hipLaunchKernelGGL(entry_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, n, max_out, S->d_cnt.p, S->d_loci.p, S->entry_at.p, S->key_a.p, S->val_a.p);
        LCTY_HIP(hipGetLastError());
        // ---- locus order: one stable pass per byte of the largest locus index
        std::vector<uint32_t> shifts;
        for (uint32_t sh = 0; sh < 32 && ((n_loci - 1) >> sh) != 0; sh += 8) shifts.push_back(sh);
        const int where = S->sorter.run(S->key_a.p, S->val_a.p, S->key_b.p, S->val_b.p, n_entries, shifts, s);
        const uint64_t* key = where ? S->key_b.p : S->key_a.p; const uint64_t* val = where ? S->val_b.p : S->val_a.p;
        // ---- places
        S->units.ensure_slack(n_entries); S->unit_at.ensure_slack(n_entries);
        hipLaunchKernelGGL(entry_units_kernel, dim3(blocks_of(n_entries, 256)), dim3(256), 0, s, n_entries, val, src.d_len.p, S->units.p);
        LCTY_HIP(hipGetLastError());
        exclusive_scan(S->units.p, S->unit_at.p, n_entries, S->scan_tmp.p, s);
        // ---- the copy
        ScatterView V{src.d_len.p, src.d_off.p, src.d_bases.p, src.d_nm.p, key, val, S->unit_at.p, n_entries, n_units,
                      reinterpret_cast<const LocusDst*>(S->d_dst.p), S->n_seen};
        hipLaunchKernelGGL(scatter_kernel, dim3(blocks_of(std::max(n_entries, n_units), 256)), dim3(256), 0, s, V);
        LCTY_HIP(hipGetLastError());
        LCTY_HIP(hipStreamSynchronize(s));                                       // dst and the caller's answers are host memory of this call
    }
    // ---- the host's side: nothing below fails for a reason of the input
    const bool named = S->keep_names && static_cast<bool>(name);
    recruited::commit_add(S->books, P, n, h_len, max_out, out_cnt, out_loci, named ? &name : static_cast<const NameFn*>(nullptr));
    if (!named && P.n_entries) S->any_unnamed = true;
    for (size_t l = 0; l < n_loci; l++) if (P.add_pairs[l]) S->views[l].valid = false;
    S->n_seen += n;
}

void check_answers(const lcty_recruited* S, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci) {
    if (!S || !out_cnt || !out_loci || max_out == 0) fail(LCTY_ERR_INVALID_INPUT, "null argument");
}

// the chunk a source handle holds, scattered from where it lies (null: the handle was null)
void add_resident(lcty_recruited* S, const ReadChunk* c, const NameFn& name, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci) {
    check_answers(S, max_out, out_cnt, out_loci);
    if (!c) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (c->ctx != S->ctx) fail(LCTY_ERR_INVALID_INPUT, "the set and the reads belong to different contexts");
    S->ctx->activate();
    add_chunk(S, *c, name, max_out, out_cnt, out_loci);
}

LocusBook& book_of(lcty_recruited* S, uint32_t locus_ix) {
    if (!S) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (locus_ix >= S->books.size()) fail(LCTY_ERR_INVALID_INPUT, "locus %u of %zu", locus_ix, S->books.size());
    return S->books[locus_ix];
}

}  // namespace

extern "C" {

int32_t lcty_recruited_create(lcty_targets* targets, int32_t keep_names, lcty_recruited** out) {
    if (out) *out = nullptr;
    return guarded([&] {
        if (!targets || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::unique_ptr<lcty_recruited> S(new lcty_recruited());
        S->ctx = targets_ctx(targets);                                           // refuses targets that are not finalized
        S->targets = targets; S->keep_names = keep_names != 0;
        const uint32_t n_loci = targets_n_loci(targets);
        S->books.resize(n_loci); S->dev.resize(n_loci); S->views.resize(n_loci);
        *out = S.release();
    });
}

void lcty_recruited_destroy(lcty_recruited* set) { delete set; }

int32_t lcty_recruited_add(lcty_recruited* set, const lcty_reads_host* h, int32_t paired, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci) {
    return guarded([&] {
        check_answers(set, max_out, out_cnt, out_loci);
        (void)paired;                                                            // an absent mate has length 0 either way
        set->ctx->activate();
        ReadChunk c(set->ctx, ReadChunk::Buffers::OneShot);
        struct Done { hipStream_t s; ~Done() { (void)hipStreamSynchronize(s); } } done{set->ctx->stream};      // the copies read the caller's chunk
        c.upload(h);
        add_chunk(set, c, NameFn(), max_out, out_cnt, out_loci);
    });
}

int32_t lcty_recruited_add_fastx(lcty_recruited* set, lcty_fastx_device* f, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci) {
    return guarded([&] { add_resident(set, f ? &fastx_device_reads(f) : nullptr, [f](uint64_t i) { return fastx_device_name(f, i); }, max_out, out_cnt, out_loci); });
}

int32_t lcty_recruited_add_sample(lcty_recruited* set, lcty_sample_reads* r, uint32_t max_out, const uint32_t* out_cnt, const uint32_t* out_loci) {
    return guarded([&] { add_resident(set, r ? &r->chunk : nullptr, [r](uint64_t i) { return sample_reads_name(r, i); }, max_out, out_cnt, out_loci); });
}

int32_t lcty_recruited_sizes(lcty_recruited* set, uint32_t locus_ix, uint64_t* n_pairs, uint64_t* n_bases) {
    return guarded([&] {
        const LocusBook& b = book_of(set, locus_ix);
        if (n_pairs) *n_pairs = b.n_pairs;
        if (n_bases) *n_bases = 32 * b.n_units;
    });
}

int32_t lcty_recruited_view(lcty_recruited* set, uint32_t locus_ix, lcty_reads_host* view, const uint64_t** src_ordinal) {
    return guarded([&] {
        const LocusBook& b = book_of(set, locus_ix);
        if (!view) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_recruited::HostView& H = set->views[locus_ix];
        if (!H.valid) {
            set->ctx->activate();
            hipStream_t s = set->ctx->stream;
            const LocusDev& d = set->dev[locus_ix];
            H.bases2.assign(2 * b.n_units + 2, 0); H.nmask.assign(b.n_units + 1, 0); H.ord.assign(b.n_pairs + 1, 0); H.zero_off.assign(b.n_pairs + 1, 0);
            if (b.n_units) {
                LCTY_HIP(hipMemcpyAsync(H.bases2.data(), d.bases.p, b.n_units * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                d.nm.download(H.nmask.data(), b.n_units, s);
            }
            if (b.n_pairs) d.ord.download(H.ord.data(), b.n_pairs, s);
            LCTY_HIP(hipStreamSynchronize(s));
            H.valid = true;
        }
        memset(view, 0, sizeof(*view));
        view->n_pairs = b.n_pairs;
        view->mate_len = b.mate_len.data(); view->mate_off = b.mate_off.data(); view->bases2 = H.bases2.data(); view->nmask = H.nmask.data();
        view->aln_off = H.zero_off.data(); view->cigar_off = H.zero_off.data();
        if (src_ordinal) *src_ordinal = H.ord.data();
    });
}

int32_t lcty_recruited_names(lcty_recruited* set, uint32_t locus_ix, const uint64_t** name_off, const char** names) {
    return guarded([&] {
        const LocusBook& b = book_of(set, locus_ix);
        if (!name_off || !names) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (!set->keep_names) fail(LCTY_ERR_INVALID_INPUT, "the set was created without keep_names");
        if (set->any_unnamed) fail(LCTY_ERR_INVALID_INPUT, "reads were added with lcty_recruited_add, which has no names");
        *name_off = b.name_off.data(); *names = b.names.c_str();
    });
}

int32_t lcty_reads_map_append_recruited(lcty_reads* reads, lcty_recruited* set, uint32_t locus_ix, uint64_t first_pair, uint64_t n_pairs,
                                        const lcty_map_params* params) {
    return guarded([&] {
        if (!reads || !params) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const LocusBook& b = book_of(set, locus_ix);
        if (reads->ctx != set->ctx) fail(LCTY_ERR_INVALID_INPUT, "the set and the batch belong to different contexts");
        if (first_pair > b.n_pairs || n_pairs > b.n_pairs - first_pair)
            fail(LCTY_ERR_INVALID_INPUT, "pairs %llu .. %llu of the %llu recruited to locus %u", static_cast<unsigned long long>(first_pair),
                 static_cast<unsigned long long>(first_pair + n_pairs), static_cast<unsigned long long>(b.n_pairs), locus_ix);
        if (n_pairs == 0) return;
        const LocusDev& d = set->dev[locus_ix];
        // the range where it lies: the bases start at a unit, so only the offsets are rebased (on the host, which has them)
        const uint64_t base = b.mate_off[2 * first_pair];
        std::vector<uint64_t> rebased;
        MapInput in{};
        in.n_pairs = n_pairs; in.mate_len = b.mate_len.data() + 2 * first_pair;
        in.d_mate_len = d.len.p + 2 * first_pair;
        in.d_bases2 = reinterpret_cast<const uint32_t*>(d.bases.p + base / 32); in.d_nmask = d.nm.p + base / 32;
        if (first_pair == 0) { in.mate_off = b.mate_off.data(); in.d_mate_off = d.off.p; }
        else {
            rebased.resize(2 * n_pairs + 1);
            for (uint64_t m = 0; m <= 2 * n_pairs; m++) rebased[m] = b.mate_off[2 * first_pair + m] - base;
            in.mate_off = rebased.data();                                        // d_mate_off stays null: these are uploaded
        }
        map_append_input(reads, in, params);
    });
}

}  // extern "C"
