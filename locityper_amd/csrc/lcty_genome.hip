// lcty_genome.hip — a genome resident on the device, and what the database side asks of it:
//   src/seq/counts.rs:258-369   JfKmerGetter::new / fetch: the genome-wide counts of the k-mers of a few sequences. No Jellyfish
//                               database is read or built: the distinct canonical k-mers of the QUERY go into a device table, the
//                               genome streams past it once, and every query position takes its counter.
//   src/seq/mod.rs:26-38, 149   standardize + fetch_seq: a window of a contig as capitals A C G T, N for everything else.
// Storage: 2 bits a base (16 bases a word, LSB first) and one "not a base" bit (32 bases a word), every contig in ONE coordinate
// space with a masked position in front of each contig but the first: a k-mer occurrence never spans two contigs, and the scan
// needs no contig table. Positions behind the last one are zero in both arrays and are cut off by the scan's own limit.
#include <memory>
#include <string>
#include <vector>

#include "lcty_common.hpp"
#include "lcty_device.hpp"
#include "lcty_lines.hpp"
#include "lcty_seq.hpp"
#include "lcty_table.hpp"

using namespace lcty;

namespace {

constexpr uint32_t RUN = LCTY_GENOME_SCAN_RUN;       // k-mer starts per thread of the scan: 8 words of bases, 4 of the mask
constexpr uint32_t WORDS_MAX = RUN / 16 + 2;         // ... plus the k - 1 <= 30 bases behind them
constexpr uint32_t SLACK_WORDS = 64;                 // what a kernel may read behind the last position's word
constexpr uint64_t PIECE = 64ull << 20;              // bases per upload of lcty_genome_append: the staging buffer's bound
constexpr uint64_t FASTA_CHUNK = 16ull << 20;        // bases per lcty_genome_append of lcty_genome_load_fasta
constexpr uint32_t THREADS = 256;
constexpr uint32_t MAX_GRID = 4096;                  // blocks of the grid-stride kernels

// 0..3 a base (case folded), 4 a letter seq::standardize turns into N, 5 anything else
__device__ inline uint32_t genome_enc(uint8_t c) {
    switch (c | 0x20u) {
        case 'a': return 0u;
        case 'c': return 1u;
        case 'g': return 2u;
        case 't': return 3u;
        case 'n': case 'r': case 'y': case 'k': case 'm': case 's': case 'w': case 'b': case 'd': case 'h': case 'v': return 4u;
        default: return 5u;
    }
}

// The pack kernel: one thread per 32 positions of the resident arrays. The piece covers [at + sep, at + sep + len); with sep the
// position `at` is the masked one between two contigs. Words the piece shares with what was packed before are OR-ed into (appends
// are in stream order, and the positions behind the last one are zero). *bad: the first byte of the piece that is neither a base
// nor a letter standardize accepts.
__global__ void genome_pack_kernel(const uint8_t* __restrict__ ascii, uint64_t at, uint32_t sep, uint64_t len, uint32_t* bases2, uint32_t* nmask,
                                   unsigned long long* bad) {
    const uint64_t first = at >> 5, last = (at + sep + len - 1) >> 5;
    const uint64_t g = first + static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g > last) return;
    const uint64_t lo = max(g << 5, at), hi = min((g + 1) << 5, at + sep + len);
    uint64_t two = 0;
    uint32_t mask = 0;
    for (uint64_t p = lo; p < hi; p++) {
        const uint32_t b = static_cast<uint32_t>(p & 31u);
        if (p < at + sep) { mask |= 1u << b; continue; }
        const uint32_t e = genome_enc(ascii[p - at - sep]);
        if (e < 4u) two |= static_cast<uint64_t>(e) << (2u * b);
        else mask |= 1u << b;
        if (e == 5u) atomicMin(bad, static_cast<unsigned long long>(p - at - sep));
    }
    if (lo == (g << 5) && hi == ((g + 1) << 5)) {
        bases2[2 * g] = static_cast<uint32_t>(two); bases2[2 * g + 1] = static_cast<uint32_t>(two >> 32); nmask[g] = mask;
    } else {
        bases2[2 * g] |= static_cast<uint32_t>(two); bases2[2 * g + 1] |= static_cast<uint32_t>(two >> 32); nmask[g] |= mask;
    }
}

__global__ void genome_unpack_kernel(const uint32_t* __restrict__ bases2, const uint32_t* __restrict__ nmask, uint64_t at, uint64_t len, uint8_t* out) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < len; i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t p = at + i;
        const bool masked = (nmask[p >> 5] >> (p & 31u)) & 1u;
        out[i] = masked ? 'N' : "ACGT"[(bases2[p >> 4] >> (2u * (p & 15u))) & 3u];
    }
}

// ---- the query side: values are numbered as they come out, value o = position o - cnt_off[a] of sequence a ----
__global__ void query_check_kernel(const uint8_t* __restrict__ seqs, uint64_t total, unsigned long long* bad) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        if (base_enc(seqs[i]) > 3u) atomicMin(bad, static_cast<unsigned long long>(i));
}

// canonical k-mer of value o (every base is one of the four capitals: query_check_kernel has run)
__device__ inline uint64_t query_kmer(const uint8_t* seqs, const uint64_t* seq_off, const uint64_t* cnt_off, uint32_t n_seqs, uint32_t k, uint64_t o) {
    const uint32_t a = flat_owner(cnt_off, n_seqs, o);
    uint64_t kmer;
    canonical_kmer_ascii<uint64_t>(seqs, seq_off[a] + (o - cnt_off[a]), k, &kmer);
    return kmer;
}

__global__ void query_insert_kernel(const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ cnt_off,
                                    uint32_t n_seqs, uint32_t k, uint64_t n_values, uint64_t* keys, uint64_t mask) {
    for (uint64_t o = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; o < n_values; o += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        keytable::claim<keytable::MixHash, UNDEF64>(keys, mask, query_kmer(seqs, seq_off, cnt_off, n_seqs, k, o));
}

// ---- the scan (the hot path). A thread owns the RUN k-mer starts from s = RUN * its index on: it reads the 8 words of their bases,
// the words of the k - 1 bases behind them and the mask words once, rolls the forward and the reverse-complement value over
// them, and counts the valid bases since the last masked one — a k-mer ends at base i iff that count has reached k, so no k-mer that
// starts before s, spans a masked base or reaches behind `n_pos` is ever looked up. The 16 lookups of a word are issued together
// (16 loads in flight a lane), then resolved: the first slot holds the key (a hit), the free marker (a miss) or another key (the
// probe goes on): keytable::find of lcty_table.hpp in a batched form, which stays written out. MERGE: equal
// consecutive hits of a thread (a homopolymer, a tandem repeat of period 1) are added as one atomic. ----
template <bool MERGE>
__global__ void __launch_bounds__(THREADS) genome_scan_kernel(const uint32_t* __restrict__ bases2, const uint32_t* __restrict__ nmask, uint64_t n_pos,
                                                             uint32_t k, const uint64_t* __restrict__ keys, uint32_t* counters, uint64_t mask,
                                                             unsigned long long* n_hits) {
    const uint64_t s = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * RUN;
    uint32_t hits = 0;
    if (s < n_pos) {
        const uint64_t lim = min(s + RUN + k - 1, n_pos);                 // bases [s, lim) are this thread's
        const uint32_t n_words = static_cast<uint32_t>((lim - s + 15) >> 4);
        const uint32_t* bw = bases2 + (s >> 4);
        const uint32_t* mw = nmask + (s >> 5);
        uint32_t wb[WORDS_MAX], wm[WORDS_MAX / 2];
        {
            const uint4 a = *reinterpret_cast<const uint4*>(bw), b = *reinterpret_cast<const uint4*>(bw + 4);
            wb[0] = a.x; wb[1] = a.y; wb[2] = a.z; wb[3] = a.w; wb[4] = b.x; wb[5] = b.y; wb[6] = b.z; wb[7] = b.w;
            wb[8] = bw[8]; wb[9] = bw[9];
            const uint4 m = *reinterpret_cast<const uint4*>(mw);
            wm[0] = m.x; wm[1] = m.y; wm[2] = m.z; wm[3] = m.w; wm[4] = mw[4];
        }
        const uint64_t kmask = (1ull << (2u * k)) - 1ull;
        const uint32_t rv_shift = 2u * k - 2u;
        uint64_t fw = 0, rv = 0;
        uint32_t valid = 0;                                               // bases since the last masked one
        uint64_t pend_slot = 0; uint32_t pend = 0;
#pragma unroll
        for (uint32_t w = 0; w < WORDS_MAX; w++) {
            if (w < n_words) {
                const uint32_t word = wb[w];
                uint32_t mbits = (wm[w >> 1] >> ((w & 1u) * 16u)) & 0xFFFFu;
                const uint64_t left = lim - (s + 16ull * w);              // bases of this word inside the limit: >= 1
                if (left < 16u) mbits |= 0xFFFFu << left;
                uint64_t key[16], first[16];
                uint32_t ends = 0;                                        // bit j: a k-mer ends at base j of the word
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) {
                    const uint32_t e = (word >> (2u * j)) & 3u;
                    fw = ((fw << 2) | e) & kmask;
                    rv = (rv >> 2) | (static_cast<uint64_t>(3u - e) << rv_shift);
                    valid = ((mbits >> j) & 1u) ? 0u : valid + 1u;
                    key[j] = fw < rv ? fw : rv;
                    if (valid >= k) ends |= 1u << j;
                }
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) first[j] = ((ends >> j) & 1u) ? keys[keytable::home<keytable::MixHash>(key[j], mask)] : UNDEF64;
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) {
                    uint64_t got = first[j];
                    if (got == UNDEF64) continue;                         // no k-mer ends here, or its first slot is free: a miss
                    uint64_t slot = keytable::home<keytable::MixHash>(key[j], mask);
                    while (got != key[j] && got != UNDEF64) { slot = keytable::step(slot, mask); got = keys[slot]; }
                    if (got != key[j]) continue;
                    hits++;
                    if (MERGE) {
                        if (pend && slot == pend_slot) { pend++; continue; }
                        if (pend) atomicAdd(&counters[pend_slot], pend);
                        pend_slot = slot; pend = 1;
                    } else {
                        atomicAdd(&counters[slot], 1u);
                    }
                }
            }
        }
        if (MERGE && pend) atomicAdd(&counters[pend_slot], pend);
    }
    // the hits of a wavefront as one add
    for (int off = 32; off > 0; off >>= 1) hits += __shfl_down(hits, off);
    if ((threadIdx.x & 63u) == 0 && hits) atomicAdd(n_hits, static_cast<unsigned long long>(hits));
}

__global__ void query_gather_kernel(const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ cnt_off,
                                    uint32_t n_seqs, uint32_t k, uint64_t n_values, const uint64_t* __restrict__ keys,
                                    const uint32_t* __restrict__ counters, uint64_t mask, uint32_t max_value, uint16_t* out) {
    for (uint64_t o = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; o < n_values; o += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t key = query_kmer(seqs, seq_off, cnt_off, n_seqs, k, o);
        const keytable::Probe p = keytable::find<keytable::MixHash, UNDEF64>(keys, mask, key);        // every query k-mer is in the table
        const uint32_t c = p.found ? counters[p.slot] : 0u;
        out[o] = static_cast<uint16_t>(max(min(c, max_value), 1u));      // counts.rs:354-355
    }
}

uint32_t grid_for(uint64_t n) { return std::max(1u, std::min(blocks_of(n, THREADS), MAX_GRID)); }

struct Contig { std::string name; uint64_t start, len; };

}  // namespace

struct lcty_genome {
    lcty_ctx* ctx = nullptr;
    int device = 0;
    DevBuf<uint32_t> bases2, nmask;
    uint64_t cap = 0;                       // positions the arrays hold (a multiple of 32), SLACK_WORDS behind them
    uint64_t n_pos = 0;                     // positions in use, separators included
    uint64_t n_bases = 0;                   // ... without them
    std::vector<Contig> contigs;
    DevBuf<uint8_t> stage; DevBuf<unsigned long long> flag;
    bool broken = false;                    // an append failed half way: the arrays hold a part of the piece

    void reserve(uint64_t positions) {
        if (positions <= cap) return;
        const uint64_t want = (std::max(positions, cap + cap / 2) + 1023) / 1024 * 1024;
        DevBuf<uint32_t> b, m;
        b.alloc(want / 16 + SLACK_WORDS); m.alloc(want / 32 + SLACK_WORDS);
        b.zero(ctx->stream); m.zero(ctx->stream);
        if (cap) {
            LCTY_HIP(hipMemcpyAsync(b.p, bases2.p, (cap / 16) * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            LCTY_HIP(hipMemcpyAsync(m.p, nmask.p, (cap / 32) * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        }
        LCTY_HIP(hipStreamSynchronize(ctx->stream));
        bases2 = std::move(b); nmask = std::move(m); cap = want;
    }
    const Contig& find(const char* name) const {
        for (const Contig& c : contigs) if (c.name == name) return c;
        fail(LCTY_ERR_INVALID_INPUT, "the genome has no contig %s", name);
    }
};

namespace {

void usable(const lcty_genome* g) {
    if (!g) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (g->broken) fail(LCTY_ERR_INVALID_INPUT, "the genome is incomplete: an earlier lcty_genome_append failed");
}

void append(lcty_genome* g, const char* name, const uint8_t* bases, uint64_t len, bool continues) {
    usable(g);
    if (len && !bases) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (continues && g->contigs.empty()) fail(LCTY_ERR_INVALID_INPUT, "no contig is open to be continued");
    if (!continues && !name) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    lcty_ctx* ctx = g->ctx;
    const uint32_t sep = (!continues && g->n_pos) ? 1u : 0u;
    // 32-bit counters must not wrap: every position counted at most once, fewer than 2^32 of them. Before anything is uploaded.
    const uint64_t limit = static_cast<uint64_t>(ctx->knob("genome_max_bases", 1ll << 32));
    if (len >= limit || g->n_pos + sep >= limit - len)
        fail(LCTY_ERR_UNSUPPORTED, "a genome of %llu bases (separators included; fewer than %llu are supported, knob genome_max_bases)",
             static_cast<unsigned long long>(g->n_pos + sep + len), static_cast<unsigned long long>(limit));
    if (!continues) g->contigs.push_back(Contig{name, g->n_pos + sep, 0});
    if (sep + len == 0) return;
    ctx->activate();
    hipStream_t s = ctx->stream;
    g->reserve(g->n_pos + sep + len);
    if (!g->flag.n) g->flag.alloc(1);
    Contig& c = g->contigs.back();
    uint64_t done = 0;
    uint32_t sep_left = sep;
    do {
        const uint64_t n = std::min(len - done, PIECE);
        g->stage.ensure_slack(std::max<uint64_t>(n, 1));
        LCTY_HIP(hipMemsetAsync(g->flag.p, 0xFF, sizeof(unsigned long long), s));
        g->stage.upload(bases + done, n, s);
        const uint64_t groups = ((g->n_pos + sep_left + n - 1) >> 5) - (g->n_pos >> 5) + 1;
        hipLaunchKernelGGL(genome_pack_kernel, dim3(blocks_of(groups, THREADS)), dim3(THREADS), 0, s, g->stage.p, g->n_pos, sep_left, n, g->bases2.p,
                           g->nmask.p, g->flag.p);
        LCTY_HIP(hipGetLastError());
        unsigned long long bad = 0;
        g->flag.download(&bad, 1, s);
        LCTY_HIP(hipStreamSynchronize(s));
        if (bad != ~0ull) {
            g->broken = true;
            const uint8_t b = bases[done + bad];
            fail(LCTY_ERR_INVALID_DATA, "contig %s: byte 0x%02x ('%c') at position %llu is not a nucleotide", c.name.c_str(), b,
                 b >= 0x20 && b < 0x7F ? b : '?', static_cast<unsigned long long>(c.len + bad));
        }
        g->n_pos += sep_left + n; g->n_bases += n; c.len += n;
        sep_left = 0; done += n;
    } while (done < len);
}

}  // namespace

extern "C" {

int32_t lcty_genome_create(lcty_ctx* ctx, lcty_genome** out) {
    return guarded([&] {
        if (!out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *out = nullptr;
        if (!ctx) {
            if (lcty_device_count() == 0) fail(LCTY_ERR_RUNTIME, "no HIP device is visible: liblocityper_hip has no CPU fallback");
            fail(LCTY_ERR_INVALID_INPUT, "null argument");
        }
        std::unique_ptr<lcty_genome> g(new lcty_genome());
        g->ctx = ctx; g->device = ctx->device;
        *out = g.release();
    });
}

void lcty_genome_destroy(lcty_genome* genome) {
    if (!genome) return;
    (void)hipSetDevice(genome->device);                  // every call has drained the stream before it returned; the context may be gone
    delete genome;
}

int32_t lcty_genome_append(lcty_genome* genome, const char* name, const uint8_t* bases, uint64_t len, int32_t continues) {
    return guarded([&] { append(genome, name, bases, len, continues != 0); });
}

int32_t lcty_genome_load_fasta(lcty_ctx* ctx, const char* path, lcty_genome** out) {
    return guarded([&] {
        if (!out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        *out = nullptr;
        if (!path) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        lcty_genome* raw = nullptr;
        if (const int32_t rc = lcty_genome_create(ctx, &raw)) throw Error(rc, lcty_last_error());
        struct Free { void operator()(lcty_genome* g) const { lcty_genome_destroy(g); } };
        std::unique_ptr<lcty_genome, Free> g(raw);
        LineReader in;
        in.open(path);
        // the lines of a contig gather in one page-locked chunk, which is the only host copy of them
        void* pinned = nullptr;
        ctx->activate();
        LCTY_HIP(hipHostMalloc(&pinned, FASTA_CHUNK, hipHostMallocDefault));
        struct Unpin { void operator()(void* p) const { (void)hipHostFree(p); } };
        std::unique_ptr<void, Unpin> hold(pinned);
        uint8_t* chunk = static_cast<uint8_t*>(pinned);
        uint64_t fill = 0;
        std::string name, l;
        bool open = false, started = false;                  // a header was read; its contig has been begun in the genome
        auto flush = [&] {
            if (!open || (started && !fill)) return;
            append(g.get(), name.c_str(), chunk, fill, started);
            started = true; fill = 0;
        };
        while (in.line(l)) {
            if (l.empty()) continue;
            if (l[0] == '>') {
                flush();
                const size_t sp = l.find_first_of(" \t");
                name.assign(l, 1, (sp == std::string::npos ? l.size() : sp) - 1);
                open = true; started = false;
                continue;
            }
            if (!open) fail(LCTY_ERR_INVALID_DATA, "%s: sequence before the first FASTA header", path);
            for (size_t at = 0; at < l.size();) {
                const size_t n = std::min<size_t>(l.size() - at, FASTA_CHUNK - fill);
                memcpy(chunk + fill, l.data() + at, n);
                fill += n; at += n;
                if (fill == FASTA_CHUNK) flush();
            }
        }
        flush();
        *out = g.release();
    });
}

int32_t lcty_genome_info(const lcty_genome* genome, uint32_t* n_contigs, uint64_t* n_bases) {
    return guarded([&] {
        usable(genome);
        if (n_contigs) *n_contigs = static_cast<uint32_t>(genome->contigs.size());
        if (n_bases) *n_bases = genome->n_bases;
    });
}

int32_t lcty_genome_contig(const lcty_genome* genome, uint32_t i, char* name_buf, uint64_t cap, uint64_t* len) {
    return guarded([&] {
        usable(genome);
        if (i >= genome->contigs.size()) fail(LCTY_ERR_INVALID_INPUT, "contig %u of %zu", i, genome->contigs.size());
        const Contig& c = genome->contigs[i];
        if (name_buf) {
            if (cap < c.name.size() + 1) fail(LCTY_ERR_INVALID_INPUT, "name buffer too small (%llu < %zu)", static_cast<unsigned long long>(cap), c.name.size() + 1);
            memcpy(name_buf, c.name.c_str(), c.name.size() + 1);
        }
        if (len) *len = c.len;
    });
}

int32_t lcty_genome_fetch(const lcty_genome* genome, const char* contig_name, uint64_t start, uint64_t end, uint8_t* out) {
    return guarded([&] {
        usable(genome);
        if (!contig_name || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const Contig& c = genome->find(contig_name);
        if (start >= end || end > c.len)
            fail(LCTY_ERR_INVALID_INPUT, "%s:%llu-%llu is not a window of a contig of %llu bases", contig_name, static_cast<unsigned long long>(start),
                 static_cast<unsigned long long>(end), static_cast<unsigned long long>(c.len));
        lcty_ctx* ctx = genome->ctx;
        ctx->activate();
        hipStream_t s = ctx->stream;
        const uint64_t n = end - start;
        DevBuf<uint8_t> d;
        d.alloc(n);
        hipLaunchKernelGGL(genome_unpack_kernel, dim3(grid_for(n)), dim3(THREADS), 0, s, genome->bases2.p, genome->nmask.p, c.start + start, n, d.p);
        LCTY_HIP(hipGetLastError());
        d.download(out, n, s);
        LCTY_HIP(hipStreamSynchronize(s));
    });
}

int32_t lcty_genome_kmer_counts(const lcty_genome* genome, uint32_t k, uint32_t counter_bytes, uint32_t n_seqs, const uint8_t* seqs,
                                const uint64_t* seq_off, uint16_t* counts, uint64_t* cnt_off, lcty_genome_count_stats* stats) {
    return guarded([&] {
        if (stats) memset(stats, 0, sizeof(*stats));
        if (k % 2 != 1) fail(LCTY_ERR_INVALID_DATA, "Jellyfish counts are calculated for an even k size (%u), odd k is required", k);
        if (k > 63) fail(LCTY_ERR_INVALID_DATA, "Jellyfish counts are calculated for too big k (%u), at most 63 can be used", k);
        if (k > 31) fail(LCTY_ERR_UNSUPPORTED, "k = %u: genome k-mer counts are built for k <= 31", k);
        if (counter_bytes < 1 || counter_bytes > 8)
            fail(LCTY_ERR_INVALID_INPUT, "Jellyfish was run with %u-byte counters, 1 to 8 bytes are allowed", counter_bytes);
        if (!cnt_off) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        usable(genome);
        const double t0 = now_ms();
        // stage 1: the query set
        const HapSet hs = check_haps(n_seqs, seqs, seq_off, HapLimits{0, 0x7FFFFFFFu, 1ull << 32});
        cnt_off[0] = 0;
        for (uint32_t a = 0; a < n_seqs; a++) cnt_off[a + 1] = cnt_off[a] + (hs.len(a) + 1 > k ? hs.len(a) + 1 - k : 0);
        const uint64_t n_values = cnt_off[n_seqs];
        if (n_values && !counts) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_values >= (1ull << 40)) fail(LCTY_ERR_UNSUPPORTED, "%llu query k-mers", static_cast<unsigned long long>(n_values));
        const uint32_t max_value = counter_bytes >= 2 ? 65535u : 255u;                    // counts.rs:297-303
        lcty_ctx* ctx = genome->ctx;
        ctx->activate();
        hipStream_t s = ctx->stream;
        lcty_genome_count_stats st{};
        st.scan_run = RUN;
        hipEvent_t ev[4];
        for (hipEvent_t& e : ev) LCTY_HIP(hipEventCreate(&e));
        struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 4; i++) (void)hipEventDestroy(e[i]); } } events{ev};

        DevHaps d;
        d.upload(ctx, hs, seqs, seq_off, 0);
        DevBuf<uint64_t> d_cnt_off;
        d_cnt_off.alloc(uint64_t(n_seqs) + 1); d_cnt_off.upload(cnt_off, uint64_t(n_seqs) + 1, s);
        DevBuf<unsigned long long> d_word;                                                // [0] first bad byte, [1] distinct keys, [2] hits
        d_word.alloc(3);
        LCTY_HIP(hipMemsetAsync(d_word.p, 0xFF, sizeof(unsigned long long), s));
        LCTY_HIP(hipMemsetAsync(d_word.p + 1, 0, 2 * sizeof(unsigned long long), s));
        LCTY_HIP(hipEventRecord(ev[0], s));
        if (hs.total) {
            hipLaunchKernelGGL(query_check_kernel, dim3(grid_for(hs.total)), dim3(THREADS), 0, s, d.seqs.p, hs.total, d_word.p);
            LCTY_HIP(hipGetLastError());
        }
        unsigned long long bad = 0;
        d_word.download(&bad, 1, s);
        LCTY_HIP(hipStreamSynchronize(s));
        if (bad != ~0ull) {
            const uint8_t b = seqs[bad];
            if (b == 'N') fail(LCTY_ERR_RUNTIME, "Cannot count k-mers for sequence with Ns");                              // counts.rs:326-328
            fail(LCTY_ERR_INVALID_INPUT, "byte 0x%02x at %llu of the query sequences: upper-case A, C, G, T only", b, bad);
        }
        // stage 2: the table. Sized for every query k-mer being distinct, counted, and rebuilt at the size the distinct ones need.
        DevBuf<uint64_t> keys;
        DevBuf<uint32_t> counters;
        uint64_t slots = keytable::table_slots(n_values, 1, 64);
        keys.alloc(slots);
        LCTY_HIP(hipMemsetAsync(keys.p, 0xFF, slots * sizeof(uint64_t), s));
        if (n_values) {
            hipLaunchKernelGGL(query_insert_kernel, dim3(grid_for(n_values)), dim3(THREADS), 0, s, d.seqs.p, d.off.p, d_cnt_off.p, n_seqs, k, n_values,
                               keys.p, slots - 1);
            LCTY_HIP(hipGetLastError());
            hipLaunchKernelGGL(keytable::table_count_kernel<UNDEF64>, dim3(grid_for(slots)), dim3(THREADS), 0, s, keys.p, slots, d_word.p + 1);
            LCTY_HIP(hipGetLastError());
        }
        unsigned long long n_distinct = 0;
        d_word.download(&n_distinct, 1, s, 1);
        LCTY_HIP(hipStreamSynchronize(s));
        const uint64_t small = keytable::table_slots(n_distinct, 1, 64);
        if (small < slots) {
            DevBuf<uint64_t> k2;
            k2.alloc(small);
            LCTY_HIP(hipMemsetAsync(k2.p, 0xFF, small * sizeof(uint64_t), s));
            hipLaunchKernelGGL((keytable::table_compact_kernel<keytable::MixHash, UNDEF64>), dim3(grid_for(slots)), dim3(THREADS), 0, s, keys.p, slots, k2.p, small - 1);
            LCTY_HIP(hipGetLastError());
            LCTY_HIP(hipStreamSynchronize(s));
            keys = std::move(k2); slots = small;
        }
        counters.alloc(slots);
        counters.zero(s);
        LCTY_HIP(hipEventRecord(ev[1], s));
        // stage 3: the scan
        if (n_values && genome->n_pos >= k) {
            const uint64_t threads = (genome->n_pos + RUN - 1) / RUN;
            const dim3 grid(blocks_of(threads, THREADS));
            bool merged = true;                                   // the other form is under measurement in the developer build only
            if constexpr (kDiag) merged = ctx->diag_knob("genome_scan_form", 0) != 1;
            if constexpr (kDiag) {
                if (!merged)
                    hipLaunchKernelGGL(genome_scan_kernel<false>, grid, dim3(THREADS), 0, s, genome->bases2.p, genome->nmask.p, genome->n_pos, k, keys.p,
                                       counters.p, slots - 1, d_word.p + 2);
            }
            if (merged)
                hipLaunchKernelGGL(genome_scan_kernel<true>, grid, dim3(THREADS), 0, s, genome->bases2.p, genome->nmask.p, genome->n_pos, k, keys.p,
                                   counters.p, slots - 1, d_word.p + 2);
            LCTY_HIP(hipGetLastError());
            st.n_scanned = genome->n_pos;
        }
        LCTY_HIP(hipEventRecord(ev[2], s));
        // stage 4: the gather
        DevBuf<uint16_t> d_counts;
        d_counts.alloc(std::max<uint64_t>(n_values, 1));
        if (n_values) {
            hipLaunchKernelGGL(query_gather_kernel, dim3(grid_for(n_values)), dim3(THREADS), 0, s, d.seqs.p, d.off.p, d_cnt_off.p, n_seqs, k, n_values,
                               keys.p, counters.p, slots - 1, max_value, d_counts.p);
            LCTY_HIP(hipGetLastError());
            d_counts.download(counts, n_values, s);
        }
        LCTY_HIP(hipEventRecord(ev[3], s));
        unsigned long long hits = 0;
        d_word.download(&hits, 1, s, 2);
        LCTY_HIP(hipStreamSynchronize(s));
        float ms = 0;
        LCTY_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); st.table_ms = ms;
        LCTY_HIP(hipEventElapsedTime(&ms, ev[1], ev[2])); st.scan_ms = ms;
        LCTY_HIP(hipEventElapsedTime(&ms, ev[2], ev[3])); st.gather_ms = ms;
        st.n_query_kmers = n_values; st.n_distinct = n_distinct; st.table_slots = slots; st.n_hits = hits;
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

}  // extern "C"
