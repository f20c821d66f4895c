// scripts/kmer_count_probe_host.cpp — for scripts/kmer_count_probe.py: the synthetic genome, and the loop of lcty_genome_kmer_counts
// (lcty_genome.hip: table of the query's distinct canonical k-mers, one pass over the genome, gather) in `threads` host threads on
// the ASCII genome. The values it returns must equal the device's. ms[3]: table, scan, gather.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
inline uint32_t enc(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}
constexpr uint64_t FREE = ~0ull;
constexpr uint64_t BLOCK = 1ull << 20;

template <typename F>
void in_threads(uint32_t threads, F&& body) {
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; t++) pool.emplace_back([&body, t] { body(t); });
    for (std::thread& th : pool) th.join();
}

// calls use(start, canonical k-mer) for every window of k bases of s[from, to) (a window may start before `first_start`: those are skipped)
template <typename F>
void roll(const uint8_t* s, uint64_t from, uint64_t to, uint64_t first_start, uint32_t k, F&& use) {
    const uint64_t kmask = (1ull << (2 * k)) - 1;
    const uint32_t shift = 2 * k - 2;
    uint64_t fw = 0, rv = 0;
    uint32_t valid = 0;
    for (uint64_t i = from; i < to; i++) {
        const uint32_t e = enc(s[i]);
        if (e > 3) { valid = 0; continue; }
        fw = ((fw << 2) | e) & kmask;
        rv = (rv >> 2) | (static_cast<uint64_t>(3 - e) << shift);
        if (++valid >= k && i + 1 - k >= first_start) use(i + 1 - k, fw < rv ? fw : rv);
    }
}
}  // namespace

// n bases, block by block from (seed, block index) alone: random bases; in `repeat_pct` % of the blocks copies of one 4 kb unit and
// poly-A runs take three quarters of the block (the planted repeats); every fourth block is lower case (soft-masked); the first
// 10 000 bases of every `contig_len` are N.
extern "C" void kmer_probe_make_genome(uint64_t seed, uint64_t n, uint64_t contig_len, uint32_t repeat_pct, uint32_t threads, uint8_t* out) {
    std::vector<uint8_t> unit(4096);
    uint64_t u = mix64(seed ^ 0x9E3779B97F4A7C15ull);
    for (uint8_t& c : unit) { u = mix64(u + 1); c = "ACGT"[u & 3]; }
    const uint64_t n_blocks = (n + BLOCK - 1) / BLOCK;
    std::atomic<uint64_t> next{0};
    in_threads(threads, [&](uint32_t) {
        for (uint64_t b = next++; b < n_blocks; b = next++) {
            const uint64_t lo = b * BLOCK, hi = std::min<uint64_t>(n, lo + BLOCK);
            uint64_t x = mix64(seed + 0x632BE59BD9B4E019ull * (b + 1));
            for (uint64_t i = lo; i < hi; i += 32) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                for (uint64_t j = i; j < std::min<uint64_t>(hi, i + 32); j++) out[j] = "ACGT"[(x >> (2 * (j - i))) & 3];
            }
            if (mix64(x) % 100 < repeat_pct)
                for (uint64_t i = lo; i + unit.size() <= hi; i += unit.size())
                    if ((i / unit.size()) % 4 == 3) memset(out + i, 'A', 1024);
                    else if ((i / unit.size()) % 4 != 0) memcpy(out + i, unit.data(), unit.size());
            if (b % 4 == 1) for (uint64_t i = lo; i < hi; i++) out[i] |= 0x20;
        }
    });
    for (uint64_t c = 0; c < n; c += contig_len) memset(out + c, 'N', std::min<uint64_t>(10000, n - c));
}

// contigs at [contig_off[c], contig_off[c + 1]) of genome; values as lcty_genome_kmer_counts lays them out (max_value 65 535)
extern "C" int kmer_probe_host_counts(const uint8_t* genome, const uint64_t* contig_off, uint32_t n_contigs, uint32_t k, const uint8_t* seqs,
                                      const uint64_t* seq_off, uint32_t n_seqs, uint32_t threads, uint16_t* counts, double* ms, uint64_t* n_distinct,
                                      uint64_t* n_hits) {
    double t = now_ms();
    uint64_t n_values = 0;
    std::vector<uint64_t> cnt_off(n_seqs + 1, 0);
    for (uint32_t a = 0; a < n_seqs; a++) {
        const uint64_t len = seq_off[a + 1] - seq_off[a];
        cnt_off[a + 1] = cnt_off[a] + (len + 1 > k ? len + 1 - k : 0);
    }
    n_values = cnt_off[n_seqs];
    uint64_t slots = 64;
    while (slots < 2 * n_values) slots <<= 1;
    std::vector<uint64_t> keys(slots, FREE);
    uint64_t distinct = 0;
    for (uint32_t a = 0; a < n_seqs; a++)
        roll(seqs, seq_off[a], seq_off[a + 1], seq_off[a], k, [&](uint64_t, uint64_t key) {
            uint64_t s = mix64(key) & (slots - 1);
            while (keys[s] != FREE && keys[s] != key) s = (s + 1) & (slots - 1);
            if (keys[s] == FREE) { keys[s] = key; distinct++; }
        });
    uint64_t small = 64;
    while (small < 2 * distinct) small <<= 1;
    if (small < slots) {
        std::vector<uint64_t> k2(small, FREE);
        for (uint64_t key : keys)
            if (key != FREE) {
                uint64_t s = mix64(key) & (small - 1);
                while (k2[s] != FREE) s = (s + 1) & (small - 1);
                k2[s] = key;
            }
        keys.swap(k2); slots = small;
    }
    std::vector<std::atomic<uint32_t>> counters(slots);
    for (auto& c : counters) c.store(0, std::memory_order_relaxed);
    ms[0] = now_ms() - t; t = now_ms();
    // the scan: every contig in spans of 4 Mb, handed out to the threads
    struct Span { uint64_t from, to, first; };
    std::vector<Span> spans;
    for (uint32_t c = 0; c < n_contigs; c++)
        for (uint64_t at = contig_off[c]; at < contig_off[c + 1]; at += 4ull << 20)
            spans.push_back(Span{at, std::min<uint64_t>(contig_off[c + 1], at + (4ull << 20) + k - 1), at});
    std::atomic<uint64_t> next{0}, hits{0};
    const uint64_t mask = slots - 1;
    in_threads(threads, [&](uint32_t) {
        uint64_t mine = 0;
        for (uint64_t i = next++; i < spans.size(); i = next++)
            roll(genome, spans[i].from, spans[i].to, spans[i].first, k, [&](uint64_t, uint64_t key) {
                uint64_t s = mix64(key) & mask;
                while (keys[s] != FREE && keys[s] != key) s = (s + 1) & mask;
                if (keys[s] == key) { counters[s].fetch_add(1, std::memory_order_relaxed); mine++; }
            });
        hits += mine;
    });
    ms[1] = now_ms() - t; t = now_ms();
    for (uint32_t a = 0; a < n_seqs; a++)
        roll(seqs, seq_off[a], seq_off[a + 1], seq_off[a], k, [&](uint64_t start, uint64_t key) {
            uint64_t s = mix64(key) & mask;
            while (keys[s] != key) s = (s + 1) & mask;
            const uint32_t c = counters[s].load(std::memory_order_relaxed);
            counts[cnt_off[a] + (start - seq_off[a])] = static_cast<uint16_t>(std::max(std::min(c, 65535u), 1u));
        });
    ms[2] = now_ms() - t;
    *n_distinct = distinct; *n_hits = hits.load();
    return 0;
}
