// lcty_map_index.hip — the k-mer index of the basis alleles (lcty_locus_build_map_index), built on the device.
//
// What the mapper's kernels look up (lcty_map.hip, lcty_map_long.hip): an open-addressing table canonical k-mer -> run of places,
// a place = basis allele << 33 | position << 1 | (the forward k-mer is the canonical one), the run of a k-mer in (basis allele,
// position) order. Round 3 made it on the host (a sort of 12.8 M pairs for 256 alleles of 50 kb: 1.1 s per locus, 2.5 times the
// mapping call of 2 048 long reads). Here: one thread per window writes (k-mer, place) — windows with a base other than ACGT get the
// key ~0 and sort behind everything —, a stable radix sort by k-mer (below; the places were written in (allele, position) order and
// stay so inside a run), heads of runs by comparison with the left neighbour, their starts by a prefix sum, and one thread per run
// claims a slot of the key table (lcty_table.hpp).
//
// The sort (RadixSort, lcty_sort.hpp): least significant digit first, eight bits a pass, over the bytes a k-mer of this
// k can differ in plus the top byte (where the key of a window without a k-mer differs from all of them). A pass is three steps over
// tiles of 4 096 pairs, a wavefront per tile: the tile's count of every digit value (LDS atomics) into a [256][tiles] matrix; the
// exclusive prefix sums of that matrix in (digit, tile) order — the first place in the output of every (digit value, tile) —; and the
// scatter, in which the wavefront goes over its tile 64 pairs at a time, in order: the lanes that hold the same digit value find each
// other by eight ballots, the first of them takes their places from the tile's running counter of that value (LDS), a lane's place is
// that plus its rank among its peers. Pairs with equal digits keep their order: stable. The run starts take ScanTotal (lcty_scan.hpp).

#include "lcty_common.hpp"
#include "lcty_map_internal.hpp"
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"

namespace lcty {
namespace {

// window w of the concatenated windows of the basis alleles: win_off[b] <= w < win_off[b + 1]
__global__ __launch_bounds__(256) void index_pairs_kernel(const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ seq_off,
                                                          const uint16_t* __restrict__ basis, const uint64_t* __restrict__ win_off, uint32_t n_basis,
                                                          uint32_t k, uint64_t n_windows, uint64_t* __restrict__ keys, uint64_t* __restrict__ places,
                                                          unsigned long long* __restrict__ n_invalid) {
    const uint64_t w = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    uint32_t bad = 0;
    if (w < n_windows) {
        const uint32_t b = flat_owner(win_off, n_basis, w);          // the allele of this window
        const uint64_t i = w - win_off[b];
        uint64_t kmer;
        bool fwd;                                                    // fw <= rv: a palindrome's place counts as forward
        const bool ok = canonical_kmer_ascii(seqs + seq_off[basis[b]], i, k, &kmer, &fwd);
        keys[w] = ok ? kmer : UNDEF64;
        places[w] = (static_cast<uint64_t>(b) << 33) | (i << 1) | (fwd ? 1ull : 0ull);
        bad = ok ? 0u : 1u;
    }
    const unsigned long long m = __ballot(bad != 0);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(n_invalid, static_cast<unsigned long long>(__popcll(m)));
}

__global__ __launch_bounds__(256) void index_heads_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) head[i] = i == 0 || keys[i] != keys[i - 1] ? 1u : 0u;
}

// run r starts at the element whose exclusive prefix sum of heads is r and that is a head
__global__ __launch_bounds__(256) void index_starts_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank, uint64_t n,
                                                           uint32_t* __restrict__ run_start) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && head[i]) run_start[rank[i]] = static_cast<uint32_t>(i);
}

__global__ __launch_bounds__(256) void index_insert_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ run_start, uint32_t n_runs,
                                                           uint32_t n_valid, keytable::Slot* __restrict__ table, uint64_t mask) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t start = run_start[r], end = r + 1 < n_runs ? run_start[r + 1] : n_valid;
    const uint64_t key = keys[start];
    const uint64_t h = keytable::claim<keytable::FastHash, UNDEF64>(table, mask, key).slot;      // every k-mer has one run: nobody else asks for this key
    table[h].start = start; table[h].count = end - start;
}

}  // namespace

std::shared_ptr<MapIndex> build_map_index_device(lcty_locus* locus, const uint16_t* basis, uint32_t n_basis, uint32_t k) {
    lcty_ctx* ctx = locus->ctx;
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> seq_off(locus->n_alleles + 1);
    locus->d_seq_off.download(seq_off.data(), seq_off.size(), s);
    LCTY_HIP(hipStreamSynchronize(s));
    std::vector<uint64_t> win_off(n_basis + 1, 0);
    for (uint32_t b = 0; b < n_basis; b++) {
        const uint64_t len = seq_off[basis[b] + 1] - seq_off[basis[b]];
        win_off[b + 1] = win_off[b] + (len >= k ? len + 1 - k : 0);
    }
    const uint64_t n_windows = win_off[n_basis];
    if (n_windows >= 0x7FFFFFF0ull) fail(LCTY_ERR_UNSUPPORTED, "more than 2^31 k-mer places in the basis alleles");   // places and run starts are 32-bit; the sort's offsets too
    auto ix = std::make_shared<MapIndex>();
    ix->basis.alloc(n_basis); ix->basis.upload(basis, n_basis, s);
    ix->k = k; ix->n_basis = n_basis;
    DevBuf<uint64_t> d_win_off, keys_a, keys_b, places_a;
    DevBuf<unsigned long long> d_counts;
    DevBuf<uint32_t> head, rank, run_start;
    d_win_off.alloc(n_basis + 1); d_win_off.upload(win_off.data(), n_basis + 1, s);
    d_counts.alloc(1); d_counts.zero(s);
    const size_t n = static_cast<size_t>(std::max<uint64_t>(n_windows, 1));
    keys_a.alloc(n); keys_b.alloc(n); places_a.alloc(n);
    ix->entries.alloc(n);
    unsigned long long n_invalid = 0;
    uint32_t n_valid = 0, n_runs = 0;
    if (n_windows) {
        // the bytes of the key that matter: those below bit 2 k, and the top one (the key of a window without a k-mer is ~0)
        std::vector<uint32_t> shifts;
        for (uint32_t b = 0; b < 8 && 8 * b < 2 * k; b++) shifts.push_back(8 * b);
        if (shifts.back() != 56) shifts.push_back(56);
        // the pairs are written where the sort's result (the parity of the number of passes) is (keys_b, entries)
        uint64_t* ka = keys_a.p; uint64_t* va = places_a.p; uint64_t* kb = keys_b.p; uint64_t* vb = ix->entries.p;
        if (shifts.size() % 2 == 0) { std::swap(ka, kb); std::swap(va, vb); }
        const uint32_t blocks = static_cast<uint32_t>((n_windows + 255) / 256);
        hipLaunchKernelGGL(index_pairs_kernel, dim3(blocks), dim3(256), 0, s, locus->d_seqs.p, locus->d_seq_off.p, ix->basis.p, d_win_off.p, n_basis, k,
                           n_windows, ka, va, d_counts.p);
        LCTY_HIP(hipGetLastError());
        RadixSort sort;
        sort.run(ka, va, kb, vb, n_windows, shifts, s);
        d_counts.download(&n_invalid, 1, s);
        LCTY_HIP(hipStreamSynchronize(s));
        n_valid = static_cast<uint32_t>(n_windows - n_invalid);
    }
    if (n_valid) {
        const uint32_t blocks = (n_valid + 255) / 256;
        head.alloc(n_valid);
        hipLaunchKernelGGL(index_heads_kernel, dim3(blocks), dim3(256), 0, s, keys_b.p, static_cast<uint64_t>(n_valid), head.p);
        LCTY_HIP(hipGetLastError());
        ScanTotal scan;
        n_runs = scan.run(head, rank, n_valid, ctx);
        run_start.alloc(n_runs);
        hipLaunchKernelGGL(index_starts_kernel, dim3(blocks), dim3(256), 0, s, head.p, rank.p, static_cast<uint64_t>(n_valid), run_start.p);
        LCTY_HIP(hipGetLastError());
    }
    const uint64_t cap = keytable::table_slots(n_runs, 1, 1024);
    ix->table.alloc(cap);
    LCTY_HIP(hipMemsetAsync(ix->table.p, 0xFF, cap * sizeof(keytable::Slot), s));   // key ~0 = free (start / count of a free slot are never read)
    ix->mask = cap - 1;
    if (n_runs) {
        hipLaunchKernelGGL(index_insert_kernel, dim3((n_runs + 255) / 256), dim3(256), 0, s, keys_b.p, run_start.p, n_runs, n_valid, ix->table.p, ix->mask);
        LCTY_HIP(hipGetLastError());
    }
    LCTY_HIP(hipStreamSynchronize(s));
    return ix;
}

}  // namespace lcty
