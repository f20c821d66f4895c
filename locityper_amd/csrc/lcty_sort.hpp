// lcty_sort.hpp — a stable least-significant-digit radix sort of 64-bit keys, with or without a 64-bit value each, eight bits a pass
// (DESIGN.md 4.18): the k-mer index of the read mapper (lcty_map_index.hip) and the variant ranges of lcty_pafvcf.hip. The kernels, the
// multi-workgroup scan they use (lcty_scan.hpp) and the pass loop are in lcty_sort.hip.
#pragma once

#include "lcty_common.hpp"

namespace lcty {

// The counts of every (digit value, tile), their prefix sums and the scratch of the scan: grow-only, so one object serves sort after sort.
struct RadixSort {
    DevBuf<uint32_t> counts, first, tmp;
    // One pass per entry of `shifts`, in that order, each by the eight bits of the key from that shift up: pass 1 reads
    // (keys_a, vals_a) and writes (keys_b, vals_b), pass 2 the other way, and so on. Pairs that agree in all those bytes keep their
    // order. vals_a and vals_b null: keys alone. n < 2^32 (the offsets are 32-bit). Asynchronous on s. Returns which pair holds the
    // result: 0 for (keys_a, vals_a), 1 for (keys_b, vals_b) — the parity of shifts.size(); the other pair holds the pass before.
    int run(uint64_t* keys_a, uint64_t* vals_a, uint64_t* keys_b, uint64_t* vals_b, uint64_t n, const std::vector<uint32_t>& shifts, hipStream_t s);
};

}  // namespace lcty
