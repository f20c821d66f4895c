// The reference's algorithm as the comparison point of scripts/db_probe.py: jaccard_distance (src/seq/minim_div.rs:16-40), the
// two-pointer merge of two sorted lists, over all pairs in `threads` host threads (divergences_multithread, minim_div.rs:74-110).
// Plain C++, -O3; returns the milliseconds and leaves the non-shared counts in uniq[n (n - 1) / 2].
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

extern "C" double db_probe_merge(uint32_t n, const uint64_t* min_off, const uint64_t* hashes, uint32_t threads, uint32_t* uniq) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> row_start(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) row_start[i + 1] = row_start[i] + (n - 1 - i);
    const uint64_t n_pairs = row_start[n];
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            const uint64_t lo = n_pairs * t / threads, hi = n_pairs * (t + 1) / threads;
            uint32_t i = 0;
            while (row_start[i + 1] <= lo && i + 1 < n) i++;
            for (uint64_t p = lo; p < hi; p++) {
                while (row_start[i + 1] <= p) i++;
                const uint32_t j = static_cast<uint32_t>(i + 1 + (p - row_start[i]));
                const uint64_t *x = hashes + min_off[i], *xe = hashes + min_off[i + 1], *y = hashes + min_off[j], *ye = hashes + min_off[j + 1];
                const uint32_t n1 = static_cast<uint32_t>(xe - x), n2 = static_cast<uint32_t>(ye - y);
                uint32_t overlap = 0;
                while (x != xe && y != ye) {
                    if (*x == *y) { overlap++; x++; y++; }
                    else if (*x < *y) x++;
                    else y++;
                }
                uniq[p] = n1 + n2 - 2 * overlap;
            }
        });
    for (auto& th : pool) th.join();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
