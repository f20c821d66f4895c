// The reference's algorithm as the comparison point of scripts/basis_probe.py: Cigar::locally_similar (src/seq/cigar.rs:660-751), the
// serial two-pointer walk, for both sides of every entry in `threads` host threads, setting the bits of update_bitarray
// (src/command/augment.rs:291-312) in the same row table as the device. Plain C++, -O3; returns the milliseconds.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

namespace {
inline bool moves(uint32_t op, bool in_query) { return op == 0 || op == 7 || op == 8 || op == (in_query ? 1u : 2u); }

template <typename F>
void locally_similar(const uint32_t* cg, uint64_t n, bool in_query, uint32_t window, uint32_t step, uint32_t max_edit, F&& push) {
    uint32_t pos2 = 0, edit = 0, rem2 = 0, op2 = 0;
    uint64_t i2 = 0;
    for (;;) {
        if (i2 == n) { if (edit <= max_edit) push(0u); return; }
        const uint32_t op = cg[i2] & 15, len = cg[i2] >> 4;
        i2++;
        if (moves(op, in_query)) {
            const uint32_t window_rem = window - pos2, shift = len < window_rem ? len : window_rem;
            edit += op != 7 ? shift : 0;
            pos2 += shift;
            if (len > window_rem) { rem2 = len - window_rem; op2 = op; break; }
        } else edit += len;
    }
    uint64_t i1 = 1;
    uint32_t op1 = cg[0] & 15, rem1 = cg[0] >> 4, pos1 = 0;
    for (;;) {
        const uint32_t shift = rem1 < rem2 ? rem1 : rem2;
        const bool m1 = moves(op1, in_query), m2 = moves(op2, in_query);
        const bool upd1 = m1 == m2 || !m1, upd2 = m1 == m2 || !m2;
        if (m1 && m2) {
            const uint32_t k1 = op1 != 7 ? ~0u : 0u, k2 = op2 != 7 ? ~0u : 0u;
            for (uint64_t pos = (uint64_t(pos1) + step - 1) / step * step; pos < uint64_t(pos1) + shift; pos += step) {
                const uint32_t cs = static_cast<uint32_t>(pos - pos1);
                if (edit + (k2 & cs) - (k1 & cs) <= max_edit) push(static_cast<uint32_t>(pos / step));
            }
            pos1 += shift; pos2 += shift;
            edit = edit + (k2 & shift) - (k1 & shift);
        } else edit = edit + (upd2 ? shift : 0) - (upd1 ? shift : 0);
        if (upd2) {
            if (shift == rem2) {
                if (i2 == n) break;
                op2 = cg[i2] & 15; rem2 = cg[i2] >> 4; i2++;
            } else rem2 -= shift;
        }
        if (upd1) {
            if (shift == rem1) { op1 = cg[i1] & 15; rem1 = cg[i1] >> 4; i1++; }
            else rem1 -= shift;
        }
    }
    if (edit <= max_edit) push((pos1 + step - 1) / step);
}
}  // namespace

extern "C" double basis_probe_walk(uint64_t n_entries, const uint32_t* id1, const uint32_t* id2, const uint32_t* n_matches, const uint32_t* aln_len,
                                   const uint64_t* cigar_off, const uint32_t* cigar, const uint32_t* lens, const uint64_t* win_off, uint32_t words,
                                   uint32_t window, uint32_t step, uint32_t max_edit, double divergence, uint32_t threads, uint32_t* bits) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (uint64_t e = t; e < n_entries; e += threads) {
                if (id1[e] == id2[e] || cigar_off[e + 1] == cigar_off[e]) continue;
                const double gdiv = aln_len[e] == 0 ? 1.0 : double(aln_len[e] - n_matches[e]) / double(aln_len[e]);
                for (int side = 0; side < 2; side++) {
                    const uint32_t contig = side ? id2[e] : id1[e], other = side ? id1[e] : id2[e];
                    auto push = [&](uint32_t w) {
                        reinterpret_cast<std::atomic<uint32_t>*>(bits + (win_off[contig] + w) * words + (other >> 5))->fetch_or(1u << (other & 31),
                                                                                                                             std::memory_order_relaxed);
                    };
                    if (lens[contig] <= window) { if (gdiv <= divergence) push(0u); }
                    else locally_similar(cigar + cigar_off[e], cigar_off[e + 1] - cigar_off[e], side == 0, window, step, max_edit, push);
                }
            }
        });
    for (auto& th : pool) th.join();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
