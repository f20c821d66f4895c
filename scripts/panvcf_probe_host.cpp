// scripts/panvcf_probe_host.cpp — the serial loops behind lcty_panvcf.hip in ONE host thread, for scripts/panvcf_probe.py: the walk of
// reconstruct_sequences (src/seq/panvcf.rs:255-314: records outside, haplotypes inside, one growing sequence per haplotype) and the
// loops of find_best_boundary (src/command/add.rs:389-428: cumulative sums, the three clipped loops per record, the penalty, the
// arg-max). Their outputs must equal the device's. Each function returns its milliseconds.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

// out / out_off[n_cols + 1]: every column's sequence, concatenated (cap bytes; -1.0 when it does not fit). Records are kept when some
// column has allele >= 1; the interval's ends are assumed clear (the probe plants no record over them).
extern "C" double panvcf_probe_host_reconstruct(uint32_t ref_start, uint32_t ref_end, const uint8_t* ref, uint32_t n_recs, const uint32_t* pos,
                                                const uint32_t* rlen, const uint32_t* rec_allele, const uint64_t* allele_off, const uint8_t* pool,
                                                uint32_t n_cols, const int16_t* gt, uint8_t* out, uint64_t cap, uint64_t* out_off, uint32_t* unknown,
                                                uint64_t* total_overlaps) {
    const double t0 = now_ms();
    std::vector<std::string> seqs(n_cols);
    for (std::string& s : seqs) s.reserve(uint64_t(ref_end - ref_start) * 3 / 2);
    std::vector<uint32_t> ref_pos(n_cols, ref_start);
    std::memset(unknown, 0, 4ull * n_cols);
    uint64_t overlaps = 0;
    for (uint32_t v = 0; v < n_recs; v++) {
        const int16_t* row = gt + uint64_t(v) * n_cols;
        bool variation = false;
        for (uint32_t c = 0; c < n_cols && !variation; c++) variation = row[c] >= 1;
        if (!variation) continue;
        const uint32_t var_start = pos[v], var_end = var_start + rlen[v];
        if (var_end <= ref_start) continue;
        if (ref_end <= var_start) break;
        for (uint32_t c = 0; c < n_cols; c++) {
            int32_t a = row[c];
            if (a < 0) { unknown[c] += rlen[v]; a = 0; }
            if (a == 0) continue;
            const uint32_t prev_end = ref_pos[c];
            if (var_start < prev_end) { overlaps++; continue; }
            seqs[c].append(reinterpret_cast<const char*>(ref) + (prev_end - ref_start), var_start - prev_end);
            const uint64_t ai = uint64_t(rec_allele[v]) + uint32_t(a);
            seqs[c].append(reinterpret_cast<const char*>(pool) + allele_off[ai], allele_off[ai + 1] - allele_off[ai]);
            ref_pos[c] = var_end;
        }
    }
    uint64_t total = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        if (ref_pos[c] < ref_end) seqs[c].append(reinterpret_cast<const char*>(ref) + (ref_pos[c] - ref_start), ref_end - ref_pos[c]);
        out_off[c] = total; total += seqs[c].size();
    }
    out_off[n_cols] = total;
    *total_overlaps = overlaps;
    const double ms = now_ms() - t0;
    if (total > cap) return -1.0;
    for (uint32_t c = 0; c < n_cols; c++) std::memcpy(out + out_off[c], seqs[c].data(), seqs[c].size());
    return ms;
}

extern "C" double panvcf_probe_host_boundary(uint32_t start, uint32_t end, uint32_t n_recs, const uint32_t* pos, const uint32_t* rlen, uint32_t k,
                                             const uint16_t* counts, uint64_t n_counts, uint32_t allowed_expansion, uint32_t moving_window, int32_t left,
                                             double* weights, int32_t* found, uint32_t* position) {
    const double t0 = now_ms();
    std::vector<uint32_t> cumul(n_counts + 1, 0);
    for (uint64_t i = 0; i < n_counts; i++) cumul[i + 1] = cumul[i] + (counts[i] <= 1 ? 1u : 0u);
    const uint32_t per_window = moving_window + 1 - k, n = end - start;
    const double divisor = static_cast<double>(per_window);
    for (uint32_t i = 0; i < n; i++) weights[i] = static_cast<double>(cumul[i + per_window] - cumul[i]) / divisor;
    auto sat = [](uint64_t a, uint64_t b) { return a > b ? a - b : 0; };
    for (uint32_t r = 0; r < n_recs; r++) {
        const uint64_t vs = pos[r], ve = vs + rlen[r];
        for (uint64_t i = sat(vs, start); i < sat(ve < end ? ve : end, start); i++) weights[i] = 0.0;
        for (uint64_t i = sat(vs, end), hi = sat(vs, start) < 9 ? sat(vs, start) : 9; i < hi; i++) weights[vs - start - i - 1] *= static_cast<double>(9 - i) / 10.0;
        for (uint64_t i = sat(start, ve), hi = sat(end, ve) < 9 ? sat(end, ve) : 9; i < hi; i++) weights[ve + i - start] *= static_cast<double>(i + 1) / 10.0;
    }
    const double per_bp_drop = 0.2 / static_cast<double>(allowed_expansion);
    uint32_t best = 0;
    if (left) {
        for (uint32_t i = 0; i < n; i++) { double& w = weights[n - 1 - i]; const double t = w * per_bp_drop; w -= t * static_cast<double>(i); }
        for (uint32_t i = 1; i < n; i++) if (weights[i] >= weights[best]) best = i;
    } else {
        for (uint32_t i = 0; i < n; i++) { double& w = weights[i]; const double t = w * per_bp_drop; w -= t * static_cast<double>(i); }
        for (uint32_t i = 1; i < n; i++) if (weights[i] > weights[best]) best = i;
    }
    *found = weights[best] != 0.0;
    *position = start + best;
    return now_ms() - t0;
}
