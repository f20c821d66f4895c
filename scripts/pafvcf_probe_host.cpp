// scripts/pafvcf_probe_host.cpp — the serial loops behind lcty_pafvcf.hip in ONE host thread, for scripts/pafvcf_probe.py, stage by stage as
// src/command/paf_vcf.rs has them: process_haplotype + move_all_left per haplotype (276-332, 242-271), the sort / dedup / merge of
// combine_variants (535-555), get_hap_ranges and the allele comparison of write_vcf per range and haplotype (420-460, 481-494), and the
// text (500-516). Every entry has the reference as its target and every haplotype one entry (the probe makes them so). The body it
// writes must equal the device's. ms[4]: variants, ranges, table, text.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct Var { uint32_t rs, re, hs, he; };
struct Slice { const uint8_t* p; uint32_t n; };
}  // namespace

extern "C" void pafvcf_probe_host_free(char* p) { free(p); }

// returns 0, or -1 for an operation other than = X I D
extern "C" int pafvcf_probe_host(uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint32_t ref_id, uint64_t n_entries, const uint32_t* id1,
                                 const uint64_t* cigar_off, const uint32_t* cigar, uint32_t n_slots, const uint32_t* slot_hap, const uint8_t* slot_first,
                                 const char* chrom, uint32_t shift, double* ms, uint64_t* n_variants, uint64_t* n_merged, char** text, uint64_t* text_len) {
    const uint8_t* ref = seqs + seq_off[ref_id];
    // 1. variants
    double t = now_ms();
    std::vector<std::vector<Var>> vars(n_seqs);
    std::vector<uint8_t> has(n_seqs, 0);
    has[ref_id] = 1;
    uint64_t total = 0;
    for (uint64_t e = 0; e < n_entries; e++) {
        const uint32_t h = id1[e];
        const uint8_t* hap = seqs + seq_off[h];
        std::vector<Var> v;
        uint32_t rpos = 0, qpos = 0;
        for (uint64_t k = cigar_off[e]; k < cigar_off[e + 1]; k++) {
            const uint32_t op = cigar[k] & 15u, len = cigar[k] >> 4;
            if (op == 7) { rpos += len; qpos += len; continue; }
            if (op != 8 && op != 1 && op != 2) return -1;
            const uint32_t qd = op == 2 ? 0 : len, rd = op == 1 ? 0 : len;
            bool need_new = true;
            if (!v.empty() && rpos <= v.back().re && qpos <= v.back().he) {
                v.back().re = std::max(v.back().re, rpos + rd); v.back().he = std::max(v.back().he, qpos + qd);
                need_new = false;
            }
            if (need_new) {
                if (rd == qd) v.push_back({rpos, rpos + rd, qpos, qpos + qd});
                else if (rpos == 0 || qpos == 0) v.push_back({rpos, rpos + rd + 1, qpos, qpos + qd + 1});
                else v.push_back({rpos - 1, rpos + rd, qpos - 1, qpos + qd});
            }
            rpos += rd; qpos += qd;
        }
        uint32_t last_end = 0;
        for (Var& x : v) {                                              // move_all_left
            const uint32_t min_start = last_end;
            last_end = x.re;
            const uint32_t rl = x.re - x.rs, al = x.he - x.hs, prefix = std::min(rl, al);
            if (rl == al || memcmp(ref + x.rs, hap + x.hs, prefix)) continue;
            const uint8_t* gap = prefix == rl ? hap + x.hs + prefix : ref + x.rs + prefix;
            const uint32_t last = std::max(rl, al) - prefix - 1;
            uint32_t gs = x.rs + prefix, k = last;
            while (gs > min_start + prefix && gap[k] == ref[gs - 1]) { gs--; k = k ? k - 1 : last; }
            const uint32_t s = x.rs + prefix - gs;
            x.rs -= s; x.re -= s; x.hs -= s; x.he -= s;
        }
        total += v.size();
        vars[h] = std::move(v); has[h] = 1;
    }
    ms[0] = now_ms() - t;
    // 2. ranges
    t = now_ms();
    std::vector<std::pair<uint32_t, uint32_t>> uniq;
    uniq.reserve(total);
    for (const auto& v : vars) for (const Var& x : v) uniq.emplace_back(x.rs, x.re);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<std::pair<uint32_t, uint32_t>> merged;
    for (const auto& r : uniq) {
        if (!merged.empty() && merged.back().second > r.first) merged.back().second = std::max(merged.back().second, r.second);
        else merged.push_back(r);
    }
    ms[1] = now_ms() - t;
    // 3. table (range-major, as write_vcf walks it) and 4. text; the two are timed apart inside one loop over the ranges
    double table_ms = 0, text_ms = 0;
    std::string out;
    std::vector<int32_t> ix(n_seqs);
    std::vector<Slice> alleles;
    const size_t chrom_len = strlen(chrom);
    for (const auto& r : merged) {
        t = now_ms();
        const uint32_t start = r.first, end = r.second, diff = end - start;
        alleles.clear();
        alleles.push_back({ref + start, diff});
        for (uint32_t h = 0; h < n_seqs; h++) {
            ix[h] = -1;
            if (!has[h]) continue;
            const std::vector<Var>& v = vars[h];
            uint32_t hs, he;
            if (v.empty()) { hs = start; he = end; }
            else {
                const size_t n = v.size();
                const size_t i = std::partition_point(v.begin(), v.end(), [&](const Var& x) { return x.re <= start; }) - v.begin();
                const size_t j = std::partition_point(v.begin() + i, v.end(), [&](const Var& x) { return x.rs < end; }) - v.begin();
                if (i == n) { hs = v[n - 1].he + (start - v[n - 1].re); he = hs + diff; }
                else if (i == j) { hs = v[i].hs - (v[i].rs - start); he = hs + diff; }
                else if (start <= v[i].rs && v[j - 1].re <= end) { hs = v[i].hs - (v[i].rs - start); he = v[j - 1].he + (end - v[j - 1].re); }
                else continue;
            }
            const uint8_t* a = seqs + seq_off[h] + hs;
            if (memchr(a, 'N', he - hs)) continue;
            size_t k = 0;
            for (; k < alleles.size(); k++) if (alleles[k].n == he - hs && !memcmp(alleles[k].p, a, he - hs)) break;
            if (k == alleles.size()) alleles.push_back({a, he - hs});
            ix[h] = static_cast<int32_t>(k);
        }
        table_ms += now_ms() - t;
        if (alleles.size() == 1) continue;
        t = now_ms();
        out.append(chrom, chrom_len); out += '\t'; out += std::to_string(uint64_t(start) + shift + 1); out += "\t.";
        for (size_t k = 0; k < alleles.size(); k++) { out += k <= 1 ? '\t' : ','; out.append(reinterpret_cast<const char*>(alleles[k].p), alleles[k].n); }
        out += "\t60\t.\t.\tGT";
        for (uint32_t s = 0; s < n_slots; s++) {
            out += slot_first[s] ? '\t' : '|';
            const int32_t v = slot_hap[s] == 0xFFFFFFFFu ? -1 : ix[slot_hap[s]];
            if (v < 0) out += '.'; else out += std::to_string(v);
        }
        out += '\n';
        text_ms += now_ms() - t;
    }
    ms[2] = table_ms; ms[3] = text_ms;
    *n_variants = total; *n_merged = merged.size();
    *text = static_cast<char*>(malloc(out.size() ? out.size() : 1));
    if (!*text) return -2;
    memcpy(*text, out.data(), out.size());
    *text_len = out.size();
    return 0;
}
