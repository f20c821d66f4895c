// scripts/prune_probe_host.cpp — the merge loop of lcty_prune.hip in ONE host thread, for scripts/prune_probe.py: the same contract
// (labels, tie rule over labels), the same caches (per matrix slot the minimum of its row and the slot of smallest label among the
// minima; after a merge only the rows whose cached partner was merged are scanned again), the full symmetric matrix in memory.
// Its steps must equal the device's. Returns the milliseconds of the merge loop; *build_ms the matrix and the first caches.
#include <chrono>
#include <cstdint>
#include <limits>
#include <vector>

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;
struct Step { uint32_t cluster1, cluster2; double dissimilarity; uint32_t size, pad; };
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void scan_row(const std::vector<double>& D, const std::vector<uint32_t>& lab, uint32_t n, uint32_t r, double& out_d, uint32_t& out_slot) {
    double bd = std::numeric_limits<double>::infinity();
    uint32_t bl = NONE, bs = NONE;
    const double* row = D.data() + uint64_t(r) * n;
    for (uint32_t x = 0; x < n; x++) {
        const uint32_t l = lab[x];
        if (l == NONE || x == r) continue;
        if (row[x] < bd || (row[x] == bd && l < bl)) { bd = row[x]; bl = l; bs = x; }
    }
    out_d = bd; out_slot = bs;
}
}  // namespace

extern "C" double prune_probe_host(uint32_t n, const double* tri, Step* steps, double* build_ms) {
    double t0 = now_ms();
    std::vector<double> D(uint64_t(n) * n, std::numeric_limits<double>::infinity());
    uint64_t k = 0;
    for (uint32_t i = 0; i + 1 < n; i++)
        for (uint32_t j = i + 1; j < n; j++, k++) D[uint64_t(i) * n + j] = D[uint64_t(j) * n + i] = tri[k];
    std::vector<uint32_t> lab(n), rpart(n), size(n, 1);
    std::vector<double> rmin(n);
    for (uint32_t i = 0; i < n; i++) lab[i] = i;
    for (uint32_t r = 0; r < n; r++) scan_row(D, lab, n, r, rmin[r], rpart[r]);
    if (build_ms) *build_ms = now_ms() - t0;
    t0 = now_ms();
    for (uint32_t s = 0; s + 1 < n; s++) {
        double bd = std::numeric_limits<double>::infinity();
        uint32_t blo = NONE, bhi = NONE, sa = NONE, sb = NONE;
        for (uint32_t r = 0; r < n; r++) {
            if (lab[r] == NONE || rpart[r] == NONE) continue;
            const uint32_t l = lab[r], pl = lab[rpart[r]];
            const uint32_t lo = l < pl ? l : pl, hi = l < pl ? pl : l;
            if (rmin[r] < bd || (rmin[r] == bd && (lo < blo || (lo == blo && hi < bhi)))) {
                bd = rmin[r]; blo = lo; bhi = hi;
                sa = l < pl ? r : rpart[r]; sb = l < pl ? rpart[r] : r;
            }
        }
        steps[s] = Step{blo, bhi, bd, size[sa] + size[sb], 0};
        std::vector<uint32_t> again;
        for (uint32_t x = 0; x < n; x++) {
            if (x == sa || x == sb || lab[x] == NONE) continue;
            const double va = D[uint64_t(sa) * n + x], vb = D[uint64_t(sb) * n + x], v = va > vb ? va : vb;
            D[uint64_t(sa) * n + x] = D[uint64_t(x) * n + sa] = v;
            if (rpart[x] == sa || rpart[x] == sb) again.push_back(x);
        }
        size[sa] += size[sb];
        lab[sa] = n + s; lab[sb] = NONE;
        again.push_back(sa);
        for (uint32_t r : again) scan_row(D, lab, n, r, rmin[r], rpart[r]);
    }
    return now_ms() - t0;
}
