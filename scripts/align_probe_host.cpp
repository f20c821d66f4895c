// The comparison point of scripts/align_probe.py: the backbone route of src/seq/align.rs (precompute_kmers, get_kmer_matches, LCSk++,
// align_from_backbone with smart_align, align_multik) for the given pairs in `threads` host threads, as the reference spreads them.
// Plain C++, -O3. Scores only: the exact aligner is a two-row Gotoh optimum without a walk back (the optimum is what WFA at accuracy 9
// returns too), so this side does LESS than the reference does per stretch. The rules the library states are restated, not shared:
// a window with a byte outside ACGT is no k-mer, such a byte is N in the gap fill, the chain's ties go to the lowest match index and a
// jump is kept over an equal diagonal continuation, a stretch beyond 16 383 bases a side or 2^26 cells takes align_simple.
// Returns the milliseconds of the pairs (the k-mer lists of the sequences, made once, are timed apart: *index_ms).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

namespace {
constexpr int PEN_X = 4, PEN_O = 6, PEN_E = 1, INF = 1 << 28;
constexpr uint32_t DP_DIM = 16383;
constexpr uint64_t DP_CELLS = 1ull << 26;

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline bool acgt(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
inline uint8_t norm(uint8_t c) { return acgt(c) ? c : 'N'; }

struct Seq { const uint8_t* p; uint32_t len; };

// positions of the k-mers of a sequence, sorted by k-mer, equal k-mers by position (precompute_kmers, align.rs:102-120)
std::vector<uint32_t> kmer_list(const Seq& s, uint32_t k) {
    std::vector<uint32_t> pos;
    if (s.len < k) return pos;
    uint32_t bad = 0;                                                          // bytes outside ACGT in the current window
    for (uint32_t i = 0; i < s.len; i++) {
        bad += !acgt(s.p[i]);
        if (i >= k) bad -= !acgt(s.p[i - k]);
        if (i + 1 >= k && !bad) pos.push_back(i + 1 - k);
    }
    std::sort(pos.begin(), pos.end(), [&](uint32_t a, uint32_t b) { const int c = memcmp(s.p + a, s.p + b, k); return c < 0 || (c == 0 && a < b); });
    return pos;
}

// get_kmer_matches (align.rs:202-224)
void matches_of(const Seq& r, const std::vector<uint32_t>& lr, const Seq& q, const std::vector<uint32_t>& lq, uint32_t k,
                std::vector<std::pair<uint32_t, uint32_t>>& out) {
    out.clear();
    size_t a = 0, b = 0;
    while (a < lr.size() && b < lq.size()) {
        const int c = memcmp(r.p + lr[a], q.p + lq[b], k);
        if (c < 0) a++;
        else if (c > 0) b++;
        else {
            size_t a2 = a, b2 = b;
            while (a2 < lr.size() && memcmp(r.p + lr[a2], r.p + lr[a], k) == 0) a2++;
            while (b2 < lq.size() && memcmp(q.p + lq[b2], q.p + lq[b], k) == 0) b2++;
            for (size_t x = a; x < a2; x++) for (size_t y = b; y < b2; y++) out.emplace_back(lr[x], lq[y]);
            a = a2; b = b2;
        }
    }
    std::sort(out.begin(), out.end());
}

// LCSk++: the path as match indices
void lcskpp(const std::vector<std::pair<uint32_t, uint32_t>>& M, uint32_t k, uint32_t qlen, std::vector<uint64_t>& fen, std::vector<uint32_t>& dp,
            std::vector<uint32_t>& prev, std::vector<uint32_t>& path) {
    const uint32_t m = static_cast<uint32_t>(M.size());
    path.clear();
    if (!m) return;
    fen.assign(qlen + 2, 0); dp.assign(m, 0); prev.assign(m, 0xFFFFFFFFu);
    uint32_t s = 0, e = 0, best = 0, best_ix = 0;
    while (e < m) {
        const bool start = s < m && (M[s].first < M[e].first + k || (M[s].first == M[e].first + k && M[s].second < M[e].second + k));
        if (start) {
            uint64_t v = 0;
            for (uint32_t p = M[s].second; p > 0; p -= p & (0u - p)) v = std::max(v, fen[p]);
            if (v >> 32) { dp[s] = k + static_cast<uint32_t>(v >> 32); prev[s] = ~static_cast<uint32_t>(v); } else dp[s] = k;
            s++;
        } else {
            if (M[e].first > 0 && M[e].second > 0) {
                const auto want = std::make_pair(M[e].first - 1, M[e].second - 1);
                const auto it = std::lower_bound(M.begin(), M.end(), want);
                if (it != M.end() && *it == want) { const uint32_t c = static_cast<uint32_t>(it - M.begin()); if (dp[c] + 1 > dp[e]) { dp[e] = dp[c] + 1; prev[e] = c; } }
            }
            const uint64_t v = (static_cast<uint64_t>(dp[e]) << 32) | static_cast<uint32_t>(~e);
            for (uint32_t p = M[e].second + k; p <= qlen; p += p & (0u - p)) if (fen[p] < v) fen[p] = v;
            if (dp[e] > best) { best = dp[e]; best_ix = e; }
            e++;
        }
    }
    for (uint32_t x = best_ix; x != 0xFFFFFFFFu; x = prev[x]) path.push_back(x);
    std::reverse(path.begin(), path.end());
}

int align_simple(const Seq& r, uint32_t i1, uint32_t n, const Seq& q, uint32_t j1, uint32_t m) {       // wfa.rs:49-84, the score
    int sc = 0;
    uint32_t i = 0, j = 0;
    if (n < m) { sc = -PEN_O - static_cast<int>(m - n) * PEN_E; j = m - n; }
    else if (n > m) { sc = -PEN_O - static_cast<int>(n - m) * PEN_E; i = n - m; }
    for (uint32_t t = 0; i + t < n && j + t < m; t++) sc -= norm(r.p[i1 + i + t]) == norm(q.p[j1 + j + t]) ? 0 : PEN_X;
    return sc;
}

int gotoh(const Seq& r, uint32_t i1, uint32_t n, const Seq& q, uint32_t j1, uint32_t m, std::vector<int>& rows) {
    rows.assign(3 * (static_cast<size_t>(m) + 1), INF);
    int* Mx = rows.data(); int* D = Mx + m + 1; int* I = D + m + 1;
    Mx[0] = 0;
    for (uint32_t b = 1; b <= m; b++) I[b] = PEN_O + static_cast<int>(b) * PEN_E;
    for (uint32_t a = 1; a <= n; a++) {
        const uint8_t rb = norm(r.p[i1 + a - 1]);
        int diag = std::min(Mx[0], std::min(D[0], I[0]));                     // best of cell (a - 1, b - 1)
        D[0] = std::min(D[0] + PEN_E, std::min(Mx[0], I[0]) + PEN_O + PEN_E); Mx[0] = INF; I[0] = INF;
        for (uint32_t b = 1; b <= m; b++) {
            const int up = std::min(Mx[b], I[b]), upd = D[b], here = std::min(Mx[b], std::min(D[b], I[b]));
            const int nm = diag + (rb == norm(q.p[j1 + b - 1]) ? 0 : PEN_X);
            const int nd = std::min(upd + PEN_E, up + PEN_O + PEN_E);
            const int ni = std::min(I[b - 1] + PEN_E, std::min(Mx[b - 1], D[b - 1]) + PEN_O + PEN_E);
            diag = here;
            Mx[b] = std::min(nm, INF); D[b] = std::min(nd, INF); I[b] = std::min(ni, INF);
        }
    }
    return -std::min(Mx[m], std::min(D[m], I[m]));
}

int smart_align(const Seq& r, uint32_t i1, uint32_t i2, const Seq& q, uint32_t j1, uint32_t j2, uint32_t max_gap, std::vector<int>& rows) {    // wfa.rs:280-321
    const uint32_t n = i2 - i1, m = j2 - j1;
    if (n && m) {
        if (max_gap < n || max_gap < m) return align_simple(r, i1, n, q, j1, m);
        if (n == m && n <= (2 * PEN_O + 2 * PEN_E) / PEN_X) {
            int sc = 0;
            for (uint32_t t = 0; t < n; t++) sc -= norm(r.p[i1 + t]) == norm(q.p[j1 + t]) ? 0 : PEN_X;
            return sc;
        }
        if (n > DP_DIM || m > DP_DIM || (static_cast<uint64_t>(n) + 1) * (m + 1) > DP_CELLS) return align_simple(r, i1, n, q, j1, m);
        return gotoh(r, i1, n, q, j1, m, rows);
    }
    if (n) return -PEN_O - static_cast<int>(n) * PEN_E;
    if (m) return -PEN_O - static_cast<int>(m) * PEN_E;
    return 0;
}
}  // namespace

extern "C" double align_probe_host(uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref, const uint32_t* query,
                                   uint32_t nk, const uint32_t* ks, uint32_t max_gap, uint32_t threads, int32_t* score, uint32_t* best_k, double* index_ms) {
    std::vector<Seq> S(n_seqs);
    for (uint32_t i = 0; i < n_seqs; i++) S[i] = Seq{seqs + seq_off[i], static_cast<uint32_t>(seq_off[i + 1] - seq_off[i])};
    std::vector<uint8_t> used(n_seqs, 0);
    for (uint64_t x = 0; x < n_pairs; x++) used[ref[x]] = used[query[x]] = 1;
    const double t0 = now_ms();
    std::vector<std::vector<uint32_t>> lists(static_cast<size_t>(n_seqs) * nk);
    {
        std::atomic<uint32_t> next{0};
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < threads; t++)
            pool.emplace_back([&] { for (uint32_t x; (x = next++) < n_seqs * nk;) if (used[x / nk]) lists[x] = kmer_list(S[x / nk], ks[x % nk]); });
        for (auto& th : pool) th.join();
    }
    const double t1 = now_ms();
    if (index_ms) *index_ms = t1 - t0;
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            std::vector<std::pair<uint32_t, uint32_t>> M;
            std::vector<uint64_t> fen; std::vector<uint32_t> dp, prev, path; std::vector<int> rows;
            // contiguous shares of the pairs, as align_pairs_parallel deals them (align.rs:721-742)
            const uint64_t lo = n_pairs * t / threads, hi = n_pairs * (t + 1) / threads;
            for (uint64_t x = lo; x < hi; x++) {
                const Seq &r = S[ref[x]], &q = S[query[x]];
                int best = INT32_MIN; uint32_t bk = 0;
                for (uint32_t ki = 0; ki < nk; ki++) {                        // align_multik, align.rs:294-318
                    const uint32_t k = ks[ki];
                    matches_of(r, lists[static_cast<size_t>(ref[x]) * nk + ki], q, lists[static_cast<size_t>(query[x]) * nk + ki], k, M);
                    lcskpp(M, k, q.len, fen, dp, prev, path);
                    int sc = 0;
                    uint32_t i1 = 0, j1 = 0;
                    for (uint32_t ix : path) {                                // align_from_backbone, align.rs:262-286
                        const uint32_t i2 = M[ix].first, j2 = M[ix].second;
                        if (i1 > i2) { i1++; j1++; continue; }
                        sc += smart_align(r, i1, i2, q, j1, j2, max_gap, rows);
                        i1 = i2 + k; j1 = j2 + k;
                    }
                    sc += smart_align(r, i1, r.len, q, j1, q.len, max_gap, rows);
                    if (sc > best) { best = sc; bk = k; }
                }
                score[x] = best; best_k[x] = bk;
            }
        });
    for (auto& th : pool) th.join();
    return now_ms() - t1;
}
