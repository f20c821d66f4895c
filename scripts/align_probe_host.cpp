// The comparison point of scripts/align_probe.py: the backbone route of src/seq/align.rs (precompute_kmers, get_kmer_matches, LCSk++,
// align_from_backbone with smart_align, align_multik) for the given pairs in `threads` host threads, as the reference spreads them.
// Plain C++, -O3. Scores only: the exact aligner is a two-row Gotoh optimum without a walk back (the optimum is what WFA at accuracy 9
// returns too), so this side does LESS than the reference does per stretch. Stages A and B are restated, not shared, because they are
// what the device's stages are compared with: a window with a byte outside ACGT is no k-mer, the chain's ties go to the lowest match
// index and a jump is kept over an equal diagonal continuation. The gap fill is NOT restated: routing, align_simple, the cell of the
// exact aligner and its walk back are the host instantiation of locityper_amd/csrc/lcty_gotoh.hpp (compile with -I to that
// directory), around this file's own loop over two rows; a byte outside ACGT is N, a stretch beyond 16 383 bases a side or 2^26
// cells takes align_simple. align_probe_stretch is the same route for one stretch WITH the walk back and a recording sink
// (tests/test_align_host.py holds it against tests/pyref_align.py).
// Returns the milliseconds of the pairs (the k-mer lists of the sequences, made once, are timed apart: *index_ms).
// align_probe_host_transitive is the transitive route (TransitiveStrategy, align.rs:452-514) in the same threads: the rounds of
// lcty_align_haplotypes_transitive, decided from the same mirror of `closest`; the pairs of a round are dealt to the threads, backbone
// pairs along the route above WITH the walk back (their CIGARs are what later pairs are composed of), transitive pairs through the
// host instantiation of lcty_cigar_walk.hpp (walk_transitive, walk_optimize — the templates the kernels run). It returns scores,
// best ks, routes and via, which must equal the device's.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "lcty_gotoh.hpp"
#include "lcty_cigar_walk.hpp"

#include <unordered_map>
#include <unordered_set>

namespace {
namespace G = lcty::gotoh;
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

// reference base i against query base j of a stretch, a byte outside ACGT as N
struct Same {
    const uint8_t* r; const uint8_t* q;
    bool operator()(uint32_t i, uint32_t j) const { return norm(r[i]) == norm(q[j]); }
};

// The exact aligner, end to end: G::cell over two rolling rows. dirs == nullptr: the optimum alone, what the timed route asks for;
// else a direction byte per cell and the walk back, push(op, 1) per operation in the order of the alignment.
template <class Push>
int gotoh(const Same& same, uint32_t n, uint32_t m, std::vector<G::Cell>& rows, std::vector<uint8_t>* dirs, Push&& push) {
    const G::Cell none{G::INF32, G::INF32, G::INF32};
    const size_t W = static_cast<size_t>(m) + 1;
    rows.assign(2 * W, none);
    G::Cell* prev = rows.data(); G::Cell* cur = prev + W;
    if (dirs) dirs->resize((static_cast<size_t>(n) + 1) * W);
    for (uint32_t a = 0; a <= n; a++) {
        G::Cell left = none, diag = none;
        for (uint32_t b = 0; b <= m; b++) {
            const G::Cell up = a > 0 ? prev[b] : none;
            uint32_t dir;
            cur[b] = G::cell(up, left, diag, (a > 0 && b > 0 && !same(a - 1, b - 1)) ? G::PEN_X : 0, a > 0, b > 0, a == 0 && b == 0, &dir);
            if (dirs) (*dirs)[a * W + b] = static_cast<uint8_t>(dir);
            left = cur[b]; diag = up;
        }
        std::swap(prev, cur);
    }
    const G::Cell end = prev[m];
    if (dirs) {
        std::vector<uint32_t> rev;
        uint32_t a = n, b = m, st = G::end_state(end);
        while (a > 0 || b > 0) {
            const uint32_t d = (*dirs)[a * W + b];
            if (st == G::ST_M) { rev.push_back(same(a - 1, b - 1) ? G::OP_EQ : G::OP_X); a--; b--; }
            else if (st == G::ST_D) { rev.push_back(G::OP_D); a--; }
            else { rev.push_back(G::OP_I); b--; }
            st = G::back_step(st, d);
        }
        for (size_t x = rev.size(); x-- > 0;) push(rev[x], 1u);
    }
    return -G::best_of(end);
}

template <class Push>
int smart_align(const Seq& r, uint32_t i1, uint32_t i2, const Seq& q, uint32_t j1, uint32_t j2, uint32_t max_gap, std::vector<G::Cell>& rows,
                std::vector<uint8_t>* dirs, Push&& push) {    // wfa.rs:280-321
    const uint32_t n = i2 - i1, m = j2 - j1;
    const Same same{r.p + i1, q.p + j1};
    switch (G::route(n, m, max_gap)) {
    case G::ROUTE_SIMPLE: return G::align_simple(n, m, same, push);
    case G::ROUTE_STRAIGHT: return G::align_straight(n, same, push);
    case G::ROUTE_EXACT:
        if (n > DP_DIM || m > DP_DIM || (static_cast<uint64_t>(n) + 1) * (m + 1) > DP_CELLS) return G::align_simple(n, m, same, push);
        return gotoh(same, n, m, rows, dirs, push);
    case G::ROUTE_DEL: push(G::OP_D, n); return G::gap_score(n);
    case G::ROUTE_INS: push(G::OP_I, m); return G::gap_score(m);
    default: return 0;
    }
}
}  // namespace

// smart_align of reference r[0, n) and query q[0, m) with every push recorded as it comes, a word an item (length << 4 | operation);
// *n_words counts the pushes, of which the first `cap` are kept. Returns the score.
extern "C" int32_t align_probe_stretch(const uint8_t* r, uint32_t n, const uint8_t* q, uint32_t m, uint32_t max_gap, uint32_t* words, uint32_t cap,
                                       uint32_t* n_words) {
    std::vector<G::Cell> rows; std::vector<uint8_t> dirs;
    uint32_t k = 0;
    const int score = smart_align(Seq{r, n}, 0, n, Seq{q, m}, 0, m, max_gap, rows, &dirs, [&](uint32_t op, uint32_t len) { if (k < cap) words[k] = (len << 4) | op; k++; });
    *n_words = k;
    return score;
}

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
            std::vector<uint64_t> fen; std::vector<uint32_t> dp, prev, path; std::vector<G::Cell> rows;
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
                        sc += smart_align(r, i1, i2, q, j1, j2, max_gap, rows, nullptr, G::NoPush{});
                        i1 = i2 + k; j1 = j2 + k;
                    }
                    sc += smart_align(r, i1, r.len, q, j1, q.len, max_gap, rows, nullptr, G::NoPush{});
                    if (sc > best) { best = sc; bk = k; }
                }
                score[x] = best; best_k[x] = bk;
            }
        });
    for (auto& th : pool) th.join();
    return now_ms() - t1;
}

namespace {
// a CIGAR under construction: raw BAM words, equal neighbours merge (the library's CigOut)
struct Cig {
    std::vector<uint32_t> w;
    void operator()(uint32_t op, uint32_t len) {
        if (!len) return;
        if (!w.empty() && (w.back() & 15u) == op) w.back() += len << 4; else w.push_back((len << 4) | op);
    }
};
struct Work { std::vector<std::pair<uint32_t, uint32_t>> M; std::vector<uint64_t> fen; std::vector<uint32_t> dp, prev, path; std::vector<G::Cell> rows; std::vector<uint8_t> dirs; };

// align_multik with the CIGAR of the winner
int backbone_cigar(const Seq& r, const Seq& q, const std::vector<uint32_t>* lr, const std::vector<uint32_t>* lq, uint32_t nk, const uint32_t* ks, uint32_t max_gap,
                   Work& wk, Cig& out, uint32_t* best_k) {
    int best = INT32_MIN;
    for (uint32_t ki = 0; ki < nk; ki++) {
        const uint32_t k = ks[ki];
        matches_of(r, lr[ki], q, lq[ki], k, wk.M);
        lcskpp(wk.M, k, q.len, wk.fen, wk.dp, wk.prev, wk.path);
        Cig cg;
        int sc = 0;
        uint32_t i1 = 0, j1 = 0, cur = 0;
        for (uint32_t ix : wk.path) {                                         // align_from_backbone, align.rs:262-286
            const uint32_t i2 = wk.M[ix].first, j2 = wk.M[ix].second;
            if (i1 > i2) { cur++; i1++; j1++; continue; }
            if (cur) { cg(G::OP_EQ, cur); cur = 0; }
            sc += smart_align(r, i1, i2, q, j1, j2, max_gap, wk.rows, &wk.dirs, cg);
            cur += k; i1 = i2 + k; j1 = j2 + k;
        }
        if (cur) cg(G::OP_EQ, cur);
        sc += smart_align(r, i1, r.len, q, j1, q.len, max_gap, wk.rows, &wk.dirs, cg);
        if (sc > best) { best = sc; *best_k = k; out.w.swap(cg.w); }
    }
    return best;
}

struct WalkVisitor {                                                           // what the kernels' FillVisitor is on the device
    const Seq& r; const Seq& q; uint32_t max_gap; Work& wk; Cig& cg;
    void item(uint32_t op, uint32_t len) { cg(op, len); }
    void stretch(uint32_t i1, uint32_t i2, uint32_t j1, uint32_t j2) { smart_align(r, i1, i2, q, j1, j2, max_gap, wk.rows, &wk.dirs, cg); }
};
}  // namespace

extern "C" double align_probe_host_transitive(uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, uint64_t n_pairs, const uint32_t* ref, const uint32_t* query,
                                              const uint8_t* aligned, uint32_t nk, const uint32_t* ks, uint32_t max_gap, double tr_div, uint32_t anchor_size,
                                              uint32_t threads, int32_t* score, uint32_t* best_k, uint8_t* route, uint32_t* via, uint64_t* n_rounds,
                                              double* index_ms) {
    namespace W = lcty::trwalk;
    std::vector<Seq> S(n_seqs);
    for (uint32_t i = 0; i < n_seqs; i++) S[i] = Seq{seqs + seq_off[i], static_cast<uint32_t>(seq_off[i + 1] - seq_off[i])};
    const double t0 = now_ms();
    std::vector<std::vector<uint32_t>> lists(static_cast<size_t>(n_seqs) * nk);
    {
        std::atomic<uint32_t> next{0};
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < threads; t++) pool.emplace_back([&] { for (uint32_t x; (x = next++) < n_seqs * nk;) lists[x] = kmer_list(S[x / nk], ks[x % nk]); });
        for (auto& th : pool) th.join();
    }
    const double t1 = now_ms();
    if (index_ms) *index_ms = t1 - t0;
    const bool accelerate = tr_div > 0.0 && n_pairs >= 16;                     // align.rs:784
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    auto key = [](uint32_t a, uint32_t b) { return (static_cast<uint64_t>(std::min(a, b)) << 32) | std::max(a, b); };
    std::vector<Cig> cig(n_pairs);
    std::vector<uint32_t> c_id(n_seqs, NONE); std::vector<double> c_dv(n_seqs, 0.0); std::vector<uint64_t> c_pair(n_seqs, 0);
    std::unordered_map<uint64_t, uint64_t> cell;
    std::vector<uint64_t> w_closest(n_seqs, 0);
    std::unordered_set<uint64_t> w_cell;
    struct Task { uint64_t pair, ij, jk; };
    std::vector<Task> members;
    std::vector<Work> work(threads);
    uint64_t rounds = 0;
    for (uint64_t x = 0; x < n_pairs; x++) { route[x] = 0; via[x] = NONE; score[x] = 0; best_k[x] = 0; }
    for (uint64_t x0 = 0, round = 1; x0 < n_pairs; round++) {
        w_cell.clear(); members.clear();
        uint64_t x = x0;
        for (; x < n_pairs; x++) {
            if (aligned && !aligned[x]) continue;
            const uint32_t k = ref[x], i = query[x];
            uint8_t rt = 1; uint32_t j = NONE; uint64_t ij = 0, jk = 0;
            if (accelerate) {
                if (w_closest[k] == round || w_closest[i] == round) break;
                bool cut = false;
                if (c_id[k] != NONE) {
                    const uint64_t kk = key(i, c_id[k]);
                    if (w_cell.count(kk)) cut = true;
                    else { const auto it = cell.find(kk); if (it != cell.end()) { rt = 2; j = c_id[k]; ij = it->second; jk = c_pair[k]; } }
                }
                if (!cut && rt == 1 && c_id[i] != NONE) {
                    const uint64_t kk = key(k, c_id[i]);
                    if (w_cell.count(kk)) cut = true;
                    else { const auto it = cell.find(kk); if (it != cell.end()) { rt = 3; j = c_id[i]; ij = c_pair[i]; jk = it->second; } }
                }
                if (cut) break;
                w_cell.insert(key(k, i)); w_closest[i] = round;
            }
            route[x] = rt; via[x] = j;
            members.push_back(Task{x, ij, jk});
        }
        std::atomic<uint64_t> next{0};
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < threads; t++)
            pool.emplace_back([&, t] {
                Work& wk = work[t];
                for (uint64_t y; (y = next++) < members.size();) {
                    const Task& tk = members[y];
                    const uint32_t k = ref[tk.pair], i = query[tk.pair];
                    Cig& out = cig[tk.pair];
                    if (route[tk.pair] == 1) {
                        score[tk.pair] = backbone_cigar(S[k], S[i], &lists[static_cast<size_t>(k) * nk], &lists[static_cast<size_t>(i) * nk], nk, ks, max_gap, wk, out,
                                                        &best_k[tk.pair]);
                        continue;
                    }
                    const uint32_t j = via[tk.pair];
                    const W::TrCig cij{cig[tk.ij].w.data(), static_cast<uint32_t>(cig[tk.ij].w.size()), ref[tk.ij] != j};
                    const W::TrCig cjk{cig[tk.jk].w.data(), static_cast<uint32_t>(cig[tk.jk].w.size()), ref[tk.jk] != k};
                    Cig walk;
                    WalkVisitor v{S[k], S[i], max_gap, wk, walk};
                    if (W::walk_transitive(cij, cjk, S[i].len, S[k].len, anchor_size, v)) out.w.swap(walk.w);
                    else {
                        WalkVisitor o{S[k], S[i], 0xFFFFFFFFu, wk, out};
                        W::walk_optimize(walk.w.data(), static_cast<uint32_t>(walk.w.size()), W::kOptGap, W::kOptAnchor, o);
                    }
                    int sc = 0;                                                // Penalties::calculate_score, wfa.rs:87-99
                    for (const uint32_t w : out.w) {
                        const uint32_t op = w & 15u; const int len = static_cast<int>(w >> 4);
                        sc -= op == G::OP_EQ ? 0 : (op == G::OP_X ? G::PEN_X * len : G::PEN_O + G::PEN_E * len);
                    }
                    score[tk.pair] = sc;
                }
            });
        for (auto& th : pool) th.join();
        for (const Task& tk : members) {                                       // save_cigar, align.rs:504-513
            const uint32_t k = ref[tk.pair], i = query[tk.pair];
            uint64_t nm = 0, ne = 0;
            for (const uint32_t w : cig[tk.pair].w) ((w & 15u) == G::OP_EQ ? nm : ne) += w >> 4;
            const double dv = static_cast<double>(ne) / static_cast<double>(nm + ne);
            if (accelerate && dv <= tr_div && !(c_id[i] != NONE && c_dv[i] <= dv)) { c_id[i] = k; c_dv[i] = dv; c_pair[i] = tk.pair; }
            cell[key(k, i)] = tk.pair;
        }
        rounds += accelerate && !members.empty() ? 1 : 0;
        x0 = x;
    }
    if (n_rounds) *n_rounds = rounds;
    return now_ms() - t1;
}
