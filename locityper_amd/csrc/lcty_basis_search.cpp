// lcty_basis_search.cpp — branch and bound for the minimum hitting set of the basis constraints (lcty_basis_search.hpp).
//
// The reference gives the model to SCIP (dom_set.rs:13-36), logs a status other than "optimal" and takes the best solution either way.
// Which of several optima a solver returns is its own business; only the size of the optimum can be compared. Here, so that the answer
// is the same from call to call, every choice is by a fixed order: rows in the order given (lcty_basis_constraints: by popcount, then by
// content), haplotypes by id.
//   presolve   rows of one haplotype are forced; rows that contain another row go (when there are few enough to compare all pairs);
//              a haplotype whose rows are a subset of another's rows goes (column dominance, the lower id stays on a tie); repeated
//              until nothing changes
//   incumbent  the greedy cover: the haplotype in most rows not yet hit, lowest id on ties
//   bound      rows not yet hit that share no haplotype pairwise need one haplotype each
//   branching  the row not yet hit with the fewest haplotypes left; its haplotypes in order of the rows they hit (then id); a haplotype
//              tried is excluded from the branches after it
// Host code only.
#include "lcty_basis_search.hpp"

#include <algorithm>
#include <cstring>

namespace lcty {
namespace {

struct Search {
    uint32_t R = 0, C = 0, Rw = 0;
    std::vector<std::vector<uint32_t>> row_cols;       // the haplotypes (local numbers, ascending) of every row
    std::vector<uint64_t> col_rows;                    // [C][Rw]: the rows of every haplotype
    std::vector<uint8_t> banned;
    std::vector<uint32_t> mark;                        // per haplotype: the node serial that used it in the bound
    uint32_t serial = 0;
    std::vector<uint64_t> stack;                       // the rows not yet hit, one bitset per depth
    std::vector<uint32_t> chosen, best;
    uint64_t nodes = 0, node_limit = 0;
    bool out_of_nodes = false;

    uint32_t hits(uint32_t c, const uint64_t* unc) const {
        uint32_t n = 0;
        const uint64_t* cr = col_rows.data() + uint64_t(c) * Rw;
        for (uint32_t k = 0; k < Rw; k++) n += static_cast<uint32_t>(__builtin_popcountll(cr[k] & unc[k]));
        return n;
    }
    // disjoint-rows bound over the rows of `unc`; *pick = the row with the fewest haplotypes left (UINT32_MAX: none unhit); false: a row cannot be hit
    bool bound(const uint64_t* unc, uint32_t* lb, uint32_t* pick) {
        serial++;
        uint32_t n = 0, best_row = UINT32_MAX, best_avail = UINT32_MAX;
        for (uint32_t k = 0; k < Rw; k++) {
            uint64_t w = unc[k];
            while (w) {
                const uint32_t r = k * 64 + static_cast<uint32_t>(__builtin_ctzll(w));
                w &= w - 1;
                uint32_t avail = 0;
                bool disjoint = true;
                for (uint32_t c : row_cols[r]) {
                    if (banned[c]) continue;
                    avail++;
                    if (mark[c] == serial) disjoint = false;
                }
                if (avail == 0) return false;
                if (avail < best_avail) { best_avail = avail; best_row = r; }
                if (disjoint) {
                    n++;
                    for (uint32_t c : row_cols[r]) if (!banned[c]) mark[c] = serial;
                }
            }
        }
        *lb = n; *pick = best_row;
        return true;
    }
    void node(uint32_t depth) {
        if (out_of_nodes) return;
        if (++nodes > node_limit) { out_of_nodes = true; return; }
        const uint64_t* unc = stack.data() + uint64_t(depth) * Rw;
        uint32_t lb = 0, pick = 0;
        if (!bound(unc, &lb, &pick)) return;
        if (pick == UINT32_MAX) {                                   // every row is hit
            if (chosen.size() < best.size()) best = chosen;
            return;
        }
        if (chosen.size() + lb >= best.size()) return;
        std::vector<std::pair<uint32_t, uint32_t>> order;           // (rows hit, haplotype)
        for (uint32_t c : row_cols[pick]) if (!banned[c]) order.push_back({hits(c, unc), c});
        std::sort(order.begin(), order.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) {
            return a.first != b.first ? a.first > b.first : a.second < b.second;
        });
        uint64_t* next = stack.data() + uint64_t(depth + 1) * Rw;
        size_t tried = 0;
        for (; tried < order.size() && !out_of_nodes; tried++) {
            const uint32_t c = order[tried].second;
            const uint64_t* cr = col_rows.data() + uint64_t(c) * Rw;
            for (uint32_t k = 0; k < Rw; k++) next[k] = unc[k] & ~cr[k];
            chosen.push_back(c);
            node(depth + 1);
            chosen.pop_back();
            banned[c] = 1;
            if (chosen.size() + 1 >= best.size()) { tried++; break; }   // one more haplotype cannot beat the incumbent any more
        }
        for (size_t t = 0; t < tried; t++) banned[order[t].second] = 0;
    }
};

}  // namespace

BasisAnswer basis_search(uint32_t n, uint64_t n_rows, const uint32_t* rows_in, uint64_t node_limit, bool* empty_row) {
    BasisAnswer ans;
    if (empty_row) *empty_row = false;
    const uint32_t words = (n + 31) / 32;
    // rows as ascending id lists, in the order given, without repeats of a whole row
    std::vector<std::vector<uint32_t>> rows;
    rows.reserve(n_rows);
    for (uint64_t r = 0; r < n_rows; r++) {
        std::vector<uint32_t> ids;
        for (uint32_t k = 0; k < words; k++) {
            uint32_t w = rows_in[r * words + k];
            if (k == words - 1 && (n & 31)) w &= (1u << (n & 31)) - 1;
            while (w) { ids.push_back(k * 32 + static_cast<uint32_t>(__builtin_ctz(w))); w &= w - 1; }
        }
        if (ids.empty()) { if (empty_row) *empty_row = true; return ans; }
        rows.push_back(std::move(ids));
    }
    std::vector<uint8_t> forced(n, 0), gone(n, 0);                  // gone: dominated haplotypes, out of every row
    for (int round = 0; round < 64; round++) {
        bool changed = false;
        // forced haplotypes, and the rows they hit
        for (bool again = true; again;) {
            again = false;
            for (const auto& r : rows) if (r.size() == 1 && !forced[r[0]]) { forced[r[0]] = 1; again = changed = true; }
            if (again) rows.erase(std::remove_if(rows.begin(), rows.end(), [&](const std::vector<uint32_t>& r) {
                              return std::any_of(r.begin(), r.end(), [&](uint32_t c) { return forced[c] != 0; }); }), rows.end());
        }
        if (rows.empty()) break;
        // equal rows (the first stays), then, where there are few enough to compare all pairs, rows that contain another row
        {
            std::vector<uint32_t> ix(rows.size());
            for (uint32_t i = 0; i < ix.size(); i++) ix[i] = i;
            std::stable_sort(ix.begin(), ix.end(), [&](uint32_t x, uint32_t y) { return rows[x] < rows[y]; });
            std::vector<uint8_t> dup(rows.size(), 0);
            for (size_t i = 1; i < ix.size(); i++) if (rows[ix[i]] == rows[ix[i - 1]]) dup[ix[i]] = 1;
            size_t at = 0;
            for (size_t a = 0; a < rows.size(); a++) if (!dup[a]) { if (at != a) rows[at] = std::move(rows[a]); at++; }
            if (at != rows.size()) { rows.resize(at); changed = true; }
        }
        if (rows.size() <= 4096) {
            std::vector<uint8_t> drop(rows.size(), 0);
            for (size_t a = 0; a < rows.size(); a++)
                for (size_t b = 0; b < rows.size() && !drop[a]; b++)
                    if (a != b && !drop[b] && rows[b].size() < rows[a].size() && std::includes(rows[a].begin(), rows[a].end(), rows[b].begin(), rows[b].end()))
                        drop[a] = 1;
            size_t at = 0;
            for (size_t a = 0; a < rows.size(); a++) if (!drop[a]) { if (at != a) rows[at] = std::move(rows[a]); at++; }
            if (at != rows.size()) { rows.resize(at); changed = true; }
        }
        // column dominance: the rows of haplotype j are among the rows of haplotype k
        {
            const uint32_t Rw = static_cast<uint32_t>((rows.size() + 63) / 64);
            std::vector<uint32_t> active;
            std::vector<uint64_t> cr(uint64_t(n) * Rw, 0);
            std::vector<uint32_t> cnt(n, 0);
            for (size_t r = 0; r < rows.size(); r++) for (uint32_t c : rows[r]) { cr[uint64_t(c) * Rw + r / 64] |= 1ull << (r % 64); cnt[c]++; }
            for (uint32_t c = 0; c < n; c++) if (cnt[c]) active.push_back(c);
            bool any = false;
            for (uint32_t j : active) {
                for (uint32_t k : active) {
                    if (j == k || gone[k] || cnt[k] < cnt[j] || (cnt[k] == cnt[j] && k > j)) continue;
                    const uint64_t* a = cr.data() + uint64_t(j) * Rw; const uint64_t* b = cr.data() + uint64_t(k) * Rw;
                    bool sub = true;
                    for (uint32_t t = 0; t < Rw; t++) if (a[t] & ~b[t]) { sub = false; break; }
                    if (sub) { gone[j] = 1; any = true; break; }
                }
            }
            if (any) {
                for (auto& r : rows) r.erase(std::remove_if(r.begin(), r.end(), [&](uint32_t c) { return gone[c] != 0; }), r.end());
                changed = true;
            }
        }
        if (!changed) break;
    }
    for (uint32_t c = 0; c < n; c++) if (forced[c]) ans.ids.push_back(c);
    ans.n_forced = static_cast<uint32_t>(ans.ids.size());
    if (rows.empty()) { ans.bound = ans.n_forced; ans.optimal = true; return ans; }

    // the search over what is left, haplotypes renumbered
    Search S;
    std::vector<uint32_t> local(n, UINT32_MAX), global;
    for (const auto& r : rows) for (uint32_t c : r) if (local[c] == UINT32_MAX) local[c] = 0;
    for (uint32_t c = 0; c < n; c++) if (local[c] == 0) { local[c] = static_cast<uint32_t>(global.size()); global.push_back(c); }
    S.R = static_cast<uint32_t>(rows.size()); S.C = static_cast<uint32_t>(global.size()); S.Rw = (S.R + 63) / 64;
    S.row_cols.resize(S.R);
    S.col_rows.assign(uint64_t(S.C) * S.Rw, 0);
    for (uint32_t r = 0; r < S.R; r++)
        for (uint32_t c : rows[r]) { S.row_cols[r].push_back(local[c]); S.col_rows[uint64_t(local[c]) * S.Rw + r / 64] |= 1ull << (r % 64); }
    S.banned.assign(S.C, 0); S.mark.assign(S.C, 0);
    S.node_limit = node_limit ? node_limit : 2000000ull;
    std::vector<uint64_t> all(S.Rw, 0);
    for (uint32_t r = 0; r < S.R; r++) all[r / 64] |= 1ull << (r % 64);
    // greedy cover
    {
        std::vector<uint64_t> unc = all;
        for (;;) {
            uint32_t bc = UINT32_MAX, bh = 0;
            for (uint32_t c = 0; c < S.C; c++) { const uint32_t h = S.hits(c, unc.data()); if (h > bh) { bh = h; bc = c; } }
            if (bc == UINT32_MAX) break;
            S.best.push_back(bc);
            for (uint32_t k = 0; k < S.Rw; k++) unc[k] &= ~S.col_rows[uint64_t(bc) * S.Rw + k];
        }
    }
    uint32_t root_lb = 0, pick = 0;
    S.bound(all.data(), &root_lb, &pick);
    S.stack.assign(uint64_t(S.best.size() + 2) * S.Rw, 0);
    std::copy(all.begin(), all.end(), S.stack.begin());
    S.node(0);
    for (uint32_t c : S.best) ans.ids.push_back(global[c]);
    std::sort(ans.ids.begin(), ans.ids.end());
    ans.nodes = S.nodes;
    ans.optimal = !S.out_of_nodes;
    ans.bound = ans.optimal ? static_cast<uint32_t>(ans.ids.size()) : ans.n_forced + root_lb;
    return ans;
}

}  // namespace lcty
