// lcty_basis_search.hpp — minimum hitting set of the basis constraints (the place of find_dominating_set, src/algo/dom_set.rs, which
// hands `min sum x, sum_{i in row} x_i >= 1 for every row` to SCIP) as plain host C++: no device types, no HIP calls.
#pragma once
#include <cstdint>
#include <vector>

namespace lcty {

struct BasisAnswer {
    std::vector<uint32_t> ids;        // the chosen haplotypes, ascending: they hit every row
    uint32_t bound = 0;               // no hitting set is smaller than this (== ids.size() when optimal)
    bool optimal = false;
    uint32_t n_forced = 0;            // ids fixed by rows of one haplotype, before the search
    uint64_t nodes = 0;
};

// rows[n_rows][ceil(n / 32)]: bit i of a row = haplotype i is in it. An empty row cannot be hit: `empty_row` is set and nothing else.
// node_limit 0 = the default (2 000 000). The limit reached: the best cover so far, optimal = false, bound = what was proved.
BasisAnswer basis_search(uint32_t n, uint64_t n_rows, const uint32_t* rows, uint64_t node_limit, bool* empty_row = nullptr);

}  // namespace lcty
