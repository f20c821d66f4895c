// table_probe_host.cpp — the host instantiation of locityper_amd/csrc/lcty_table.hpp (no HIP: g++ -O3 -std=c++17 -shared -fPIC), for
// tests/test_table_host.py: claim and find under a hash policy the caller controls, over plain key arrays and over Slots, with either
// free marker; and the sizing rule.
#include <cstdint>

#include "lcty_table.hpp"

using namespace lcty::keytable;

namespace {

uint64_t g_home = 0;
struct Identity { uint64_t operator()(uint64_t key) const { return key; } };
struct Constant { uint64_t operator()(uint64_t) const { return g_home; } };

template <typename Hash, uint64_t FREE> Probe run(bool take, uint32_t stride, uint64_t* words, uint64_t mask, uint64_t key) {
    if (stride == 1) return take ? claim<Hash, FREE>(words, mask, key) : find<Hash, FREE>(words, mask, key);
    Slot* slots = reinterpret_cast<Slot*>(words);
    return take ? claim<Hash, FREE>(slots, mask, key) : find<Hash, FREE>(slots, mask, key);
}

}  // namespace

extern "C" {

void table_probe_set_home(uint64_t home) { g_home = home; }
uint32_t table_probe_slot_stride() { return sizeof(Slot) / sizeof(uint64_t); }

// take: claim (else find); constant: the Constant policy (else Identity); free_zero: free marker 0 (else all-ones); stride: 1 = `words`
// are keys, table_probe_slot_stride() = they are Slots. Returns found, *slot = where the probe ended.
int table_probe(int take, int constant, int free_zero, uint32_t stride, uint64_t* words, uint64_t mask, uint64_t key, uint64_t* slot) {
    Probe p;
    if (constant) p = free_zero ? run<Constant, 0ull>(take, stride, words, mask, key) : run<Constant, ~0ull>(take, stride, words, mask, key);
    else p = free_zero ? run<Identity, 0ull>(take, stride, words, mask, key) : run<Identity, ~0ull>(take, stride, words, mask, key);
    *slot = p.slot;
    return p.found ? 1 : 0;
}

uint64_t table_probe_slots(uint64_t n_keys, uint32_t load_shift, uint64_t floor) { return table_slots(n_keys, load_shift, floor); }

}
