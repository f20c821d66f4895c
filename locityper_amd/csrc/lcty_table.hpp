// lcty_table.hpp — the open-addressing key table every stage looks k-mers and minimizers up in, one definition each: home slot and
// step, claim, find, the {key, start, count} slot, the sizing rule, the count and compact kernels. No state, no
// allocation: the caller keeps its arrays. A table is a power-of-two array of 64-bit keys, alone or each leading a Slot, mask =
// slots - 1. A hash policy picks a key's home slot, probing is linear, and a slot is free while it holds the free marker FREE, a
// compile-time value (UNDEF64, or 0 for the transfer table).
//   The free-marker rule: a key equal to FREE is never stored and never asked for. Where the data can hold such a key the caller keeps
//   its value somewhere else (lcty_db.hip: slot `cap`, one behind the table).
//   Termination: claim and find walk from the home slot until they meet the key or a free slot; nothing else stops them and no probe is
//   counted. A table sized by table_slots has at least as many free slots as keys (and one when it is empty), so they end.
// Compiles without HIP (scripts/table_probe_host.cpp is the host instantiation): claim is then a plain compare, and the project's hash
// policies and the kernels are left out.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include "lcty_scan.hpp"
#include "lcty_seq.hpp"
#define LCTY_TABLE_FN __host__ __device__ __forceinline__
#else
#define LCTY_TABLE_FN inline __attribute__((always_inline))
#endif

namespace lcty {
namespace keytable {

// a key and the run of entries it stands for (minimizer -> loci in lcty_recruit.hip, k-mer -> places in lcty_map_index.hip)
struct Slot { uint64_t key; uint32_t start, count; };

// where a probe ended: at the key (found) or at the free slot that ends its chain
struct Probe { uint64_t slot; bool found; };

template <typename Hash> LCTY_TABLE_FN uint64_t home(uint64_t key, uint64_t mask) { return Hash{}(key) & mask; }
LCTY_TABLE_FN uint64_t step(uint64_t slot, uint64_t mask) { return (slot + 1) & mask; }

// what a table is made of: plain keys, or Slots that a key leads
LCTY_TABLE_FN uint64_t key_of(uint64_t key) { return key; }
LCTY_TABLE_FN uint64_t key_of(const Slot& s) { return s.key; }
LCTY_TABLE_FN uint64_t* key_at(uint64_t* key) { return key; }
LCTY_TABLE_FN uint64_t* key_at(Slot* s) { return &s->key; }

// The slot of `key`, taken now if nobody had it: found says that the key was there already (or that another thread got there first).
// On the device a 64-bit compare-and-swap, with no read in front of it: equal keys claimed at once all end in one slot. Which slot
// that is depends on who comes first; what find answers does not. On the host a plain compare, one caller at a time.
template <typename Hash, uint64_t FREE, typename T> LCTY_TABLE_FN Probe claim(T* table, uint64_t mask, uint64_t key) {
    for (uint64_t slot = home<Hash>(key, mask);; slot = step(slot, mask)) {
        uint64_t* at = key_at(table + slot);
#ifdef __HIP_DEVICE_COMPILE__
        const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(at), static_cast<unsigned long long>(FREE), static_cast<unsigned long long>(key));
#else
        const uint64_t old = *at; if (old == FREE) *at = key;
#endif
        if (old == FREE || old == key) return Probe{slot, old == key};
    }
}

// The slot of `key`, or, with found false, the free slot that ends its chain (where a single writer may put it: lcty_transfer.hip).
template <typename Hash, uint64_t FREE, typename T> LCTY_TABLE_FN Probe find(const T* table, uint64_t mask, uint64_t key) {
    for (uint64_t slot = home<Hash>(key, mask);; slot = step(slot, mask)) {
        const T seen = table[slot];
        if (key_of(seen) == FREE) return Probe{slot, false};
        if (key_of(seen) == key) return Probe{slot, true};
    }
}

// The sizing rule: the power of two that holds n_keys << load_shift slots (load_shift >= 1: half of them free at least), not below
// `floor` (>= 1).
inline uint64_t table_slots(uint64_t n_keys, uint32_t load_shift, uint64_t floor) {
    uint64_t slots = 1;
    while (slots < floor || slots < (n_keys << load_shift)) slots <<= 1;
    return slots;
}

#ifdef __HIPCC__
// ---- the hash policies of the project's tables (DESIGN.md 4.20 says why there are three) ----
struct MixHash { __host__ __device__ uint64_t operator()(uint64_t key) const { return mix64(key); } };             // k-mer set, genome table, recruitment, transfer
struct FastHash { __host__ __device__ uint64_t operator()(uint64_t key) const { return fast_hash64(key); } };      // map index
struct MulHash { __host__ __device__ uint64_t operator()(uint64_t key) const { return (key * 0x9E3779B97F4A7C15ull) >> 20; } };      // lcty_db.hip

// keys in a table, added to *out (grid-stride; one atomic per wavefront)
template <uint64_t FREE> __global__ void table_count_kernel(const uint64_t* __restrict__ keys, uint64_t slots, unsigned long long* out) {
    uint64_t local = 0;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < slots; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        local += keys[i] != FREE;
    local = wave_reduce(local, AddOp{});
    if ((threadIdx.x & (WAVE - 1)) == 0 && local) atomicAdd(out, static_cast<unsigned long long>(local));
}

// every key of `big` claimed in `keys` (free before, sized for the keys that table_count_kernel counted)
template <typename Hash, uint64_t FREE>
__global__ void table_compact_kernel(const uint64_t* __restrict__ big, uint64_t big_slots, uint64_t* keys, uint64_t mask) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < big_slots; i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t key = big[i];
        if (key != FREE) claim<Hash, FREE>(keys, mask, key);
    }
}
#endif

}  // namespace keytable
}  // namespace lcty
