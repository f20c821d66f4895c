// lcty_host.hpp — host-only plumbing of the C interface: the error type, the arrays handed to the caller (Handoff), the one check of a
// haplotype set (check_haps) and two helpers of the locus-file stages. Standard library and the C header only: a user of it compiles
// without HIP (tests/native/host_harness.cpp). The device side of the same things (from, DevHaps) is in lcty_common.hpp.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/locityper_hip.h"

namespace lcty {

// Thread-local message of the last failure (lcty_last_error()).
void set_last_error(const std::string& msg);

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] inline void fail(int32_t code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    throw Error(code, buf);
}

// Wraps a C-ABI body: exceptions -> status code + last-error string.
template <typename F>
int32_t guarded(F&& body) {
    try {
        body();
        return LCTY_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory");
        return LCTY_ERR_RUNTIME;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return LCTY_ERR_RUNTIME;
    }
}

// A copy of n host values that the caller of the C interface frees with free(). n == 0 still gives a pointer.
template <typename T> T* malloc_copy(const T* p, size_t n) {
    T* out = static_cast<T*>(malloc(std::max<size_t>(n, 1) * sizeof(T)));
    if (!out) throw std::bad_alloc();
    if (n) memcpy(out, p, n * sizeof(T));
    return out;
}

// Arrays on their way to the caller. An entry point gathers them in a local out struct through a Handoff, and only when nothing can
// fail any more writes the struct to *out and commits: until then the destructor frees every block, so on any failure *out stays as
// the entry point zeroed it and nothing is leaked (the contract of include/locityper_hip.h).
class Handoff {
public:
    Handoff() = default;
    Handoff(Handoff&& o) noexcept : blocks(std::move(o.blocks)) { o.blocks.clear(); }
    Handoff(const Handoff&) = delete;
    Handoff& operator=(const Handoff&) = delete;
    ~Handoff() { for (void* b : blocks) free(b); }
    template <typename T> T* copy(const T* p, size_t n) {
        blocks.reserve(blocks.size() + 1);                                    // nothing throws between malloc and push_back
        T* out = malloc_copy(p, n);
        blocks.push_back(out);
        return out;
    }
    template <typename T> T* copy(const std::vector<T>& v) { return copy(v.data(), v.size()); }
    uint8_t* bytes(const std::string& s) { return copy(reinterpret_cast<const uint8_t*>(s.data()), s.size()); }
    void* raw(size_t n_bytes) {                                               // a block the caller fills in place
        blocks.reserve(blocks.size() + 1);
        void* out = malloc(std::max<size_t>(n_bytes, 1));
        if (!out) throw std::bad_alloc();
        blocks.push_back(out);
        return out;
    }
    void commit() { blocks.clear(); }                                         // the caller owns them now
private:
    std::vector<void*> blocks;
};

// A haplotype set as the C interface takes it: n sequences back to back in seqs, sequence a at [seq_off[a], seq_off[a + 1]), seq_off[0] = 0.
// A stage states what its kernels can take: the number of sequences within [min_seqs, max_seqs], every length below max_len.
struct HapLimits { uint32_t min_seqs, max_seqs; uint64_t max_len; };
struct HapSet {
    uint32_t n; uint64_t total, max_len; const uint64_t* off;
    uint64_t len(uint32_t a) const { return off[a + 1] - off[a]; }
};
// Malformed -> LCTY_ERR_INVALID_INPUT, too long or too many -> LCTY_ERR_UNSUPPORTED. Reads the offsets only, no base.
inline HapSet check_haps(uint32_t n_seqs, const uint8_t* seqs, const uint64_t* seq_off, const HapLimits& lim) {
    if (!seq_off) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (n_seqs < lim.min_seqs) fail(LCTY_ERR_INVALID_INPUT, "%u haplotypes (at least %u are needed)", n_seqs, lim.min_seqs);
    if (n_seqs > lim.max_seqs) fail(LCTY_ERR_UNSUPPORTED, "%u haplotypes (at most %u)", n_seqs, lim.max_seqs);
    if (seq_off[0] != 0) fail(LCTY_ERR_INVALID_INPUT, "seq_off[0] must be 0");
    HapSet hs{n_seqs, seq_off[n_seqs], 0, seq_off};
    for (uint32_t a = 0; a < n_seqs; a++) {
        if (seq_off[a + 1] < seq_off[a]) fail(LCTY_ERR_INVALID_INPUT, "seq_off is not ascending at %u", a);
        if (hs.len(a) >= lim.max_len)
            fail(LCTY_ERR_UNSUPPORTED, "haplotype %u has %llu bases (fewer than %llu are supported)", a, static_cast<unsigned long long>(hs.len(a)),
                 static_cast<unsigned long long>(lim.max_len));
        hs.max_len = std::max(hs.max_len, hs.len(a));
    }
    if (hs.total && !seqs) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    return hs;
}

// n 0-terminated names, one behind the other
inline std::vector<std::string> split_names(const char* names, uint32_t n) {
    if (!names) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    std::vector<std::string> v;
    const char* p = names;
    for (uint32_t i = 0; i < n; i++) { v.emplace_back(p); p += v.back().size() + 1; }
    return v;
}

// A writer of the C interface, called for its size and then with a buffer of that size: call(out, cap, &needed) -> status
template <typename F>
void sized(F&& call, std::vector<uint8_t>& v) {
    uint64_t need = 0;
    int32_t rc = call(nullptr, 0, &need);
    if (rc == LCTY_OK) { v.resize(need); rc = call(v.data(), need, &need); }
    if (rc != LCTY_OK) throw Error(rc, lcty_last_error());
}

}  // namespace lcty
