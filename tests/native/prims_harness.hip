// TEST INFRASTRUCTURE. The device primitives of DESIGN.md 4.18 against plain host code, every case once: the wavefront scan and the
// one-workgroup scan of lcty_scan.hpp, exclusive_scan / ScanTotal and RadixSort of lcty_sort.hip, the bitonic network of lcty_bitonic.hpp.
// Compiled by tests/test_gpu_prims.py together with locityper_amd/csrc/lcty_sort.hip; prints the first mismatch of every failing case
// and returns the number of failing cases.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "lcty_bitonic.hpp"
#include "lcty_scan.hpp"
#include "lcty_sort.hpp"

namespace lcty { thread_local hipStream_t tl_stream = nullptr; }       // the library has it in lcty_api.hip

using namespace lcty;

namespace {

int n_failed = 0, n_cases = 0;
std::mt19937_64 rng(20240607);

template <typename T> std::vector<T> to_host(const DevBuf<T>& d, size_t n, hipStream_t s, size_t from = 0) {
    std::vector<T> h(n);
    d.download(h.data(), n, s, from);
    LCTY_HIP(hipStreamSynchronize(s));
    return h;
}
template <typename T> void to_dev(DevBuf<T>& d, const std::vector<T>& h, hipStream_t s, size_t room = 0) {
    d.alloc(std::max<size_t>(std::max(h.size(), room), 1));
    d.upload(h.data(), h.size(), s);
    LCTY_HIP(hipStreamSynchronize(s));
}
template <typename T> void expect_equal(const std::string& what, const std::vector<T>& got, const std::vector<T>& want) {
    n_cases++;
    size_t i = 0;
    while (i < want.size() && i < got.size() && got[i] == want[i]) i++;
    if (got.size() == want.size() && i == want.size()) return;
    n_failed++;
    if (i < want.size() && i < got.size())
        printf("FAIL %s: element %zu of %zu is %lld, expected %lld\n", what.c_str(), i, want.size(), static_cast<long long>(got[i]), static_cast<long long>(want[i]));
    else printf("FAIL %s: %zu elements, expected %zu\n", what.c_str(), got.size(), want.size());
}
void expect(const std::string& what, bool ok) {
    n_cases++;
    if (!ok) { n_failed++; printf("FAIL %s\n", what.c_str()); }
}

// ---- wavefront scan: one workgroup of 256 threads, four wavefronts that must not see each other
template <typename T, typename Op> __global__ __launch_bounds__(256) void wave_scan_kernel(const T* __restrict__ in, T* __restrict__ out, Op op) {
    out[threadIdx.x] = wave_scan_incl(in[threadIdx.x], op);
}
template <typename T, typename Op, typename HostOp> void wave_scan_case(const std::string& what, const std::vector<T>& in, Op op, HostOp host_op, hipStream_t s) {
    DevBuf<T> d_in, d_out;
    to_dev(d_in, in, s); d_out.alloc(256);
    hipLaunchKernelGGL((wave_scan_kernel<T, Op>), dim3(1), dim3(256), 0, s, d_in.p, d_out.p, op);
    LCTY_HIP(hipGetLastError());
    std::vector<T> want(256);
    for (size_t i = 0; i < 256; i++) want[i] = i % 64 ? host_op(want[i - 1], in[i]) : in[i];
    expect_equal(what, to_host(d_out, 256, s), want);
}
template <typename T> void wave_scan_cases(const std::string& type, T small_lo, T small_hi, T type_min, T type_max, hipStream_t s) {
    std::vector<T> add(256), mx(256);
    for (size_t i = 0; i < 256; i++) {
        add[i] = rng() % 3 == 0 ? T(0) : static_cast<T>(small_lo + static_cast<T>(rng() % static_cast<uint64_t>(small_hi - small_lo + 1)));
        const uint64_t r = rng() % 8;
        mx[i] = r == 0 ? T(0) : r == 1 ? type_max : r == 2 ? type_min : static_cast<T>(rng());
    }
    mx[70] = type_max;                                                  // the maximum early in wavefront 1: wavefronts 2 and 3 must not inherit it
    wave_scan_case("wave scan add " + type, add, AddOp{}, [](T a, T b) { return static_cast<T>(a + b); }, s);
    wave_scan_case("wave scan max " + type, mx, MaxOp{}, [](T a, T b) { return a > b ? a : b; }, s);
}

// ---- one-workgroup scan (launch_scan)
template <typename T, typename Load> void block_scan_cases(const std::string& type, hipStream_t s) {
    for (uint64_t n : {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049}) {
        std::vector<T> in(n);
        for (T& x : in) x = rng() % 4 == 0 ? T(0) : static_cast<T>(rng() % 1000);
        if (n > 3) in[n / 3] = static_cast<T>(1) << (sizeof(T) * 8 - 2);  // a running maximum that stays, a sum that needs the type's width
        DevBuf<T> d_in, d_out;
        to_dev(d_in, in, s); d_out.alloc(n + 1);
        std::vector<T> want(n + 1, T(0));
        for (uint64_t i = 0; i < n; i++) want[i + 1] = static_cast<T>(want[i] + in[i]);
        launch_scan<T>(s, n, Load{d_in.p}, AddOp{}, T(0), d_out.p, true);
        expect_equal("workgroup scan exclusive add " + type + " n=" + std::to_string(n), to_host(d_out, n + 1, s), want);
        for (uint64_t i = 0; i < n; i++) want[i] = i ? std::max(want[i - 1], in[i]) : in[i];
        want.resize(n);
        launch_scan<T>(s, n, Load{d_in.p}, MaxOp{}, T(0), d_out.p, false);
        expect_equal("workgroup scan inclusive max " + type + " n=" + std::to_string(n), to_host(d_out, n, s), want);
    }
}

// ---- exclusive_scan and ScanTotal
void multi_scan_cases(lcty_ctx* ctx) {
    hipStream_t s = ctx->stream;
    ScanTotal scan;
    for (uint64_t n : {1ull, 15ull, 16ull, 17ull, 4095ull, 4096ull, 4097ull, 2 * 4096ull + 1, 4096ull * 4096 + 1})
        for (int ones = 0; ones < 2; ones++) {
            std::vector<uint32_t> in(n, 1u);
            if (!ones) for (uint32_t& x : in) x = static_cast<uint32_t>(rng() & 3);
            DevBuf<uint32_t> d_in, d_out;
            to_dev(d_in, in, s);
            const uint32_t total = scan.run(d_in, d_out, n, ctx);
            std::vector<uint32_t> want(n + 1, 0u);
            std::partial_sum(in.begin(), in.end(), want.begin() + 1);
            const std::string what = std::string("ScanTotal ") + (ones ? "ones" : "random") + " n=" + std::to_string(n);
            expect_equal(what, to_host(d_out, n + 1, s), want);
            expect(what + ": returned total", total == want[n]);
        }
    {   // exclusive_scan itself, its scratch sized by scan_scratch_words and fenced by words that must stay
        const uint64_t n = 2 * 4096 + 1;
        const size_t words = scan_scratch_words(n);
        std::vector<uint32_t> in(n), fence(words + 64, 0xDEADBEEFu);
        for (uint32_t& x : in) x = static_cast<uint32_t>(rng() & 3);
        DevBuf<uint32_t> d_in, d_out, d_tmp;
        to_dev(d_in, in, s); to_dev(d_tmp, fence, s); d_out.alloc(n);
        exclusive_scan(d_in.p, d_out.p, n, d_tmp.p, s);
        std::vector<uint32_t> want(n, 0u);
        std::partial_sum(in.begin(), in.end() - 1, want.begin() + 1);
        expect_equal("exclusive_scan n=" + std::to_string(n), to_host(d_out, n, s), want);
        expect_equal("exclusive_scan keeps to scan_scratch_words", to_host(d_tmp, 64, s, words), std::vector<uint32_t>(64, 0xDEADBEEFu));
    }
    {
        DevBuf<uint32_t> d_in, d_out;
        to_dev(d_in, std::vector<uint32_t>(), s);
        const uint32_t total = scan.run(d_in, d_out, 0, ctx);
        expect_equal("ScanTotal n=0", to_host(d_out, 1, s), std::vector<uint32_t>{0u});
        expect("ScanTotal n=0: returned total", total == 0);
    }
    for (uint32_t first : {0x7FFFFFEEu, 0x7FFFFFEFu}) {                 // a total of 0x7FFFFFEF passes, 0x7FFFFFF0 is refused
        DevBuf<uint32_t> d_in, d_out;
        to_dev(d_in, std::vector<uint32_t>{first, 1u}, s);
        int32_t code = LCTY_OK; uint32_t total = 0;
        try { total = scan.run(d_in, d_out, 2, ctx); } catch (const Error& e) { code = e.code; }
        if (first == 0x7FFFFFEEu) expect("ScanTotal with a total of 0x7FFFFFEF", code == LCTY_OK && total == 0x7FFFFFEFu);
        else expect("ScanTotal with a total of 0x7FFFFFF0 raises LCTY_ERR_UNSUPPORTED", code == LCTY_ERR_UNSUPPORTED);
    }
}

// ---- radix sort: the passes restated on the host, a stable sort by the digit of every shift in turn
void radix_case(const std::string& what, const std::vector<uint64_t>& keys, bool with_vals, const std::vector<uint32_t>& shifts, RadixSort& sort, hipStream_t s) {
    const uint64_t n = keys.size();
    std::vector<uint64_t> vals(n);
    std::iota(vals.begin(), vals.end(), 0ull);
    DevBuf<uint64_t> ka, va, kb, vb;
    to_dev(ka, keys, s); to_dev(va, vals, s); kb.alloc(n); vb.alloc(n);
    const int where = sort.run(ka.p, with_vals ? va.p : nullptr, kb.p, with_vals ? vb.p : nullptr, n, shifts, s);
    std::vector<uint64_t> order = vals;
    for (uint32_t shift : shifts)
        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return ((keys[a] >> shift) & 0xFF) < ((keys[b] >> shift) & 0xFF); });
    std::vector<uint64_t> want(n);
    for (uint64_t i = 0; i < n; i++) want[i] = keys[order[i]];
    expect(what + ": the result is where the parity of the passes says", where == static_cast<int>(shifts.size() & 1));
    expect_equal(what + ": keys", to_host(where ? kb : ka, n, s), want);
    if (with_vals) expect_equal(what + ": values (stable)", to_host(where ? vb : va, n, s), order);
}
void radix_cases(hipStream_t s) {
    RadixSort sort;
    const std::vector<uint32_t> all{0, 8, 16, 24, 32, 40, 48, 56}, ends{0, 56}, three{0, 8, 16};
    for (uint64_t n : {1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5}) {
        const std::string at = " n=" + std::to_string(n);
        std::vector<uint64_t> rnd(n), four(n), same(n, 0x0123456789ABCDEFull);
        for (uint64_t i = 0; i < n; i++) { rnd[i] = rng(); four[i] = (rng() & 3) * 0x0101010101010101ull; }
        radix_case("radix sort random keys" + at, rnd, true, all, sort, s);
        std::vector<uint64_t> sorted = rnd;
        std::sort(sorted.begin(), sorted.end());
        {   // eight passes order the whole key
            DevBuf<uint64_t> ka, kb;
            to_dev(ka, rnd, s); kb.alloc(n);
            const int where = sort.run(ka.p, nullptr, kb.p, nullptr, n, all, s);
            expect_equal("radix sort keys alone" + at, to_host(where ? kb : ka, n, s), sorted);
        }
        radix_case("radix sort four key values" + at, four, true, all, sort, s);
        radix_case("radix sort equal keys" + at, same, true, all, sort, s);
        radix_case("radix sort by bytes 0 and 7" + at, rnd, true, ends, sort, s);
        radix_case("radix sort three passes" + at, rnd, true, three, sort, s);
        radix_case("radix sort three passes, keys alone" + at, four, false, three, sort, s);
    }
}

// ---- bitonic network: the kernel pads as its users do (all-ones keys, index 0xFFFFFFFF)
template <uint32_t THREADS, bool PAIRS>
__global__ __launch_bounds__(THREADS) void bitonic_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ ixs, uint32_t n, uint32_t P) {
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t* key = reinterpret_cast<uint64_t*>(smem);
    uint32_t* ix = reinterpret_cast<uint32_t*>(key + P);
    for (uint32_t i = threadIdx.x; i < P; i += THREADS) { key[i] = i < n ? keys[i] : ~0ull; if (PAIRS) ix[i] = i < n ? ixs[i] : 0xFFFFFFFFu; }
    __syncthreads();
    if (PAIRS) bitonic_sort_lds<THREADS>(P, BitonicKeyIx{key, ix});
    else bitonic_sort_lds<THREADS>(P, BitonicKeys{key});
    for (uint32_t i = threadIdx.x; i < n; i += THREADS) { keys[i] = key[i]; if (PAIRS) ixs[i] = ix[i]; }
}
template <uint32_t THREADS, bool PAIRS> void bitonic_case(uint32_t n, hipStream_t s) {
    uint32_t P = 1;
    while (P < n) P <<= 1;
    std::vector<uint64_t> keys(n); std::vector<uint32_t> ixs(n);
    for (uint32_t i = 0; i < n; i++) {
        // keys alone: the padding value itself is among them (a db list may hold UNDEF64); pairs: few key values, every index once
        keys[i] = PAIRS ? rng() % 5 : rng() % 6 == 0 ? ~0ull : rng();
        ixs[i] = i;
    }
    std::shuffle(ixs.begin(), ixs.end(), rng);
    DevBuf<uint64_t> d_keys; DevBuf<uint32_t> d_ixs;
    to_dev(d_keys, keys, s); to_dev(d_ixs, ixs, s);
    const size_t lds = static_cast<size_t>(P) * (PAIRS ? 12 : 8);
    LCTY_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bitonic_kernel<THREADS, PAIRS>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    hipLaunchKernelGGL((bitonic_kernel<THREADS, PAIRS>), dim3(1), dim3(THREADS), lds, s, d_keys.p, d_ixs.p, n, P);
    LCTY_HIP(hipGetLastError());
    std::vector<std::pair<uint64_t, uint32_t>> want(n);
    for (uint32_t i = 0; i < n; i++) want[i] = {keys[i], PAIRS ? ixs[i] : 0u};
    std::sort(want.begin(), want.end());
    std::vector<uint64_t> want_keys(n); std::vector<uint32_t> want_ixs(n);
    for (uint32_t i = 0; i < n; i++) { want_keys[i] = want[i].first; want_ixs[i] = want[i].second; }
    const std::string what = std::string("bitonic ") + (PAIRS ? "(key, index)" : "keys") + " threads=" + std::to_string(THREADS) + " n=" + std::to_string(n);
    expect_equal(what + ": keys", to_host(d_keys, n, s), want_keys);
    if (PAIRS) expect_equal(what + ": indices", to_host(d_ixs, n, s), want_ixs);
}

}  // namespace

int main() {
    try {
        LCTY_HIP(hipSetDevice(0));
        lcty_ctx ctx;
        LCTY_HIP(hipStreamCreate(&ctx.stream.main));
        hipStream_t s = ctx.stream;
        wave_scan_cases<uint32_t>("uint32_t", 1u, 1000u, 0u, UINT32_MAX, s);
        wave_scan_cases<uint64_t>("uint64_t", 1ull << 32, (1ull << 32) + 1000, 0ull, UINT64_MAX, s);
        wave_scan_cases<long long>("long long", -1000ll, 1000ll, LLONG_MIN, LLONG_MAX, s);
        block_scan_cases<uint32_t, LoadU32>("uint32_t", s);
        block_scan_cases<uint64_t, LoadU64>("uint64_t", s);
        multi_scan_cases(&ctx);
        radix_cases(s);
        for (uint32_t n : {0, 1, 2, 3, 64, 65, 1000, 1024, 8192}) { bitonic_case<1024, false>(n, s); bitonic_case<1024, true>(n, s); }
        for (uint32_t n : {0, 1, 2, 3, 64, 65, 1000, 1024}) { bitonic_case<64, false>(n, s); bitonic_case<64, true>(n, s); }
        LCTY_HIP(hipStreamSynchronize(s));
        LCTY_HIP(hipStreamDestroy(ctx.stream.main));
    } catch (const std::exception& e) {
        printf("FAIL: %s\n", e.what());
        return 2;
    }
    printf("%d checks, %d failed\n", n_cases, n_failed);
    return n_failed ? 1 : 0;
}
