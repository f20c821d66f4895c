// host_harness.cpp — the host-only plumbing of the C interface (locityper_amd/csrc/lcty_host.hpp) on its own: check_haps, split_names,
// sized and Handoff. No HIP, no device: tests/test_host_plumbing.py builds it with g++ and the address and undefined-behaviour
// sanitizers and runs it as a program; a leak, a double free or a read past a buffer ends it with a non-zero status, and so does the
// first expectation that does not hold.
#include "../../locityper_amd/csrc/lcty_host.hpp"

#include <functional>

static std::string g_last;
void lcty::set_last_error(const std::string& m) { g_last = m; }
extern "C" const char* lcty_last_error(void) { return g_last.c_str(); }

using namespace lcty;

static int n_checks = 0;
#define EXPECT(cond)                                                                    \
    do {                                                                                \
        n_checks++;                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); exit(1); }  \
    } while (0)

// the status a body ends with: LCTY_OK, or the code of the Error it threw
static int32_t status_of(const std::function<void()>& body) { return guarded(body); }

// the three limits in use (lcty_db.hip, lcty_align.hip, lcty_pafvcf.hip) and the one without a bound on the length (lcty_prune.hip)
static const HapLimits kDb{1, UINT32_MAX, 1ull << 31}, kAlign{2, UINT32_MAX, 1ull << 28}, kPafVcf{1, 65535, 0x7FFFFFF0ull}, kPrune{1, UINT32_MAX, UINT64_MAX};

static void test_check_haps() {
    const uint8_t seqs[16] = {'A', 'C', 'G', 'T', 'A', 'C', 'G', 'T', 'A', 'C', 'G', 'T', 'A', 'C', 'G', 'T'};
    const uint64_t off[5] = {0, 4, 4, 10, 16};                                         // an empty sequence in the middle
    HapSet hs{};
    EXPECT(status_of([&] { hs = check_haps(4, seqs, off, kDb); }) == LCTY_OK);
    EXPECT(hs.n == 4 && hs.total == 16 && hs.max_len == 6 && hs.len(0) == 4 && hs.len(1) == 0 && hs.len(2) == 6 && hs.len(3) == 6);
    // null pointers
    EXPECT(status_of([&] { check_haps(4, seqs, nullptr, kDb); }) == LCTY_ERR_INVALID_INPUT);
    EXPECT(status_of([&] { check_haps(4, nullptr, off, kDb); }) == LCTY_ERR_INVALID_INPUT);
    // total 0: no base is there to point at
    const uint64_t none[3] = {0, 0, 0};
    EXPECT(status_of([&] { hs = check_haps(2, nullptr, none, kAlign); }) == LCTY_OK);
    EXPECT(hs.n == 2 && hs.total == 0 && hs.max_len == 0);
    // the count
    EXPECT(status_of([&] { check_haps(1, seqs, off, kAlign); }) == LCTY_ERR_INVALID_INPUT);
    EXPECT(status_of([&] { check_haps(0, seqs, off, kDb); }) == LCTY_ERR_INVALID_INPUT);
    EXPECT(status_of([&] { check_haps(4, seqs, off, HapLimits{1, 3, 1ull << 31}); }) == LCTY_ERR_UNSUPPORTED);
    EXPECT(status_of([&] { check_haps(4, seqs, off, HapLimits{1, 4, 1ull << 31}); }) == LCTY_OK);
    {
        std::vector<uint64_t> many(65537 + 1, 0);
        EXPECT(status_of([&] { check_haps(65535, nullptr, many.data(), kPafVcf); }) == LCTY_OK);
        EXPECT(status_of([&] { check_haps(65536, nullptr, many.data(), kPafVcf); }) == LCTY_ERR_UNSUPPORTED);
    }
    // seq_off[0] = 1
    const uint64_t late[5] = {1, 4, 4, 10, 16};
    for (const HapLimits& lim : {kDb, kAlign, kPafVcf, kPrune}) EXPECT(status_of([&] { check_haps(4, seqs, late, lim); }) == LCTY_ERR_INVALID_INPUT);
    // a descending offset at the first, a middle and the last position
    const uint64_t d_first[5] = {0, 4, 3, 10, 16}, d_mid[5] = {0, 4, 8, 7, 16}, d_last[5] = {0, 4, 8, 12, 11};
    EXPECT(status_of([&] { check_haps(4, seqs, d_first, kDb); }) == LCTY_ERR_INVALID_INPUT);
    EXPECT(status_of([&] { check_haps(4, seqs, d_mid, kDb); }) == LCTY_ERR_INVALID_INPUT);
    EXPECT(status_of([&] { check_haps(4, seqs, d_last, kDb); }) == LCTY_ERR_INVALID_INPUT);
    // the length: max_len - 1 is taken, max_len is not. The offsets are made up and no base is read (seqs holds 16).
    for (const HapLimits& lim : {kDb, kAlign, kPafVcf}) {
        for (int where = 0; where < 3; where++) {                                      // the long one first, in the middle, last
            uint64_t o[4] = {0, 2, 4, 6};
            for (int a = where + 1; a <= 3; a++) o[a] += lim.max_len - 1 - 2;
            EXPECT(status_of([&] { hs = check_haps(3, seqs, o, lim); }) == LCTY_OK);
            EXPECT(hs.max_len == lim.max_len - 1 && hs.len(where) == lim.max_len - 1 && hs.total == lim.max_len - 1 + 4);
            for (int a = where + 1; a <= 3; a++) o[a] += 1;
            EXPECT(status_of([&] { check_haps(3, seqs, o, lim); }) == LCTY_ERR_UNSUPPORTED);
        }
    }
    const uint64_t huge[3] = {0, 1ull << 62, 1ull << 63};                              // no bound: only the order counts
    EXPECT(status_of([&] { check_haps(2, seqs, huge, kPrune); }) == LCTY_OK);
}

static void test_split_names() {
    const char blob[] = "a\0\0bc\0";                                                   // "a", "", "bc"
    std::vector<std::string> v;
    EXPECT(status_of([&] { v = split_names(blob, 3); }) == LCTY_OK);
    EXPECT(v.size() == 3 && v[0] == "a" && v[1].empty() && v[2] == "bc");
    EXPECT(status_of([&] { v = split_names(blob, 0); }) == LCTY_OK);
    EXPECT(v.empty());
    EXPECT(status_of([&] { split_names(nullptr, 3); }) == LCTY_ERR_INVALID_INPUT);
}

static void test_sized() {
    const std::vector<uint8_t> text = {1, 2, 3, 4, 5};
    int calls = 0;
    auto writer = [&](int fail_at, int32_t code) {
        return [&, fail_at, code](uint8_t* out, uint64_t cap, uint64_t* needed) -> int32_t {
            if (++calls == fail_at) { set_last_error("writer failed"); return code; }
            *needed = text.size();
            if (out) { if (cap < text.size()) return LCTY_ERR_INVALID_INPUT; memcpy(out, text.data(), text.size()); }
            return LCTY_OK;
        };
    };
    std::vector<uint8_t> v;
    EXPECT(status_of([&] { sized(writer(0, 0), v); }) == LCTY_OK);
    EXPECT(calls == 2 && v == text);
    calls = 0; v.clear();
    EXPECT(status_of([&] { sized(writer(1, LCTY_ERR_INVALID_DATA), v); }) == LCTY_ERR_INVALID_DATA);   // fails when asked for its size
    EXPECT(calls == 1 && v.empty() && g_last == "writer failed");
    calls = 0;
    EXPECT(status_of([&] { sized(writer(2, LCTY_ERR_RUNTIME), v); }) == LCTY_ERR_RUNTIME);             // fails with the buffer in hand
    EXPECT(calls == 2);
}

struct Out { uint32_t* a; double* b; uint8_t* c; uint8_t* d; char* e; uint64_t n; };

static void test_handoff() {
    const std::vector<uint32_t> a = {1, 2, 3};
    const std::vector<double> b = {0.5, 0.25};
    const std::string c = "text";
    // five blocks, then commit: the caller frees them, and nothing else does
    Out out{};
    EXPECT(status_of([&] {
        Out o{}; Handoff h;
        o.a = h.copy(a); o.b = h.copy(b.data(), b.size()); o.c = h.bytes(c); o.d = static_cast<uint8_t*>(h.raw(7)); o.e = h.copy(c.data(), c.size()); o.n = 5;
        memset(o.d, 0xAB, 7);
        out = o; h.commit();
    }) == LCTY_OK);
    EXPECT(out.n == 5 && out.a[2] == 3 && out.b[1] == 0.25 && memcmp(out.c, "text", 4) == 0 && out.d[6] == 0xAB && memcmp(out.e, "text", 4) == 0);
    free(out.a); free(out.b); free(out.c); free(out.d); free(out.e);
    // three blocks, then a failure: nothing is leaked and the struct that was to receive them is as it was
    Out kept{};
    memset(&kept, 0, sizeof(kept));
    EXPECT(status_of([&] {
        Out o{}; Handoff h;
        o.a = h.copy(a); o.b = h.copy(b); o.c = h.bytes(c);
        fail(LCTY_ERR_INVALID_DATA, "after %d blocks", 3);
        kept = o; h.commit();
    }) == LCTY_ERR_INVALID_DATA);
    const Out zero{};
    EXPECT(memcmp(&kept, &zero, sizeof(kept)) == 0 && g_last == "after 3 blocks");
    // n == 0 still gives a pointer
    {
        Handoff h;
        const std::vector<uint32_t> none;
        EXPECT(h.copy(none) != nullptr && h.copy(static_cast<const double*>(nullptr), 0) != nullptr && h.bytes(std::string()) != nullptr && h.raw(0) != nullptr);
        uint32_t* lone = malloc_copy(a.data(), 0);
        EXPECT(lone != nullptr);
        free(lone);
    }
    // a moved-from and a committed Handoff free nothing twice
    {
        Handoff h;
        uint32_t* p = h.copy(a);
        Handoff g(std::move(h));                                                       // g frees p, h has nothing
        EXPECT(p[0] == 1);
        uint32_t* q = h.copy(a);                                                       // the moved-from one can be used again
        EXPECT(q != p);
    }
    {
        Handoff h;
        uint32_t* p = h.copy(a);
        h.commit();
        h.commit();
        uint32_t* q = h.copy(a);                                                       // freed by h, p by us
        EXPECT(q != p);
        free(p);
    }
}

int main() {
    test_check_haps();
    test_split_names();
    test_sized();
    test_handoff();
    printf("host_harness: %d checks passed\n", n_checks);
    return 0;
}
