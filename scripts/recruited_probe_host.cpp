// recruited_probe_host.cpp — the host's half of a resident set of recruited reads (locityper_amd/csrc/lcty_recruited_host.hpp: the plan
// of an add with its checks and the byte cap, the growth of a locus's capacity, the commit of lengths, offsets and names) on the CPU,
// no HIP, for tests/test_recruited_host.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I locityper_amd/csrc scripts/recruited_probe_host.cpp
//       -o recruited_probe_host && ./recruited_probe_host DIR/corpus.txt
// The corpus is text, one token after the other:
//   set NAME n_loci keep_names init_units max_bytes      a new set
//   add n max_out named                                  an add of n pairs, then per pair:  len1 len2 cnt locus{cnt} name
//   end                                                  the set is printed
// In place of the device arrays a locus has two vectors of exactly its capacity (units, pairs): an add writes a tag to every unit and
// pair it plans, where the copy kernel would write, so that a capacity below the contents is the sanitizer's to see. A failed add must
// leave every book as it was. Output: per add "NAME add K status S", per locus at the end "NAME locus L pairs units last_offset
// cap_units cap_pairs name,name,..", which the test holds to tests/pyref_recruited.py. Exit 1 on a broken invariant.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <functional>
#include <string>
#include <vector>

#include "lcty_recruited_host.hpp"

using namespace lcty;
using namespace lcty::recruited;

namespace lcty { void set_last_error(const std::string&) {} }

namespace {

struct Set {
    std::string name;
    bool keep_names = false;
    uint64_t init_units = 1, max_bytes = 0;
    std::vector<LocusBook> books;
    std::vector<std::vector<uint64_t>> units, pairs;          // stand-ins of the device arrays, exactly cap_units / cap_pairs long
    unsigned adds = 0;
};

int broken(const Set& S, const char* what) { fprintf(stderr, "%s: %s\n", S.name.c_str(), what); return 1; }

bool same(const LocusBook& a, const LocusBook& b) {
    return a.n_pairs == b.n_pairs && a.n_units == b.n_units && a.cap_pairs == b.cap_pairs && a.cap_units == b.cap_units && a.mate_len == b.mate_len &&
           a.mate_off == b.mate_off && a.name_off == b.name_off && a.names == b.names;
}

int check(const Set& S) {
    for (const LocusBook& b : S.books) {
        if (b.mate_len.size() != 2 * b.n_pairs || b.mate_off.size() != 2 * b.n_pairs + 1) return broken(S, "lengths and offsets do not match the pairs");
        uint64_t at = 0;
        for (uint64_t m = 0; m < 2 * b.n_pairs; m++) {
            if (b.mate_off[m] != at) return broken(S, "offsets are not consecutive units");
            at += 32ull * units_of(b.mate_len[m]);
        }
        if (b.mate_off.back() != at || at != 32 * b.n_units) return broken(S, "the last offset is not the units");
        if (b.n_units > b.cap_units || b.n_pairs > b.cap_pairs) return broken(S, "contents above the capacity");
        if (S.keep_names && b.name_off.size() == b.n_pairs + 1) {
            for (uint64_t i = 0; i < b.n_pairs; i++)
                if (b.name_off[i + 1] <= b.name_off[i]) return broken(S, "names are not runs one behind the other");
            if (b.name_off.back() != b.names.size()) return broken(S, "the last name offset is not the size of the names");
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: recruited_probe_host DIR/corpus.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Set S;
    std::string tok;
    unsigned sets = 0;
    while (in >> tok) {
        if (tok == "set") {
            size_t n_loci; int keep;
            S = Set();
            in >> S.name >> n_loci >> keep >> S.init_units >> S.max_bytes;
            S.keep_names = keep != 0;
            S.books.assign(n_loci, LocusBook()); S.units.assign(n_loci, {}); S.pairs.assign(n_loci, {});
            sets++;
        } else if (tok == "add") {
            uint64_t n; uint32_t max_out; int named;
            in >> n >> max_out >> named;
            // arrays of exactly the size the interface states
            std::vector<uint32_t> mate_len(2 * n), cnt(n), loci(n * max_out, 0xFFFFFFFFu);
            std::vector<std::string> names(n);
            for (uint64_t i = 0; i < n; i++) {
                in >> mate_len[2 * i] >> mate_len[2 * i + 1] >> cnt[i];
                for (uint32_t j = 0; j < cnt[i]; j++) { uint32_t l; in >> l; if (j < max_out) loci[i * max_out + j] = l; }
                in >> names[i];
            }
            if (!in) { fprintf(stderr, "bad corpus\n"); return 2; }
            const std::vector<LocusBook> before = S.books;
            int32_t status = LCTY_OK;
            try {
                const Plan P = plan_add(S.books, n, mate_len.data(), max_out, cnt.data(), loci.data(), S.max_bytes);
                for (size_t l = 0; l < S.books.size(); l++) {
                    LocusBook& b = S.books[l];
                    if (!P.add_pairs[l]) continue;
                    const uint64_t cu = grown(b.cap_units, b.n_units + P.add_units[l], S.init_units);
                    const uint64_t cp = grown(b.cap_pairs, b.n_pairs + P.add_pairs[l], std::max<uint64_t>(S.init_units / 8, 1));
                    if (cu < b.cap_units || cp < b.cap_pairs) return broken(S, "a capacity shrank");
                    if (b.cap_units && cu != b.cap_units && cu % b.cap_units) return broken(S, "growth is not by doubling");
                    S.units[l].resize(cu); S.pairs[l].resize(cp);
                    S.units[l].shrink_to_fit(); S.pairs[l].shrink_to_fit();
                    b.cap_units = cu; b.cap_pairs = cp;
                    for (uint64_t u = 0; u < P.add_units[l]; u++) S.units[l][b.n_units + u] = S.adds;
                    for (uint64_t p = 0; p < P.add_pairs[l]; p++) S.pairs[l][b.n_pairs + p] = S.adds;
                }
                std::function<std::string(uint64_t)> name = [&](uint64_t i) { return names[i]; };
                if (S.keep_names && named) commit_add(S.books, P, n, mate_len.data(), max_out, cnt.data(), loci.data(), &name);
                else commit_add(S.books, P, n, mate_len.data(), max_out, cnt.data(), loci.data(), static_cast<std::function<std::string(uint64_t)>*>(nullptr));
                uint64_t bytes = 0;
                for (const LocusBook& b : S.books) bytes += b.bytes();
                if (bytes != P.bytes_after || bytes > S.max_bytes) return broken(S, "the contents are not what the plan said");
            } catch (const Error& e) {
                status = e.code;
                for (size_t l = 0; l < S.books.size(); l++) if (!same(S.books[l], before[l])) return broken(S, "a failed add changed the set");
            }
            if (check(S)) return 1;
            printf("%s add %u status %d\n", S.name.c_str(), S.adds, status);
            S.adds++;
        } else if (tok == "end") {
            for (size_t l = 0; l < S.books.size(); l++) {
                const LocusBook& b = S.books[l];
                printf("%s locus %zu %llu %llu %llu %llu %llu ", S.name.c_str(), l, static_cast<unsigned long long>(b.n_pairs), static_cast<unsigned long long>(b.n_units),
                       static_cast<unsigned long long>(b.mate_off.back()), static_cast<unsigned long long>(b.cap_units), static_cast<unsigned long long>(b.cap_pairs));
                for (uint64_t i = 0; i + 1 < b.name_off.size(); i++) printf("%s%s", i ? "," : "", b.names.substr(b.name_off[i], b.name_off[i + 1] - b.name_off[i]).c_str());
                printf("\n");
            }
        } else { fprintf(stderr, "bad corpus token %s\n", tok.c_str()); return 2; }
    }
    printf("recruited_probe_host: %u sets\n", sets);
    return 0;
}
