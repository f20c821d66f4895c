// lcty_prune.hip — `locityper prune` for one locus (src/command/prune.rs): divergences from the PAF, complete-linkage clustering of the
// haplotypes on the device, the cut, one representative per cluster, the Newick / discarded texts and the thinned files of the locus
// directory. The contract of the clustering (labels, tie rule) is stated at lcty_prune_linkage in the header and in DESIGN.md 5j.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "lcty_common.hpp"
#include "lcty_device.hpp"

namespace {

using namespace lcty;

constexpr uint32_t NO_LABEL = 0xFFFFFFFFu;          // a matrix slot that holds no active cluster
constexpr int MERGE_THREADS = 1024;                 // the one workgroup of the merge loop: 16 wavefronts
constexpr int MERGE_WAVES = MERGE_THREADS / WAVE;
constexpr int REPR_THREADS = 256;

// ---- device ---------------------------------------------------------------------------------------------------------------------------

// TriangleMatrix::to_linear_index (src/ext/trimat.rs:43-46), i < j
__host__ __device__ inline uint64_t tri_index(uint64_t n, uint64_t i, uint64_t j) { return (2 * n - 3 - i) * i / 2 + j - 1; }

// the full symmetric matrix from the triangle; the diagonal is never read and holds +inf
__global__ void prune_expand_kernel(const double* __restrict__ tri, uint32_t n, double* __restrict__ D) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= uint64_t(n) * n) return;
    const uint32_t i = static_cast<uint32_t>(t / n), j = static_cast<uint32_t>(t % n);
    D[t] = i == j ? __longlong_as_double(0x7FF0000000000000ll) : tri[i < j ? tri_index(n, i, j) : tri_index(n, j, i)];
}

// (dissimilarity, label) order of a row's candidates: the smaller value, on equal values the smaller LABEL
__device__ inline bool row_better(double d, uint32_t lab, double bd, uint32_t blab) { return d < bd || (d == bd && lab < blab); }

// One wavefront scans matrix row r: the minimum over the other active slots and, among the minima, the slot of smallest label.
// Every lane returns the result. A row with no other active slot returns (+inf, NO_LABEL).
__device__ inline void wave_scan_row(const double* __restrict__ D, const uint32_t* __restrict__ lab, uint32_t n, uint32_t r, double& out_d,
                                     uint32_t& out_slot) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const double* row = D + uint64_t(r) * n;
    double bd = __longlong_as_double(0x7FF0000000000000ll);
    uint32_t bl = NO_LABEL, bs = NO_LABEL;
    for (uint32_t x = lane; x < n; x += WAVE) {
        const uint32_t l = lab[x];
        if (l == NO_LABEL || x == r) continue;
        const double d = row[x];
        if (row_better(d, l, bd, bl)) { bd = d; bl = l; bs = x; }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double od = __shfl_xor(bd, off);
        const uint32_t ol = __shfl_xor(bl, off), os = __shfl_xor(bs, off);
        if (row_better(od, ol, bd, bl)) { bd = od; bl = ol; bs = os; }
    }
    out_d = bd; out_slot = bs;
}

// the caches of the leaves: one wavefront per row, many workgroups
__global__ void prune_init_rows_kernel(const double* __restrict__ D, const uint32_t* __restrict__ lab, uint32_t n, double* __restrict__ rmin,
                                       uint32_t* __restrict__ rpart) {
    const uint32_t r = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (r >= n) return;
    double d; uint32_t s;
    wave_scan_row(D, lab, n, r, d, s);
    if ((threadIdx.x & (WAVE - 1)) == 0) { rmin[r] = d; rpart[r] = s; }
}

// a candidate merge: dissimilarity, the two labels (lo < hi) and their slots
struct Cand { double d; uint32_t lo, hi, slo, shi; };
__device__ inline bool cand_better(const Cand& a, const Cand& b) {
    return a.d < b.d || (a.d == b.d && (a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi)));
}
__device__ inline Cand cand_shfl_xor(const Cand& c, int off) {
    Cand o;
    o.d = __shfl_xor(c.d, off); o.lo = __shfl_xor(c.lo, off); o.hi = __shfl_xor(c.hi, off); o.slo = __shfl_xor(c.slo, off); o.shi = __shfl_xor(c.shi, off);
    return o;
}

// The n - 1 merges, ONE workgroup (launched with grid 1): nothing here waits for another workgroup.
//   D      [n][n] symmetric, rows / columns are SLOTS; lab[slot] = label of the active cluster it holds, or NO_LABEL
//   rmin / rpart [n]: per active slot the minimum of its row over the other active slots and the slot of smallest LABEL among the minima
//   csize  [n] cluster size per slot; list [n] scratch: the rows to scan again after a merge
// With max-linkage the new cluster's distance to x is never below x's cached minimum, and its label is the largest so far, so a row whose
// cached partner is neither merged cluster keeps its cache; the others, and the new row, are scanned again.
__global__ __launch_bounds__(MERGE_THREADS) void prune_merge_kernel(double* __restrict__ D, uint32_t* __restrict__ lab, double* __restrict__ rmin,
                                                                    uint32_t* __restrict__ rpart, uint32_t* __restrict__ csize,
                                                                    uint32_t* __restrict__ list, uint32_t n, lcty_prune_step* __restrict__ steps,
                                                                    unsigned long long* __restrict__ n_rescans) {
    __shared__ Cand part[MERGE_WAVES];
    __shared__ Cand best;
    __shared__ uint32_t n_list;
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    unsigned long long rescans = 0;
    if (tid == 0) n_list = 0;
    __syncthreads();
    for (uint32_t step = 0; step + 1 < n; step++) {
        // 1. the pair to merge: argmin over the cached rows by (dissimilarity, smaller label, larger label)
        Cand c{inf, NO_LABEL, NO_LABEL, NO_LABEL, NO_LABEL};
        for (uint32_t r = tid; r < n; r += MERGE_THREADS) {
            const uint32_t l = lab[r];
            if (l == NO_LABEL) continue;
            const uint32_t p = rpart[r];
            if (p == NO_LABEL) continue;
            const uint32_t pl = lab[p];
            Cand m;
            m.d = rmin[r];
            if (l < pl) { m.lo = l; m.hi = pl; m.slo = r; m.shi = p; } else { m.lo = pl; m.hi = l; m.slo = p; m.shi = r; }
            if (cand_better(m, c)) c = m;
        }
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const Cand o = cand_shfl_xor(c, off);
            if (cand_better(o, c)) c = o;
        }
        if (lane == 0) part[wave] = c;
        __syncthreads();
        if (wave == 0) {
            Cand w = lane < MERGE_WAVES ? part[lane] : Cand{inf, NO_LABEL, NO_LABEL, NO_LABEL, NO_LABEL};
            for (int off = MERGE_WAVES / 2; off > 0; off >>= 1) {
                const Cand o = cand_shfl_xor(w, off);
                if (cand_better(o, w)) w = o;
            }
            if (lane == 0) best = w;
        }
        __syncthreads();
        const Cand b = best;
        const uint32_t sa = b.slo, sb = b.shi;              // the new cluster takes the slot of the smaller label
        if (sa >= n || sb >= n) break;                      // cannot happen while two clusters are active; the host checks the steps it gets
        // 2. new row and column = elementwise maximum; collect the rows whose cached partner is gone
        double* row_a = D + uint64_t(sa) * n;
        const double* row_b = D + uint64_t(sb) * n;
        for (uint32_t x = tid; x < n; x += MERGE_THREADS) {
            if (x == sa || x == sb || lab[x] == NO_LABEL) continue;
            const double va = row_a[x], vb = row_b[x];
            const double v = va > vb ? va : vb;
            row_a[x] = v;
            D[uint64_t(x) * n + sa] = v;
            const uint32_t p = rpart[x];
            if (p == sa || p == sb) list[atomicAdd(&n_list, 1u)] = x;
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t sz = csize[sa] + csize[sb];
            steps[step].cluster1 = b.lo; steps[step].cluster2 = b.hi; steps[step].dissimilarity = b.d; steps[step].size = sz; steps[step]._pad0 = 0;
            csize[sa] = sz;
            lab[sa] = n + step;
            lab[sb] = NO_LABEL;
            list[n_list] = sa;                              // at most n - 2 other rows: the list holds n
            n_list = n_list + 1;
        }
        __syncthreads();
        // 3. scan those rows again, one wavefront per row
        const uint32_t cnt = n_list;
        for (uint32_t t = wave; t < cnt; t += MERGE_WAVES) {
            const uint32_t r = list[t];
            double d; uint32_t s;
            wave_scan_row(D, lab, n, r, d, s);
            if (lane == 0) { rmin[r] = d; rpart[r] = s; }
        }
        if (tid == 0) rescans += cnt;
        __syncthreads();
        if (tid == 0) n_list = 0;
    }
    if (tid == 0 && n_rescans) *n_rescans = rescans;
}

// PowerMean (src/math/mod.rs:269-295). power: LCTY_PRUNE_POWER_MIN / _MAX or the exponent.
// powi: compiler-rt's __powidf2, which Rust's f64::powi reaches with a run-time exponent.
__host__ __device__ inline double powi_rt(double a, int b) {
    const bool recip = b < 0;
    double r = 1.0;
    while (true) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0 / r : r;
}
__device__ inline double update_mult(int32_t power, double acc, double val, double mult) {
    if (power == LCTY_PRUNE_POWER_MIN) return fmin(acc, val);
    if (power == LCTY_PRUNE_POWER_MAX) return fmax(acc, val);
    if (power == 0) return acc + mult * log(val);
    const double p = powi_rt(val, power);
    const double t = mult * p;                          // kept apart from the add: -ffp-contract=off, Rust never fuses
    return acc + t;
}

// select_representative (prune.rs:276-304): one workgroup per cluster, a thread per member x; buf[x] receives, in this order, the pairs
// (y, x) for y < x, its own term (mult_x > 1), the pairs (x, y) for y > x.
__global__ __launch_bounds__(REPR_THREADS) void prune_repr_kernel(const double* __restrict__ tri, uint32_t n, const uint32_t* __restrict__ mult,
                                                                  const uint32_t* __restrict__ cluster_off, const uint32_t* __restrict__ members,
                                                                  double epsilon, int32_t power, double* __restrict__ acc) {
    const uint32_t lo = cluster_off[blockIdx.x], hi = cluster_off[blockIdx.x + 1], m = hi - lo;
    if (m < 2) return;
    for (uint32_t x = threadIdx.x; x < m; x += REPR_THREADS) {
        const uint32_t idx = members[lo + x], mx = mult[idx];
        double a = 0.0;
        for (uint32_t y = 0; y < m; y++) {
            if (y == x) {
                if (mx > 1) a = update_mult(power, a, epsilon, double(mx - 1));
                continue;
            }
            const uint32_t idy = members[lo + y];
            const double div = epsilon + tri[idx < idy ? tri_index(n, idx, idy) : tri_index(n, idy, idx)];
            a = update_mult(power, a, div, double(mult[idy]));
        }
        acc[lo + x] = a;
    }
}

// ---- host: linkage --------------------------------------------------------------------------------------------------------------------

uint64_t tri_len(uint64_t n) { return n < 2 ? 0 : n * (n - 1) / 2; }

void check_n(uint32_t n) {
    if (n < 1) fail(LCTY_ERR_INVALID_INPUT, "no haplotypes");
    if (n > LCTY_PRUNE_MAX_N)
        fail(LCTY_ERR_UNSUPPORTED, "%u haplotypes: the clustering handles at most LCTY_PRUNE_MAX_N = %u", n, LCTY_PRUNE_MAX_N);
}

void check_tri(uint32_t n, const double* tri) {
    if (n > 1 && !tri) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    const uint64_t len = tri_len(n);
    for (uint64_t t = 0; t < len; t++) if (std::isnan(tri[t])) fail(LCTY_ERR_INVALID_INPUT, "divergence %llu is NaN", static_cast<unsigned long long>(t));
}

// steps[n - 1] from the triangle; d_tri is left on the device for the representatives
void linkage(lcty_ctx* ctx, uint32_t n, const double* tri, lcty_prune_step* steps, DevBuf<double>& d_tri, lcty_prune_stats& st) {
    if (n < 2) return;
    ctx->activate();
    hipStream_t s = ctx->stream;
    double t0 = now_ms();
    const uint64_t len = tri_len(n), cells = uint64_t(n) * n;
    DevBuf<double> D, rmin; DevBuf<uint32_t> lab, rpart, csize, list; DevBuf<lcty_prune_step> d_steps; DevBuf<unsigned long long> d_resc;
    d_tri.alloc(len); D.alloc(cells); rmin.alloc(n); lab.alloc(n); rpart.alloc(n); csize.alloc(n); list.alloc(n); d_steps.alloc(n - 1); d_resc.alloc(1);
    st.matrix_bytes = 8 * cells;
    d_tri.upload(tri, len, s);
    std::vector<uint32_t> h_lab(n), h_one(n, 1);
    for (uint32_t i = 0; i < n; i++) h_lab[i] = i;
    lab.upload(h_lab.data(), n, s); csize.upload(h_one.data(), n, s);
    d_resc.zero(s); d_steps.zero(s);
    st.bytes_h2d += 8 * len + 8ull * n;
    hipLaunchKernelGGL(prune_expand_kernel, dim3(static_cast<uint32_t>((cells + 255) / 256)), dim3(256), 0, s, d_tri.p, n, D.p);
    hipLaunchKernelGGL(prune_init_rows_kernel, dim3((n + 3) / 4), dim3(4 * WAVE), 0, s, D.p, lab.p, n, rmin.p, rpart.p);
    LCTY_HIP(hipGetLastError());
    LCTY_HIP(hipStreamSynchronize(s));
    st.build_ms += now_ms() - t0;
    t0 = now_ms();
    hipLaunchKernelGGL(prune_merge_kernel, dim3(1), dim3(MERGE_THREADS), 0, s, D.p, lab.p, rmin.p, rpart.p, csize.p, list.p, n, d_steps.p, d_resc.p);
    LCTY_HIP(hipGetLastError());
    unsigned long long resc = 0;
    d_steps.download(steps, n - 1, s);
    d_resc.download(&resc, 1, s);
    LCTY_HIP(hipStreamSynchronize(s));
    for (uint32_t t = 0; t + 1 < n; t++)
        if (!(steps[t].cluster1 < steps[t].cluster2 && steps[t].cluster2 < n + t)) fail(LCTY_ERR_RUNTIME, "the merge loop stopped at step %u", t);
    st.n_rescans = resc;
    st.bytes_d2h += sizeof(lcty_prune_step) * uint64_t(n - 1);
    st.merge_ms += now_ms() - t0;
}

// ---- host: the cut (cluster_haplotypes, prune.rs:380-420, without the texts) --------------------------------------------------------------

struct Cut {
    double threshold = 0.0;
    std::vector<uint32_t> cluster_off{0}, members;          // clusters in the order process_cluster meets them
};

Cut cut_tree(uint32_t n, const std::vector<lcty_prune_step>& steps, double threshold, uint32_t n_clusters) {
    Cut c;
    c.threshold = threshold;
    if (n_clusters) c.threshold = n > n_clusters ? steps[n - n_clusters - 1].dissimilarity : 0.0;       // select_cut_threshold, 327-347
    std::vector<std::vector<uint32_t>> haps(2 * size_t(n) - 1);
    for (uint32_t i = 0; i < n; i++) haps[i] = {i};
    auto process = [&](std::vector<uint32_t>& h) {                                                       // process_cluster, 387-399
        if (h.empty()) return;
        c.members.insert(c.members.end(), h.begin(), h.end());
        c.cluster_off.push_back(static_cast<uint32_t>(c.members.size()));
        h.clear();
    };
    for (uint32_t s = 0; s + 1 < n; s++) {
        const lcty_prune_step& st = steps[s];
        if (st.cluster1 >= n + s || st.cluster2 >= n + s || st.cluster1 == st.cluster2) fail(LCTY_ERR_RUNTIME, "step %u names a cluster that does not exist", s);
        std::vector<uint32_t>& a = haps[st.cluster1];
        std::vector<uint32_t>& b = haps[st.cluster2];
        if (st.dissimilarity > c.threshold) { process(a); process(b); }
        std::vector<uint32_t>& m = haps[n + s];                                                          // merge_and_clear, 263-274
        m.reserve(a.size() + b.size());
        m.insert(m.end(), a.begin(), a.end()); m.insert(m.end(), b.begin(), b.end());
        std::vector<uint32_t>().swap(a); std::vector<uint32_t>().swap(b);
    }
    for (std::vector<uint32_t>& h : haps) process(h);                                                    // 418-420: only the root can be left
    return c;
}

constexpr HapLimits kPruneHaps{1, UINT32_MAX, UINT64_MAX};                                              // the bases go to the FASTA text only: no kernel reads them

void check_params(const lcty_prune_params* p) {
    if (!p) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    if (!(p->threshold >= 0.0)) fail(LCTY_ERR_INVALID_INPUT, "Divergence threshold (%g) should be non-negative", p->threshold);
    if (p->power != LCTY_PRUNE_POWER_MIN && p->power != LCTY_PRUNE_POWER_MAX && (p->power < -128 || p->power > 127))
        fail(LCTY_ERR_INVALID_INPUT, "power %d: min, max or an integer -128 to 127", p->power);
    if (p->only_tree && p->skip_tree) fail(LCTY_ERR_INVALID_INPUT, "--skip-tree and --only-tree cannot be used together");
}

void prune_out_free(lcty_prune_out* o) {
    free(o->steps); free(o->keep_ids); free(o->cluster_off); free(o->members); free(o->repr); free(o->acc);
    memset(o, 0, sizeof(*o));
}

void cluster(lcty_ctx* ctx, uint32_t n, const double* tri, const uint32_t* mult, const lcty_prune_params* prm, Handoff& h, lcty_prune_out& o) {
    const double t_all = now_ms();
    lcty_prune_stats st{};
    std::vector<lcty_prune_step> steps(n - 1);
    DevBuf<double> d_tri;
    linkage(ctx, n, tri, steps.data(), d_tri, st);
    double t0 = now_ms();
    const uint64_t len = tri_len(n);
    double min_val = std::numeric_limits<double>::infinity();
    for (uint64_t t = 0; t < len; t++) min_val = std::fmin(min_val, tri[t]);
    const double epsilon = len ? std::fmax(1e-6 * min_val, 1e-12) : 1e-12;                              // prune.rs:362-368
    Cut c = cut_tree(n, steps, prm->threshold, prm->n_clusters);
    const uint32_t nc = static_cast<uint32_t>(c.cluster_off.size() - 1);
    std::vector<uint32_t> h_mult(n, 1);
    if (mult) for (uint32_t i = 0; i < n; i++) { if (!mult[i]) fail(LCTY_ERR_INVALID_INPUT, "mult[%u] is 0", i); h_mult[i] = mult[i]; }
    std::vector<double> acc(n, 0.0);
    bool any = false;
    for (uint32_t k = 0; k < nc; k++) {
        const uint64_t m = c.cluster_off[k + 1] - c.cluster_off[k];
        if (m > 1) { any = true; st.n_rep_pairs += m * (m - 1); }
    }
    st.host_ms += now_ms() - t0;
    if (any) {
        t0 = now_ms();
        hipStream_t s = ctx->stream;
        DevBuf<uint32_t> d_mult, d_off, d_mem; DevBuf<double> d_acc;
        d_mult.alloc(n); d_off.alloc(nc + 1); d_mem.alloc(n); d_acc.alloc(n);
        d_mult.upload(h_mult.data(), n, s); d_off.upload(c.cluster_off.data(), nc + 1, s); d_mem.upload(c.members.data(), n, s);
        d_acc.zero(s);
        hipLaunchKernelGGL(prune_repr_kernel, dim3(nc), dim3(REPR_THREADS), 0, s, d_tri.p, n, d_mult.p, d_off.p, d_mem.p, epsilon, prm->power, d_acc.p);
        LCTY_HIP(hipGetLastError());
        d_acc.download(acc.data(), n, s);
        LCTY_HIP(hipStreamSynchronize(s));
        st.bytes_h2d += 4ull * (2 * n + nc + 1); st.bytes_d2h += 8ull * n;
        st.repr_ms += now_ms() - t0;
    }
    t0 = now_ms();
    std::vector<uint32_t> repr(nc), keep(nc);
    for (uint32_t k = 0; k < nc; k++) {
        const uint32_t lo = c.cluster_off[k], hi = c.cluster_off[k + 1];
        uint32_t best = lo;
        const bool want_max = prm->power < 0 && prm->power != LCTY_PRUNE_POWER_MIN;                      // prune.rs:299-302
        for (uint32_t x = lo + 1; x < hi; x++)
            if (want_max ? acc[x] > acc[best] : acc[x] < acc[best]) best = x;                            // the first optimum (vec.rs:223-232)
        repr[k] = keep[k] = c.members[best];
    }
    std::sort(keep.begin(), keep.end());
    st.host_ms += now_ms() - t0;
    st.total_ms = now_ms() - t_all;
    o.n = n; o.n_clusters = nc; o.threshold = c.threshold; o.epsilon = epsilon; o.stats = st;
    o.steps = h.copy(steps); o.keep_ids = h.copy(keep); o.cluster_off = h.copy(c.cluster_off); o.members = h.copy(c.members);
    o.repr = h.copy(repr); o.acc = h.copy(acc);
}

// ---- host: texts ----------------------------------------------------------------------------------------------------------------------

std::unordered_map<std::string, uint32_t> name_ids(const std::vector<std::string>& names) {
    std::unordered_map<std::string, uint32_t> ids;
    ids.reserve(names.size() * 2);
    for (uint32_t i = 0; i < names.size(); i++) ids.emplace(names[i], i);
    return ids;
}

bool is_space(char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); }

// `BufRead::lines`: pieces between '\n', a '\r' before it dropped, no piece after a final '\n'
template <typename F>
void for_lines(const char* text, uint64_t len, F&& fn) {
    uint64_t p = 0;
    while (p < len) {
        const char* nl = static_cast<const char*>(memchr(text + p, '\n', len - p));
        uint64_t e = nl ? static_cast<uint64_t>(nl - text) : len;
        uint64_t le = e;
        if (nl && le > p && text[le - 1] == '\r') le--;
        fn(text + p, le - p);
        p = e + 1;
    }
}

// DiscardedHaplotypes::load (contigs.rs:488-528): the names listed per contig of the locus, in file order
std::vector<std::vector<std::string>> discarded_by_contig(const char* text, uint64_t len, const std::vector<std::string>& names, bool* all_identical) {
    const std::unordered_map<std::string, uint32_t> ids = name_ids(names);
    std::vector<std::vector<std::string>> by_contig(names.size());
    std::unordered_map<std::string, std::vector<std::string>> unknown;
    bool all_id = true;
    if (text) for_lines(text, len, [&](const char* l, uint64_t ll) {
        std::vector<std::string> cols;
        uint64_t p = 0;
        while (p < ll) {
            while (p < ll && is_space(l[p])) p++;
            uint64_t q = p;
            while (q < ll && !is_space(l[q])) q++;
            if (q > p) cols.emplace_back(l + p, q - p);
            p = q;
        }
        if (cols.size() < 3) fail(LCTY_ERR_INVALID_INPUT, "Each line in discarded haplotypes must have at least 3 columns");
        all_id = all_id && cols[1] == "=";
        std::vector<std::string> rhs;
        for (size_t t = 2; t < cols.size(); t++) {
            std::string c = cols[t];
            if (!c.empty() && c.back() == ',') c.pop_back();
            if (ids.count(c)) continue;                                   // listed as discarded, yet in the FASTA: the reference warns and skips
            rhs.push_back(c);
            auto it = unknown.find(c);
            if (it != unknown.end()) { rhs.insert(rhs.end(), it->second.begin(), it->second.end()); unknown.erase(it); }
        }
        auto id = ids.find(cols[0]);
        if (id != ids.end()) by_contig[id->second] = rhs; else unknown[cols[0]] = rhs;
    });
    if (all_identical) *all_identical = all_id;
    return by_contig;
}

// Rust's {:.8}: NaN and inf are spelled its way
std::string fmt8(double v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char b[400]; snprintf(b, sizeof(b), "%.8f", v); return b;
}

void texts(uint32_t n, const std::vector<std::string>& names, const std::vector<std::vector<std::string>>& disc, const lcty_prune_out* res,
           std::string* newick, std::string* new_lines) {
    if (res->n != n || (n > 1 && !res->steps) || !res->cluster_off || !res->members || !res->repr) fail(LCTY_ERR_INVALID_INPUT, "the result does not belong to these names");
    if (newick) {
        std::vector<std::string> nwk(2 * size_t(n) - 1);
        std::vector<double> div(2 * size_t(n) - 1, 0.0);
        for (uint32_t i = 0; i < n; i++) {
            nwk[i] = names[i];
            if (!disc[i].empty()) {                                       // add_identical, 251-260
                nwk[i] = "(" + names[i] + ":0";
                for (const std::string& h : disc[i]) nwk[i] += "," + h + ":0";
                nwk[i] += ")";
            }
        }
        for (uint32_t s = 0; s + 1 < n; s++) {
            const lcty_prune_step& st = res->steps[s];
            if (st.cluster1 >= n + s || st.cluster2 >= n + s) fail(LCTY_ERR_INVALID_INPUT, "step %u names a cluster that does not exist", s);
            const double d = st.dissimilarity;
            nwk[n + s] = "(" + nwk[st.cluster1] + ":" + fmt8(0.5 * (d - div[st.cluster1])) + "," + nwk[st.cluster2] + ":" + fmt8(0.5 * (d - div[st.cluster2])) + ")";
            div[n + s] = d;
            std::string().swap(nwk[st.cluster1]); std::string().swap(nwk[st.cluster2]);
        }
        *newick = nwk.back() + ";\n";
    }
    if (new_lines) {
        new_lines->clear();
        for (uint32_t k = 0; k < res->n_clusters; k++) {                  // write_discarded_haplotypes, 306-323
            const uint32_t lo = res->cluster_off[k], hi = res->cluster_off[k + 1];
            if (hi - lo < 2) continue;
            if (hi > n || res->repr[k] >= n) fail(LCTY_ERR_INVALID_INPUT, "cluster %u is out of range", k);
            *new_lines += names[res->repr[k]] + " ";
            char sep = '~';
            for (uint32_t x = lo; x < hi; x++) {
                const uint32_t h = res->members[x];
                if (h >= n) fail(LCTY_ERR_INVALID_INPUT, "cluster %u is out of range", k);
                if (h == res->repr[k]) continue;
                *new_lines += sep; *new_lines += " "; *new_lines += names[h];
                sep = ',';
            }
            *new_lines += "\n";
        }
    }
}

// ---- host: divergences from the PAF (load_divergences, prune.rs:159-230) -------------------------------------------------------------------

// str::parse::<f64>: [+-] then inf | infinity | nan (any case), or digits [. digits] [e [+-] digits] with a digit before the exponent
bool parse_f64(const char* s, uint64_t len, double* out) {
    if (len == 0 || len > 400) return false;
    uint64_t p = 0;
    if (s[p] == '+' || s[p] == '-') p++;
    auto ieq = [&](const char* w) {
        const uint64_t wl = strlen(w);
        if (len - p != wl) return false;
        for (uint64_t t = 0; t < wl; t++) if ((s[p + t] | 0x20) != w[t]) return false;
        return true;
    };
    bool special = ieq("inf") || ieq("infinity") || ieq("nan");
    if (!special) {
        uint64_t q = p, digits = 0;
        while (q < len && s[q] >= '0' && s[q] <= '9') { q++; digits++; }
        if (q < len && s[q] == '.') { q++; while (q < len && s[q] >= '0' && s[q] <= '9') { q++; digits++; } }
        if (!digits) return false;
        if (q < len && (s[q] == 'e' || s[q] == 'E')) {
            q++;
            if (q < len && (s[q] == '+' || s[q] == '-')) q++;
            uint64_t ed = 0;
            while (q < len && s[q] >= '0' && s[q] <= '9') { q++; ed++; }
            if (!ed) return false;
        }
        if (q != len) return false;
    }
    const std::string z(s, len);
    *out = strtod(z.c_str(), nullptr);
    return true;
}

void paf_divergences(const uint8_t* text, uint64_t len, const std::vector<std::string>& names, const char* field, double repl_missing, double* tri,
                     lcty_paf_div_stats* stats) {
    const uint32_t n = static_cast<uint32_t>(names.size());
    const std::string fld = field ? field : "dv";
    if (fld.find(':') != std::string::npos) fail(LCTY_ERR_INVALID_INPUT, "PAF divergence field (%s) must not contain :", fld.c_str());
    const std::string prefix = fld + ":";
    const uint64_t crop = prefix.size() + 2, tl = tri_len(n);
    const std::unordered_map<std::string, uint32_t> ids = name_ids(names);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(tri, tri + tl, nan);
    lcty_paf_div_stats st{};
    st.missing_i = st.missing_j = 0xFFFFFFFFu;
    if (len && !text) fail(LCTY_ERR_INVALID_INPUT, "null argument");
    for_lines(reinterpret_cast<const char*>(text), len, [&](const char* l, uint64_t ll) {
        while (ll && is_space(l[ll - 1])) ll--;                           // trim_end
        std::vector<std::pair<const char*, uint64_t>> cols;
        uint64_t p = 0;
        while (true) {
            const char* tab = static_cast<const char*>(memchr(l + p, '\t', ll - p));
            const uint64_t e = tab ? static_cast<uint64_t>(tab - l) : ll;
            cols.emplace_back(l + p, e - p);
            if (!tab) break;
            p = e + 1;
        }
        auto id1 = ids.find(std::string(cols[0].first, cols[0].second));
        if (id1 == ids.end()) return;
        if (cols.size() < 6) fail(LCTY_ERR_INVALID_DATA, "Could not parse PAF line `%.*s`", static_cast<int>(std::min<uint64_t>(ll, 200)), l);
        auto id2 = ids.find(std::string(cols[5].first, cols[5].second));
        if (id2 == ids.end()) return;
        if (id1->second == id2->second) return;
        if (cols.size() < 12) fail(LCTY_ERR_INVALID_DATA, "Could not parse PAF line `%.*s`", static_cast<int>(std::min<uint64_t>(ll, 200)), l);
        bool have = false; double val = 0.0;
        for (size_t t = 12; t < cols.size(); t++) {
            if (cols[t].second >= prefix.size() && memcmp(cols[t].first, prefix.data(), prefix.size()) == 0) {
                if (cols[t].second < crop || !parse_f64(cols[t].first + crop, cols[t].second - crop, &val))
                    fail(LCTY_ERR_INVALID_DATA, "Cannot parse divergence `%.*s`", static_cast<int>(std::min<uint64_t>(cols[t].second, 200)), cols[t].first);
                have = true;
                break;
            }
        }
        if (!have) return;
        if (val < 0.0) { st.n_negative++; return; }
        const uint32_t i = std::min(id1->second, id2->second), j = std::max(id1->second, id2->second);
        double& d = tri[tri_index(n, i, j)];
        if (!std::isnan(d) && d != val) { st.n_conflicting++; return; }
        d = val;
    });
    uint64_t k = 0;
    for (uint32_t i = 0; i + 1 < n; i++)
        for (uint32_t j = i + 1; j < n; j++, k++)
            if (std::isnan(tri[k])) { st.n_missing++; st.missing_i = i; st.missing_j = j; tri[k] = repl_missing; }
    if (stats) *stats = st;
    if (st.n_missing == tl) fail(LCTY_ERR_INVALID_INPUT, "Divergence missing for all haplotype pairs");
}

// ---- host: the thinned files (prune_files, prune.rs:471-518) ------------------------------------------------------------------------------

void throw_rc(int32_t rc) { if (rc != LCTY_OK) throw Error(rc, lcty_last_error()); }

// one KmerCounts block at buf: thinned to `keep` and saved again; false when it does not match the haplotypes (KmerCounts::validate)
bool thin_kmer_block(const uint8_t* buf, uint64_t len, const std::vector<uint32_t>& keep, const std::vector<uint64_t>& seq_len, uint64_t* consumed,
                     std::vector<uint8_t>& out) {
    uint32_t k = 0, nc = 0;
    throw_rc(lcty_kmer_counts_parse(buf, len, &k, &nc, nullptr, 0, nullptr, 0, consumed));
    std::vector<uint64_t> off(nc + 1);
    std::vector<uint16_t> counts(std::max<uint64_t>(*consumed, 1));
    throw_rc(lcty_kmer_counts_parse(buf, len, &k, &nc, off.data(), nc + 1, counts.data(), counts.size(), consumed));
    if (nc != seq_len.size()) return false;
    for (uint32_t a = 0; a < nc; a++) {
        const uint64_t expected = seq_len[a] + 1 > k ? seq_len[a] + 1 - k : 0;
        if (expected != off[a + 1] - off[a]) return false;
    }
    std::vector<uint64_t> toff{0}; std::vector<uint16_t> tc;
    for (uint32_t a : keep) { tc.insert(tc.end(), counts.begin() + off[a], counts.begin() + off[a + 1]); toff.push_back(tc.size()); }
    // KmerCounts::save writes max_value.count_ones() / 8, and max_value is at most 65535 (counts.rs:114, 133): 1 stays 1, anything above is 2
    const uint32_t counter_bytes = buf[1] <= 1 ? 1 : 2;
    std::vector<uint8_t> block;
    sized([&](uint8_t* o, uint64_t c, uint64_t* nd) { return lcty_kmer_counts_write(k, counter_bytes, static_cast<uint32_t>(keep.size()), toff.data(), tc.data(), o, c, nd); }, block);
    out.insert(out.end(), block.begin(), block.end());
    return true;
}

// prune_paf (src/seq/paf.rs:237-267)
std::string prune_paf(const uint8_t* text, uint64_t len, const std::vector<std::string>& names, const std::vector<uint32_t>& keep_ids) {
    const std::unordered_map<std::string, uint32_t> ids = name_ids(names);
    std::vector<uint8_t> keep(names.size(), 0);
    for (uint32_t id : keep_ids) keep[id] = 1;
    std::string out;
    for_lines(reinterpret_cast<const char*>(text), len, [&](const char* l, uint64_t ll) {
        if (ll && l[0] == '#') { out.append(l, ll); out += '\n'; return; }
        const char* col[7]; uint64_t cl[7]; int nc = 0;                   // splitn(7, '\t')
        uint64_t p = 0;
        while (nc < 7) {
            const char* tab = nc < 6 ? static_cast<const char*>(memchr(l + p, '\t', ll - p)) : nullptr;
            const uint64_t e = tab ? static_cast<uint64_t>(tab - l) : ll;
            col[nc] = l + p; cl[nc] = e - p; nc++;
            if (!tab) break;
            p = e + 1;
        }
        if (nc < 7) fail(LCTY_ERR_INVALID_DATA, "Could not parse PAF line `%.*s`", static_cast<int>(std::min<uint64_t>(ll, 200)), l);
        auto a = ids.find(std::string(col[0], cl[0])), b = ids.find(std::string(col[5], cl[5]));
        if (a != ids.end() && b != ids.end() && keep[a->second] && keep[b->second]) { out.append(l, ll); out += '\n'; }
    });
    return out;
}

// prune_files (471-518) below the copy branch: the files of the kept haplotypes into f
void thin_files(uint32_t n, const std::vector<std::string>& nm, const uint8_t* seqs, const uint64_t* seq_off, const uint8_t* paf, uint64_t paf_len,
                const uint8_t* kmers, uint64_t kmers_len, const uint8_t* distances, uint64_t distances_len, const std::vector<uint32_t>& keep,
                Handoff& h, lcty_prune_files& f) {
    std::string fa;
    for (uint32_t a : keep) {                                                                            // fastx::write_fasta: one line per sequence
        fa += ">" + nm[a] + "\n";
        fa.append(reinterpret_cast<const char*>(seqs) + seq_off[a], seq_off[a + 1] - seq_off[a]);
        fa += "\n";
    }
    f.fasta = h.bytes(fa); f.fasta_len = fa.size();
    if (kmers && kmers_len) {                                                                            // 488-503: both blocks, or none
        std::vector<uint64_t> slen(n);
        for (uint32_t a = 0; a < n; a++) slen[a] = seq_off[a + 1] - seq_off[a];
        std::vector<uint8_t> blocks;
        uint64_t used1 = 0, used2 = 0;
        bool ok = thin_kmer_block(kmers, kmers_len, keep, slen, &used1, blocks);
        ok = thin_kmer_block(kmers + used1, kmers_len - used1, keep, slen, &used2, blocks) && ok;
        if (ok) { f.kmers = h.copy(blocks); f.kmers_len = blocks.size(); }
        else f.warn_bits |= LCTY_PRUNE_WARN_KMERS;
    }
    if (distances && distances_len) {                                                                    // 505-513
        uint32_t dk = 0, dw = 0;
        std::vector<uint32_t> dist(uint64_t(n) * n);
        throw_rc(lcty_distances_parse(distances, distances_len, n, &dk, &dw, dist.data()));
        const uint32_t m = static_cast<uint32_t>(keep.size());
        std::vector<uint32_t> sub;
        for (uint32_t i = 0; i + 1 < m; i++)
            for (uint32_t j = i + 1; j < m; j++) sub.push_back(dist[uint64_t(keep[i]) * n + keep[j]]);
        std::vector<uint8_t> db;
        sub.push_back(0);                                                                                // never read: a valid pointer for m = 1
        sized([&](uint8_t* o, uint64_t c, uint64_t* nd) { return lcty_distances_write(dk, dw, m, sub.data(), o, c, nd); }, db);
        f.distances = h.copy(db); f.distances_len = db.size();
    }
    const std::string pp = prune_paf(paf, paf_len, nm, keep);
    f.paf = h.bytes(pp); f.paf_len = pp.size();
}

void prune_files_free(lcty_prune_files* f) {
    free(f->newick); free(f->discarded); free(f->fasta); free(f->kmers); free(f->distances); free(f->paf); free(f->keep);
    memset(f, 0, sizeof(*f));
}

}  // namespace

extern "C" {

void lcty_prune_params_default(lcty_prune_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->threshold = 0.0002;                      // prune.rs:49
    p->n_clusters = 0;
    p->power = 2;                               // prune.rs:51
}

int32_t lcty_paf_divergences(const uint8_t* text, uint64_t len, const char* const* names, uint32_t n, const char* field, double repl_missing, double* tri,
                             lcty_paf_div_stats* stats) {
    return guarded([&] {
        if (!names || (n > 1 && !tri)) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n < 1) fail(LCTY_ERR_INVALID_INPUT, "no haplotypes");
        std::vector<std::string> nm(n);
        for (uint32_t i = 0; i < n; i++) { if (!names[i]) fail(LCTY_ERR_INVALID_INPUT, "null argument"); nm[i] = names[i]; }
        double dummy = 0.0;
        paf_divergences(text, len, nm, field, repl_missing, n > 1 ? tri : &dummy, stats);
    });
}

int32_t lcty_prune_multiplicities(const char* text, uint64_t len, const char* const* names, uint32_t n, uint32_t* mult, int32_t* all_identical) {
    return guarded([&] {
        if (!names || !mult) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        std::vector<std::string> nm(n);
        for (uint32_t i = 0; i < n; i++) { if (!names[i]) fail(LCTY_ERR_INVALID_INPUT, "null argument"); nm[i] = names[i]; }
        bool all_id = true;
        const std::vector<std::vector<std::string>> by = discarded_by_contig(text, text ? len : 0, nm, &all_id);
        for (uint32_t i = 0; i < n; i++) mult[i] = 1 + static_cast<uint32_t>(by[i].size());
        if (all_identical) *all_identical = all_id ? 1 : 0;
    });
}

int32_t lcty_prune_linkage(lcty_ctx* ctx, uint32_t n, const double* tri, lcty_prune_step* steps, lcty_prune_stats* stats) {
    return guarded([&] {
        if (!ctx) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_n(n);
        if (n > 1 && !steps) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_tri(n, tri);
        const double t0 = now_ms();
        lcty_prune_stats st{};
        DevBuf<double> d_tri;
        linkage(ctx, n, tri, steps, d_tri, st);
        st.total_ms = now_ms() - t0;
        if (stats) *stats = st;
    });
}

int32_t lcty_prune_cluster(lcty_ctx* ctx, uint32_t n, const double* tri, const uint32_t* mult, const lcty_prune_params* params, lcty_prune_out* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_n(n);
        check_params(params);
        check_tri(n, tri);
        lcty_prune_out o{}; Handoff h;
        cluster(ctx, n, tri, mult, params, h, o);
        *out = o; h.commit();
    });
}

void lcty_prune_out_free(lcty_prune_out* out) {
    if (out) prune_out_free(out);
}

int32_t lcty_prune_texts(uint32_t n, const char* names, const char* old_discarded, uint64_t old_len, const lcty_prune_out* res, uint8_t** newick,
                         uint64_t* newick_len, uint8_t** discarded, uint64_t* discarded_len) {
    return guarded([&] {
        if (newick) *newick = nullptr;
        if (newick_len) *newick_len = 0;
        if (discarded) *discarded = nullptr;
        if (discarded_len) *discarded_len = 0;
        if (!res || !newick || !newick_len || !discarded || !discarded_len) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n < 1) fail(LCTY_ERR_INVALID_INPUT, "no haplotypes");
        const std::vector<std::string> nm = split_names(names, n);
        if (!old_discarded) old_len = 0;
        const std::vector<std::vector<std::string>> disc = discarded_by_contig(old_discarded, old_len, nm, nullptr);
        std::string nwk, lines;
        texts(n, nm, disc, res, &nwk, &lines);
        std::string all(old_discarded ? old_discarded : "", old_len);
        all += lines;
        Handoff h;
        uint8_t* a = h.bytes(nwk); uint8_t* b = h.bytes(all);
        *newick = a; *newick_len = nwk.size(); *discarded = b; *discarded_len = all.size();
        h.commit();
    });
}

int32_t lcty_prune_thin(uint32_t n, const char* names, const uint8_t* seqs, const uint64_t* seq_off, const uint8_t* paf, uint64_t paf_len,
                        const uint8_t* kmers, uint64_t kmers_len, const uint8_t* distances, uint64_t distances_len, const uint32_t* keep, uint32_t n_keep,
                        lcty_prune_files* out) {
    return guarded([&] {
        if (!out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        memset(out, 0, sizeof(*out));
        if (!paf || !keep) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        if (n_keep < 1) fail(LCTY_ERR_INVALID_INPUT, "no haplotypes");
        check_haps(n, seqs, seq_off, kPruneHaps);
        for (uint32_t t = 0; t < n_keep; t++)
            if (keep[t] >= n || (t && keep[t] <= keep[t - 1])) fail(LCTY_ERR_INVALID_INPUT, "keep must be ascending ids below %u", n);
        const std::vector<std::string> nm = split_names(names, n);
        const std::vector<uint32_t> kv(keep, keep + n_keep);
        lcty_prune_files f{}; Handoff h;
        f.keep = h.copy(kv); f.n_keep = n_keep;
        thin_files(n, nm, seqs, seq_off, paf, paf_len, kmers, kmers_len, distances, distances_len, kv, h, f);
        *out = f; h.commit();
    });
}

int32_t lcty_db_prune_locus(lcty_ctx* ctx, uint32_t n, const char* names, const uint8_t* seqs, const uint64_t* seq_off, const uint8_t* paf, uint64_t paf_len,
                            const uint8_t* kmers, uint64_t kmers_len, const uint8_t* distances, uint64_t distances_len, const char* discarded,
                            uint64_t discarded_len, const char* field, const lcty_prune_params* params, lcty_prune_files* out) {
    return guarded([&] {
        if (out) memset(out, 0, sizeof(*out));
        if (!ctx || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_params(params);
        if (n < 1) fail(LCTY_ERR_INVALID_DATA, "No haplotypes found");                                   // process_locus, 528-530
        check_n(n);
        if (!paf) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        check_haps(n, seqs, seq_off, kPruneHaps);
        const std::vector<std::string> nm = split_names(names, n);
        lcty_prune_files f{}; Handoff h;
        lcty_prune_out res{}; Handoff h_res;                                                             // the clustering: used here, never handed out
        const double repl = params->n_clusters ? std::numeric_limits<double>::infinity() : 10.0 * params->threshold;   // 537
        std::vector<double> tri(std::max<uint64_t>(tri_len(n), 1));
        paf_divergences(paf, paf_len, nm, field, repl, tri.data(), &f.div);
        if (params->skip_tree || !discarded) { discarded = nullptr; discarded_len = 0; }             // 542-547: not read with --skip-tree
        const std::vector<std::vector<std::string>> disc = discarded_by_contig(discarded, discarded_len, nm, nullptr);
        std::vector<uint32_t> mult(n);
        for (uint32_t i = 0; i < n; i++) mult[i] = 1 + static_cast<uint32_t>(disc[i].size());
        cluster(ctx, n, tri.data(), mult.data(), params, h_res, res);
        f.stats = res.stats; f.threshold = res.threshold;
        std::string nwk, lines;
        texts(n, nm, disc, &res, params->skip_tree ? nullptr : &nwk, &lines);
        f.newick = h.bytes(nwk); f.newick_len = nwk.size();
        const std::vector<uint32_t> keep(res.keep_ids, res.keep_ids + res.n_clusters);
        f.keep = h.copy(keep); f.n_keep = res.n_clusters;
        if (!params->only_tree) {
            std::string all(discarded ? discarded : "", discarded_len);
            all += lines;
            f.discarded = h.bytes(all); f.discarded_len = all.size();
            if (keep.size() == n) {
                f.unchanged = 1;                                                                     // copy_output_files, 475-478
            } else {
                thin_files(n, nm, seqs, seq_off, paf, paf_len, kmers, kmers_len, distances, distances_len, keep, h, f);
            }
        }
        *out = f; h.commit();
    });
}

void lcty_prune_files_free(lcty_prune_files* files) {
    if (files) prune_files_free(files);
}

}  // extern "C"
