// lcty_bg.hip — the background distributions of a sample (PREPROC/distr.gz) from its alignments to one background region:
// estimate_bg_distrs (src/command/preproc.rs:1157-1192) on the existing-alignments path with a background region (`preproc -a`),
// both branches: estimate_bg_from_paired (1065-1121) and estimate_bg_from_unpaired (1123-1155).
//   device  windows_kernel   filter_windows (bg/windows.rs:44-101) on the windows of Windows::create (121-160): GC content and the
//                            fraction of k-mer counts <= 1 over each window's neighbourhood, one wavefront per window
//           counts_kernel    Cigar::infer_ext_cigar (seq/cigar.rs:434-476) + count_region_operations (seq/aln.rs:241-281) with the
//                            background interval as the region, edit_distance (bg/err_prof.rs:73-79) and the window of the
//                            alignment middle (model/windows.rs:62-68); no extended CIGAR is built: an M base matches iff the read
//                            base is the same A/C/G/T as the reference base, 16 bases per packed-word compare. One lane per short
//                            record, one wavefront per long one
//           pairs_kernel     insert_size / pair_orientation (seq/aln.rs:223-233) of every pair
//           depth_kernel     count_reads (bg/depth.rs:27-39): integer atomics per (window, read end), every window
//   host    InsertDistr::estimate (bg/insertsz.rs:67-143) + confidence_interval (158-166); ErrorProfile::estimate (err_prof.rs:152-197)
//           with to_ln_probs (82-108) and BetaBinomial::max_lik_estimate (math/distr/betabinom.rs:105-160); SingleEditDistCache
//           (err_prof.rs:333-355); ReadDepth::estimate (depth.rs:300-345): LOESS (algo/loess.rs:79-160), blur_boundary_values
//           (98-126), RegularizedEstimator (math/distr/nbinom.rs:154-244). Both fits use one Nelder–Mead routine (argmin's defaults).
// Not here (see include/locityper_hip.h): mapping, jellyfish, --similar-dataset, subsampling the input, OpCounter::Unbounded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <numeric>
#include <vector>

#include "lcty_bg_reads.hpp"
#include "lcty_common.hpp"
#include "lcty_seq.hpp"
#include "lcty_math.hpp"
#include "lcty_scan.hpp"

using namespace lcty;

namespace {

constexpr uint32_t NONE = LCTY_NONE_U32;
constexpr uint32_t LONG_RECORD = 2048;       // query bases from which a record is walked by a whole wavefront

// ---------------------------------------------------------------------------------------------------------------------------------
// device
// 16 packed bases (2 bits each) starting at base `off`; the arrays carry one spare word at their end
__device__ __forceinline__ uint32_t get16(const uint32_t* w, uint64_t off) {
    const uint64_t i = off >> 4;
    const uint32_t s = 2u * static_cast<uint32_t>(off & 15);
    return s ? (w[i] >> s) | (w[i + 1] << (32 - s)) : w[i];
}
__device__ __forceinline__ uint32_t get16_mask(const uint32_t* m, uint64_t off) {     // 16 "not ACGT" bits starting at base `off`
    const uint64_t i = off >> 5;
    const uint32_t s = static_cast<uint32_t>(off & 31);
    return (s ? (m[i] >> s) | (m[i + 1] << (32 - s)) : m[i]) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t spread16(uint32_t v) {                             // bit i -> bit 2i
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

// filter_windows: window i over its neighbourhood [start_ix, end_ix) of the region sequence (clipped as saturating_sub / min do)
__global__ void windows_kernel(const uint8_t* __restrict__ seq, uint32_t seq_len, const uint16_t* __restrict__ counts,
                               uint32_t first_start, uint32_t window, uint32_t left_pad, uint32_t right_pad, uint32_t k,
                               uint32_t n_windows, uint32_t* __restrict__ gc_out, uint32_t* __restrict__ low_out, uint32_t* __restrict__ span_out) {
    const uint32_t wi = blockIdx.x;
    if (wi >= n_windows) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t ws = first_start + wi * window;                 // relative to the region start
    const uint32_t start_ix = ws > left_pad ? ws - left_pad : 0u;
    const uint32_t end_ix = min(ws + window + right_pad, seq_len);
    const uint32_t end_ix2 = end_ix + 1 - k;
    uint32_t gc = 0, low = 0;
    for (uint32_t i = start_ix + lane; i < end_ix; i += 64) { const uint8_t c = seq[i]; gc += (c == 'C') | (c == 'G'); }
    for (uint32_t i = start_ix + lane; i < end_ix2; i += 64) low += counts[i] <= 1;
    gc = wave_reduce(gc, AddOp{}); low = wave_reduce(low, AddOp{});
    if (lane == 0) { gc_out[wi] = gc; low_out[wi] = low; span_out[2 * wi] = end_ix - start_ix; span_out[2 * wi + 1] = end_ix2 - start_ix; }
}

struct RecArgs {
    const uint32_t* pos; const uint32_t* end; const uint64_t* cigar_off; const uint32_t* cigar; const uint64_t* seq_off;
    const uint32_t* bases2; const uint32_t* nmask; const uint32_t* ref2;
    uint32_t padded_start, region_start, region_end, win_start, win_end, window;
    const uint32_t* list; uint32_t n_list;
    uint32_t* counts;            // [5 n] =, X, I, D, S
    uint32_t* edit; uint32_t* read_len; uint32_t* middle; uint32_t* win;
};

// One record by W lanes: the operations are walked by every lane alike, the bases of an M run inside the region are compared in
// 16-base chunks dealt out to the lanes; the equal counts are summed over the lanes (integers: the same in any order).
template <int W>
__device__ void count_record(const RecArgs& a, uint32_t r, uint32_t lane) {
    const uint32_t rs = a.region_start, re = a.region_end;
    uint32_t m = 0, x = 0, ins = 0, del = 0, clip = 0, eq_lane = 0;
    uint32_t rpos = a.pos[r];
    uint64_t qpos = a.seq_off[r];
    const uint64_t c0 = a.cigar_off[r], c1 = a.cigar_off[r + 1];
    for (uint64_t c = c0; c < c1; c++) {
        const uint32_t op = a.cigar[c] & 15u, len = a.cigar[c] >> 4;
        const uint32_t lo = max(rpos, rs), hi = min(rpos + len, re);
        const uint32_t ov = hi > lo ? hi - lo : 0u;
        switch (op) {
            case 0: {                                               // M: = / X from the bases
                if (ov) {
                    const uint64_t ra = lo - a.padded_start, qa = qpos + (lo - rpos);
                    for (uint32_t ch = lane; 16u * ch < ov; ch += W) {
                        const uint32_t nb = min(16u, ov - 16u * ch);
                        const uint32_t d = get16(a.ref2, ra + 16u * ch) ^ get16(a.bases2, qa + 16u * ch);
                        uint32_t bad = ((d | (d >> 1)) & 0x55555555u) | spread16(get16_mask(a.nmask, qa + 16u * ch));
                        if (nb < 16) bad &= (1u << (2 * nb)) - 1u;
                        eq_lane += nb - __popc(bad);
                    }
                    x += ov;                                        // minus the matches below
                }
                rpos += len; qpos += len; break;
            }
            case 7: m += ov; rpos += len; qpos += len; break;       // =
            case 8: x += ov; rpos += len; qpos += len; break;       // X
            case 2: del += ov; rpos += len; break;                  // D
            case 1: ins += (rs <= rpos && rpos < re) ? len : 0u; qpos += len; break;
            case 4:                                                 // S: the first op up to the region start, any other up to its end
                clip += c == c0 ? min(len, rpos > rs ? rpos - rs : 0u) : min(len, re > rpos ? re - rpos : 0u);
                qpos += len; break;
            default: break;                                         // refused by the reader
        }
    }
    const uint32_t eq = W > 1 ? wave_reduce(eq_lane, AddOp{}) : eq_lane;
    if (lane == 0) {
        m += eq; x -= eq;
        uint32_t* o = a.counts + 5ull * r;
        o[0] = m; o[1] = x; o[2] = ins; o[3] = del; o[4] = clip;
        const uint32_t common = x + ins + clip;
        a.edit[r] = common + del; a.read_len[r] = common + m;
        const uint32_t mid = static_cast<uint32_t>((static_cast<uint64_t>(a.pos[r]) + a.end[r]) / 2);   // Interval::middle
        a.middle[r] = mid;
        a.win[r] = (a.win_start <= mid && mid < a.win_end) ? (mid - a.win_start) / a.window : NONE;
    }
}

__global__ void counts_short_kernel(RecArgs a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.n_list) count_record<1>(a, a.list[t], 0);
}
__global__ void counts_long_kernel(RecArgs a) {
    const uint32_t t = blockIdx.x;
    if (t < a.n_list) count_record<64>(a, a.list[t], threadIdx.x);
}

__global__ void pairs_kernel(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ end, const uint8_t* __restrict__ flags,
                             const uint32_t* __restrict__ first, const uint32_t* __restrict__ second, uint32_t n,
                             uint32_t* __restrict__ insert, uint8_t* __restrict__ same) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = first[t], j = second[t];
    insert[t] = max(end[i], end[j]) - min(pos[i], pos[j]);                              // Interval::furthest_distance
    same[t] = ((flags[i] ^ flags[j]) & LCTY_BG_REVERSE) == 0;
}

__global__ void depth_kernel(const uint32_t* __restrict__ list, uint32_t n, const uint32_t* __restrict__ win,
                             const uint8_t* __restrict__ flags, uint32_t* __restrict__ depth) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t r = list[t];
    if (win[r] != NONE) atomicAdd(&depth[2 * win[r] + ((flags[r] & LCTY_BG_SECOND) ? 1 : 0)], 1u);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host fits
using Vec2 = std::array<double, 2>;

// Nelder–Mead as argmin's NelderMead (reflection 1, expansion 2, contraction 0.5, shrink 0.5) from three given vertices, until the
// standard deviation of the vertex costs is below `sd_tol`. argmin itself is not reproduced iterate for iterate.
template <typename F>
Vec2 nelder_mead(F&& cost, const std::array<Vec2, 3>& start, double sd_tol) {
    std::array<std::pair<Vec2, double>, 3> v;
    for (int i = 0; i < 3; i++) v[i] = {start[i], cost(start[i])};
    auto order = [&] { std::stable_sort(v.begin(), v.end(), [](const auto& p, const auto& q) { return p.second < q.second; }); };
    order();
    for (int it = 0; it < 1000000; it++) {
        const double mean = (v[0].second + v[1].second + v[2].second) / 3.0;
        double ss = 0.0;
        for (const auto& p : v) ss += (p.second - mean) * (p.second - mean);
        if (std::sqrt(ss / 2.0) < sd_tol) break;
        const Vec2 c = {(v[0].first[0] + v[1].first[0]) / 2.0, (v[0].first[1] + v[1].first[1]) / 2.0};
        auto along = [&](const Vec2& to, double t) { return Vec2{c[0] + t * (to[0] - c[0]), c[1] + t * (to[1] - c[1])}; };
        const Vec2 xr = along(v[2].first, -1.0);
        const double fr = cost(xr);
        if (fr < v[1].second && fr >= v[0].second) {
            v[2] = {xr, fr};
        } else if (fr < v[0].second) {
            const Vec2 xe = along(xr, 2.0);
            const double fe = cost(xe);
            v[2] = fe < fr ? std::make_pair(xe, fe) : std::make_pair(xr, fr);
        } else {
            const Vec2 xc = along(v[2].first, 0.5);
            const double fc = cost(xc);
            if (fc < v[2].second) {
                v[2] = {xc, fc};
            } else {
                for (int i = 1; i < 3; i++) {
                    const Vec2 y = {v[0].first[0] + 0.5 * (v[i].first[0] - v[0].first[0]), v[0].first[1] + 0.5 * (v[i].first[1] - v[0].first[1])};
                    v[i] = {y, cost(y)};
                }
            }
        }
        order();
    }
    return v[0].first;
}

// RegularizedEstimator::estimate (nbinom.rs:222-244) with the cost of NBinomProblem (176-210)
math::NBinom nbinom_regularized(double mean, double var, double rate, double lambda) {
    auto cost = [&](const Vec2& x) {
        const double n = x[0], p = x[1];
        if (n <= 0.0 || p <= 0.0 || p >= 1.0) return 1e30;
        const double me = rate * n * (1.0 - p) / p - mean;
        const double ve = rate * n * (1.0 - p) * (p + rate - p * rate) / (p * p) - var;
        return me * me + ve * ve + lambda * n;
    };
    const Vec2 r = nelder_mead(cost, {Vec2{10.0, 0.3}, Vec2{20.0, 0.7}, Vec2{30.0, 0.3}}, 1e-6);
    return math::NBinom(r[0], r[1]);
}

// NBinom::estimate_corrected (nbinom.rs:53-65)
math::NBinom nbinom_corrected(double m, double v) {
    if (!(m > 0.0)) fail(LCTY_ERR_INVALID_DATA, "Cannot estimate N.Binom. parameters from mean %.3f and variance %.3f", m, v);
    const double PMAX = 0.99999, p = m / v;
    if (p > PMAX) return math::NBinom(PMAX * m / (1.0 - PMAX), PMAX);
    return math::NBinom(m * m / (v - m), p);
}

struct Triple { uint32_t k, n; double w; };

// BetaBinomial::max_lik_estimate (betabinom.rs:105-160)
Vec2 betabinom_mle(const std::vector<Triple>& obs, double unif_coef) {
    const double bb_mult = std::log1p(-unif_coef), unif_mult = std::log(unif_coef);
    auto cost = [&](const Vec2& x) {
        const double alpha = x[0], beta = x[1];
        if (alpha <= 0.0 || beta <= 0.0 || alpha >= 100000.0 || beta >= 100000.0) return 1e30;
        const double lb = math::ln_beta(alpha, beta);
        double s = 0.0;
        for (const Triple& t : obs) {
            const double k = t.k, n = t.n;
            const double lp = -math::ln_beta(n - k + 1.0, k + 1.0) + math::ln_beta(k + alpha, n - k + beta) - std::log(n + 1.0) - lb;
            s += t.w * math::ln_add(bb_mult + lp, unif_mult);
        }
        return -s;
    };
    return nelder_mead(cost, {Vec2{0.7, 50.0}, Vec2{0.3, 100.0}, Vec2{0.5, 10.0}}, 1e-6);
}

// BetaBinomial::inv_cdf (betabinom.rs:55-70)
uint32_t betabinom_inv_cdf(double alpha, double beta, uint32_t n, double cdf) {
    const double m = n;
    const double const_term = -std::log(m + 1.0) - math::ln_beta(alpha, beta);
    double ln_cdf = -math::ln_beta(m + 1.0, 1.0) + math::ln_beta(alpha, m + beta) + const_term;
    for (uint32_t i = 0; i < n; i++) {
        const double k = i + 1.0;
        ln_cdf = math::ln_add(ln_cdf, -math::ln_beta(m - k + 1.0, k + 1.0) + math::ln_beta(k + alpha, m - k + beta) + const_term);
        if (std::exp(ln_cdf) > cdf) return i;
    }
    return n;
}

// loess (algo/loess.rs:79-160), degree 1: x sorted ascending. The weighted least squares (weights w * tricube, as the rows of the
// reference's design matrix) are solved in closed form around xval; the reference solves them by SVD.
std::vector<double> loess(const std::vector<double>& x, const std::vector<double>& y, const std::vector<double>* w, double frac) {
    const size_t n = x.size();
    if (n == 0) fail(LCTY_ERR_RUNTIME, "Cannot calculate LOESS on an empty vector");
    const size_t n_frac = std::max<size_t>(1, static_cast<size_t>(std::round(static_cast<double>(n) * frac)));
    const double range = x[n - 1] - x[0];
    if (!(range > 0.0)) fail(LCTY_ERR_RUNTIME, "Cannot calculate LOESS: x contains a single value %g", x[0]);
    std::vector<double> out(LCTY_GC_BINS);
    for (int g = 0; g < LCTY_GC_BINS; g++) {
        const double xv = g;
        size_t a = std::lower_bound(x.begin(), x.end(), xv) - x.begin();
        size_t b = std::upper_bound(x.begin() + a, x.end(), xv) - x.begin();
        const size_t cur = b - a;
        if (cur >= n_frac) {
            double s = 0.0;
            for (size_t i = a; i < b; i++) s += y[i];
            out[g] = s / static_cast<double>(cur);
            continue;
        }
        const size_t rem = n_frac - cur;
        size_t left, right;
        if (a < n - b) { left = std::min(a, rem / 2); right = std::min(n - b, rem - left); }
        else { right = std::min(n - b, rem / 2); left = std::min(a, rem - right); }
        a -= left; b += right;
        double s0 = 0, s1 = 0, s2 = 0, t0 = 0, t1 = 0;
        for (size_t i = a; i < b; i++) {
            const double v = std::fabs((x[i] - xv) / range);
            const double u = 1.0 - std::pow(std::min(v, 1.0), 3);
            double wt = 70.0 / 81.0 * u * u * u;
            if (w) wt *= (*w)[i];
            const double ww = wt * wt, dx = x[i] - xv;
            s0 += ww; s1 += ww * dx; s2 += ww * dx * dx; t0 += ww * y[i]; t1 += ww * dx * y[i];
        }
        const double det = s0 * s2 - s1 * s1;
        out[g] = det != 0.0 ? (s2 * t0 - s1 * t1) / det : t0 / s0;
    }
    return out;
}

double interpol_quantile_sorted(const std::vector<double>& a, double q) {          // ext/vec.rs:140-156
    const double f = static_cast<double>(a.size() - 1) * q;
    const size_t i = static_cast<size_t>(f);
    const double r = f - std::floor(f);
    return r < 1e-6 ? a[i] : a[i] + (a[i + 1] - a[i]) * r;
}

void mean_variance(const double* a, size_t n, double* mean, double* var) {          // F64Ext::mean_variance (ext/vec.rs:74-99)
    double s = 0.0;
    for (size_t i = 0; i < n; i++) s += a[i];
    const double m = s / static_cast<double>(n);
    double acc = 0.0;
    for (size_t i = 0; i < n; i++) { const double d = a[i] - m; acc += d * d; }
    *mean = m; *var = acc / static_cast<double>(n - 1);
}

struct Layout { uint32_t window, neighb, n_windows, first_start; };

Layout window_layout(const lcty_bg_reads_view& v, uint32_t region_start, uint32_t region_end, const lcty_bg_params& prm) {
    Layout L;
    const uint32_t len = region_end - region_start;
    L.window = prm.window_size ? prm.window_size
                               : std::clamp(static_cast<uint32_t>(std::round(v.read_len * (2.0 / 3.0))), 20u, 5000u);
    L.neighb = std::max(L.window, 300u);
    if (static_cast<uint64_t>(len) < static_cast<uint64_t>(L.window) + 2ull * prm.boundary_size)
        fail(LCTY_ERR_INVALID_INPUT, "Input interval is too short (%u bp for %u bp windows and %u bp boundaries)", len, L.window, prm.boundary_size);
    L.n_windows = (len - 2 * prm.boundary_size) / L.window;
    L.first_start = (len - L.n_windows * L.window) / 2;                // relative to the region start
    return L;
}

// events around the kernels of one call when the caller asks for the diagnostics (nothing is recorded otherwise)
struct Events {
    bool on;
    hipEvent_t ev[8] = {};
    explicit Events(bool on_) : on(on_) { if (on) for (auto& e : ev) LCTY_HIP(hipEventCreate(&e)); }
    ~Events() { if (on) for (auto& e : ev) (void)hipEventDestroy(e); }
    void rec(int i, hipStream_t s) { if (on) LCTY_HIP(hipEventRecord(ev[i], s)); }
    double ms(int a, int b) const { float t = 0.f; if (on) LCTY_HIP(hipEventElapsedTime(&t, ev[a], ev[b])); return t; }
};

template <typename T> void put(T* dst, const std::vector<T>& src) { if (dst && !src.empty()) memcpy(dst, src.data(), src.size() * sizeof(T)); }
template <typename T> T* dev_copy(DevBuf<T>& d, const T* h, size_t n, hipStream_t s) { d.alloc(std::max<size_t>(n, 1)); d.upload(h, n, s); return d.p; }

}  // namespace

extern "C" {

int32_t lcty_bg_diag_sizes(const lcty_bg_reads* reads, uint32_t region_start, uint32_t region_end, const lcty_bg_params* params,
                           uint64_t* n_windows, uint64_t* n_records, uint64_t* n_pairs) {
    return guarded([&] {
        if (!reads || !params || region_end <= region_start) fail(LCTY_ERR_INVALID_INPUT, "null argument or empty region");
        lcty_bg_reads_view v;
        if (lcty_bg_reads_view_get(reads, &v) != LCTY_OK) fail(LCTY_ERR_INVALID_INPUT, "bad reads handle");
        const Layout L = window_layout(v, region_start, region_end, *params);
        uint64_t np = 0;
        for (uint64_t r = 0; r < v.n_records; r++) np += v.mate[r] != NONE && !(v.flags[r] & LCTY_BG_SECOND);
        if (n_windows) *n_windows = L.n_windows;
        if (n_records) *n_records = v.n_records;
        if (n_pairs) *n_pairs = np;
    });
}

int32_t lcty_bg_estimate(lcty_ctx* ctx, const lcty_bg_reads* reads, const uint8_t* padded_seq, uint32_t padded_start, uint32_t padded_len,
                         const uint16_t* kmer_counts, uint32_t k, uint32_t region_start, uint32_t region_end, const lcty_bg_params* params,
                         lcty_bg* out, double* read_len, lcty_bg_diag* diag) {
    return guarded([&] {
        if (!ctx || !reads || !padded_seq || !kmer_counts || !params || !out) fail(LCTY_ERR_INVALID_INPUT, "null argument");
        const lcty_bg_params& prm = *params;
        if (prm.technology < 0 || prm.technology > 3) fail(LCTY_ERR_INVALID_INPUT, "unknown technology %d", prm.technology);
        if (prm.ploidy == 0) fail(LCTY_ERR_INVALID_INPUT, "Ploidy cannot be zero");
        if (!(prm.subsampling_rate > 0.0 && prm.subsampling_rate <= 1.0)) fail(LCTY_ERR_INVALID_INPUT, "Subsampling rate (%g) must be within (0, 1]", prm.subsampling_rate);
        if (!(prm.uniq_kmer_perc > 1.0 && prm.uniq_kmer_perc <= 100.0)) fail(LCTY_ERR_INVALID_INPUT, "Unique k-mer percentile (%g) must be within (1, 100]", prm.uniq_kmer_perc);
        if (!(prm.frac_windows > 0.0 && prm.frac_windows <= 1.0)) fail(LCTY_ERR_INVALID_INPUT, "Fraction of windows (%g) must be within (0, 1]", prm.frac_windows);
        if (region_start >= region_end || region_start < padded_start || static_cast<uint64_t>(region_end) > static_cast<uint64_t>(padded_start) + padded_len)
            fail(LCTY_ERR_INVALID_INPUT, "background interval [%u, %u) is not inside the padded sequence", region_start, region_end);
        if (k == 0 || k > 64 || padded_len < k) fail(LCTY_ERR_INVALID_INPUT, "k-mer size %u does not fit the padded sequence", k);
        for (uint32_t i = 0; i < padded_len; i++) {
            const uint8_t c = padded_seq[i];
            if (base_enc(c) > 3u) fail(LCTY_ERR_INVALID_INPUT, "Cannot count k-mers for sequence with Ns (position %u)", padded_start + i);
        }
        lcty_bg_reads_view v;
        if (lcty_bg_reads_view_get(reads, &v) != LCTY_OK) fail(LCTY_ERR_INVALID_INPUT, "bad reads handle");
        // SequencingInfo::new (bg/mod.rs:304-322)
        static const double len_lo[4] = {100.0, 5000.0, 5000.0, 5000.0}, len_hi[4] = {400.0, 30000.0, 150000.0, 500000.0};
        if ((v.read_len < len_lo[prm.technology] || v.read_len > len_hi[prm.technology]) && !prm.explicit_technology)
            fail(LCTY_ERR_INVALID_INPUT, "Unusual mean read length (%.0f) for the sequencing technology. Please specify technology explicitly",
                 v.read_len);
        const Layout L = window_layout(v, region_start, region_end, prm);
        if (!(L.neighb > k)) fail(LCTY_ERR_INVALID_INPUT, "window neighbourhood %u must exceed k = %u", L.neighb, k);
        const uint32_t n = static_cast<uint32_t>(v.n_records);
        const bool paired = v.paired != 0;
        hipStream_t s = ctx->stream;
        LCTY_HIP(hipSetDevice(ctx->device));
        const double t_call = now_ms();
        Events E(diag != nullptr);

        // ---- device: windows, per-record counts, pairs --------------------------------------------------------------------------
        const uint32_t region_len = region_end - region_start, off = region_start - padded_start;
        const uint32_t n_counts = region_len + 1 - k;                   // KmerCounts::subregion (seq/counts.rs:234-246)
        std::vector<uint32_t> ref2(padded_len / 16 + 2, 0);
        for (uint32_t i = 0; i < padded_len; i++) {
            const uint8_t c = padded_seq[i];
            ref2[i >> 4] |= base_enc(c) << (2 * (i & 15));                  // ACGT only: checked above
        }
        DevBuf<uint8_t> d_seq; DevBuf<uint16_t> d_cnt; DevBuf<uint32_t> d_gc, d_low, d_span, d_ref2;
        dev_copy(d_seq, padded_seq + off, region_len, s);
        dev_copy(d_cnt, kmer_counts + off, n_counts, s);
        d_gc.alloc(L.n_windows); d_low.alloc(L.n_windows); d_span.alloc(2ull * L.n_windows);
        const uint32_t left_pad = (L.neighb - L.window) / 2, right_pad = L.neighb - L.window - left_pad;
        E.rec(0, s);
        hipLaunchKernelGGL(windows_kernel, dim3(L.n_windows), dim3(64), 0, s, d_seq.p, region_len, d_cnt.p, L.first_start, L.window,
                           left_pad, right_pad, k, L.n_windows, d_gc.p, d_low.p, d_span.p);
        LCTY_HIP(hipGetLastError());
        E.rec(1, s);

        const uint64_t n_cig = v.cigar_off[n], n_bases = v.seq_off[n];
        DevBuf<uint32_t> d_pos, d_end, d_cig, d_b2, d_nm, d_list, d_rc, d_edit, d_rl, d_mid, d_win; DevBuf<uint64_t> d_coff, d_soff; DevBuf<uint8_t> d_flags;
        RecArgs A{};
        // a handle of lcty_bg_reads_fetch on this context holds the eight arrays on the device already, equal to the view's word for word
        const bool resident = reads->ctx == ctx;
        const uint8_t* rec_flags;
        if (resident) {
            A.pos = reads->d_pos.p; A.end = reads->d_end.p; A.cigar_off = reads->d_cigar_off.p; A.cigar = reads->d_cigar.p;
            A.seq_off = reads->d_seq_off.p; A.bases2 = reads->d_bases2.p; A.nmask = reads->d_nmask.p; rec_flags = reads->d_flags.p;
        } else {
            A.pos = dev_copy(d_pos, v.pos, n, s); A.end = dev_copy(d_end, v.end, n, s);
            A.cigar_off = dev_copy(d_coff, v.cigar_off, n + 1ull, s); A.cigar = dev_copy(d_cig, v.cigar, n_cig, s);
            A.seq_off = dev_copy(d_soff, v.seq_off, n + 1ull, s);
            A.bases2 = dev_copy(d_b2, v.bases2, n_bases / 16 + 2, s); A.nmask = dev_copy(d_nm, v.nmask, n_bases / 32 + 1, s);
            rec_flags = dev_copy(d_flags, v.flags, n, s);
        }
        A.ref2 = dev_copy(d_ref2, ref2.data(), ref2.size(), s);
        A.padded_start = padded_start; A.region_start = region_start; A.region_end = region_end;
        A.win_start = region_start + L.first_start; A.win_end = A.win_start + L.n_windows * L.window; A.window = L.window;
        d_rc.alloc(5ull * n); d_edit.alloc(n); d_rl.alloc(n); d_mid.alloc(n); d_win.alloc(n);
        A.counts = d_rc.p; A.edit = d_edit.p; A.read_len = d_rl.p; A.middle = d_mid.p; A.win = d_win.p;
        std::vector<uint32_t> list(n);
        uint32_t n_short = 0;
        for (uint32_t r = 0; r < n; r++) if (v.qlen[r] < LONG_RECORD) list[n_short++] = r;
        uint32_t nl = n_short;
        for (uint32_t r = 0; r < n; r++) if (v.qlen[r] >= LONG_RECORD) list[nl++] = r;
        dev_copy(d_list, list.data(), n, s);
        E.rec(2, s);
        if (n_short) {
            RecArgs S = A; S.list = d_list.p; S.n_list = n_short;
            hipLaunchKernelGGL(counts_short_kernel, dim3((n_short + 255) / 256), dim3(256), 0, s, S);
            LCTY_HIP(hipGetLastError());
        }
        if (n > n_short) {
            RecArgs Lg = A; Lg.list = d_list.p + n_short; Lg.n_list = n - n_short;
            hipLaunchKernelGGL(counts_long_kernel, dim3(n - n_short), dim3(64), 0, s, Lg);
            LCTY_HIP(hipGetLastError());
        }
        E.rec(3, s);
        std::vector<uint32_t> pf, ps;                                 // full pairs in order of their first end
        if (paired)
            for (uint32_t r = 0; r < n; r++) if (v.mate[r] != NONE && !(v.flags[r] & LCTY_BG_SECOND)) { pf.push_back(r); ps.push_back(v.mate[r]); }
        const uint32_t np = static_cast<uint32_t>(pf.size());
        DevBuf<uint32_t> d_pf, d_ps, d_ins; DevBuf<uint8_t> d_same;
        std::vector<uint32_t> ins(np); std::vector<uint8_t> same(np);
        if (np) {
            dev_copy(d_pf, pf.data(), np, s); dev_copy(d_ps, ps.data(), np, s);
            d_ins.alloc(np); d_same.alloc(np);
            E.rec(4, s);
            hipLaunchKernelGGL(pairs_kernel, dim3((np + 255) / 256), dim3(256), 0, s, A.pos, A.end, rec_flags, d_pf.p, d_ps.p, np, d_ins.p, d_same.p);
            LCTY_HIP(hipGetLastError());
            E.rec(5, s);
            d_ins.download(ins.data(), np, s); d_same.download(same.data(), np, s);
        }
        std::vector<uint32_t> gcc(L.n_windows), low(L.n_windows), span(2ull * L.n_windows);
        std::vector<uint32_t> rc(5ull * n), edit(n), rlen(n), mid(n), win(n);
        d_gc.download(gcc.data(), L.n_windows, s); d_low.download(low.data(), L.n_windows, s); d_span.download(span.data(), 2ull * L.n_windows, s);
        d_rc.download(rc.data(), 5ull * n, s); d_edit.download(edit.data(), n, s); d_rl.download(rlen.data(), n, s);
        d_mid.download(mid.data(), n, s); d_win.download(win.data(), n, s);
        LCTY_HIP(hipStreamSynchronize(s));
        const double t_fit0 = now_ms();
        double dev_wait_ms = 0.0;

        // ---- window table (filter_windows) --------------------------------------------------------------------------------------
        std::vector<double> wgc(L.n_windows), wfrac(L.n_windows);
        std::vector<uint8_t> keep(L.n_windows);
        const double uniq_frac = 0.01 * prm.uniq_kmer_perc;
        uint32_t selected = 0;
        for (uint32_t w = 0; w < L.n_windows; w++) {
            wgc[w] = 100.0 * static_cast<double>(gcc[w]) / static_cast<double>(span[2 * w]);
            wfrac[w] = static_cast<double>(low[w]) / static_cast<double>(span[2 * w + 1]);
            keep[w] = wfrac[w] >= uniq_frac;
            selected += keep[w];
        }
        if (selected == 0) fail(LCTY_ERR_RUNTIME, "Retained 0 windows after filtering");
        uint64_t n_stage[6] = {n, np, 0, 0, 0, 0};

        // ---- insert sizes (InsertDistr::estimate) -------------------------------------------------------------------------------
        std::map<uint32_t, uint32_t> hist;
        uint64_t orient[2] = {0, 0};
        double ins_limit = NAN, ins_mean = NAN, ins_var = NAN;
        uint32_t ci_lo = 0, ci_hi = 0;
        std::vector<uint32_t> ep;                                      // error-profile records (pairs: first, second, ...)
        if (paired) {
            if (np == 0) fail(LCTY_ERR_INVALID_DATA, "BAM records are supposed to be paired!");
            if (np < 1000) fail(LCTY_ERR_INVALID_DATA, "Not enough paired reads (%u) to calculate insert size distribution", np);
            std::vector<double> sizes;
            sizes.reserve(np);
            for (uint32_t t = 0; t < np; t++) {
                if (ins[t] >= 500000u) continue;
                sizes.push_back(ins[t]);
                hist[ins[t]]++;
                orient[same[t]]++;
            }
            n_stage[2] = sizes.size();
            if (sizes.empty()) fail(LCTY_ERR_INVALID_DATA, "No read pairs with insert size under 500 kb");
            const double total = static_cast<double>(orient[0] + orient[1]);
            if (static_cast<double>(orient[0]) / total < 0.05 || static_cast<double>(orient[1]) / total >= 0.05)
                fail(LCTY_ERR_INVALID_DATA, "FF orientation is not supported by Locityper");
            std::sort(sizes.begin(), sizes.end());
            ins_limit = 3.0 * interpol_quantile_sorted(sizes, 0.99);
            const size_t m = std::upper_bound(sizes.begin(), sizes.end(), ins_limit) - sizes.begin();
            mean_variance(sizes.data(), m, &ins_mean, &ins_var);
            const math::NBinom nb = nbinom_corrected(ins_mean, ins_var);
            out->ins_n = nb.n; out->ins_p = nb.p;
            const double q = 0.5 * prm.insert_pval;                  // confidence_interval(1 - insert_pval)
            ci_lo = static_cast<uint32_t>(std::max(0.0, std::floor(nb.quantile(q) - 1e-8)));
            ci_hi = static_cast<uint32_t>(std::ceil(nb.quantile(1.0 - q) + 1e-8));
            for (uint32_t t = 0; t < np; t++)
                if (ci_lo <= ins[t] && ins[t] <= ci_hi) { ep.push_back(pf[t]); ep.push_back(ps[t]); }
        } else {
            ep.resize(n);
            std::iota(ep.begin(), ep.end(), 0u);
        }
        n_stage[3] = ep.size();

        // ---- error profile (ErrorProfile::estimate) -----------------------------------------------------------------------------
        uint64_t tot[5] = {0, 0, 0, 0, 0};
        std::map<std::pair<uint32_t, uint32_t>, uint64_t> edits;
        for (const uint32_t r : ep) {
            if (win[r] == NONE || !keep[win[r]]) continue;
            n_stage[4]++;
            for (int o = 0; o < 5; o++) tot[o] += rc[5ull * r + o];
            edits[{edit[r], rlen[r]}]++;
        }
        {
            const double sum_len = static_cast<double>(tot[0] + tot[1] + tot[2] + tot[3]);
            const double mism = std::max(static_cast<double>(tot[1]) / sum_len, 1e-5), insp = std::max(static_cast<double>(tot[2]) / sum_len, 1e-5);
            const double delp = std::max(static_cast<double>(tot[3]) / sum_len, 1e-5);
            const double matchp = 1.0 - mism - insp - delp;
            if (!(matchp > 0.5)) fail(LCTY_ERR_INVALID_DATA, "Match probability (%.5f) must be over 50%%", matchp);
            out->op_lnprobs[0] = std::log(matchp); out->op_lnprobs[1] = std::log(mism); out->op_lnprobs[2] = std::log(insp);
            out->op_lnprobs[3] = std::log(delp); out->op_lnprobs[4] = std::log(std::max(insp, mism));
        }
        std::vector<Triple> triples;
        for (const auto& kv : edits) triples.push_back({std::min(kv.first.first, kv.first.second), kv.first.second, static_cast<double>(kv.second)});
        const double unif_coef = std::min(3.0 / static_cast<double>(ep.size()), 0.1);
        const Vec2 ab = betabinom_mle(triples, unif_coef);
        out->edit_alpha = ab[0]; out->edit_beta = ab[1];

        // ---- edit filter (SingleEditDistCache) and read depth (ReadDepth::estimate) --------------------------------------------
        std::map<uint32_t, uint32_t> thr;
        auto passes = [&](uint32_t r) {
            auto it = thr.find(rlen[r]);
            if (it == thr.end()) it = thr.emplace(rlen[r], betabinom_inv_cdf(ab[0], ab[1], rlen[r], 1.0 - prm.edit_pval)).first;
            return edit[r] <= it->second;
        };
        std::vector<uint32_t> dl;
        if (paired) { for (size_t t = 0; t + 1 < ep.size(); t += 2) if (passes(ep[t]) && passes(ep[t + 1])) { dl.push_back(ep[t]); dl.push_back(ep[t + 1]); } }
        else for (const uint32_t r : ep) if (passes(r)) dl.push_back(r);
        n_stage[5] = dl.size();
        std::vector<uint32_t> depth(2ull * L.n_windows, 0);
        DevBuf<uint32_t> d_dl, d_depth;
        d_depth.alloc(2ull * L.n_windows); d_depth.zero(s);
        const double t_dev0 = now_ms();
        if (!dl.empty()) {
            dev_copy(d_dl, dl.data(), dl.size(), s);
            E.rec(6, s);
            hipLaunchKernelGGL(depth_kernel, dim3((static_cast<uint32_t>(dl.size()) + 255) / 256), dim3(256), 0, s, d_dl.p,
                               static_cast<uint32_t>(dl.size()), d_win.p, rec_flags, d_depth.p);
            LCTY_HIP(hipGetLastError());
            E.rec(7, s);
        }
        d_depth.download(depth.data(), 2ull * L.n_windows, s);
        LCTY_HIP(hipStreamSynchronize(s));
        dev_wait_ms += now_ms() - t_dev0;

        std::vector<uint32_t> kept;
        for (uint32_t w = 0; w < L.n_windows; w++) if (keep[w]) kept.push_back(w);
        std::stable_sort(kept.begin(), kept.end(), [&](uint32_t p, uint32_t q) { return wgc[p] < wgc[q]; });
        std::vector<double> xs(kept.size()), ys(kept.size());
        for (size_t i = 0; i < kept.size(); i++) { xs[i] = wgc[kept[i]]; ys[i] = depth[2ull * kept[i]]; }
        std::array<std::pair<size_t, size_t>, LCTY_GC_BINS> bins;        // find_gc_bins (depth.rs:47-59)
        {
            size_t i = 0;
            for (int g = 0; g < LCTY_GC_BINS; g++) {
                const size_t j = std::upper_bound(xs.begin() + i, xs.end(), g + 0.5) - xs.begin();
                bins[g] = {i, j}; i = j;
            }
        }
        std::vector<double> lm(LCTY_GC_BINS, NAN), lv(LCTY_GC_BINS, NAN), bm(LCTY_GC_BINS, NAN), bv(LCTY_GC_BINS, NAN);
        double dmean = NAN, dvar = NAN;
        const double ploidy = prm.ploidy;
        if (prm.technology == LCTY_TECH_ILLUMINA) {                     // has_gc_bias (bg/mod.rs:226-228)
            lm = loess(xs, ys, nullptr, prm.frac_windows);               // predict_mean_var (depth.rs:69-91)
            std::vector<double> vx, vy, vw;
            for (int g = 0; g < LCTY_GC_BINS; g++) {
                const size_t i = bins[g].first, j = bins[g].second;
                if (j - i < 10) continue;
                double m, var;
                mean_variance(ys.data() + i, j - i, &m, &var);
                vx.push_back(g); vy.push_back(var); vw.push_back(std::sqrt(static_cast<double>(j - i) / static_cast<double>(xs.size())));
            }
            lv = loess(vx, vy, &vw, 1.0);
            // blur_boundary_values (depth.rs:98-126)
            const size_t nb = LCTY_GC_BINS, mtot = bins[nb - 1].second, min_obs = prm.min_tail_obs;
            size_t left_ix = nb, right_ix = 0;
            for (size_t g = 0; g < nb; g++) if (bins[g].second >= min_obs) { left_ix = g; break; }
            for (size_t p = 0; p < nb; p++) if (mtot - bins[nb - 1 - p].first >= min_obs) { right_ix = nb - p; break; }
            if (!(left_ix < right_ix)) fail(LCTY_ERR_RUNTIME, "Too few windows to calculate read depth!");
            bm = lm; bv = lv;
            for (size_t g = 0; g < left_ix; g++) {
                bm[g] = lm[left_ix];
                bv[g] = std::max((1.0 + static_cast<double>(left_ix - g) * prm.tail_var_mult) * lv[left_ix], lv[g]);
            }
            for (size_t g = right_ix + 1; g < nb; g++) {
                bm[g] = lm[right_ix];
                bv[g] = std::max((1.0 + static_cast<double>(g - right_ix) * prm.tail_var_mult) * lv[right_ix], lv[g]);
            }
            for (int g = 0; g < LCTY_GC_BINS; g++) {                     // estimate_nbinoms (depth.rs:260-273)
                const math::NBinom d = nbinom_regularized(bm[g], bv[g], prm.subsampling_rate, 1e-5).mul(1.0 / ploidy);
                out->depth_n[g] = d.n; out->depth_p[g] = d.p;
            }
        } else {
            if (xs.size() < 2) fail(LCTY_ERR_RUNTIME, "Too few windows to calculate read depth!");
            mean_variance(ys.data(), ys.size(), &dmean, &dvar);
            const math::NBinom d = nbinom_regularized(dmean, dvar, prm.subsampling_rate, 1e-5).mul(1.0 / ploidy);
            for (int g = 0; g < LCTY_GC_BINS; g++) { out->depth_n[g] = d.n; out->depth_p[g] = d.p; }
        }

        // ---- the lcty_bg (as lcty_bg_from_json would leave it) ------------------------------------------------------------------
        out->window = L.window; out->neighb = L.neighb;
        out->is_paired = paired ? 1 : 0; out->technology = prm.technology; out->_pad0 = 0;
        if (!paired) { out->ins_n = 0.0; out->ins_p = 0.0; }
        if (prm.technology == LCTY_TECH_ILLUMINA) { out->edit_kind = LCTY_EDIT_FRACTION; out->edit_p1 = 0.03; out->edit_p2 = 0.06; }
        else { out->edit_kind = LCTY_EDIT_PVALUE; out->edit_p1 = 0.99; out->edit_p2 = 0.999; }
        if (read_len) *read_len = v.read_len;

        if (diag) {
            lcty_bg_diag& D = *diag;
            if (D.n_windows < L.n_windows || D.n_records < n || D.n_pairs < np)
                fail(LCTY_ERR_INVALID_INPUT, "diag sized for %llu windows / %llu records / %llu pairs; lcty_bg_diag_sizes gives %u / %u / %u",
                     static_cast<unsigned long long>(D.n_windows), static_cast<unsigned long long>(D.n_records),
                     static_cast<unsigned long long>(D.n_pairs), L.n_windows, n, np);
            D.n_windows = L.n_windows; D.n_records = n; D.n_pairs = np;
            std::vector<uint32_t> ws(L.n_windows);
            for (uint32_t w = 0; w < L.n_windows; w++) ws[w] = A.win_start + w * L.window;
            put(D.win_start, ws); put(D.win_gc, wgc); put(D.win_kmer_frac, wfrac); put(D.win_keep, keep); put(D.win_depth, depth);
            put(D.rec_counts, rc); put(D.rec_edit, edit); put(D.rec_read_len, rlen); put(D.rec_middle, mid); put(D.rec_window, win);
            put(D.pair_first, pf); put(D.pair_second, ps); put(D.pair_insert, ins); put(D.pair_same_strand, same);
            D.n_hist = hist.size();
            size_t t = 0;
            for (const auto& kv : hist) { if (D.hist_size) D.hist_size[t] = kv.first; if (D.hist_count) D.hist_count[t] = kv.second; t++; }
            D.orient[0] = orient[0]; D.orient[1] = orient[1];
            D.ins_limit = ins_limit; D.ins_mean = ins_mean; D.ins_var = ins_var; D.ci_low = ci_lo; D.ci_high = ci_hi;
            for (int o = 0; o < 5; o++) D.op_totals[o] = tot[o];
            D.n_edit = edits.size();
            t = 0;
            for (const auto& kv : edits) {
                if (D.edit_edit) D.edit_edit[t] = kv.first.first;
                if (D.edit_len) D.edit_len[t] = kv.first.second;
                if (D.edit_count) D.edit_count[t] = kv.second;
                t++;
            }
            D.unif_coef = unif_coef;
            for (int st = 0; st < 6; st++) D.n_stage[st] = n_stage[st];
            for (int g = 0; g < LCTY_GC_BINS; g++) {
                D.gc_nwin[g] = static_cast<uint32_t>(bins[g].second - bins[g].first);
                D.loess_mean[g] = lm[g]; D.loess_var[g] = lv[g]; D.blur_mean[g] = bm[g]; D.blur_var[g] = bv[g];
                D.nb_n[g] = out->depth_n[g]; D.nb_p[g] = out->depth_p[g];
            }
            D.depth_mean = dmean; D.depth_var = dvar;
            D.kernel_ms[0] = E.ms(0, 1); D.kernel_ms[1] = E.ms(2, 3);
            D.kernel_ms[2] = np ? E.ms(4, 5) : 0.0; D.kernel_ms[3] = dl.empty() ? 0.0 : E.ms(6, 7);
            D.fit_ms = now_ms() - t_fit0 - dev_wait_ms; D.total_ms = now_ms() - t_call;
        }
    });
}

}  // extern "C"
