// Exact score distributions, host side: the limit checks both paths share, the host twin
// (device == -1: the definition of include/tfbs_amd.h, "Thresholds from a p-value", in
// unsigned __int128, threaded over strands) and the C ABI of both paths.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <thread>

#include "score_dist.hpp"

namespace tfbs {

typedef unsigned __int128 u128;

std::string strand_label(const Pat &p) {
    return "'" + p.name + "' (" + (p.direction == TFBS_DIR_N ? "-" : "+") + ")";
}

int dist_check_pvalue(double p) {
    if (!std::isfinite(p) || p < 0.0 || p >= 1.0) return fail(TFBS_E_ARG, "p-value outside [0, 1)");
    return TFBS_OK;
}

int dist_strand(const Patterns &P, size_t i, DistStrand *out) {
    if (i >= P.pats.size()) return fail(TFBS_E_ARG, "pattern index out of range");
    const Pat &p = P.pats[i];
    if (p.kind != TFBS_KIND_PWM && p.kind != TFBS_KIND_DIPWM)
        return fail(TFBS_E_ARG, "strand " + strand_label(p) + " is neither a PWM nor a dinucleotide PWM: no score distribution");
    DistStrand S;
    S.index = (uint32_t)i;
    S.L = p.len;
    if (p.len > kDistMaxLen)
        return fail(TFBS_E_ARG, "strand " + strand_label(p) + " has more than 63 bases: 4^L does not fit 128 bits");
    const bool di = p.kind == TFBS_KIND_DIPWM;
    S.width = di ? 16 : 4;
    S.steps = di ? (p.len ? p.len - 1 : 0) : p.len;
    const int32_t *w = di ? p.w16.data() : p.w5.data();
    const size_t stride = di ? 16 : 5;
    const uint64_t cap = di ? kDistMaxBinsDi : kDistMaxBinsMono;
    uint64_t mag = 0, bins = 1;
    int64_t base = 0;
    S.shift.resize((size_t)S.steps * S.width);
    S.span.resize(S.steps);
    for (uint32_t j = 0; j < S.steps; j++) {
        const int32_t *c = w + stride * j;
        int64_t lo = c[0], hi = c[0];
        for (uint32_t k = 1; k < S.width; k++) {
            lo = std::min<int64_t>(lo, c[k]);
            hi = std::max<int64_t>(hi, c[k]);
        }
        mag += (uint64_t)std::max(std::llabs(lo), std::llabs(hi));
        if (mag > (uint64_t)INT32_MAX)
            return fail(TFBS_E_ARG, "the scores of strand " + strand_label(p) + " can wrap int32");
        bins += (uint64_t)(hi - lo);
        if (bins > cap)
            return fail(TFBS_E_ARG, "the scores of strand " + strand_label(p) + " span more than " +
                                        std::to_string(cap) + " bins");
        base += lo;
        for (uint32_t k = 0; k < S.width; k++) S.shift[(size_t)j * S.width + k] = (uint32_t)(c[k] - lo);
        S.span[j] = (uint32_t)bins;
    }
    S.bins = bins;
    S.base = base;
    *out = std::move(S);
    return TFBS_OK;
}

int dist_strands(const Patterns &P, std::vector<DistStrand> *out) {
    out->clear();
    for (size_t i = 0; i < P.pats.size(); i++) {
        if (P.pats[i].kind == TFBS_KIND_OTHER) continue;
        DistStrand S;
        if (int rc = dist_strand(P, i, &S)) return rc;
        out->push_back(std::move(S));
    }
    return TFBS_OK;
}

// ---------------------------------------------------------------------------
// Host twin
// ---------------------------------------------------------------------------
namespace {

// cnt over the final bins: a gather per step, reads outside the previous span count 0.
std::vector<u128> host_counts(const DistStrand &S) {
    const size_t n = (size_t)S.bins;
    if (!S.di()) {
        std::vector<u128> a(n, 0), b(n, 0);
        a[0] = 1;
        size_t prev = 1;
        for (uint32_t j = 0; j < S.steps; j++) {
            const uint32_t *sh = &S.shift[4 * (size_t)j];
            const size_t cur = S.span[j];
            for (size_t s = 0; s < cur; s++) {
                u128 v = 0;
                for (int k = 0; k < 4; k++)
                    if (s >= sh[k] && s - sh[k] < prev) v += a[s - sh[k]];
                b[s] = v;
            }
            a.swap(b);
            prev = cur;
        }
        a.resize(prev);
        return a;
    }
    std::vector<u128> a(4 * n, 0), b(4 * n, 0);
    for (int t = 0; t < 4; t++) a[t * n] = 1;
    size_t prev = 1;
    for (uint32_t j = 0; j < S.steps; j++) {
        const uint32_t *sh = &S.shift[16 * (size_t)j];
        const size_t cur = S.span[j];
        for (int t = 0; t < 4; t++)  // the new last base
            for (size_t s = 0; s < cur; s++) {
                u128 v = 0;
                for (int f = 0; f < 4; f++) {  // the old one
                    const uint32_t d = sh[4 * f + t];
                    if (s >= d && s - d < prev) v += a[f * n + s - d];
                }
                b[t * n + s] = v;
            }
        a.swap(b);
        prev = cur;
    }
    std::vector<u128> c(prev);
    for (size_t s = 0; s < prev; s++) c[s] = a[s] + a[n + s] + a[2 * n + s] + a[3 * n + s];
    return c;
}

std::vector<u128> host_tails(const DistStrand &S) {
    std::vector<u128> t = host_counts(S);
    u128 run = 0;
    for (size_t s = t.size(); s-- > 0;) {
        run += t[s];
        t[s] = run;
    }
    return t;
}

// floor(p * 4^L) for 0 <= p < 1: the mantissa shifted inside 128 bits.
u128 host_x(double p, uint32_t L) {
    if (p == 0.0) return 0;
    int e;
    const double f = std::frexp(p, &e);  // p = f 2^e, 0.5 <= f < 1
    const u128 m = (u128)(uint64_t)std::ldexp(f, 53);
    const int sh = e - 53 + 2 * (int)L;
    if (sh >= 0) return m << sh;  // (p < 1: below 4^L <= 2^126)
    return -sh >= 64 ? (u128)0 : m >> -sh;
}

int32_t host_threshold(const DistStrand &S, double p) {
    const std::vector<u128> t = host_tails(S);
    const u128 x = host_x(p, S.L);
    size_t b = t.size() - 1;
    while (b > 0 && !(t[b] > x)) b--;  // (t[0] = 4^L > x)
    return (int32_t)(S.base + (int64_t)b);
}

uint32_t host_threads() {
    const char *env = getenv("TFBS_HOST_THREADS");
    uint32_t n = env && *env ? (uint32_t)std::max(1, atoi(env)) : std::max(1u, std::thread::hardware_concurrency());
    return std::min(16u, n);
}

}  // namespace

static int host_score_tails(const DistStrand &S, const int32_t *scores, size_t n, uint64_t *lo, uint64_t *hi) {
    const std::vector<u128> t = host_tails(S);
    for (size_t k = 0; k < n; k++) {
        const int64_t b = (int64_t)scores[k] - S.base;
        const u128 v = b <= 0 ? t[0] : b >= (int64_t)t.size() ? (u128)0 : t[(size_t)b];
        lo[k] = (uint64_t)v;
        hi[k] = (uint64_t)(v >> 64);
    }
    return TFBS_OK;
}

static int host_pvalue_thresholds(const std::vector<DistStrand> &S, double p, int32_t *out) {
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t k; (k = next.fetch_add(1)) < S.size();) out[S[k].index] = host_threshold(S[k], p);
    };
    const uint32_t nt = (uint32_t)std::min<size_t>(host_threads(), S.size());
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    return TFBS_OK;
}

int score_tails(const Patterns &P, int device, size_t i, const int32_t *scores, size_t n, uint64_t *lo, uint64_t *hi) {
    if (device < -1) return fail(TFBS_E_ARG, "device is -1 (the host) or a HIP device");
    DistStrand S;
    if (int rc = dist_strand(P, i, &S)) return rc;
    if (!n) return TFBS_OK;
    return device < 0 ? host_score_tails(S, scores, n, lo, hi) : dev_score_tails(S, device, scores, n, lo, hi);
}

int pvalue_thresholds(const Patterns &P, int device, double p, int32_t *min_scores) {
    if (device < -1) return fail(TFBS_E_ARG, "device is -1 (the host) or a HIP device");
    if (int rc = dist_check_pvalue(p)) return rc;
    std::vector<DistStrand> S;
    if (int rc = dist_strands(P, &S)) return rc;
    for (size_t i = 0; i < P.pats.size(); i++) min_scores[i] = P.pats[i].min_score;  // (an OTHER strand keeps its own)
    if (S.empty()) return TFBS_OK;
    return device < 0 ? host_pvalue_thresholds(S, p, min_scores) : dev_pvalue_thresholds(S, device, p, min_scores);
}

}  // namespace tfbs

extern "C" {

int tfbs_patterns_score_tails(const tfbs_patterns *p, int device, size_t i, const int32_t *scores, size_t n,
                              uint64_t *tail_lo, uint64_t *tail_hi) {
    if (!p || (n && (!scores || !tail_lo || !tail_hi))) return tfbs::fail(TFBS_E_ARG, "null argument");
    return tfbs::score_tails(tfbs::patterns_of(p), device, i, scores, n, tail_lo, tail_hi);
}

int tfbs_patterns_pvalue_thresholds(const tfbs_patterns *p, int device, double pvalue, int32_t *min_scores) {
    if (!p || (!min_scores && !tfbs::patterns_of(p).pats.empty())) return tfbs::fail(TFBS_E_ARG, "null argument");
    return tfbs::pvalue_thresholds(tfbs::patterns_of(p), device, pvalue, min_scores);
}

void tfbs_pvalue_tile_widths(uint32_t out[2]) {
    out[0] = tfbs::kDistStepTile;
    out[1] = tfbs::kDistScanTile;
}

}  // extern "C"
