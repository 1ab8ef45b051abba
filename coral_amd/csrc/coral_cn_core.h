// coral_cn_core.h - the copy-number segmenter's rule, written once: small inline functions that the host backend
// (coral_cn_host.h, coral_cn.cpp) and the kernels (coral_cngpu.hip) both call, so that `cnv` gives the same rows on either.
// A deterministic Haar-wavelet segmenter after HaarSeg (Ben-Yaacov & Eldar 2008); DESIGN.md §4 states the rule in words.
//
// Everything up to the FDR cut is integer arithmetic:
//   - a bin is a candidate when it has the full bin size and bases > 0 (and, with a reference table, reference bases > 0);
//   - the centre C is the lower median of bases over the candidate bins of the centring contigs; a candidate is kept when
//     bases * 32 >= C (log2 ratio >= -5), with a reference the same against the reference's own centre;
//   - the signal of a kept bin is s = L(bases) - L(C) [- (L(ref) - L(C_ref))], L = log2 in Q16 by repeated squaring (log2_q16);
//   - per contig, over its n kept bins x[0..n) with mirror padding, the Haar detail of half-size h at k = 1..n-1 is
//     sum x[k..k+h-1] - sum x[k-h..k-1], taken from the contig's prefix sums (haar_detail); c[0] = c[n] = 0; peaks by peak_mag.
//   - with the reference's composition per bin (gc, at) a candidate also needs enough called bases, and the lower median of s over
//     the centring contigs' kept bins of its GC stratum (pooled with the nearest strata up to gc_min_bins) is subtracted from
//     every kept bin's s in front of the details (called_enough, gc_stratum, gc_pool below);
// The cut (fdr_cut) is the one floating-point step: a host function, called by both backends on the sorted magnitudes.
// No HIP in this header beyond the host / device markers.
#ifndef CORAL_CN_CORE_H
#define CORAL_CN_CORE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CORAL_CN_HD __host__ __device__ inline
#else
#define CORAL_CN_HD inline
#endif

namespace coral_cn {

constexpr int MAX_LEVELS = 20;
constexpr int64_t NO_CUT = INT64_MAX;          // fdr_cut: no peak of the level passes
constexpr int64_t MAX_BINS = (int64_t)1 << 28;

// hi:lo = a * b
CORAL_CN_HD uint64_t mul_hi_lo(uint64_t a, uint64_t b, uint64_t &lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    return __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    return (uint64_t)(p >> 64);
#endif
}

// L(x), x >= 1: log2 in Q16.  e = the top bit; the mantissa m = x << (63 - e) in [2^63, 2^64) is squared 16 times, each
// squaring giving one bit (1 when the square reaches 2, and then it is halved).
CORAL_CN_HD int32_t log2_q16(uint64_t x) {
    const int e = 63 - __builtin_clzll(x);
    uint64_t m = x << (63 - e);
    uint32_t bits = 0;
    for (int i = 0; i < 16; ++i) {
        uint64_t lo;
        const uint64_t hi = mul_hi_lo(m, m, lo);
        if (hi >> 63) { bits = (bits << 1) | 1u; m = hi; }
        else { bits <<= 1; m = (hi << 1) | (lo >> 63); }
    }
    return (int32_t)(((uint32_t)e << 16) | bits);
}

// bin `b` of a contig (0-based within it) has the full size
CORAL_CN_HD bool full_bin(int64_t b, int64_t bin_size, int64_t length) { return (b + 1) * bin_size <= length; }
CORAL_CN_HD int64_t bin_end(int64_t b, int64_t bin_size, int64_t length) { const int64_t e = (b + 1) * bin_size; return e < length ? e : length; }

CORAL_CN_HD bool candidate(bool full, int64_t bases, bool has_ref, int64_t ref_bases) { return full && bases > 0 && (!has_ref || ref_bases > 0); }
// bases * 32 >= C without the product: bases >= ceil(C / 32).  C == 0 (no candidate in the centring contigs): nothing is kept.
CORAL_CN_HD bool above_floor(int64_t bases, int64_t C) { return C > 0 && bases >= (C + 31) / 32; }

// ---- with the reference's composition per bin (gc, at: G/C and A/T bases of the bin): the uncalled-base mask and the GC bias -----
//   - a candidate must also have acgt = gc + at > 0 and acgt * 1000 >= bin_size * min_called_permille;
//   - a kept bin's stratum is g = gc * G / acgt in 0..G (G = gc_strata);
//   - over P, the kept bins of the centring contigs: for each g the smallest w >= 0 whose strata [max(0, g - w), min(G, g + w)]
//     hold at least min(gc_min_bins, |P|) bins of P (gc_pool); bias[g] = the lower median of s over those bins;
//   - s' = s - bias[g] for every kept bin of every contig; detail, noise, cut, unify and rows run on s'.
constexpr int32_t MAX_GC_STRATA = 1000;

CORAL_CN_HD bool gc_params_ok(int32_t strata, int64_t min_bins, int32_t min_called_permille) {
    return strata >= 1 && strata <= MAX_GC_STRATA && min_bins >= 1 && min_called_permille >= 0 && min_called_permille <= 1000;
}
CORAL_CN_HD bool called_enough(uint32_t gc, uint32_t at, int64_t bin_size, int32_t min_called_permille) {
    const int64_t acgt = (int64_t)gc + (int64_t)at;
    return acgt > 0 && acgt * 1000 >= bin_size * (int64_t)min_called_permille;
}
CORAL_CN_HD int32_t gc_stratum(uint32_t gc, uint32_t at, int32_t strata) { return (int32_t)((uint64_t)gc * (uint64_t)strata / ((uint64_t)gc + (uint64_t)at)); }
// start[g] = the bins of P in the strata below g, g = 0..G + 1.  The pool of stratum g: strata lo..hi.
CORAL_CN_HD void gc_pool(const int64_t *start, int32_t strata, int32_t g, int64_t need, int32_t &lo, int32_t &hi) {
    for (int32_t w = 0;; ++w) {
        lo = g - w < 0 ? 0 : g - w;
        hi = g + w > strata ? strata : g + w;
        if (start[hi + 1] - start[lo] >= need || (lo == 0 && hi == strata)) return;
    }
}
// the order-preserving 32-bit key of a signal, and back
CORAL_CN_HD uint32_t signal_key(int32_t s) { return (uint32_t)s ^ 0x80000000u; }
CORAL_CN_HD int32_t key_signal(uint32_t k) { return (int32_t)(k ^ 0x80000000u); }

// the contig of bin b: the last c with bin_off[c] <= b (empty contigs share an offset; the last of them holds the bin)
CORAL_CN_HD int32_t contig_of(const int64_t *bin_off, int32_t n_contigs, int64_t b) {
    int32_t lo = 0, hi = n_contigs;
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (bin_off[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// P: the contig's n + 1 prefix sums (P[i] = P[0] + x[0] + .. + x[i-1]).  E(j) = sum of the mirror-padded x over [0, j) - negative
// for j < 0 - for -n <= j <= 2n.
CORAL_CN_HD int64_t ext_prefix(const int64_t *P, int64_t n, int64_t j) {
    if (j < 0) return -(P[-j] - P[0]);
    if (j > n) return 2 * (P[n] - P[0]) - (P[2 * n - j] - P[0]);
    return P[j] - P[0];
}

// c_h[k]; 0 at k <= 0 and k >= n.  Needs h <= n.
CORAL_CN_HD int64_t haar_detail(const int64_t *P, int64_t n, int64_t k, int64_t h) {
    if (k <= 0 || k >= n) return 0;
    return ext_prefix(P, n, k + h) - 2 * ext_prefix(P, n, k) + ext_prefix(P, n, k - h);
}

// |c_h[k]| when k is a peak of its sign, else 0
CORAL_CN_HD int64_t peak_mag(const int64_t *P, int64_t n, int64_t k, int64_t h) {
    const int64_t c = haar_detail(P, n, k, h);
    if (c == 0) return 0;
    const int64_t a = haar_detail(P, n, k - 1, h), b = haar_detail(P, n, k + 1, h);
    if (c > 0) return (c > a && c >= b) ? c : 0;
    return (c < a && c <= b) ? -c : 0;
}

// the clamp of [a - r, a + r] to the contig's kept bins [first, last]: where another breakpoint blocks a
CORAL_CN_HD void unify_window(int64_t a, int64_t r, int64_t first, int64_t last, int64_t &lo, int64_t &hi) {
    lo = a - r < first ? first : a - r;
    hi = a + r > last ? last : a + r;
}

// ---- the host's part: the noise and the cut ------------------------------------------------------------------------------------
// d: the lower median of |c_1| over the contig
inline double sigma_of(int64_t d) { return 1.4826 * (double)d / sqrt(2.0); }

// mags: the M peaks' magnitudes of one (contig, level), descending.  p_i = erfc(m_i / (sqrt(2h) * sigma * sqrt(2))); with the
// largest 1-based i such that p_i <= q * i / M the cut is m_i - peaks of at least that magnitude are breakpoints -, NO_CUT
// without one.  sigma == 0: every peak passes.  p rises with i and q * i / M <= q, so the walk ends at the first p_i > q.
inline int64_t fdr_cut(const int64_t *mags, int64_t M, int64_t h, double sigma, double q) {
    if (M <= 0) return NO_CUT;
    if (sigma == 0) return 1;
    const double denom = sqrt(2.0 * (double)h) * sigma * sqrt(2.0);
    int64_t best = -1;
    for (int64_t i = 0; i < M; ++i) {
        const double p = erfc((double)mags[i] / denom);
        if (p > q) break;
        if (p <= q * (double)(i + 1) / (double)M) best = i;
    }
    return best < 0 ? NO_CUT : mags[best];
}

}  // namespace coral_cn
#endif
