// coral_cn_host.h - the host backend of the copy-number segmenter: loops over coral_cn_core.h, one thread.  It is what
// coral_cn_segment_host (coral_cn.cpp) runs, what the device path (coral_cngpu.hip) is compared against, and - with no HIP in
// it - what tests/native/cnv_host.cpp builds with g++ alone.
#ifndef CORAL_CN_HOST_H
#define CORAL_CN_HOST_H

#include <algorithm>
#include <functional>
#include <utility>
#include <vector>

#include "coral_cn_core.h"

namespace coral_cn {

struct Table {                       // a BinnedDepth, and optionally a second one with the same bins
    int32_t n_contigs;
    const int64_t *bin_off;          // n_contigs + 1
    const int64_t *lengths;          // n_contigs
    int64_t bin_size;
    const int64_t *bases;            // bin_off[n_contigs]
    const int64_t *ref_bases;        // the same, or null
    const uint8_t *centre;           // n_contigs: 1 = a centring contig
    const uint32_t *gc = nullptr, *at = nullptr;         // the reference's G/C and A/T bases per bin, or both null
    int32_t gc_strata = 100;
    int64_t gc_min_bins = 256;
    int32_t min_called_permille = 500;
};

struct Rows {
    std::vector<int32_t> contig;
    std::vector<int64_t> start, end, probes, sum_s, sum_bases;
    size_t size() const { return contig.size(); }
};

struct Counts { int64_t rows = 0, kept = 0, centre = 0, ref_centre = 0, breakpoints = 0, uncalled = 0; };

struct GcBias {                      // per stratum 0..gc_strata: the bias in Q16 and the bins of P (empty without a composition)
    std::vector<int64_t> bias, stratum_bins;
};

inline bool table_ok(const Table &T, int32_t levels, double q) {
    if (T.n_contigs < 0 || !T.bin_off || T.bin_size < 1 || levels < 1 || levels > MAX_LEVELS || !(q > 0 && q < 1)) return false;
    if (T.n_contigs > 0 && (!T.lengths || !T.centre)) return false;
    if (T.bin_off[0] != 0) return false;
    for (int32_t c = 0; c < T.n_contigs; ++c) {
        const int64_t len = T.lengths[c] < 0 ? 0 : T.lengths[c];
        if (T.bin_off[c + 1] - T.bin_off[c] != (len + T.bin_size - 1) / T.bin_size) return false;
    }
    const int64_t n = T.bin_off[T.n_contigs];
    if ((T.gc != nullptr) != (T.at != nullptr)) return false;
    if (T.gc && (!gc_params_ok(T.gc_strata, T.gc_min_bins, T.min_called_permille) || T.bin_size > 0x7fffffff)) return false;
    return n <= MAX_BINS && (n == 0 || T.bases);
}

inline int64_t lower_median(std::vector<int64_t> &v) {
    const size_t at = (v.size() - 1) / 2;
    std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)at, v.end());
    return v[at];
}

// the cut of every level of one contig from its sorted peaks; also used by the device path with the peaks it brought back
inline int64_t level_cut(const int64_t *mags_desc, int64_t M, int64_t n, int32_t level, int64_t d, double q) {
    const int64_t h = (int64_t)1 << level;
    if (h > n || d < 0) return NO_CUT;
    return fdr_cut(mags_desc, M, h, sigma_of(d), q);
}

// bias[g] and stratum_bins[g] from P's (stratum, signal) pairs
inline void gc_bias_host(std::vector<std::pair<int32_t, int32_t>> &P, int32_t strata, int64_t min_bins, GcBias &out) {
    out.bias.assign((size_t)strata + 1, 0);
    out.stratum_bins.assign((size_t)strata + 1, 0);
    std::sort(P.begin(), P.end());
    std::vector<int64_t> start((size_t)strata + 2, 0), pool;
    for (const auto &p : P) ++out.stratum_bins[(size_t)p.first];
    for (int32_t g = 0; g <= strata; ++g) start[(size_t)g + 1] = start[(size_t)g] + out.stratum_bins[(size_t)g];
    const int64_t need = std::min<int64_t>(min_bins, (int64_t)P.size());
    for (int32_t g = 0; g <= strata; ++g) {
        int32_t lo, hi;
        gc_pool(start.data(), strata, g, need, lo, hi);
        pool.clear();
        for (int64_t i = start[(size_t)lo]; i < start[(size_t)hi + 1]; ++i) pool.push_back(P[(size_t)i].second);
        if (!pool.empty()) out.bias[(size_t)g] = lower_median(pool);
    }
}

inline void segment_host(const Table &T, int32_t levels, double q, Rows &R, Counts &X, GcBias *gc_out = nullptr) {
    const bool has_ref = T.ref_bases != nullptr, has_gc = T.gc != nullptr;
    // today's candidate test, then the called-base mask: 0 = no candidate, 1 = a candidate, 2 = one lost to the mask
    auto cand = [&](int32_t c, int64_t b) {
        if (!candidate(full_bin(b - T.bin_off[c], T.bin_size, T.lengths[c]), T.bases[b], has_ref, has_ref ? T.ref_bases[b] : 0)) return 0;
        return !has_gc || called_enough(T.gc[b], T.at[b], T.bin_size, T.min_called_permille) ? 1 : 2;
    };
    std::vector<int64_t> mid, ref_mid;
    for (int32_t c = 0; c < T.n_contigs; ++c) {
        for (int64_t b = T.bin_off[c]; b < T.bin_off[c + 1]; ++b) {
            const int k = cand(c, b);
            X.uncalled += k == 2;
            if (k == 1 && T.centre[c]) {
                mid.push_back(T.bases[b]);
                if (has_ref) ref_mid.push_back(T.ref_bases[b]);
            }
        }
    }
    if (has_gc && gc_out) { gc_out->bias.assign((size_t)T.gc_strata + 1, 0); gc_out->stratum_bins.assign((size_t)T.gc_strata + 1, 0); }
    if (mid.empty()) return;
    const int64_t C = X.centre = lower_median(mid);
    const int64_t Cr = X.ref_centre = has_ref ? lower_median(ref_mid) : 0;
    const int32_t LC = log2_q16((uint64_t)C), LCr = has_ref ? log2_q16((uint64_t)Cr) : 0;

    // the kept bins of every contig back to back: bin within the contig, signal, bases, stratum
    std::vector<int64_t> kbin, ks, kv, koff((size_t)T.n_contigs + 1, 0);
    std::vector<int32_t> kg;
    for (int32_t c = 0; c < T.n_contigs; ++c) {
        for (int64_t b = T.bin_off[c]; b < T.bin_off[c + 1]; ++b) {
            const int64_t v = T.bases[b], r = has_ref ? T.ref_bases[b] : 0;
            if (cand(c, b) != 1 || !above_floor(v, C) || (has_ref && !above_floor(r, Cr))) continue;
            int64_t s = (int64_t)log2_q16((uint64_t)v) - LC;
            if (has_ref) s -= (int64_t)log2_q16((uint64_t)r) - LCr;
            kbin.push_back(b - T.bin_off[c]);
            ks.push_back(s);
            kv.push_back(v);
            if (has_gc) kg.push_back(gc_stratum(T.gc[b], T.at[b], T.gc_strata));
        }
        koff[(size_t)c + 1] = (int64_t)kbin.size();
    }
    if (has_gc) {
        std::vector<std::pair<int32_t, int32_t>> P;
        for (int32_t c = 0; c < T.n_contigs; ++c)
            if (T.centre[c]) for (int64_t i = koff[(size_t)c]; i < koff[(size_t)c + 1]; ++i) P.emplace_back(kg[(size_t)i], (int32_t)ks[(size_t)i]);
        GcBias local;
        GcBias &G = gc_out ? *gc_out : local;
        gc_bias_host(P, T.gc_strata, T.gc_min_bins, G);
        for (size_t i = 0; i < ks.size(); ++i) ks[i] -= G.bias[(size_t)kg[i]];
    }

    std::vector<int64_t> P, B, a1, mags, set, add;
    for (int32_t c = 0; c < T.n_contigs; ++c) {
        const int64_t *bin = kbin.data() + koff[(size_t)c];
        const int64_t n = koff[(size_t)c + 1] - koff[(size_t)c];
        if (n == 0) continue;
        P.assign(1, 0); B.assign(1, 0);
        for (int64_t i = koff[(size_t)c]; i < koff[(size_t)c + 1]; ++i) { P.push_back(P.back() + ks[(size_t)i]); B.push_back(B.back() + kv[(size_t)i]); }
        X.kept += n;
        set.clear();
        if (n >= 2) {
            a1.clear();
            for (int64_t k = 1; k < n; ++k) { const int64_t v = haar_detail(P.data(), n, k, 1); a1.push_back(v < 0 ? -v : v); }
            const int64_t d = lower_median(a1);
            for (int32_t l = 1; l <= levels; ++l) {
                const int64_t h = (int64_t)1 << l;
                if (h > n) break;
                mags.clear();
                for (int64_t k = 1; k < n; ++k) { const int64_t m = peak_mag(P.data(), n, k, h); if (m > 0) mags.push_back(m); }
                std::sort(mags.begin(), mags.end(), std::greater<int64_t>());
                const int64_t cut = level_cut(mags.data(), (int64_t)mags.size(), n, l, d, q);
                if (cut == NO_CUT) continue;
                add.clear();
                for (int64_t k = 1; k < n; ++k) {
                    if (peak_mag(P.data(), n, k, h) < cut) continue;
                    int64_t lo, hi;
                    unify_window(k, (int64_t)1 << (l - 1), 0, n - 1, lo, hi);
                    const auto it = std::lower_bound(set.begin(), set.end(), lo);
                    if (it == set.end() || *it > hi) add.push_back(k);
                }
                const size_t old = set.size();
                set.insert(set.end(), add.begin(), add.end());
                std::inplace_merge(set.begin(), set.begin() + (std::ptrdiff_t)old, set.end());
            }
        }
        X.breakpoints += (int64_t)set.size();
        set.push_back(n);
        int64_t a = 0;
        for (const int64_t b : set) {
            R.contig.push_back(c);
            R.start.push_back(bin[(size_t)a] * T.bin_size);
            R.end.push_back(bin_end(bin[(size_t)b - 1], T.bin_size, T.lengths[c]));
            R.probes.push_back(b - a);
            R.sum_s.push_back(P[(size_t)b] - P[(size_t)a]);
            R.sum_bases.push_back(B[(size_t)b] - B[(size_t)a]);
            a = b;
        }
    }
    X.rows = (int64_t)R.size();
}

}  // namespace coral_cn
#endif
