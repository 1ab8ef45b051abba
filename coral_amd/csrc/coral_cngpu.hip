// coral_cngpu.hip - the device backend of `cnv`: coral_cn_segment_gpu and coral_cn_workspace_bytes (include/coral_hip.h).  The rule
// is coral_cn_core.h's, the same functions the host backend (coral_cn_host.h) loops over; the kernels here only spread it over the
// bins.  Everything runs on the caller's stream in the caller's workspace:
//
//   k_cn_keys      per bin: its contig, the candidate test, the median keys (bases of the centring candidates, else all ones)
//   (radix sort)   -> k_cn_centre: C, C_ref and their L() stay in device memory, so no wait is needed for them
//   k_cn_signal    per bin: keep flag and s = L(bases) - L(C) [- (L(ref) - L(C_ref))]
//   with a composition (coral_cn_segment_gc_gpu): k_cn_keys also applies the called-base mask, k_cn_signal also leaves each bin's
//                  stratum and P's sort keys (stratum << 32 | signal); (one radix sort), k_cn_gc_starts (the strata's starts by
//                  binary search), k_cn_gc_bias (a wave per stratum: the pool from the prefix counts, its lower median by
//                  bisection on the value), k_cn_gc_apply (s' = s - bias); no merge, no floating point, no host wait
//   (scan)         -> k_cn_compact: the kept bins back to back (s, bases, bin, contig), k_cn_offsets: each contig's first kept bin
//   (2 scans)      the prefix sums of s and of bases over the kept bins; a contig's are differences against its first entry
//   k_cn_abs1      |c_1[k]| with its contig, (sort by contig: two radix sorts, by value, then stably by contig) -> k_cn_median: d
//   per level:     k_haar_detail (|c_h| where k is a peak, else 0, from the prefix sums with contig-aware mirror indices),
//                  (scan), k_haar_scatter (the peaks back to back with their contigs), (sort by contig, falling within each)
//   wait 1: d, the peak counts.   wait 2: the sorted magnitudes.   The host calls fdr_cut per (contig, level) - the one
//   floating-point step - and sends the cuts back.
//   per level:     (scan of the breakpoint flags as they stood), k_haar_unify: a peak at or above its cut becomes a breakpoint
//                  unless the earlier levels' set has one within 2^(l-1) kept bins of the same contig
//   k_cn_starts, (scan), k_cn_rowstart, k_cn_segments: a row per segment from differences of the prefix sums
//   wait 3: the rows.
//
// One thread per (kept) bin everywhere but k_cn_gc_bias, grid-stride, 64-bit coalesced loads and plain vector stores; the one atomic
// is k_cn_keys' count of the bins lost to the called-base mask, one add per workgroup.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_cn_host.h"
#include "coral_stream_gpu.h"

namespace coral_bam { void set_error(const std::string &msg); }      // coral_bam_last_error() of the calling thread (coral_bam.cpp)

namespace {

using namespace coral_cn;

constexpr int CN_BLOCK = 256;
constexpr long long CN_GRID_CAP = 2048;

// what stays in device memory between the kernels
struct CnScalars { int64_t centre, ref_centre, n_centring; int32_t l_centre, l_ref_centre; };

struct CnTable {                     // the table in device memory
    int32_t n_contigs;
    int64_t n_bins, bin_size;
    const int64_t *bin_off, *lengths, *bases, *ref;
    const uint8_t *centre;
    const uint32_t *gc, *at;             // the reference's composition per bin, or both null
    int32_t strata, permille;
};

#define CN_FOR(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

__global__ __launch_bounds__(CN_BLOCK) void k_cn_keys(CnTable T, int32_t *__restrict__ bin_contig, uint64_t *__restrict__ key, uint64_t *__restrict__ ref_key,
                                                       unsigned long long *__restrict__ lost) {
    using Reduce = hipcub::BlockReduce<uint32_t, CN_BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    uint32_t uncalled = 0;
    CN_FOR(b, T.n_bins) {
        const int32_t c = contig_of(T.bin_off, T.n_contigs, b);
        const int64_t v = T.bases[b], r = T.ref ? T.ref[b] : 0;
        bool cand = candidate(full_bin(b - T.bin_off[c], T.bin_size, T.lengths[c]), v, T.ref != nullptr, r);
        if (cand && T.gc && !called_enough(T.gc[b], T.at[b], T.bin_size, T.permille)) { cand = false; ++uncalled; }
        const bool mid = cand && T.centre[c];
        bin_contig[b] = cand ? c : -1 - c;
        key[b] = mid ? (uint64_t)v : ~0ull;
        if (T.ref) ref_key[b] = mid ? (uint64_t)r : ~0ull;
    }
    if (T.gc) {                                          // (the same for every thread) the candidates lost to the called-base mask
        const uint32_t sum = Reduce(tmp).Sum(uncalled);
        if (threadIdx.x == 0 && sum) atomicAdd(lost, (unsigned long long)sum);
    }
}

// sorted keys -> the lower medians (one thread)
__global__ void k_cn_centre(const uint64_t *__restrict__ key, const uint64_t *__restrict__ ref_key, long long n_bins, CnScalars *S) {
    if (blockIdx.x || threadIdx.x) return;
    long long lo = 0, hi = n_bins;                       // the first key of all ones
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (key[mid] == ~0ull) hi = mid; else lo = mid + 1;
    }
    CnScalars s{0, 0, lo, 0, 0};
    if (lo > 0) {
        s.centre = (int64_t)key[(lo - 1) / 2];
        s.l_centre = log2_q16((uint64_t)s.centre);
        if (ref_key) { s.ref_centre = (int64_t)ref_key[(lo - 1) / 2]; s.l_ref_centre = log2_q16((uint64_t)s.ref_centre); }
    }
    *S = s;
}

__global__ __launch_bounds__(CN_BLOCK) void k_cn_signal(CnTable T, const int32_t *__restrict__ bin_contig, const CnScalars *__restrict__ S, int32_t *__restrict__ keep,
                                                         int32_t *__restrict__ signal, int32_t *__restrict__ stratum, uint64_t *__restrict__ gc_key) {
    const CnScalars s = *S;
    CN_FOR(b, T.n_bins + 1) {                            // (entry n_bins: the scan's closing 0)
        int32_t k = 0, x = 0;
        if (b < T.n_bins && bin_contig[b] >= 0) {
            const int64_t v = T.bases[b], r = T.ref ? T.ref[b] : 0;
            if (above_floor(v, s.centre) && (!T.ref || above_floor(r, s.ref_centre))) {
                k = 1;
                x = log2_q16((uint64_t)v) - s.l_centre;
                if (T.ref) x -= log2_q16((uint64_t)r) - s.l_ref_centre;
            }
        }
        keep[b] = k;
        if (b < T.n_bins) signal[b] = x;
        if (T.gc && b < T.n_bins) {                      // the stratum, and the sort key of P: the kept bins of the centring contigs
            const int32_t g = k ? gc_stratum(T.gc[b], T.at[b], T.strata) : 0;
            stratum[b] = g;
            gc_key[b] = k && T.centre[bin_contig[b]] ? ((uint64_t)g << 32) | signal_key(x) : ~0ull;
        }
    }
}

// sorted keys of P -> start[g] = the bins of P in the strata below g, g = 0..strata + 1
__global__ __launch_bounds__(CN_BLOCK) void k_cn_gc_starts(const uint64_t *__restrict__ key, long long n_bins, int32_t strata, int64_t *__restrict__ start) {
    CN_FOR(g, (long long)strata + 2) {
        const uint64_t want = (uint64_t)g << 32;
        long long lo = 0, hi = n_bins;                   // the first key of at least `want` (the keys of all ones lie behind every stratum)
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (key[mid] < want) lo = mid + 1; else hi = mid;
        }
        start[g] = lo;
    }
}

// One wave per stratum g: the pool's strata from the prefix counts, then the pool's lower median by bisection on the value - per
// step every lane counts, by binary search in its strata's sorted runs, the pool's signals at or below the probe.
__global__ __launch_bounds__(64) void k_cn_gc_bias(const uint64_t *__restrict__ key, const int64_t *__restrict__ start, int32_t strata, int64_t min_bins, int64_t *__restrict__ bias,
                                                   int64_t *__restrict__ stratum_bins) {
    const int32_t g = blockIdx.x, lane = threadIdx.x;
    if (g > strata) return;
    const int64_t need = min_bins < start[strata + 1] ? min_bins : start[strata + 1];
    int32_t w = 0;
    for (int32_t base = 0;; base += 64) {                // the smallest w whose strata hold `need` bins (gc_pool, 64 widths a step)
        const int32_t mine = base + lane, l = g - mine < 0 ? 0 : g - mine, h = g + mine > strata ? strata : g + mine;
        const unsigned long long hit = __ballot(start[h + 1] - start[l] >= need || (l == 0 && h == strata));
        if (hit) { w = base + __builtin_ctzll(hit); break; }
    }
    const int32_t lo = g - w < 0 ? 0 : g - w, hi = g + w > strata ? strata : g + w;
    const int64_t cnt = start[hi + 1] - start[lo];
    int64_t out = 0;
    if (cnt > 0) {
        const int64_t rank = (cnt - 1) / 2;              // the lower median: the smallest value with more than `rank` signals at or below it
        uint64_t vlo = 0, vhi = 0xffffffffull;
        while (vlo < vhi) {
            const uint64_t mid = (vlo + vhi) / 2;
            int64_t below = 0;
            for (int32_t t = lo + lane; t <= hi; t += 64) {
                const uint64_t probe = ((uint64_t)t << 32) | mid;
                int64_t a = start[t], b = start[t + 1];  // the first key above the probe within stratum t's run
                while (a < b) {
                    const int64_t m = a + (b - a) / 2;
                    if (key[m] <= probe) a = m + 1; else b = m;
                }
                below += a - start[t];
            }
            for (int d = 32; d >= 1; d >>= 1) below += __shfl_xor(below, d);
            if (below > rank) vhi = mid; else vlo = mid + 1;
        }
        out = key_signal((uint32_t)vlo);
    }
    if (lane == 0) { bias[g] = out; stratum_bins[g] = start[g + 1] - start[g]; }
}

__global__ __launch_bounds__(CN_BLOCK) void k_cn_gc_apply(long long n_bins, const int32_t *__restrict__ keep, const int32_t *__restrict__ stratum, const int64_t *__restrict__ bias,
                                                          int32_t *__restrict__ signal) {
    CN_FOR(b, n_bins) if (keep[b]) signal[b] -= (int32_t)bias[stratum[b]];
}

__global__ __launch_bounds__(CN_BLOCK) void k_cn_compact(CnTable T, const int32_t *__restrict__ bin_contig, const int32_t *__restrict__ keep, const int32_t *__restrict__ kpos,
                                                          const int32_t *__restrict__ signal, int64_t *__restrict__ xs, int64_t *__restrict__ kb, int32_t *__restrict__ kbin,
                                                          int32_t *__restrict__ kcontig) {
    CN_FOR(b, T.n_bins) {
        if (!keep[b]) continue;
        const int32_t ki = kpos[b];
        xs[ki] = signal[b];
        kb[ki] = T.bases[b];
        kbin[ki] = (int32_t)b;
        kcontig[ki] = bin_contig[b];
    }
}

// koff[c] = the kept index of contig c's first kept bin (c = n_contigs: the number of kept bins); mcnt[c]: how many |c_1| values it has
__global__ __launch_bounds__(CN_BLOCK) void k_cn_offsets(CnTable T, const int32_t *__restrict__ kpos, int32_t *__restrict__ koff, int32_t *__restrict__ mcnt) {
    CN_FOR(c, (long long)T.n_contigs + 1) {
        const int32_t a = kpos[T.bin_off[c]];
        koff[c] = a;
        mcnt[c] = c < T.n_contigs && kpos[T.bin_off[c + 1]] > a ? kpos[T.bin_off[c + 1]] - a - 1 : 0;
    }
}

__global__ __launch_bounds__(CN_BLOCK) void k_cn_abs1(long long n_bins, const int32_t *__restrict__ koff, int32_t n_contigs, const int32_t *__restrict__ kcontig,
                                                       const int64_t *__restrict__ G, int64_t *__restrict__ a1, uint32_t *__restrict__ cid) {
    const long long K = koff[n_contigs];
    CN_FOR(ki, n_bins) {
        int64_t v = 0;
        uint32_t id = (uint32_t)n_contigs;                // k = 0 and what lies behind the kept bins: sorted behind every contig
        if (ki < K) {
            const int32_t c = kcontig[ki];
            const int64_t first = koff[c];
            if (ki > first) {
                v = haar_detail(G + first, koff[c + 1] - first, ki - first, 1);
                id = (uint32_t)c;
            }
        }
        a1[ki] = v < 0 ? -v : v;
        cid[ki] = id;
    }
}

__global__ __launch_bounds__(CN_BLOCK) void k_cn_median(int32_t n_contigs, const int32_t *__restrict__ koff, const int32_t *__restrict__ mbeg, const int64_t *__restrict__ sorted,
                                                         int64_t *__restrict__ med) {
    CN_FOR(c, (long long)n_contigs) {
        const int64_t n = koff[c + 1] - koff[c];
        med[c] = n >= 2 ? sorted[mbeg[c] + (n - 2) / 2] : -1;
    }
}

// the magnitude of the peak at kept bin ki of level `level`, 0 where there is none (or the level is skipped for the contig)
__device__ __forceinline__ int64_t peak_at(long long ki, int32_t level, const int32_t *__restrict__ koff, const int32_t *__restrict__ kcontig, const int64_t *__restrict__ G,
                                           int32_t &c, int64_t &first, int64_t &n) {
    c = kcontig[ki];
    first = koff[c];
    n = koff[c + 1] - first;
    const int64_t h = (int64_t)1 << level;
    return h <= n ? peak_mag(G + first, n, ki - first, h) : 0;
}

__global__ __launch_bounds__(CN_BLOCK) void k_haar_detail(long long n_bins, int32_t level, const int32_t *__restrict__ koff, int32_t n_contigs, const int32_t *__restrict__ kcontig,
                                                           const int64_t *__restrict__ G, int64_t *__restrict__ mag, int32_t *__restrict__ pflag) {
    const long long K = koff[n_contigs];
    CN_FOR(ki, n_bins + 1) {
        int64_t m = 0;
        if (ki < K) {
            int32_t c;
            int64_t first, n;
            m = peak_at(ki, level, koff, kcontig, G, c, first, n);
        }
        if (ki < n_bins) mag[ki] = m;
        pflag[ki] = m > 0;
    }
}

// the peaks back to back with their contigs; behind them, up to n_bins entries, magnitude 0 of contig n_contigs
__global__ __launch_bounds__(CN_BLOCK) void k_haar_scatter(long long n_bins, const int64_t *__restrict__ mag, const int32_t *__restrict__ ppos, const int32_t *__restrict__ kcontig,
                                                            int64_t *__restrict__ dense, uint32_t *__restrict__ cid, const int32_t *__restrict__ koff, int32_t n_contigs,
                                                            int32_t *__restrict__ poff) {
    const long long total = ppos[n_bins];
    CN_FOR(ki, n_bins) {
        const int64_t m = mag[ki];
        if (m > 0) { dense[ppos[ki]] = m; cid[ppos[ki]] = (uint32_t)kcontig[ki]; }
        if (ki >= total) { dense[ki] = 0; cid[ki] = (uint32_t)n_contigs; }
    }
    CN_FOR(c, (long long)n_contigs + 1) poff[c] = ppos[koff[c]];
}

__global__ __launch_bounds__(CN_BLOCK) void k_haar_unify(long long n_bins, int32_t level, const int32_t *__restrict__ koff, int32_t n_contigs, const int32_t *__restrict__ kcontig,
                                                          const int64_t *__restrict__ G, const int64_t *__restrict__ cut, const int32_t *__restrict__ before,
                                                          int32_t *__restrict__ bp) {
    const long long K = koff[n_contigs];
    CN_FOR(ki, K) {
        int32_t c;
        int64_t first, n;
        const int64_t m = peak_at(ki, level, koff, kcontig, G, c, first, n);
        if (m == 0 || m < cut[c]) continue;
        int64_t lo, hi;
        unify_window(ki, (int64_t)1 << (level - 1), first, first + n - 1, lo, hi);
        if (before[hi + 1] == before[lo]) bp[ki] = 1;     // (before: the exclusive sums of bp as it stood in front of this level)
    }
}

__global__ __launch_bounds__(CN_BLOCK) void k_cn_starts(long long n_bins, const int32_t *__restrict__ koff, int32_t n_contigs, const int32_t *__restrict__ kcontig,
                                                         const int32_t *__restrict__ bp, int32_t *__restrict__ starts) {
    const long long K = koff[n_contigs];
    CN_FOR(ki, n_bins + 1) starts[ki] = ki < K && (bp[ki] || ki == koff[kcontig[ki]]);
}

__global__ __launch_bounds__(CN_BLOCK) void k_cn_rowstart(long long n_bins, const int32_t *__restrict__ koff, int32_t n_contigs, const int32_t *__restrict__ starts,
                                                           const int32_t *__restrict__ row_of, int32_t *__restrict__ rowstart, long long row_cap) {
    const long long K = koff[n_contigs];
    CN_FOR(ki, K + 1) {
        const int32_t r = row_of[ki];
        if ((ki == K || starts[ki]) && r <= row_cap) rowstart[r] = (int32_t)ki;      // (entry K closes the last row)
    }
}

struct CnRows { int32_t *contig; int64_t *start, *end, *probes, *sum_s, *sum_bases; };

__global__ __launch_bounds__(CN_BLOCK) void k_cn_segments(CnTable T, const int32_t *__restrict__ row_of, const int32_t *__restrict__ rowstart, const int32_t *__restrict__ kbin,
                                                           const int32_t *__restrict__ kcontig, const int64_t *__restrict__ G, const int64_t *__restrict__ B, long long row_cap,
                                                           CnRows R) {
    long long n_rows = row_of[T.n_bins];
    if (n_rows > row_cap) n_rows = row_cap;
    CN_FOR(r, n_rows) {
        const int32_t a = rowstart[r], b = rowstart[r + 1], c = kcontig[a];
        R.contig[r] = c;
        R.start[r] = (kbin[a] - T.bin_off[c]) * T.bin_size;
        R.end[r] = bin_end(kbin[b - 1] - T.bin_off[c], T.bin_size, T.lengths[c]);
        R.probes[r] = b - a;
        R.sum_s[r] = G[b] - G[a];
        R.sum_bases[r] = B[b] - B[a];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
using coral_stream::Carver;          // hands the workspace out in 256-byte steps
using coral_stream::up256;

// hipcub's temporary storage for the largest of the calls below
size_t cub_tmp_bytes(long long n_bins, int32_t n_contigs) {
    size_t need = 0, b = 0;
    const int n = (int)std::max<long long>(n_bins + 1, (long long)n_contigs + 1);
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int32_t *)nullptr, (int32_t *)nullptr, n) == hipSuccess) need = std::max(need, b);
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int64_t *)nullptr, (int64_t *)nullptr, n) == hipSuccess) need = std::max(need, b);
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, n) == hipSuccess) need = std::max(need, b);
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, b, (int64_t *)nullptr, (int64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, n) == hipSuccess) need = std::max(need, b);
    if (hipcub::DeviceRadixSort::SortPairsDescending(nullptr, b, (int64_t *)nullptr, (int64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, n) == hipSuccess)
        need = std::max(need, b);
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr, n) == hipSuccess) need = std::max(need, b);
    return need + 256;
}

struct CnWorkspace {
    int64_t *bin_off, *lengths, *bases, *ref, *xs, *kb, *G, *B, *a1, *a1s, *med, *mag, *dense_in, *dense_tmp, *dense_out, *cut;
    uint8_t *centre;
    uint64_t *key, *key_s, *ref_key, *ref_key_s;
    int32_t *bin_contig, *keep, *kpos, *signal, *kbin, *kcontig, *koff, *mcnt, *mbeg, *pflag, *ppos, *poff, *bp, *before, *starts, *row_of, *rowstart;
    uint32_t *cid, *cid_tmp;
    CnScalars *scal;
    CnRows rows;
    uint32_t *gc, *at;               // with a composition: the two tables, each bin's stratum, the strata's starts, bias and bins
    int32_t *stratum;
    int64_t *gc_start, *gc_bias, *gc_bins;
    unsigned long long *lost;
    void *tmp;
    size_t tmp_bytes, bytes;
    CnWorkspace(void *base, long long n_bins, int32_t n_contigs, int32_t levels, bool has_ref, long long row_cap, size_t cub_bytes, bool has_gc = false, int32_t strata = 0) {
        Carver cv{(uintptr_t)base};
        const size_t N = (size_t)n_bins + 1, NC = (size_t)n_contigs + 1;
        bin_off = cv.take<int64_t>(NC); lengths = cv.take<int64_t>(NC); centre = cv.take<uint8_t>(NC);
        bases = cv.take<int64_t>(N); ref = has_ref ? cv.take<int64_t>(N) : nullptr;
        key = cv.take<uint64_t>(N); key_s = cv.take<uint64_t>(N);
        ref_key = has_ref ? cv.take<uint64_t>(N) : nullptr; ref_key_s = has_ref ? cv.take<uint64_t>(N) : nullptr;
        bin_contig = cv.take<int32_t>(N); keep = cv.take<int32_t>(N); kpos = cv.take<int32_t>(N); signal = cv.take<int32_t>(N);
        xs = cv.take<int64_t>(N); kb = cv.take<int64_t>(N); G = cv.take<int64_t>(N); B = cv.take<int64_t>(N);
        kbin = cv.take<int32_t>(N); kcontig = cv.take<int32_t>(N);
        koff = cv.take<int32_t>(NC); mcnt = cv.take<int32_t>(NC); mbeg = cv.take<int32_t>(NC); med = cv.take<int64_t>(NC);
        a1 = cv.take<int64_t>(N); a1s = cv.take<int64_t>(N);
        mag = cv.take<int64_t>(N); dense_in = cv.take<int64_t>(N); dense_tmp = cv.take<int64_t>(N); cid = cv.take<uint32_t>(N); cid_tmp = cv.take<uint32_t>(N);
        dense_out = cv.take<int64_t>(N * (size_t)levels);
        pflag = cv.take<int32_t>(N); ppos = cv.take<int32_t>(N); poff = cv.take<int32_t>(NC * (size_t)levels); cut = cv.take<int64_t>(NC * (size_t)levels);
        bp = cv.take<int32_t>(N); before = cv.take<int32_t>(N); starts = cv.take<int32_t>(N); row_of = cv.take<int32_t>(N);
        const size_t RC = (size_t)row_cap + 1;
        rowstart = cv.take<int32_t>(RC + 1);
        rows.contig = cv.take<int32_t>(RC); rows.start = cv.take<int64_t>(RC); rows.end = cv.take<int64_t>(RC); rows.probes = cv.take<int64_t>(RC);
        rows.sum_s = cv.take<int64_t>(RC); rows.sum_bases = cv.take<int64_t>(RC);
        scal = cv.take<CnScalars>(1);
        const size_t NG = (size_t)strata + 2;
        gc = has_gc ? cv.take<uint32_t>(N) : nullptr; at = has_gc ? cv.take<uint32_t>(N) : nullptr; stratum = has_gc ? cv.take<int32_t>(N) : nullptr;
        gc_start = has_gc ? cv.take<int64_t>(NG) : nullptr; gc_bias = has_gc ? cv.take<int64_t>(NG) : nullptr; gc_bins = has_gc ? cv.take<int64_t>(NG) : nullptr;
        lost = has_gc ? cv.take<unsigned long long>(1) : nullptr;
        tmp = cv.take<uint8_t>(cub_bytes);
        tmp_bytes = cub_bytes;
        bytes = cv.used;
    }
};

int cn_fail(int rc, const std::string &msg) { coral_bam::set_error(msg); return rc; }

unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + CN_BLOCK - 1) / CN_BLOCK, CN_GRID_CAP)); }

}  // namespace

extern "C" int64_t coral_cn_workspace_gc_bytes(int64_t n_bins, int32_t n_contigs, int32_t levels, int32_t has_reference, int64_t row_cap, int32_t has_composition,
                                               int32_t gc_strata) {
    if (n_bins < 0 || n_bins > MAX_BINS || n_contigs < 0 || levels < 1 || levels > MAX_LEVELS || row_cap < 0) return CORAL_ERR_ARG;
    if (has_composition && (gc_strata < 1 || gc_strata > MAX_GC_STRATA)) return CORAL_ERR_ARG;
    if (row_cap > n_bins) row_cap = n_bins;
    const CnWorkspace W(nullptr, n_bins, n_contigs, levels, has_reference != 0, row_cap, cub_tmp_bytes(n_bins, n_contigs), has_composition != 0, gc_strata);
    return (int64_t)W.bytes + 256;
}

extern "C" int64_t coral_cn_workspace_bytes(int64_t n_bins, int32_t n_contigs, int32_t levels, int32_t has_reference, int64_t row_cap) {
    return coral_cn_workspace_gc_bytes(n_bins, n_contigs, levels, has_reference, row_cap, 0, 0);
}

// seconds: n_seconds entries (6: the stages without a composition; 7: and the gc stage)
static int segment_gpu(int32_t device, int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases, const int64_t *ref_bases,
                       const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end, int64_t *row_probes,
                       int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, void *workspace, int64_t workspace_bytes, void *stream_, double *seconds, int n_seconds,
                       const uint32_t *gc, const uint32_t *at, int32_t gc_strata, int64_t gc_min_bins, int32_t min_called_permille, int64_t *bias, int64_t *stratum_bins) {
    const bool has_gc = gc != nullptr;
    const std::string me = has_gc ? "coral_cn_segment_gc_gpu: " : "coral_cn_segment_gpu: ";
    Table T{n_contigs, bin_off, lengths, bin_size, bases, ref_bases, centre};
    T.gc = gc; T.at = at;
    if (has_gc) { T.gc_strata = gc_strata; T.gc_min_bins = gc_min_bins; T.min_called_permille = min_called_permille; }
    else gc_strata = 0;
    if (!counts || row_cap < 0 || !table_ok(T, levels, fdr_q) || (has_gc && (!bias || !stratum_bins)))
        return cn_fail(CORAL_ERR_ARG, me + "a missing array, bins that do not fit the contigs, more than 2^28 bins, levels outside 1..20, fdr_q outside (0, 1), gc_strata outside "
                                           "1..1000, gc_min_bins below 1 or min_called_permille outside 0..1000");
    const long long N = bin_off[n_contigs];
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    if (seconds) for (int k = 0; k < n_seconds; ++k) seconds[k] = 0;
    if (has_gc) for (int32_t g = 0; g <= gc_strata; ++g) { bias[g] = 0; stratum_bins[g] = 0; }
    if (N == 0) return CORAL_OK;
    if (row_cap > N) row_cap = N;
    if (row_cap > 0 && (!row_contig || !row_start || !row_end || !row_probes || !row_sum_s || !row_sum_bases)) return cn_fail(CORAL_ERR_ARG, me + "a missing row array");
    if (hipSetDevice(device) != hipSuccess) return cn_fail(CORAL_ERR_HIP, me + "hipSetDevice failed");
    const bool has_ref = ref_bases != nullptr;
    const size_t cub_bytes = cub_tmp_bytes(N, n_contigs);
    const CnWorkspace sized(nullptr, N, n_contigs, levels, has_ref, row_cap, cub_bytes, has_gc, gc_strata);
    if (!workspace || workspace_bytes < (int64_t)sized.bytes + 256) return cn_fail(CORAL_ERR_ARG, me + "the workspace is smaller than coral_cn_workspace_gc_bytes");
    const CnWorkspace W((void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255), N, n_contigs, levels, has_ref, row_cap, cub_bytes, has_gc, gc_strata);
    hipStream_t stream = (hipStream_t)stream_;

    int rc = CORAL_OK;
    std::string err;
    auto bad = [&](int code, const std::string &what) { if (rc == CORAL_OK) { rc = code; err = what; } return false; };
    auto ok = [&](hipError_t e, const char *what) { return e == hipSuccess || bad(CORAL_ERR_HIP, me + what + ": " + hipGetErrorString(e)); };
    auto launched = [&](const char *what) { return ok(hipGetLastError(), what); };
    constexpr int N_EV = 9;
    hipEvent_t ev[N_EV] = {};
    bool good = true;
    for (int i = 0; i < N_EV && good; ++i) good = ok(hipEventCreate(&ev[i]), "hipEventCreate");
    auto mark = [&](int i) { return ok(hipEventRecord(ev[i], stream), "hipEventRecord"); };
    auto up = [&](void *dst, const void *src, size_t n) { return n == 0 || ok(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream), "hipMemcpyAsync"); };
    auto down = [&](void *dst, const void *src, size_t n) { return n == 0 || ok(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync"); };
    auto zero = [&](void *p, size_t n) { return ok(hipMemsetAsync(p, 0, n, stream), "hipMemsetAsync"); };
    auto wait = [&]() { return ok(hipStreamSynchronize(stream), "hipStreamSynchronize"); };
    auto scan32 = [&](const int32_t *in, int32_t *out) { size_t b = W.tmp_bytes; return ok(hipcub::DeviceScan::ExclusiveSum(W.tmp, b, in, out, (int)(N + 1), stream), "scan"); };
    auto scan64 = [&](const int64_t *in, int64_t *out) { size_t b = W.tmp_bytes; return ok(hipcub::DeviceScan::ExclusiveSum(W.tmp, b, in, out, (int)(N + 1), stream), "scan"); };
    // N values with their contigs -> the values of each contig back to back, rising (or falling) within it: two stable radix sorts of
    // the whole array, by value and then by the contig's few bits.  (One segment per contig in a segmented sort leaves a
    // chromosome to one workgroup: measured 30 times slower, profiles/cnv.md.)
    int contig_bits = 1;
    while (((int64_t)1 << contig_bits) <= n_contigs) ++contig_bits;
    auto by_contig = [&](bool falling, const int64_t *val, const uint32_t *id, int64_t *out, const char *what) {
        size_t b = W.tmp_bytes;
        const hipError_t e = falling ? hipcub::DeviceRadixSort::SortPairsDescending(W.tmp, b, val, W.dense_tmp, id, W.cid_tmp, (int)N, 0, 64, stream)
                                     : hipcub::DeviceRadixSort::SortPairs(W.tmp, b, val, W.dense_tmp, id, W.cid_tmp, (int)N, 0, 64, stream);
        b = W.tmp_bytes;
        return ok(e, what) && ok(hipcub::DeviceRadixSort::SortPairs(W.tmp, b, W.cid_tmp, W.cid, W.dense_tmp, out, (int)N, 0, contig_bits, stream), what);
    };
    const CnTable D{n_contigs, N, bin_size, W.bin_off, W.lengths, W.bases, W.ref, W.centre, W.gc, W.at, gc_strata, min_called_permille};
    const unsigned g_bins = grid_of(N + 1), g_contigs = grid_of((long long)n_contigs + 1);
    const size_t NC = (size_t)n_contigs + 1;

    std::vector<int64_t> med((size_t)n_contigs), cuts(NC * (size_t)levels, NO_CUT), peaks;
    std::vector<int32_t> koff(NC), poff(NC * (size_t)levels);
    CnScalars scal{};
    unsigned long long lost = 0;
    long long bound = 0;
    int32_t n_rows = 0;

    // ---- up, centre, signal, compaction, prefix sums, noise ----------------------------------------------------------------------
    good = good && mark(0) && up(W.bin_off, bin_off, NC * 8) && up(W.lengths, lengths, (size_t)n_contigs * 8) && up(W.centre, centre, (size_t)n_contigs) &&
           up(W.bases, bases, (size_t)N * 8) && (!has_ref || up(W.ref, ref_bases, (size_t)N * 8)) &&
           (!has_gc || (up(W.gc, gc, (size_t)N * 4) && up(W.at, at, (size_t)N * 4) && zero(W.lost, 8))) && mark(1);
    if (good) {
        hipLaunchKernelGGL(k_cn_keys, dim3(g_bins), dim3(CN_BLOCK), 0, stream, D, W.bin_contig, W.key, W.ref_key, W.lost);
        size_t b = W.tmp_bytes;
        good = launched("k_cn_keys") && ok(hipcub::DeviceRadixSort::SortKeys(W.tmp, b, W.key, W.key_s, (int)N, 0, 64, stream), "sort of the centring keys");
        b = W.tmp_bytes;
        good = good && (!has_ref || ok(hipcub::DeviceRadixSort::SortKeys(W.tmp, b, W.ref_key, W.ref_key_s, (int)N, 0, 64, stream), "sort of the centring keys"));
    }
    if (good) {
        hipLaunchKernelGGL(k_cn_centre, dim3(1), dim3(64), 0, stream, W.key_s, has_ref ? W.ref_key_s : nullptr, N, W.scal);
        hipLaunchKernelGGL(k_cn_signal, dim3(g_bins), dim3(CN_BLOCK), 0, stream, D, W.bin_contig, W.scal, W.keep, W.signal, W.stratum, W.key);      // (the centring keys are through)
        good = launched("k_cn_signal");
    }
    if (good && has_gc) {                                // the GC bias: P sorted by (stratum, signal), the strata's starts, a wave per stratum, s' = s - bias
        size_t b = W.tmp_bytes;
        good = mark(7) && ok(hipcub::DeviceRadixSort::SortKeys(W.tmp, b, W.key, W.key_s, (int)N, 0, 42, stream), "sort of the strata");
        if (good) {
            hipLaunchKernelGGL(k_cn_gc_starts, dim3(grid_of((long long)gc_strata + 2)), dim3(CN_BLOCK), 0, stream, W.key_s, N, gc_strata, W.gc_start);
            hipLaunchKernelGGL(k_cn_gc_bias, dim3((unsigned)gc_strata + 1), dim3(64), 0, stream, W.key_s, W.gc_start, gc_strata, gc_min_bins, W.gc_bias, W.gc_bins);
            hipLaunchKernelGGL(k_cn_gc_apply, dim3(g_bins), dim3(CN_BLOCK), 0, stream, N, W.keep, W.stratum, W.gc_bias, W.signal);
            good = launched("k_cn_gc_apply") && mark(8);
        }
    }
    good = good && scan32(W.keep, W.kpos) && zero(W.xs, ((size_t)N + 1) * 8) && zero(W.kb, ((size_t)N + 1) * 8);
    if (good) {
        hipLaunchKernelGGL(k_cn_compact, dim3(g_bins), dim3(CN_BLOCK), 0, stream, D, W.bin_contig, W.keep, W.kpos, W.signal, W.xs, W.kb, W.kbin, W.kcontig);
        hipLaunchKernelGGL(k_cn_offsets, dim3(g_contigs), dim3(CN_BLOCK), 0, stream, D, W.kpos, W.koff, W.mcnt);
        good = launched("k_cn_compact") && scan64(W.xs, W.G) && scan64(W.kb, W.B) && mark(2);
    }
    if (good) {
        hipLaunchKernelGGL(k_cn_abs1, dim3(g_bins), dim3(CN_BLOCK), 0, stream, N, W.koff, n_contigs, W.kcontig, W.G, W.a1, W.cid);
        size_t b = W.tmp_bytes;
        good = launched("k_cn_abs1") && ok(hipcub::DeviceScan::ExclusiveSum(W.tmp, b, W.mcnt, W.mbeg, (int)NC, stream), "scan of the contigs' |c_1| counts") &&
               by_contig(false, W.a1, W.cid, W.a1s, "sort of |c_1|");
    }
    if (good) {
        hipLaunchKernelGGL(k_cn_median, dim3(g_contigs), dim3(CN_BLOCK), 0, stream, n_contigs, W.koff, W.mbeg, W.a1s, W.med);
        good = launched("k_cn_median") && mark(3);
    }
    // ---- every level's peaks, sorted per contig ------------------------------------------------------------------------------------
    for (int32_t l = 1; l <= levels && good; ++l) {
        int64_t *out = W.dense_out + (size_t)(l - 1) * ((size_t)N + 1);
        int32_t *po = W.poff + (size_t)(l - 1) * NC;
        hipLaunchKernelGGL(k_haar_detail, dim3(g_bins), dim3(CN_BLOCK), 0, stream, N, l, W.koff, n_contigs, W.kcontig, W.G, W.mag, W.pflag);
        good = launched("k_haar_detail") && scan32(W.pflag, W.ppos);
        if (!good) break;
        hipLaunchKernelGGL(k_haar_scatter, dim3(g_bins), dim3(CN_BLOCK), 0, stream, N, W.mag, W.ppos, W.kcontig, W.dense_in, W.cid, W.koff, n_contigs, po);
        good = launched("k_haar_scatter") && by_contig(true, W.dense_in, W.cid, out, "sort of the peaks");
    }
    // wait 1: the noise and the counts;  wait 2: the magnitudes
    good = good && mark(4) && down(med.data(), W.med, (size_t)n_contigs * 8) && down(koff.data(), W.koff, NC * 4) && down(poff.data(), W.poff, poff.size() * 4) &&
           down(&scal, W.scal, sizeof(scal)) &&
           (!has_gc || (down(&lost, W.lost, 8) && down(bias, W.gc_bias, ((size_t)gc_strata + 1) * 8) && down(stratum_bins, W.gc_bins, ((size_t)gc_strata + 1) * 8))) && wait();
    if (good) {
        size_t total = 0;
        for (int32_t l = 0; l < levels; ++l) total += (size_t)poff[(size_t)l * NC + n_contigs];
        peaks.resize(total);
        size_t at = 0;
        for (int32_t l = 0; l < levels && good; ++l) {
            const size_t n = (size_t)poff[(size_t)l * NC + n_contigs];
            good = down(peaks.data() + at, W.dense_out + (size_t)l * ((size_t)N + 1), n * 8);
            at += n;
        }
        good = good && wait();
    }
    const auto t_cut = std::chrono::steady_clock::now();
    std::vector<char> level_on((size_t)levels, 0);
    if (good) {
        size_t at = 0;
        for (int32_t l = 0; l < levels; ++l) {
            const int32_t *po = poff.data() + (size_t)l * NC;
            for (int32_t c = 0; c < n_contigs; ++c) {
                const int64_t M = po[c + 1] - po[c], n = koff[(size_t)c + 1] - koff[(size_t)c];
                const int64_t *m = peaks.data() + at + po[c];
                const int64_t cut = level_cut(m, M, n, l + 1, med[(size_t)c], fdr_q);
                cuts[(size_t)l * NC + c] = cut;
                if (cut != NO_CUT) {
                    level_on[(size_t)l] = 1;
                    bound += std::upper_bound(m, m + M, cut, std::greater<int64_t>()) - m;      // peaks of at least the cut
                }
            }
            at += (size_t)po[n_contigs];
        }
        for (int32_t c = 0; c < n_contigs; ++c) bound += koff[(size_t)c + 1] > koff[(size_t)c];
        bound = std::min<long long>(bound, koff[(size_t)n_contigs]);      // (a bin that is a peak at several levels starts one row: no more rows than kept bins)
        counts[1] = koff[(size_t)n_contigs]; counts[2] = scal.centre; counts[3] = scal.ref_centre; counts[5] = (int64_t)lost;
        if (bound > row_cap) { counts[0] = bound; bad(CORAL_ERR_CAPACITY, me + "more rows than row_cap"); good = false; }
    }
    const double cut_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_cut).count();
    // ---- unify, rows -----------------------------------------------------------------------------------------------------------------
    good = good && mark(5) && up(W.cut, cuts.data(), cuts.size() * 8) && zero(W.bp, ((size_t)N + 1) * 4);
    for (int32_t l = 1; l <= levels && good; ++l) {
        if (!level_on[(size_t)l - 1]) continue;
        good = scan32(W.bp, W.before);
        if (!good) break;
        hipLaunchKernelGGL(k_haar_unify, dim3(g_bins), dim3(CN_BLOCK), 0, stream, N, l, W.koff, n_contigs, W.kcontig, W.G, W.cut + (size_t)(l - 1) * NC, W.before, W.bp);
        good = launched("k_haar_unify");
    }
    if (good) {
        hipLaunchKernelGGL(k_cn_starts, dim3(g_bins), dim3(CN_BLOCK), 0, stream, N, W.koff, n_contigs, W.kcontig, W.bp, W.starts);
        good = launched("k_cn_starts") && scan32(W.starts, W.row_of);
    }
    if (good) {
        hipLaunchKernelGGL(k_cn_rowstart, dim3(g_bins), dim3(CN_BLOCK), 0, stream, N, W.koff, n_contigs, W.starts, W.row_of, W.rowstart, (long long)row_cap);
        hipLaunchKernelGGL(k_cn_segments, dim3(grid_of(bound)), dim3(CN_BLOCK), 0, stream, D, W.row_of, W.rowstart, W.kbin, W.kcontig, W.G, W.B, (long long)row_cap, W.rows);
        const size_t nb = (size_t)bound;
        good = launched("k_cn_segments") && down(&n_rows, W.row_of + N, 4) && down(row_contig, W.rows.contig, nb * 4) && down(row_start, W.rows.start, nb * 8) &&
               down(row_end, W.rows.end, nb * 8) && down(row_probes, W.rows.probes, nb * 8) && down(row_sum_s, W.rows.sum_s, nb * 8) &&
               down(row_sum_bases, W.rows.sum_bases, nb * 8) && mark(6) && wait();      // wait 3
    }
    (void)hipStreamSynchronize(stream);                  // nothing of this call is left on the stream, whatever happened
    if (good && n_rows > bound) good = bad(CORAL_ERR_HIP, me + "more rows than the cuts allow");
    if (good) {
        int64_t nonempty = 0;
        for (int32_t c = 0; c < n_contigs; ++c) nonempty += koff[(size_t)c + 1] > koff[(size_t)c];
        counts[0] = n_rows; counts[4] = n_rows - nonempty;
        if (seconds) {
            auto span = [&](int a, int b) { float ms = 0; return hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess ? ms * 1e-3 : 0.0; };
            const double gc_s = has_gc ? span(7, 8) : 0.0;
            seconds[0] = span(0, 1); seconds[1] = span(1, 2) - gc_s; seconds[2] = span(2, 3); seconds[3] = span(3, 4); seconds[4] = cut_s; seconds[5] = span(5, 6);
            if (n_seconds > 6) seconds[6] = gc_s;
        }
    }
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    return rc == CORAL_OK ? CORAL_OK : cn_fail(rc, err);
}

extern "C" int coral_cn_segment_gc_gpu(int32_t device, int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases,
                                       const int64_t *ref_bases, const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap, int32_t *row_contig, int64_t *row_start,
                                       int64_t *row_end, int64_t *row_probes, int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, void *workspace, int64_t workspace_bytes,
                                       void *stream, double *seconds, const uint32_t *gc, const uint32_t *at, int32_t gc_strata, int64_t gc_min_bins, int32_t min_called_permille,
                                       int64_t *bias, int64_t *stratum_bins) {
    return segment_gpu(device, n_contigs, bin_off, lengths, bin_size, bases, ref_bases, centre, levels, fdr_q, row_cap, row_contig, row_start, row_end, row_probes, row_sum_s,
                       row_sum_bases, counts, workspace, workspace_bytes, stream, seconds, 7, gc, at, gc_strata, gc_min_bins, min_called_permille, bias, stratum_bins);
}

extern "C" int coral_cn_segment_gpu(int32_t device, int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases, const int64_t *ref_bases,
                                    const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end,
                                    int64_t *row_probes, int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, void *workspace, int64_t workspace_bytes, void *stream,
                                    double *seconds) {
    return segment_gpu(device, n_contigs, bin_off, lengths, bin_size, bases, ref_bases, centre, levels, fdr_q, row_cap, row_contig, row_start, row_end, row_probes, row_sum_s,
                       row_sum_bases, counts, workspace, workspace_bytes, stream, seconds, 6, nullptr, nullptr, 0, 0, 0, nullptr, nullptr);
}
