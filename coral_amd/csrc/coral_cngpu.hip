// coral_cngpu.hip - the device backend of `cnv`: coral_cn_segment_gpu and coral_cn_workspace_bytes (include/coral_hip.h).  The rule
// is coral_cn_core.h's, the same functions the host backend (coral_cn_host.h) loops over; the kernels here only spread it over the
// bins.  Everything runs on the caller's stream in the caller's workspace:
//
//   k_cn_keys      per bin: its contig, the candidate test, the median keys (bases of the centring candidates, else all ones)
//   (radix sort)   -> k_cn_centre: C, C_ref and their L() stay in device memory, so no wait is needed for them
//   k_cn_signal    per bin: keep flag and s = L(bases) - L(C) [- (L(ref) - L(C_ref))]
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
// One thread per (kept) bin everywhere, grid-stride, 64-bit coalesced loads and plain vector stores; no atomics.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_cn_host.h"

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
};

#define CN_FOR(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

__global__ __launch_bounds__(CN_BLOCK) void k_cn_keys(CnTable T, int32_t *__restrict__ bin_contig, uint64_t *__restrict__ key, uint64_t *__restrict__ ref_key) {
    CN_FOR(b, T.n_bins) {
        const int32_t c = contig_of(T.bin_off, T.n_contigs, b);
        const int64_t v = T.bases[b], r = T.ref ? T.ref[b] : 0;
        const bool cand = candidate(full_bin(b - T.bin_off[c], T.bin_size, T.lengths[c]), v, T.ref != nullptr, r);
        const bool mid = cand && T.centre[c];
        bin_contig[b] = cand ? c : -1 - c;
        key[b] = mid ? (uint64_t)v : ~0ull;
        if (T.ref) ref_key[b] = mid ? (uint64_t)r : ~0ull;
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
                                                         int32_t *__restrict__ signal) {
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
    }
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
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {                      // hands the workspace out in 256-byte steps (p == 0: only the size is counted)
    uintptr_t p;
    size_t used = 0;
    template <class T> T *take(size_t n) { used += up256(n * sizeof(T)); return (T *)(p + used - up256(n * sizeof(T))); }
};

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
    void *tmp;
    size_t tmp_bytes, bytes;
    CnWorkspace(void *base, long long n_bins, int32_t n_contigs, int32_t levels, bool has_ref, long long row_cap, size_t cub_bytes) {
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
        tmp = cv.take<uint8_t>(cub_bytes);
        tmp_bytes = cub_bytes;
        bytes = cv.used;
    }
};

int cn_fail(int rc, const std::string &msg) { coral_bam::set_error(msg); return rc; }

unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + CN_BLOCK - 1) / CN_BLOCK, CN_GRID_CAP)); }

}  // namespace

extern "C" int64_t coral_cn_workspace_bytes(int64_t n_bins, int32_t n_contigs, int32_t levels, int32_t has_reference, int64_t row_cap) {
    if (n_bins < 0 || n_bins > MAX_BINS || n_contigs < 0 || levels < 1 || levels > MAX_LEVELS || row_cap < 0) return CORAL_ERR_ARG;
    if (row_cap > n_bins) row_cap = n_bins;
    const CnWorkspace W(nullptr, n_bins, n_contigs, levels, has_reference != 0, row_cap, cub_tmp_bytes(n_bins, n_contigs));
    return (int64_t)W.bytes + 256;
}

extern "C" int coral_cn_segment_gpu(int32_t device, int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases, const int64_t *ref_bases,
                                    const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end,
                                    int64_t *row_probes, int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, void *workspace, int64_t workspace_bytes, void *stream_,
                                    double *seconds) {
    const std::string me = "coral_cn_segment_gpu: ";
    const Table T{n_contigs, bin_off, lengths, bin_size, bases, ref_bases, centre};
    if (!counts || row_cap < 0 || !table_ok(T, levels, fdr_q))
        return cn_fail(CORAL_ERR_ARG, me + "a missing array, bins that do not fit the contigs, more than 2^28 bins, levels outside 1..20 or fdr_q outside (0, 1)");
    const long long N = bin_off[n_contigs];
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    if (seconds) for (int k = 0; k < 6; ++k) seconds[k] = 0;
    if (N == 0) return CORAL_OK;
    if (row_cap > N) row_cap = N;
    if (row_cap > 0 && (!row_contig || !row_start || !row_end || !row_probes || !row_sum_s || !row_sum_bases)) return cn_fail(CORAL_ERR_ARG, me + "a missing row array");
    if (hipSetDevice(device) != hipSuccess) return cn_fail(CORAL_ERR_HIP, me + "hipSetDevice failed");
    const bool has_ref = ref_bases != nullptr;
    const size_t cub_bytes = cub_tmp_bytes(N, n_contigs);
    const CnWorkspace sized(nullptr, N, n_contigs, levels, has_ref, row_cap, cub_bytes);
    if (!workspace || workspace_bytes < (int64_t)sized.bytes + 256) return cn_fail(CORAL_ERR_ARG, me + "the workspace is smaller than coral_cn_workspace_bytes");
    const CnWorkspace W((void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255), N, n_contigs, levels, has_ref, row_cap, cub_bytes);
    hipStream_t stream = (hipStream_t)stream_;

    int rc = CORAL_OK;
    std::string err;
    auto bad = [&](int code, const std::string &what) { if (rc == CORAL_OK) { rc = code; err = what; } return false; };
    auto ok = [&](hipError_t e, const char *what) { return e == hipSuccess || bad(CORAL_ERR_HIP, me + what + ": " + hipGetErrorString(e)); };
    auto launched = [&](const char *what) { return ok(hipGetLastError(), what); };
    constexpr int N_EV = 7;
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
    const CnTable D{n_contigs, N, bin_size, W.bin_off, W.lengths, W.bases, W.ref, W.centre};
    const unsigned g_bins = grid_of(N + 1), g_contigs = grid_of((long long)n_contigs + 1);
    const size_t NC = (size_t)n_contigs + 1;

    std::vector<int64_t> med((size_t)n_contigs), cuts(NC * (size_t)levels, NO_CUT), peaks;
    std::vector<int32_t> koff(NC), poff(NC * (size_t)levels);
    CnScalars scal{};
    long long bound = 0;
    int32_t n_rows = 0;

    // ---- up, centre, signal, compaction, prefix sums, noise ----------------------------------------------------------------------
    good = good && mark(0) && up(W.bin_off, bin_off, NC * 8) && up(W.lengths, lengths, (size_t)n_contigs * 8) && up(W.centre, centre, (size_t)n_contigs) &&
           up(W.bases, bases, (size_t)N * 8) && (!has_ref || up(W.ref, ref_bases, (size_t)N * 8)) && mark(1);
    if (good) {
        hipLaunchKernelGGL(k_cn_keys, dim3(g_bins), dim3(CN_BLOCK), 0, stream, D, W.bin_contig, W.key, W.ref_key);
        size_t b = W.tmp_bytes;
        good = launched("k_cn_keys") && ok(hipcub::DeviceRadixSort::SortKeys(W.tmp, b, W.key, W.key_s, (int)N, 0, 64, stream), "sort of the centring keys");
        b = W.tmp_bytes;
        good = good && (!has_ref || ok(hipcub::DeviceRadixSort::SortKeys(W.tmp, b, W.ref_key, W.ref_key_s, (int)N, 0, 64, stream), "sort of the centring keys"));
    }
    if (good) {
        hipLaunchKernelGGL(k_cn_centre, dim3(1), dim3(64), 0, stream, W.key_s, has_ref ? W.ref_key_s : nullptr, N, W.scal);
        hipLaunchKernelGGL(k_cn_signal, dim3(g_bins), dim3(CN_BLOCK), 0, stream, D, W.bin_contig, W.scal, W.keep, W.signal);
        good = launched("k_cn_signal") && scan32(W.keep, W.kpos) && zero(W.xs, ((size_t)N + 1) * 8) && zero(W.kb, ((size_t)N + 1) * 8);
    }
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
           down(&scal, W.scal, sizeof(scal)) && wait();
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
        counts[1] = koff[(size_t)n_contigs]; counts[2] = scal.centre; counts[3] = scal.ref_centre;
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
            seconds[0] = span(0, 1); seconds[1] = span(1, 2); seconds[2] = span(2, 3); seconds[3] = span(3, 4); seconds[4] = cut_s; seconds[5] = span(5, 6);
        }
    }
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    return rc == CORAL_OK ? CORAL_OK : cn_fail(rc, err);
}
