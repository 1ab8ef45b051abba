// coral_satable.hip — K3: the chimeric-alignment table of ALL reads from the tokenised SA tags, on the GPU.
//
// Replaces the per-record loop of fetch() (/root/reference/src/infer_breakpoint_graph.py:139-174: first-seen
// de-duplication of SA entries per read name, read_length from the first record with flag < 256, reads without a
// primary dropped) and alignment_from_satags + the nine cigar2pos* functions
// (/root/reference/src/cigar_parsing.py:17-269: query interval, reference interval, stable (qs, qe) sort).
//
// Pipeline (rocPRIM/hipCUB primitives for the radix sorts and prefix sums, hand-written kernels for the rest):
//   rows keyed by read-name id -> stable radix sort -> one thread per read: de-duplicate, parse, insertion-sort its
//   (few) rows -> reads ordered by their first SA-bearing record (the reference's dict order) -> compaction.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "../../include/coral_hip.h"
#include "coral_query_plan.h"

#define INVALID_KEY 0x7fffffff

static thread_local char g_sa_err[256] = "";
extern "C" const char *coral_sa_last_error(void) { return g_sa_err; }
static int sa_err(int code, const char *msg) {
    snprintf(g_sa_err, sizeof(g_sa_err), "%s", msg);
    return code;
}

__global__ void k_first_primary(int n_rec, const int32_t *__restrict__ tid, const int32_t *__restrict__ flagmq,
                                const int32_t *__restrict__ name, int32_t *__restrict__ first_primary) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rec && tid[r] >= 0 && (flagmq[r] & 0xFFFF) < 256) atomicMin(&first_primary[name[r]], r);
}

__global__ void k_row_keys(int n_sa, const int32_t *__restrict__ sa_rec, const int32_t *__restrict__ tid,
                           const int32_t *__restrict__ name, int32_t *__restrict__ keys, int32_t *__restrict__ vals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sa) return;
    const int r = sa_rec[i];
    keys[i] = tid[r] >= 0 ? name[r] : INVALID_KEY;        // whole-file fetch() skips unplaced records
    vals[i] = i;
}

__global__ void k_heads(int n, const int32_t *__restrict__ keys, int32_t *__restrict__ head) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

__global__ void k_group_starts(int n, const int32_t *__restrict__ head, const int32_t *__restrict__ gid_incl,
                               int32_t *__restrict__ gstart) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head[i]) gstart[gid_incl[i] - 1] = i;
    if (i == n - 1) gstart[gid_incl[i]] = n;
}

struct ParsedRow {
    int qs, qe, tid, ra, rb, strand, mapq, nm;
};

// cigar2pos* for the nine shapes (cp:17-215), from the tokenised [c5 S] m M [x I | -x D] [c3 S]
__device__ __forceinline__ void parse_row(const int32_t *__restrict__ f, int nm, int rl, ParsedRow &o) {
    const int tid = f[0], pos1 = f[1], strand = f[2], c5 = f[3], m = f[4], x = f[5], c3 = f[6];
    const bool fwd = strand == 0, has5 = c5 > 0, has3 = c3 > 0, ins = x > 0, del = x < 0;
    const int al = m + (del ? -x : 0);
    int qs, qe;
    if (has5 && has3) {
        if (!ins && !del) { qs = fwd ? c5 : c3; qe = qs + al - 1; }
        else if (fwd) { qs = c5; qe = rl - c3 - 1; }
        else { qs = c3; qe = rl - c5 - 1; }
    } else if (has5) {
        if (fwd) { qs = c5; qe = rl - 1; }
        else { qs = 0; qe = ins ? rl - c5 - 1 : (del ? m - 1 : al - 1); }
    } else {
        if (!fwd) { qs = c3; qe = rl - 1; }
        else { qs = 0; qe = ins ? rl - c3 - 1 : (del ? m - 1 : al - 1); }
    }
    o.qs = qs; o.qe = qe; o.tid = tid; o.strand = strand; o.mapq = f[7]; o.nm = nm;
    o.ra = fwd ? pos1 - 1 : pos1 + al - 2;
    o.rb = fwd ? pos1 + al - 2 : pos1 - 1;
}

// The error field of a table: 0 = none, else ~(2 * ordinal + (code == 4)) of the FIRST offending read, where ordinal is the
// read's first SA row in file order - the key the reads are sorted by, i.e. the reference's dict order, in which fetch()
// walks the reads and raises at the first one that offends (ibg:163-173).  A read offends with one code only (an unknown
// shape ends it at once), ordinal < 2^31, and the complement turns "smallest ordinal" into an unsigned atomicMax over a
// field that starts at zero.
__device__ __forceinline__ void sa_report(int32_t *__restrict__ err, int ordinal, int code) {
    atomicMax(reinterpret_cast<unsigned int *>(err), ~(2u * (unsigned int)ordinal + (code == 4 ? 1u : 0u)));
}
// the code (3: unknown SA CIGAR shape, 4: zero-length query interval) of an error field, 0 for none
__host__ __device__ __forceinline__ int sa_error_code(int32_t field) {
    return field == 0 ? 0 : ((~(unsigned int)field & 1u) ? 4 : 3);
}

// one read (group g of the name-sorted SA rows): de-duplicate, check, parse and sort its rows
__device__ __forceinline__ void group_process_one(int g, const int32_t *__restrict__ gstart, const int32_t *__restrict__ keys,
                                                  const int32_t *__restrict__ vals, const int32_t *__restrict__ sa,
                                                  const int32_t *__restrict__ sa_nm, const int32_t *__restrict__ first_primary,
                                                  const int32_t *__restrict__ rec_qlen, int32_t *__restrict__ kept_ws /* [n_sa] */,
                                                  int32_t *__restrict__ tmp_rows /* [n_sa][8] */, int32_t *__restrict__ n_kept,
                                                  int32_t *__restrict__ g_first, int32_t *__restrict__ g_failed, int32_t *__restrict__ err) {
    const int a = gstart[g], b = gstart[g + 1];
    const int name = keys[a];
    n_kept[g] = 0;
    g_failed[g] = 0;
    g_first[g] = INVALID_KEY;
    if (name == INVALID_KEY) return;
    const int fp = first_primary[name];
    if (fp == INVALID_KEY) return;                       // chimeric read without a primary alignment: dropped (ibg:163-173)
    g_first[g] = vals[a];                                // stable sort: the read's first SA row in file order
    const int rl = rec_qlen[fp];
    // The group owns slots a..b of kept_ws and tmp_rows (it has b - a SA rows), so a read may have any number of
    // alignments: nothing is kept in per-thread arrays.
    // first-seen de-duplication (ibg:146-151), then cp:246-255: the read fails as a whole at its first offending entry
    int32_t *__restrict__ kept_idx = kept_ws + a;
    int nk = 0;
    for (int i = a; i < b; ++i) {
        const int32_t *fi = sa + 8ll * vals[i];
        const int nmi = sa_nm[vals[i]];
        bool dup = false;
        for (int j = 0; j < nk && !dup; ++j) {
            const int32_t *fj = sa + 8ll * kept_idx[j];
            bool same = sa_nm[kept_idx[j]] == nmi;
            for (int c = 0; c < 8 && same; ++c) same = fi[c] == fj[c];
            dup = same;
        }
        if (dup) continue;
        kept_idx[nk++] = vals[i];
    }
    for (int j = 0; j < nk; ++j) {
        const int32_t *f = sa + 8ll * kept_idx[j];
        if (f[3] == -2) { sa_report(err, vals[a], 3); return; }               // unknown shape: KeyError in the reference
        if ((f[3] <= 0 && f[6] <= 0) || f[4] <= 0) { g_failed[g] = 1; return; }   // no S or no M: ([], [], [])
    }
    // parse + stable insertion sort by (qs, qe) (cp:263), in place in the group's slots of tmp_rows
    ParsedRow *__restrict__ rows = reinterpret_cast<ParsedRow *>(tmp_rows + 8ll * a);
    bool zero_len = false;
    for (int j = 0; j < nk; ++j) {
        ParsedRow p;
        parse_row(sa + 8ll * kept_idx[j], sa_nm[kept_idx[j]], rl, p);
        zero_len |= p.qe == p.qs;                                             // ZeroDivisionError at cp:268
        int k = j;
        while (k > 0) {
            const ParsedRow q = rows[k - 1];
            if (!(q.qs > p.qs || (q.qs == p.qs && q.qe > p.qe))) break;
            rows[k] = q;
            --k;
        }
        rows[k] = p;
    }
    if (zero_len) sa_report(err, vals[a], 4);
    n_kept[g] = nk;
}

__global__ void k_group_process(int n_groups, const int32_t *__restrict__ gstart, const int32_t *__restrict__ keys,
                                const int32_t *__restrict__ vals, const int32_t *__restrict__ sa,
                                const int32_t *__restrict__ sa_nm, const int32_t *__restrict__ first_primary,
                                const int32_t *__restrict__ rec_qlen, int32_t *__restrict__ kept_ws, int32_t *__restrict__ tmp_rows,
                                int32_t *__restrict__ n_kept, int32_t *__restrict__ g_first, int32_t *__restrict__ g_failed,
                                int32_t *__restrict__ err) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    group_process_one(g, gstart, keys, vals, sa, sa_nm, first_primary, rec_qlen, kept_ws, tmp_rows, n_kept, g_first, g_failed, err);
}

// The same with the number of groups read from device memory (coral_sa_table_async: nobody on the host has seen it yet).
// The grid covers `cap` (= n_sa >= the number of groups) slots; the slots behind the groups become empty groups whose
// key sorts behind every read, so the sort and the scan that follow run over `cap` entries and leave the reads where
// they are.
__global__ void k_group_process_n(const int32_t *__restrict__ n_groups_p, int cap, const int32_t *__restrict__ gstart,
                                  const int32_t *__restrict__ keys, const int32_t *__restrict__ vals, const int32_t *__restrict__ sa,
                                  const int32_t *__restrict__ sa_nm, const int32_t *__restrict__ first_primary,
                                  const int32_t *__restrict__ rec_qlen, int32_t *__restrict__ kept_ws, int32_t *__restrict__ tmp_rows,
                                  int32_t *__restrict__ n_kept, int32_t *__restrict__ g_first, int32_t *__restrict__ g_failed,
                                  int32_t *__restrict__ err) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= cap) return;
    const int n_groups = *n_groups_p < cap ? *n_groups_p : cap;
    if (g >= n_groups) {
        n_kept[g] = 0;
        g_failed[g] = 0;
        g_first[g] = INVALID_KEY;
        return;
    }
    group_process_one(g, gstart, keys, vals, sa, sa_nm, first_primary, rec_qlen, kept_ws, tmp_rows, n_kept, g_first, g_failed, err);
}

__global__ void k_order_counts(int n_groups, const int32_t *__restrict__ gf_sorted, const int32_t *__restrict__ g_sorted,
                               const int32_t *__restrict__ n_kept, int32_t *__restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_groups) cnt[i] = gf_sorted[i] != INVALID_KEY ? n_kept[g_sorted[i]] : 0;
}

__global__ void k_scatter(int n_reads, const int32_t *__restrict__ g_sorted, const int32_t *__restrict__ off,
                          const int32_t *__restrict__ gstart, const int32_t *__restrict__ keys,
                          const int32_t *__restrict__ n_kept, const int32_t *__restrict__ g_failed,
                          const int32_t *__restrict__ tmp_rows, int32_t *__restrict__ out_rows,
                          int32_t *__restrict__ out_name, int32_t *__restrict__ out_failed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    const int g = g_sorted[i];
    out_name[i] = keys[gstart[g]];
    out_failed[i] = g_failed[g];
    const int nk = n_kept[g];
    const int32_t *src = tmp_rows + 8ll * gstart[g];
    int32_t *dst = out_rows + 8ll * off[i];
    for (int j = 0; j < 8 * nk; ++j) dst[j] = src[j];
}

__global__ void k_read_length(int n_names, int32_t *__restrict__ fp, const int32_t *__restrict__ qlen, int32_t *__restrict__ rl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_names) return;
    const int v = fp[i];
    if (v == 0x7f7f7f7f) { fp[i] = INVALID_KEY; rl[i] = -1; } else rl[i] = qlen[v];
}

__global__ void k_iota(int n, int32_t *__restrict__ v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

__global__ void k_count_valid(int n, const int32_t *__restrict__ gf, int32_t *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && gf[i] != INVALID_KEY && (i == n - 1 || gf[i + 1] == INVALID_KEY)) out[0] = i + 1;
}

template <typename T>
static T *carve(char *&p, size_t n) {
    T *r = reinterpret_cast<T *>(p);
    p += (n * sizeof(T) + 255) / 256 * 256;
    return r;
}

extern "C" int coral_sa_table(int32_t n_rec, const int32_t *rec_tid, const int32_t *rec_flagmq, const int32_t *rec_qlen,
                              const int32_t *rec_name, int32_t n_names, int32_t n_sa, const int32_t *sa,
                              const int32_t *sa_nm, const int32_t *sa_rec, void *workspace, int64_t workspace_bytes,
                              int32_t *out_rows, int32_t *out_off, int32_t *out_name, int32_t *out_failed,
                              int32_t *out_read_length, int32_t *counts /* host [2]: n_reads, n_rows */, void *stream) {
    if (!counts) return sa_err(CORAL_ERR_ARG, "sa_table: counts is null");
    counts[0] = counts[1] = 0;
    if (n_rec < 0 || n_sa < 0 || n_names < 0) return sa_err(CORAL_ERR_ARG, "sa_table: negative size");
    hipStream_t s = (hipStream_t)stream;
    // ---- workspace layout (and its size)
    size_t cub_bytes = 0, b1 = 0, b2 = 0, b3 = 0;
    {
        int32_t *n32 = nullptr;
        hipcub::DeviceRadixSort::SortPairs(nullptr, b1, n32, n32, n32, n32, n_sa > 0 ? n_sa : 1, 0, 32, s);
        hipcub::DeviceScan::InclusiveSum(nullptr, b2, n32, n32, n_sa > 0 ? n_sa : 1, s);
        hipcub::DeviceScan::ExclusiveSum(nullptr, b3, n32, n32, n_sa > 0 ? n_sa + 1 : 1, s);
        cub_bytes = b1 > b2 ? b1 : b2;
        cub_bytes = cub_bytes > b3 ? cub_bytes : b3;
    }
    const size_t ns = (size_t)(n_sa > 0 ? n_sa : 1);
    size_t need = 0;
    {
        char *p = nullptr;
        carve<char>(p, cub_bytes);
        for (int k = 0; k < 13; ++k) carve<int32_t>(p, ns + 2);
        carve<int32_t>(p, 8 * ns);
        carve<int32_t>(p, (size_t)n_names + 1);
        need = (size_t)p;
    }
    if (!workspace || (size_t)workspace_bytes < need) {
        counts[0] = (int32_t)(need >> 20) + 1;          // MiB needed
        return sa_err(CORAL_ERR_CAPACITY, "sa_table: workspace too small");
    }
    if (out_read_length == nullptr) return sa_err(CORAL_ERR_ARG, "sa_table: null output");
    char *p = (char *)workspace;
    void *cub_tmp = carve<char>(p, cub_bytes);
    int32_t *keys = carve<int32_t>(p, ns + 2), *vals = carve<int32_t>(p, ns + 2), *keys_s = carve<int32_t>(p, ns + 2),
            *vals_s = carve<int32_t>(p, ns + 2), *head = carve<int32_t>(p, ns + 2), *gid = carve<int32_t>(p, ns + 2),
            *gstart = carve<int32_t>(p, ns + 2), *n_kept = carve<int32_t>(p, ns + 2), *g_first = carve<int32_t>(p, ns + 2),
            *g_failed = carve<int32_t>(p, ns + 2), *g_ids = carve<int32_t>(p, ns + 2), *scratch = carve<int32_t>(p, ns + 2),
            *kept_ws = carve<int32_t>(p, ns + 2);
    int32_t *tmp_rows = carve<int32_t>(p, 8 * ns);
    int32_t *first_primary = carve<int32_t>(p, (size_t)n_names + 1);
    const int B = 256;
    // ---- read_length = query_length of the first record with flag < 256 per name (ibg:142-143)
    (void)hipMemsetAsync(first_primary, 0x7f, sizeof(int32_t) * ((size_t)n_names + 1), s);      // 0x7f7f7f7f > any ordinal
    if (n_rec > 0) hipLaunchKernelGGL(k_first_primary, dim3((n_rec + B - 1) / B), dim3(B), 0, s, n_rec, rec_tid, rec_flagmq, rec_name, first_primary);
    // first_primary values of 0x7f7f7f7f mean "none": normalise to INVALID_KEY and produce read_length
    hipError_t e = hipSuccess;
    if (out_off) (void)hipMemsetAsync(out_off, 0, sizeof(int32_t), s);      // a table without reads still has its one offset
    if (n_names > 0) hipLaunchKernelGGL(k_read_length, dim3((n_names + B - 1) / B), dim3(B), 0, s, n_names, first_primary, rec_qlen, out_read_length);
    if (n_sa == 0) {
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e));
        return CORAL_OK;
    }
    if (!out_rows || !out_off || !out_name || !out_failed) return sa_err(CORAL_ERR_ARG, "sa_table: null output");
    const int G = (n_sa + B - 1) / B;
    int32_t *err = scratch;            // scratch[0] = error code, scratch[1..] reused below
    (void)hipMemsetAsync(err, 0, sizeof(int32_t), s);
    hipLaunchKernelGGL(k_row_keys, dim3(G), dim3(B), 0, s, n_sa, sa_rec, rec_tid, rec_name, keys, vals);
    size_t tb = cub_bytes;
    hipcub::DeviceRadixSort::SortPairs(cub_tmp, tb, keys, keys_s, vals, vals_s, n_sa, 0, 32, s);
    hipLaunchKernelGGL(k_heads, dim3(G), dim3(B), 0, s, n_sa, keys_s, head);
    tb = cub_bytes;
    hipcub::DeviceScan::InclusiveSum(cub_tmp, tb, head, gid, n_sa, s);
    hipLaunchKernelGGL(k_group_starts, dim3(G), dim3(B), 0, s, n_sa, head, gid, gstart);
    int32_t n_groups = 0;
    e = hipMemcpyAsync(&n_groups, gid + (n_sa - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e));
    const int GG = (n_groups + B - 1) / B;
    hipLaunchKernelGGL(k_group_process, dim3(GG), dim3(B), 0, s, n_groups, gstart, keys_s, vals_s, sa, sa_nm, first_primary,
                       rec_qlen, kept_ws, tmp_rows, n_kept, g_first, g_failed, err);
    // ---- reads in the reference's dict order = by first SA-bearing record = by their first SA row
    hipLaunchKernelGGL(k_iota, dim3(GG), dim3(B), 0, s, n_groups, g_ids);
    int32_t *gf_sorted = keys, *g_sorted = vals;          // the unsorted row keys are no longer needed
    tb = cub_bytes;
    hipcub::DeviceRadixSort::SortPairs(cub_tmp, tb, g_first, gf_sorted, g_ids, g_sorted, n_groups, 0, 32, s);
    int32_t *cnt = head, *off = gid;                      // reuse
    hipLaunchKernelGGL(k_order_counts, dim3(GG), dim3(B), 0, s, n_groups, gf_sorted, g_sorted, n_kept, cnt);
    (void)hipMemsetAsync(cnt + n_groups, 0, sizeof(int32_t), s);
    tb = cub_bytes;
    hipcub::DeviceScan::ExclusiveSum(cub_tmp, tb, cnt, off, n_groups + 1, s);
    // number of reads = groups with a valid key (they sort first)
    (void)hipMemsetAsync(scratch + 1, 0, sizeof(int32_t), s);
    hipLaunchKernelGGL(k_count_valid, dim3(GG), dim3(B), 0, s, n_groups, gf_sorted, scratch + 1);
    int32_t h[2] = {0, 0};
    e = hipMemcpyAsync(h, scratch, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    int32_t n_rows = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&n_rows, off + n_groups, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e));
    const int code = sa_error_code(h[0]);                // of the first offending read in table order
    if (code == 3) return sa_err(CORAL_ERR_FORMAT, "sa_table: SA CIGAR shape outside SM/MS/SMS/SMD/MDS/SMDS/SMI/MIS/SMIS");
    if (code == 4) return sa_err(CORAL_ERR_ZERODIV, "sa_table: zero-length query interval (ZeroDivisionError in the reference)");
    const int n_reads = h[1];
    if (n_reads > 0) {
        hipLaunchKernelGGL(k_scatter, dim3((n_reads + B - 1) / B), dim3(B), 0, s, n_reads, g_sorted, off, gstart, keys_s, n_kept,
                           g_failed, tmp_rows, out_rows, out_name, out_failed);
        e = hipMemcpyAsync(out_off, off, sizeof(int32_t) * ((size_t)n_reads + 1), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e));
    }
    counts[0] = n_reads;
    counts[1] = n_rows;
    return CORAL_OK;
}

// ---------------------------------------------------------------------------------------------
// coral_hash_rows — hash_alignment_to_seg (/root/reference/src/infer_breakpoint_graph.py:181-210) on the SA table's
// device rows: the CN segment holding each end of every local alignment (the reference's two IntervalTree point queries
// per alignment) and the inverted index (contig, segment) -> alignments in the reference's append order.
//   k_hash_rows: one thread per table row, two binary searches over the (contig, start)-sorted disjoint segment table;
//   the up to two (segment, row) entries of a row get the key contig << 32 | segment, and ONE stable radix sort of the
//   keys (values = 2 * row + end, i.e. already in append order) yields every per-segment list in order.
// ---------------------------------------------------------------------------------------------
#define HASH_INVALID 0x7fffffffffffffffLL

__device__ __forceinline__ int seg_lookup(const int32_t *__restrict__ seg_tid, const int32_t *__restrict__ seg_start,
                                          const int32_t *__restrict__ seg_end, const int32_t *__restrict__ seg_idx, int n_seg,
                                          int t, int p) {
    int lo = 0, hi = n_seg;                 // last segment with (tid, start) <= (t, p)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int mt = seg_tid[mid];
        if (mt < t || (mt == t && seg_start[mid] <= p)) lo = mid + 1; else hi = mid;
    }
    const int k = lo - 1;
    return (k >= 0 && seg_tid[k] == t && p < seg_end[k]) ? seg_idx[k] : -1;
}

__global__ __launch_bounds__(256) void k_hash_rows(int n_rows, const int32_t *__restrict__ rows, int n_seg,
                                                   const int32_t *__restrict__ seg_tid, const int32_t *__restrict__ seg_start,
                                                   const int32_t *__restrict__ seg_end, const int32_t *__restrict__ seg_idx,
                                                   const int32_t *__restrict__ tid_has_segs, int n_tid,
                                                   int32_t *__restrict__ cni0, int32_t *__restrict__ cni1,
                                                   long long *__restrict__ keys, int32_t *__restrict__ vals,
                                                   uint32_t *__restrict__ n_valid) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    int nv = 0;
    if (r < n_rows) {
        const int32_t *f = rows + 8ll * r;
        const int t = f[2], a = f[3], b = f[4];
        int c0 = -3, c1 = -3;                                  // -3: the contig has no CN segments (ibg:210: set([-1]))
        if (t >= 0 && t < n_tid && tid_has_segs[t]) {
            c0 = seg_lookup(seg_tid, seg_start, seg_end, seg_idx, n_seg, t, a < b ? a : b);
            c1 = seg_lookup(seg_tid, seg_start, seg_end, seg_idx, n_seg, t, a < b ? b : a);
        }
        cni0[r] = c0;
        cni1[r] = c1;
        const bool v0 = c0 >= 0, v1 = c1 >= 0 && c1 != c0;
        keys[2ll * r] = v0 ? (((long long)t << 32) | (long long)c0) : HASH_INVALID;
        keys[2ll * r + 1] = v1 ? (((long long)t << 32) | (long long)c1) : HASH_INVALID;
        vals[2ll * r] = 2 * r;
        vals[2ll * r + 1] = 2 * r + 1;
        nv = (v0 ? 1 : 0) + (v1 ? 1 : 0);
    }
    // one atomic per wave
    for (int d = 32; d > 0; d >>= 1) nv += __shfl_xor(nv, d);
    if ((threadIdx.x & 63) == 0 && nv) atomicAdd(n_valid, (uint32_t)nv);
}

__global__ void k_hash_finish(int n, const int32_t *__restrict__ vals_sorted, int32_t *__restrict__ e_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) e_row[i] = vals_sorted[i] >> 1;
}

extern "C" int coral_hash_rows(int32_t n_rows, const int32_t *rows, int32_t n_seg, const int32_t *seg_tid,
                               const int32_t *seg_start, const int32_t *seg_end, const int32_t *seg_idx,
                               const int32_t *tid_has_segs, int32_t n_tid, void *workspace, int64_t workspace_bytes,
                               int32_t *cni0, int32_t *cni1, int64_t *e_key, int32_t *e_row, int32_t *n_ent, void *stream) {
    if (!n_ent) return sa_err(CORAL_ERR_ARG, "hash_rows: n_ent is null");
    *n_ent = 0;
    if (n_rows < 0 || n_seg < 0 || n_tid < 0) return sa_err(CORAL_ERR_ARG, "hash_rows: negative size");
    if (n_rows == 0) return CORAL_OK;
    if (!rows || !tid_has_segs || !cni0 || !cni1 || !e_key || !e_row || (n_seg > 0 && (!seg_tid || !seg_start || !seg_end || !seg_idx)))
        return sa_err(CORAL_ERR_ARG, "hash_rows: null argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t ne = 2 * (size_t)n_rows;
    size_t cub_bytes = 0;
    {
        long long *k64 = nullptr;
        int32_t *v32 = nullptr;
        hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, k64, k64, v32, v32, (int)ne, 0, 63, s);
    }
    size_t need;
    {
        char *p = nullptr;
        carve<char>(p, cub_bytes);
        carve<long long>(p, ne);
        carve<int32_t>(p, ne);
        carve<int32_t>(p, ne);
        carve<uint32_t>(p, 4);
        need = (size_t)p;
    }
    if (!workspace || (size_t)workspace_bytes < need) {
        *n_ent = (int32_t)(need >> 20) + 1;               // MiB needed
        return sa_err(CORAL_ERR_CAPACITY, "hash_rows: workspace too small");
    }
    char *p = (char *)workspace;
    void *cub_tmp = carve<char>(p, cub_bytes);
    long long *keys = carve<long long>(p, ne);
    int32_t *vals = carve<int32_t>(p, ne), *vals_s = carve<int32_t>(p, ne);
    uint32_t *counter = carve<uint32_t>(p, 4);
    (void)hipMemsetAsync(counter, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(k_hash_rows, dim3((n_rows + 255) / 256), dim3(256), 0, s, (int)n_rows, rows, (int)n_seg, seg_tid, seg_start,
                       seg_end, seg_idx, tid_has_segs, (int)n_tid, cni0, cni1, keys, vals, counter);
    size_t tb = cub_bytes;
    // sorted keys go straight to e_key; the invalid entries (key 2^63 - 1) sort behind every valid one
    hipcub::DeviceRadixSort::SortPairs(cub_tmp, tb, keys, reinterpret_cast<long long *>(e_key), vals, vals_s, (int)ne, 0, 63, s);
    hipLaunchKernelGGL(k_hash_finish, dim3((int)((ne + 255) / 256)), dim3(256), 0, s, (int)ne, vals_s, e_row);
    uint32_t h = 0;
    hipError_t e = hipMemcpyAsync(&h, counter, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e));
    *n_ent = (int32_t)h;
    return CORAL_OK;
}

// ---------------------------------------------------------------------------------------------
// Device queries of a graph build as ONE native call each: coral_segment_coverage_host, coral_hash_rows_host,
// coral_point_cover_host.  The results are small and the inputs are a few hundred bytes of host data plus arrays already in
// HBM, so a query stages its arguments (and the zeros its counters start from) in pinned memory, sends them with one copy,
// queues its kernels on the caller's stream, copies the result back and waits once (twice where the size of the result is
// only known on the device).
//
// The query arena — one pinned host block and one device block per device, owned by the library — holds the arguments, the
// scratch and the small results.  It grows when a call needs more than it has and is reused otherwise: in steady state a
// query allocates nothing.  A call holds the arena's mutex from staging to its last wait, so nothing a call returns may
// point into the arena; large results land in buffers of the caller's.
// ---------------------------------------------------------------------------------------------
#define QUERY_MAX_DEVICES 16
#define QUERY_COUNTER_BYTES 256          // a device counter that kernels add to keeps clear of the tables staged behind it
struct QueryArena {
    char *host;
    size_t host_bytes;
    char *dev;
    size_t dev_bytes;
};
static std::mutex g_arena_mu;
static QueryArena g_arena[QUERY_MAX_DEVICES];

// the device of a stream (the current one for the null stream), made current for the duration of a call
struct QueryDevice {
    int prev = -1, dev = -1;
    explicit QueryDevice(hipStream_t s) {
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; return; }
        dev = prev;
        hipDevice_t d;
        if (s && hipStreamGetDevice(s, &d) == hipSuccess) dev = (int)d;
        if (dev != prev && hipSetDevice(dev) != hipSuccess) dev = -1;
    }
    ~QueryDevice() {
        if (prev >= 0 && dev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
};

// the arena of the current device with at least the asked sizes; the previous call on it has ended (callers hold the mutex)
static int arena_reserve(int dev, size_t host_need, size_t dev_need, QueryArena **out) {
    if (dev < 0 || dev >= QUERY_MAX_DEVICES) return sa_err(CORAL_ERR_ARG, "query arena: device ordinal out of range");
    QueryArena &a = g_arena[dev];
    if (a.host_bytes < host_need) {
        if (a.host) (void)hipHostFree(a.host);
        a.host = nullptr;
        a.host_bytes = 0;
        const size_t want = coral_plan::round_up(host_need + host_need / 2, 1 << 20);
        hipError_t e = hipHostMalloc((void **)&a.host, want, hipHostMallocDefault);
        if (e != hipSuccess) { a.host = nullptr; return sa_err(CORAL_ERR_HIP, hipGetErrorString(e)); }
        a.host_bytes = want;
    }
    if (a.dev_bytes < dev_need) {
        if (a.dev) (void)hipFree(a.dev);
        a.dev = nullptr;
        a.dev_bytes = 0;
        const size_t want = coral_plan::round_up(dev_need + dev_need / 2, 4 << 20);
        hipError_t e = hipMalloc((void **)&a.dev, want);
        if (e != hipSuccess) { a.dev = nullptr; return sa_err(CORAL_ERR_HIP, hipGetErrorString(e)); }
        a.dev_bytes = want;
    }
    *out = &a;
    return CORAL_OK;
}

extern "C" int coral_query_arena_release(void) {
    std::lock_guard<std::mutex> lock(g_arena_mu);
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (int d = 0; d < QUERY_MAX_DEVICES; ++d) {
        QueryArena &a = g_arena[d];
        if (!a.host && !a.dev) continue;
        (void)hipSetDevice(d);
        if (a.host) (void)hipHostFree(a.host);
        if (a.dev) (void)hipFree(a.dev);
        a = QueryArena{nullptr, 0, nullptr, 0};
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    return CORAL_OK;
}

#define QUERY_HIP(call)                                                          \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e_)); \
    } while (0)

// ---- coral_segment_coverage_host -------------------------------------------------------------
extern "C" int coral_segment_coverage_host(const coral_records_t *rec, const int32_t *summary, int32_t n_seg,
                                           const int64_t *segs, int64_t *n_reads, int64_t *n_bases, void *stream) {
    if (!rec || n_seg < 0) return sa_err(CORAL_ERR_ARG, "segment_coverage_host: bad argument");
    if (n_seg == 0) return CORAL_OK;
    if (!segs || !n_reads || !n_bases) return sa_err(CORAL_ERR_ARG, "segment_coverage_host: null argument");
    for (int32_t i = 0; i < n_seg; ++i) n_reads[i] = n_bases[i] = 0;
    if (rec->n_rec <= 0) return CORAL_OK;
    if (!summary) return sa_err(CORAL_ERR_ARG, "segment_coverage_host: null summary");
    hipStream_t s = (hipStream_t)stream;
    const coral_plan::BatchPlan plan = coral_plan::plan_disjoint_batches(segs, n_seg);
    const int nb = plan.n_batches();
    const coral_plan::CoverageLayout lay = coral_plan::coverage_layout(n_seg, nb);
    const size_t strad_off = lay.bytes;                                   // device only: the straddler list, n_rec words
    const size_t dev_need = strad_off + sizeof(uint32_t) * (size_t)rec->n_rec;
    std::lock_guard<std::mutex> lock(g_arena_mu);
    QueryDevice qd(s);
    QueryArena *A = nullptr;
    int rc = arena_reserve(qd.dev, lay.bytes, dev_need, &A);
    if (rc) return rc;
    memset(A->host, 0, lay.bytes);                                        // the sums and the counters start at zero
    int32_t *h_tab = reinterpret_cast<int32_t *>(A->host + lay.tables);
    for (int32_t k = 0; k < n_seg; ++k) {
        const int64_t *sg = segs + 3 * (size_t)plan.order[(size_t)k];
        h_tab[k] = (int32_t)sg[0];
        h_tab[(size_t)n_seg + k] = (int32_t)sg[1];
        h_tab[2 * (size_t)n_seg + k] = (int32_t)sg[2];
    }
    QUERY_HIP(hipMemcpyAsync(A->dev, A->host, lay.bytes, hipMemcpyHostToDevice, s));
    const int32_t *d_tab = reinterpret_cast<const int32_t *>(A->dev + lay.tables);
    unsigned long long *d_sums = reinterpret_cast<unsigned long long *>(A->dev + lay.sums);
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(A->dev + lay.counts);
    uint32_t *d_strad = reinterpret_cast<uint32_t *>(A->dev + strad_off);
    for (int b = 0; b < nb; ++b) {
        const int32_t o = plan.batch_off[(size_t)b], n = plan.batch_off[(size_t)b + 1] - o;
        rc = coral_segment_coverage(rec, summary, n, d_tab + o, d_tab + (size_t)n_seg + o, d_tab + 2 * (size_t)n_seg + o, d_sums + o,
                                    d_sums + (size_t)n_seg + o, d_strad, d_counts + b, stream);
        if (rc) {
            (void)hipStreamSynchronize(s);                                // the arena is free again when the lock is
            return sa_err(rc, coral_last_error());
        }
    }
    hipError_t e = hipMemcpyAsync(A->host + lay.sums, A->dev + lay.sums, 2 * sizeof(uint64_t) * (size_t)n_seg, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e != hipSuccess || e2 != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e != hipSuccess ? e : e2));
    const int64_t *h_sums = reinterpret_cast<const int64_t *>(A->host + lay.sums);
    for (int32_t k = 0; k < n_seg; ++k) {
        n_reads[plan.order[(size_t)k]] = h_sums[k];
        n_bases[plan.order[(size_t)k]] = h_sums[(size_t)n_seg + k];
    }
    return CORAL_OK;
}

// ---- coral_hash_rows_host ----------------------------------------------------------------------
// cni0 / cni1 and the row of every entry, widened to the int64 the host logic indexes with (one launch for all three)
__global__ void k_hash_widen(int n_rows, const int32_t *__restrict__ c0, const int32_t *__restrict__ c1,
                             const int32_t *__restrict__ vals_sorted, long long *__restrict__ c0w, long long *__restrict__ c1w,
                             long long *__restrict__ e_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rows) {
        c0w[i] = c0[i];
        c1w[i] = c1[i];
    }
    if (i < 2 * n_rows) e_row[i] = vals_sorted[i] >> 1;
}

extern "C" int coral_hash_rows_host(int32_t n_rows, const int32_t *rows, int32_t n_seg, const int32_t *seg, const int32_t *tid_has_segs,
                                    int32_t n_tid, int64_t *cni0, int64_t *cni1, int64_t *e_key, int64_t *e_row, int32_t *n_ent,
                                    void *stream) {
    if (!n_ent) return sa_err(CORAL_ERR_ARG, "hash_rows_host: n_ent is null");
    *n_ent = 0;
    if (n_rows < 0 || n_seg < 0 || n_tid < 0) return sa_err(CORAL_ERR_ARG, "hash_rows_host: negative size");
    if (n_rows == 0) return CORAL_OK;
    if (n_rows > 0x3fffffff) return sa_err(CORAL_ERR_ARG, "hash_rows_host: too many rows");
    if (!rows || !cni0 || !cni1 || !e_key || !e_row || (n_seg > 0 && !seg) || (n_tid > 0 && !tid_has_segs))
        return sa_err(CORAL_ERR_ARG, "hash_rows_host: null argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t nr = (size_t)n_rows, ne = 2 * nr, ns = (size_t)n_seg, nt = (size_t)n_tid;
    size_t cub_bytes = 0;
    {
        long long *k64 = nullptr;
        int32_t *v32 = nullptr;
        hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, k64, k64, v32, v32, (int)ne, 0, 63, s);
    }
    // staged block (host and device alike): the counter (zero; a line of its own: every wave adds to it), the segment table,
    // the contig flags
    const size_t arg_bytes = coral_plan::round_up(QUERY_COUNTER_BYTES + sizeof(int32_t) * (4 * ns + nt + 1), 256);
    size_t dev_need;
    {
        char *p = nullptr;
        carve<char>(p, arg_bytes);
        carve<char>(p, cub_bytes);
        carve<long long>(p, ne);       // keys
        carve<long long>(p, ne);       // keys, sorted
        carve<int32_t>(p, ne);         // values
        carve<int32_t>(p, ne);         // values, sorted
        carve<int32_t>(p, nr);         // cni0
        carve<int32_t>(p, nr);         // cni1
        carve<long long>(p, nr);       // cni0, widened
        carve<long long>(p, nr);       // cni1, widened
        carve<long long>(p, ne);       // entry rows, widened
        dev_need = (size_t)p;
    }
    std::lock_guard<std::mutex> lock(g_arena_mu);
    QueryDevice qd(s);
    QueryArena *A = nullptr;
    int rc = arena_reserve(qd.dev, arg_bytes, dev_need, &A);
    if (rc) return rc;
    memset(A->host, 0, QUERY_COUNTER_BYTES);
    int32_t *h_seg = reinterpret_cast<int32_t *>(A->host + QUERY_COUNTER_BYTES);
    if (ns) memcpy(h_seg, seg, sizeof(int32_t) * 4 * ns);
    if (nt) memcpy(h_seg + 4 * ns, tid_has_segs, sizeof(int32_t) * nt);
    char *p = A->dev;
    char *d_args = carve<char>(p, arg_bytes);
    void *cub_tmp = carve<char>(p, cub_bytes);
    long long *keys = carve<long long>(p, ne), *keys_s = carve<long long>(p, ne);
    int32_t *vals = carve<int32_t>(p, ne), *vals_s = carve<int32_t>(p, ne), *c0 = carve<int32_t>(p, nr), *c1 = carve<int32_t>(p, nr);
    long long *c0w = carve<long long>(p, nr), *c1w = carve<long long>(p, nr), *rows_w = carve<long long>(p, ne);
    uint32_t *counter = reinterpret_cast<uint32_t *>(d_args);
    const int32_t *d_seg = reinterpret_cast<const int32_t *>(d_args + QUERY_COUNTER_BYTES);
    QUERY_HIP(hipMemcpyAsync(d_args, A->host, arg_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_hash_rows, dim3((n_rows + 255) / 256), dim3(256), 0, s, (int)n_rows, rows, (int)n_seg, d_seg, d_seg + ns,
                       d_seg + 2 * ns, d_seg + 3 * ns, d_seg + 4 * ns, (int)n_tid, c0, c1, keys, vals, counter);
    size_t tb = cub_bytes;
    hipcub::DeviceRadixSort::SortPairs(cub_tmp, tb, keys, keys_s, vals, vals_s, (int)ne, 0, 63, s);
    hipLaunchKernelGGL(k_hash_widen, dim3((int)((ne + 255) / 256)), dim3(256), 0, s, (int)n_rows, c0, c1, vals_s, c0w, c1w, rows_w);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cni0, c0w, sizeof(int64_t) * nr, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cni1, c1w, sizeof(int64_t) * nr, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(A->host, counter, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    hipError_t e2 = hipStreamSynchronize(s);                              // wait 1: the entry count (and the two columns)
    if (e != hipSuccess || e2 != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e != hipSuccess ? e : e2));
    const size_t k = *reinterpret_cast<const uint32_t *>(A->host);
    if (k > ne) return sa_err(CORAL_ERR_HIP, "hash_rows_host: entry count beyond its bound");
    if (k) {
        e = hipMemcpyAsync(e_key, keys_s, sizeof(int64_t) * k, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(e_row, rows_w, sizeof(int64_t) * k, hipMemcpyDeviceToHost, s);
        e2 = hipStreamSynchronize(s);                                     // wait 2: exactly k entries
        if (e != hipSuccess || e2 != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e != hipSuccess ? e : e2));
    }
    *n_ent = (int32_t)k;
    return CORAL_OK;
}

// ---- coral_point_cover_host --------------------------------------------------------------------
// The (point, record) pairs are sorted; per point the start of its slice (bounds[n_pts] = the number of pairs) and the
// record ordinal of every pair as int32.  n_pairs comes from device memory, pair_cap by value: nothing is read past either.
__global__ void k_point_finish(const unsigned long long *__restrict__ sorted, const uint32_t *__restrict__ n_pairs, uint32_t pair_cap,
                               int n_pts, long long *__restrict__ bounds, int32_t *__restrict__ rec) {
    const uint32_t cnt = *n_pairs;
    const long long n = cnt < pair_cap ? cnt : pair_cap;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rec[i] = (int32_t)(uint32_t)(sorted[i] & 0xFFFFFFFFull);
    if (i <= n_pts) {
        const unsigned long long key = (unsigned long long)i << 32;       // first pair of point i or a later one
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (sorted[mid] < key) lo = mid + 1; else hi = mid;
        }
        bounds[i] = lo;
    }
}

extern "C" int coral_point_cover_host(const coral_records_t *rec, int32_t n_pts, const int32_t *pt_tid, const int32_t *pt_pos,
                                      int32_t max_span, uint32_t pair_cap, int32_t *rec_out, int64_t *bounds, uint32_t *n_pairs,
                                      void *stream) {
    if (!n_pairs) return sa_err(CORAL_ERR_ARG, "point_cover_host: n_pairs is null");
    *n_pairs = 0;
    if (!rec || n_pts < 0) return sa_err(CORAL_ERR_ARG, "point_cover_host: bad argument");
    if (n_pts > 0 && (!pt_tid || !pt_pos)) return sa_err(CORAL_ERR_ARG, "point_cover_host: null argument");
    if (!bounds || (pair_cap && !rec_out)) return sa_err(CORAL_ERR_ARG, "point_cover_host: null output");
    if (pair_cap == 0 || pair_cap > 0x7fffffffu) return sa_err(CORAL_ERR_ARG, "point_cover_host: pair_cap outside 1 .. 2^31 - 1");
    for (int32_t i = 0; i <= n_pts; ++i) bounds[i] = 0;
    if (n_pts == 0 || rec->n_rec <= 0) return CORAL_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t np = (size_t)n_pts, cap = (size_t)pair_cap;
    int point_bits = 1;
    while (point_bits < 31 && (1ll << point_bits) < (long long)n_pts) ++point_bits;
    size_t cub_bytes = 0;
    {
        unsigned long long *k64 = nullptr;
        hipcub::DeviceRadixSort::SortKeys(nullptr, cub_bytes, k64, k64, (int)cap, 0, 32 + point_bits, s);
    }
    // staged block: the pair counter (zero), the points; behind it on the host the bounds come back
    const size_t arg_bytes = coral_plan::round_up(QUERY_COUNTER_BYTES + 2 * sizeof(int32_t) * np, 256);
    const size_t bounds_bytes = coral_plan::round_up(sizeof(int64_t) * (np + 1), 256);
    size_t dev_need;
    {
        char *p = nullptr;
        carve<char>(p, arg_bytes);
        carve<char>(p, cub_bytes);
        carve<unsigned long long>(p, cap);
        carve<unsigned long long>(p, cap);
        carve<long long>(p, np + 1);
        carve<int32_t>(p, cap);
        dev_need = (size_t)p;
    }
    std::lock_guard<std::mutex> lock(g_arena_mu);
    QueryDevice qd(s);
    QueryArena *A = nullptr;
    int rc = arena_reserve(qd.dev, arg_bytes + bounds_bytes, dev_need, &A);
    if (rc) return rc;
    memset(A->host, 0, QUERY_COUNTER_BYTES);
    int32_t *h_pts = reinterpret_cast<int32_t *>(A->host + QUERY_COUNTER_BYTES);
    memcpy(h_pts, pt_tid, sizeof(int32_t) * np);
    memcpy(h_pts + np, pt_pos, sizeof(int32_t) * np);
    char *p = A->dev;
    char *d_args = carve<char>(p, arg_bytes);
    void *cub_tmp = carve<char>(p, cub_bytes);
    unsigned long long *pairs = carve<unsigned long long>(p, cap), *sorted = carve<unsigned long long>(p, cap);
    long long *d_bounds = carve<long long>(p, np + 1);
    int32_t *d_rec = carve<int32_t>(p, cap);
    uint32_t *counter = reinterpret_cast<uint32_t *>(d_args);
    const int32_t *d_pts = reinterpret_cast<const int32_t *>(d_args + QUERY_COUNTER_BYTES);
    QUERY_HIP(hipMemcpyAsync(d_args, A->host, arg_bytes, hipMemcpyHostToDevice, s));
    rc = coral_point_cover(rec, n_pts, d_pts, d_pts + np, max_span, pairs, counter, pair_cap, stream);
    hipError_t e = hipMemcpyAsync(A->host, counter, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    hipError_t e2 = hipStreamSynchronize(s);                              // wait 1: the number of pairs
    if (rc) return sa_err(rc, coral_last_error());
    if (e != hipSuccess || e2 != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e != hipSuccess ? e : e2));
    const uint32_t k = *reinterpret_cast<const uint32_t *>(A->host);
    *n_pairs = k;
    if (k > pair_cap) return sa_err(CORAL_ERR_CAPACITY, "point_cover_host: more pairs than pair_cap");
    if (k == 0) return CORAL_OK;                                          // (bounds are all zero)
    size_t tb = cub_bytes;
    hipcub::DeviceRadixSort::SortKeys(cub_tmp, tb, pairs, sorted, (int)k, 0, 32 + point_bits, s);
    const long long threads = (long long)k > (long long)n_pts + 1 ? (long long)k : (long long)n_pts + 1;
    hipLaunchKernelGGL(k_point_finish, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, sorted, counter, pair_cap, (int)n_pts,
                       d_bounds, d_rec);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(rec_out, d_rec, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(A->host + arg_bytes, d_bounds, sizeof(int64_t) * (np + 1), hipMemcpyDeviceToHost, s);
    e2 = hipStreamSynchronize(s);                                         // wait 2: exactly k record ordinals and the bounds
    if (e != hipSuccess || e2 != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e != hipSuccess ? e : e2));
    memcpy(bounds, A->host + arg_bytes, sizeof(int64_t) * (np + 1));
    return CORAL_OK;
}

// ---- coral_sa_table_async ----------------------------------------------------------------------
// coral_sa_table + coral_bp_pair_table as ONE chain on the stream, without a host wait at all: the number of groups, of reads
// and of rows stay in device memory (d_cnt = n_reads, n_rows, error field of sa_report - its code when the chain ends -, n_groups) and the kernels that need them
// read them there; grids, the second sort and the scan are sized by n_sa, which bounds all three.  The call returns when the chain is
// queued; the caller puts other work behind it (the CIGAR scan of a build) and looks at the counts when its stream is through.
__global__ void k_group_starts_n(int n, const int32_t *__restrict__ head, const int32_t *__restrict__ gid_incl,
                                 int32_t *__restrict__ gstart, int32_t *__restrict__ d_cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) d_cnt[0] = d_cnt[1] = d_cnt[2] = 0;         // reads, rows, error code: the kernels behind this one set them
    if (i < n && head[i]) gstart[gid_incl[i] - 1] = i;
    if (i == n - 1) {
        gstart[gid_incl[i]] = n;
        d_cnt[3] = gid_incl[i];
    }
}

// k_scatter for d_cnt[0] reads (grid over cap >= that).  The offsets leave as they are, all cap + 1 of them: behind the
// last read every entry equals the number of rows, so a consumer that walks `cap` reads finds the ones behind the last
// empty (coral_bp_pair_table is launched that way, with n_sa for the number of reads).
__global__ void k_scatter_n(int cap, int32_t *__restrict__ d_cnt, const int32_t *__restrict__ g_sorted, const int32_t *__restrict__ off,
                            const int32_t *__restrict__ gstart, const int32_t *__restrict__ keys, const int32_t *__restrict__ n_kept,
                            const int32_t *__restrict__ g_failed, const int32_t *__restrict__ tmp_rows, int32_t *__restrict__ out_rows,
                            int32_t *__restrict__ out_off, int32_t *__restrict__ out_name, int32_t *__restrict__ out_failed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    out_off[i] = off[i];
    if (i == cap - 1) {
        out_off[cap] = off[cap];
        d_cnt[1] = off[cap];                                // the number of rows
    }
    const int n_reads = d_cnt[0] < cap ? d_cnt[0] : cap;
    if (i >= n_reads) return;
    const int g = g_sorted[i];
    out_name[i] = keys[gstart[g]];
    out_failed[i] = g_failed[g];
    const int nk = n_kept[g];
    const int32_t *src = tmp_rows + 8ll * gstart[g];
    int32_t *dst = out_rows + 8ll * off[i];
    for (int j = 0; j < 8 * nk; ++j) dst[j] = src[j];
}

// The table in the layout the host logic reads: the eight columns of the rows one after the other (column stride = the
// number of rows) and the per-read arrays, all widened to int64 (failed: one byte, 0 / 1).
// The last kernel of the chain also turns the error field of sa_report into the code the caller reads (d_cnt[2] = 0, 3 or 4:
// no other thread of this kernel looks at it).
__global__ void k_table_host_layout(int cap, int32_t *__restrict__ d_cnt, const int32_t *__restrict__ rows,
                                    const int32_t *__restrict__ off, const int32_t *__restrict__ name, const int32_t *__restrict__ failed,
                                    long long *__restrict__ cols, long long *__restrict__ off_w, long long *__restrict__ name_w,
                                    uint8_t *__restrict__ failed_b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_reads = d_cnt[0] < cap ? d_cnt[0] : cap, n_rows = d_cnt[1] < cap ? d_cnt[1] : cap;
    if (i == 0) d_cnt[2] = sa_error_code(d_cnt[2]);
    if (i < n_rows) {
        const int4 lo = reinterpret_cast<const int4 *>(rows)[2ll * i], hi = reinterpret_cast<const int4 *>(rows)[2ll * i + 1];
        const int v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) cols[(long long)c * n_rows + i] = v[c];
    }
    if (i <= n_reads) off_w[i] = off[i];
    if (i < n_reads) {
        name_w[i] = name[i];
        failed_b[i] = failed[i] ? 1 : 0;
    }
}

extern "C" int coral_sa_table_async(int32_t n_rec, const int32_t *rec_tid, const int32_t *rec_flagmq, const int32_t *rec_qlen,
                                    const int32_t *rec_name, int32_t n_names, int32_t n_sa, const int32_t *sa, const int32_t *sa_nm,
                                    const int32_t *sa_rec, void *workspace, int64_t workspace_bytes, int32_t *out_rows,
                                    int32_t *out_off, int32_t *out_read_length, const int32_t *chr_rank, int32_t n_tid,
                                    int32_t min_bp_match_cutoff, int32_t min_mapq, int32_t gap_, int32_t gap_mapq, int32_t *pairs,
                                    int64_t *cols, int64_t *off_w, int64_t *name_w, uint8_t *failed_b, int32_t *counts, void *stream) {
    if (!counts) return sa_err(CORAL_ERR_ARG, "sa_table_async: counts is null");
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n_rec < 0 || n_sa < 0 || n_names < 0 || n_tid < 0) return sa_err(CORAL_ERR_ARG, "sa_table_async: negative size");
    hipStream_t s = (hipStream_t)stream;
    // ---- workspace layout: coral_sa_table's, and the two per-read arrays that stay on the device
    size_t cub_bytes = 0, b1 = 0, b2 = 0, b3 = 0;
    {
        int32_t *n32 = nullptr;
        hipcub::DeviceRadixSort::SortPairs(nullptr, b1, n32, n32, n32, n32, n_sa > 0 ? n_sa : 1, 0, 32, s);
        hipcub::DeviceScan::InclusiveSum(nullptr, b2, n32, n32, n_sa > 0 ? n_sa : 1, s);
        hipcub::DeviceScan::ExclusiveSum(nullptr, b3, n32, n32, n_sa > 0 ? n_sa + 1 : 1, s);
        cub_bytes = b1 > b2 ? b1 : b2;
        cub_bytes = cub_bytes > b3 ? cub_bytes : b3;
    }
    const size_t ns = (size_t)(n_sa > 0 ? n_sa : 1);
    size_t need = 0;
    {
        char *p = nullptr;
        carve<char>(p, cub_bytes);
        for (int k = 0; k < 14; ++k) carve<int32_t>(p, ns + 2);
        carve<int32_t>(p, 8 * ns);
        carve<int32_t>(p, (size_t)n_names + 1);
        carve<int32_t>(p, 4);
        need = (size_t)p;
    }
    if (!workspace || (size_t)workspace_bytes < need) {
        counts[0] = (int32_t)(need >> 20) + 1;          // MiB needed
        return sa_err(CORAL_ERR_CAPACITY, "sa_table_async: workspace too small");
    }
    if (out_read_length == nullptr) return sa_err(CORAL_ERR_ARG, "sa_table_async: null output");
    if (n_sa > 0 && (!out_rows || !out_off || !pairs || !cols || !off_w || !name_w || !failed_b || (n_tid > 0 && !chr_rank)))
        return sa_err(CORAL_ERR_ARG, "sa_table_async: null argument");
    if (((uintptr_t)out_rows) & 15u) return sa_err(CORAL_ERR_ARG, "sa_table_async: out_rows must be 16-byte aligned");
    char *p = (char *)workspace;
    void *cub_tmp = carve<char>(p, cub_bytes);
    int32_t *keys = carve<int32_t>(p, ns + 2), *vals = carve<int32_t>(p, ns + 2), *keys_s = carve<int32_t>(p, ns + 2),
            *vals_s = carve<int32_t>(p, ns + 2), *head = carve<int32_t>(p, ns + 2), *gid = carve<int32_t>(p, ns + 2),
            *gstart = carve<int32_t>(p, ns + 2), *n_kept = carve<int32_t>(p, ns + 2), *g_first = carve<int32_t>(p, ns + 2),
            *g_failed = carve<int32_t>(p, ns + 2), *g_ids = carve<int32_t>(p, ns + 2), *out_name = carve<int32_t>(p, ns + 2),
            *kept_ws = carve<int32_t>(p, ns + 2), *out_failed = carve<int32_t>(p, ns + 2);
    int32_t *tmp_rows = carve<int32_t>(p, 8 * ns);
    int32_t *first_primary = carve<int32_t>(p, (size_t)n_names + 1);
    int32_t *d_cnt = carve<int32_t>(p, 4);
    const int B = 256;
    // ---- read_length = query_length of the first record with flag < 256 per name (ibg:142-143)
    (void)hipMemsetAsync(first_primary, 0x7f, sizeof(int32_t) * ((size_t)n_names + 1), s);      // 0x7f7f7f7f > any ordinal
    if (n_rec > 0) hipLaunchKernelGGL(k_first_primary, dim3((n_rec + B - 1) / B), dim3(B), 0, s, n_rec, rec_tid, rec_flagmq, rec_name, first_primary);
    if (n_names > 0) hipLaunchKernelGGL(k_read_length, dim3((n_names + B - 1) / B), dim3(B), 0, s, n_names, first_primary, rec_qlen, out_read_length);
    if (n_sa > 0) {
        const int G = (n_sa + B - 1) / B;
        int32_t *err = d_cnt + 2;
        hipLaunchKernelGGL(k_row_keys, dim3(G), dim3(B), 0, s, n_sa, sa_rec, rec_tid, rec_name, keys, vals);
        size_t tb = cub_bytes;
        hipcub::DeviceRadixSort::SortPairs(cub_tmp, tb, keys, keys_s, vals, vals_s, n_sa, 0, 32, s);
        hipLaunchKernelGGL(k_heads, dim3(G), dim3(B), 0, s, n_sa, keys_s, head);
        tb = cub_bytes;
        hipcub::DeviceScan::InclusiveSum(cub_tmp, tb, head, gid, n_sa, s);
        hipLaunchKernelGGL(k_group_starts_n, dim3(G), dim3(B), 0, s, n_sa, head, gid, gstart, d_cnt);
        hipLaunchKernelGGL(k_group_process_n, dim3(G), dim3(B), 0, s, d_cnt + 3, n_sa, gstart, keys_s, vals_s, sa, sa_nm, first_primary,
                           rec_qlen, kept_ws, tmp_rows, n_kept, g_first, g_failed, err);
        // ---- reads in the reference's dict order = by first SA-bearing record = by their first SA row; empty slots last
        hipLaunchKernelGGL(k_iota, dim3(G), dim3(B), 0, s, n_sa, g_ids);
        int32_t *gf_sorted = keys, *g_sorted = vals;          // the unsorted row keys are no longer needed
        tb = cub_bytes;
        hipcub::DeviceRadixSort::SortPairs(cub_tmp, tb, g_first, gf_sorted, g_ids, g_sorted, n_sa, 0, 32, s);
        int32_t *cnt = head, *off = gid;                      // reuse
        hipLaunchKernelGGL(k_order_counts, dim3(G), dim3(B), 0, s, n_sa, gf_sorted, g_sorted, n_kept, cnt);
        (void)hipMemsetAsync(cnt + n_sa, 0, sizeof(int32_t), s);
        tb = cub_bytes;
        hipcub::DeviceScan::ExclusiveSum(cub_tmp, tb, cnt, off, n_sa + 1, s);
        // number of reads = slots with a valid key (they sort first)
        hipLaunchKernelGGL(k_count_valid, dim3(G), dim3(B), 0, s, n_sa, gf_sorted, d_cnt);
        hipLaunchKernelGGL(k_scatter_n, dim3(G), dim3(B), 0, s, n_sa, d_cnt, g_sorted, off, gstart, keys_s, n_kept, g_failed, tmp_rows,
                           out_rows, out_off, out_name, out_failed);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return sa_err(CORAL_ERR_HIP, hipGetErrorString(e));
        // the pair table of n_sa "reads": the ones behind the last have no rows (see k_scatter_n)
        const int rc = coral_bp_pair_table(n_sa, n_sa, out_off, out_rows, chr_rank, n_tid, min_bp_match_cutoff, min_mapq, gap_, gap_mapq, pairs, stream);
        if (rc) return sa_err(rc, coral_last_error());
        hipLaunchKernelGGL(k_table_host_layout, dim3((n_sa + 1 + B - 1) / B), dim3(B), 0, s, n_sa, d_cnt, out_rows, out_off, out_name,
                           out_failed, reinterpret_cast<long long *>(cols), reinterpret_cast<long long *>(off_w),
                           reinterpret_cast<long long *>(name_w), failed_b);
    } else {
        QUERY_HIP(hipMemsetAsync(d_cnt, 0, 4 * sizeof(int32_t), s));
        if (off_w) QUERY_HIP(hipMemsetAsync(off_w, 0, sizeof(int64_t), s));      // a table without reads still has its one offset
    }
    QUERY_HIP(hipGetLastError());
    QUERY_HIP(hipMemcpyAsync(counts, d_cnt, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));      // lands when the stream gets there
    return CORAL_OK;
}
