// coral_bamgpu_cov.h — the window-coverage / pileup request of the GPU BAM decoder (has_cov, per_base).
//   k_bam_cov_plan + k_bam_cov_count   window coverage: pysam count_coverage with a base-quality threshold over the segments
//   k_bam_cov_plan + k_bam_pileup      the same split by position and base (per_base): one 32-bit atomic per counted base
//                   (both kernels are cov_walk, the one CIGAR walk that applies the coverage rule, with a sink each)
// Kernels, device structs and the host-side request in one place; included by coral_bamgpu.hip inside its anonymous namespace
// (once, behind coral_bamgpu_common.h), not a header of its own.

// ---------------------------------------------------------------------------------------------
// K_cov: window coverage with a base-quality threshold (the segments of the request), counted while SEQ and QUAL are in HBM
// ---------------------------------------------------------------------------------------------
#define COV_SLICE 16384ll                // query bases per work item: a 1 Mb read is 62 waves' work, not one wave's

struct CovSegs {                         // the request's sorted, disjoint segments (device arrays in the workspace)
    const int32_t *tid, *lo, *hi;
    int n;
};

// first segment at or after (t, pos) in (tid, hi) order, searching [from, n); wave-uniform when its arguments are
__device__ __forceinline__ int cov_first(const CovSegs &S, int32_t t, long long pos, int from) {
    int a = from, b = S.n;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (S.tid[m] < t || (S.tid[m] == t && (long long)S.hi[m] <= pos)) a = m + 1; else b = m;
    }
    return a;
}

// one thread per record: how many work items (COV_SLICE query bases each) the record needs; 0 when it is filtered out, has no
// SEQ, has no QUAL at a threshold above 0, or overlaps no segment.  Slot n_rec gets 0 (the scan's extra entry).
__global__ __launch_bounds__(256) void k_bam_cov_plan(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M,
                                                       const int32_t *__restrict__ end_in, CovSegs S, int threshold, int filter_all,
                                                       long long *__restrict__ n_items) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    long long cnt = 0;
    if (i < n_rec) {
        const int32_t tid = M.tid[i], l_seq = M.l_seq[i], flag = M.flag[i];
        if (tid >= 0 && l_seq > 0 && M.n_cigar[i] > 0 && !(filter_all && (flag & 0x704))) {
            const uint8_t *qual = buf + M.seq_src[i] + ((long long)l_seq + 1) / 2;
            if (threshold == 0 || qual[0] != 0xff) {
                const int32_t pos = M.pos[i];
                // end_in is htslib's bam_endpos: pos + 1 for an unmapped record, whose CIGAR is walked all the same
                const long long end = (flag & 4) ? (1ll << 40) : (long long)end_in[i];
                const int s = cov_first(S, tid, pos, 0);
                if (s < S.n && S.tid[s] == tid && (long long)S.lo[s] < end) cnt = ((long long)l_seq + COV_SLICE - 1) / COV_SLICE;
            }
        }
    }
    n_items[i] = cnt;
}

// The CIGAR walk of one work item, the query bases [q_lo, q_hi) of record i, for both coverage kernels: the coverage rule
// (CovTable in coral_bam_common.h) is applied here and nowhere else on the device.  The wave walks the CIGAR 64 ops at a time
// (prefix sums of the query / reference advance), and for every aligned op that meets the query range the lanes stride over the
// op's bases inside each segment, testing the SEQ code and QUAL.  What becomes of a counted base is the sink's business:
//   segment(t, lo)   wave-uniform, in front of the bases of an op inside segment t (lo = S.lo[t]); segments are met in
//                    increasing order, the same one again for every further op inside it
//   base(x, col)     per lane: the base at reference position x counts, col = 0..3 for A, C, G, T
template <class Segment, class Base>
__device__ __forceinline__ void cov_walk(const uint8_t *__restrict__ buf, const MetaArrays &M, const CovSegs &S, uint32_t thr, long long i,
                                         long long q_lo, long long q_hi, int lane, Segment segment, Base base) {
    const int32_t tid = M.tid[i], l_seq = M.l_seq[i], pos = M.pos[i];
    const int n_ops = M.n_cigar[i];
    const uint8_t *ops = buf + M.cig_src[i];
    const uint8_t *seq = buf + M.seq_src[i];
    const uint8_t *qual = seq + ((long long)l_seq + 1) / 2;
    int s = cov_first(S, tid, pos, 0);
    long long q_base = 0, r_base = pos;
    for (int c = 0; c < n_ops && q_base < q_hi; c += WAVE) {
        if (s >= S.n || S.tid[s] != tid) break;                   // no segment left on this contig
        const int kk = c + lane;
        const uint32_t wd = kk < n_ops ? ld32(ops + 4ll * kk) : 15u;
        const uint32_t op = wd & 15u;
        const long long len = (long long)(wd >> 4);
        const long long qa = ((0x193u >> op) & 1u) ? len : 0;     // M I S = X advance the query
        const long long ra = ((0x18Du >> op) & 1u) ? len : 0;     // M D N = X advance the reference
        long long qs = qa, rs = ra;
        for (int d = 1; d < WAVE; d <<= 1) {
            const long long tq = __shfl_up(qs, d), tr = __shfl_up(rs, d);
            if (lane >= d) { qs += tq; rs += tr; }
        }
        const long long q_op = q_base + qs - qa, r_op = r_base + rs - ra;
        const bool cand = ((0x181u >> op) & 1u) && len > 0 && q_op < q_hi && q_op + len > q_lo;     // M = X meeting the item
        unsigned long long m = __ballot(cand);
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const long long oq = __shfl(q_op, j), orf = __shfl(r_op, j), ol = __shfl(len, j);
            const long long aq = max(oq, q_lo), bq = min(oq + ol, q_hi);
            const long long r0 = orf + (aq - oq), r1 = orf + (bq - oq);
            // r0 only grows: the cursor is usually still right (this op ends inside its segment) or one further
            if (s < S.n && S.tid[s] == tid && (long long)S.hi[s] <= r0)
                s = (s + 1 < S.n && S.tid[s + 1] == tid && (long long)S.hi[s + 1] > r0) ? s + 1 : cov_first(S, tid, r0, s + 1);
            for (int t = s; t < S.n && S.tid[t] == tid && (long long)S.lo[t] < r1; ++t) {
                const long long lo = S.lo[t], xa = max(r0, lo), xb = min(r1, (long long)S.hi[t]);
                segment(t, lo);
                for (long long x = xa + lane; x < xb; x += WAVE) {
                    const long long qi = aq + (x - r0);                    // < bq <= q_hi <= l_seq
                    const uint8_t byte = seq[qi >> 1];
                    const uint32_t code = (qi & 1) ? (byte & 15u) : (uint32_t)(byte >> 4);
                    uint32_t col;
                    if (pileup_base(code, &col) && qual[qi] >= thr) base(x, col);
                }
            }
        }
        q_base += __shfl(qs, WAVE - 1);
        r_base += __shfl(rs, WAVE - 1);
    }
}

// one wave per work item (grid-stride): the query bases [k * COV_SLICE, (k + 1) * COV_SLICE) of record i.  The counting sink:
// per-lane counts, reduced in the wave and added with ONE 64-bit atomic per (work item, segment).
__global__ __launch_bounds__(256) void k_bam_cov_count(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M, CovSegs S,
                                                        int threshold, const long long *__restrict__ item_off,
                                                        unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long total = item_off[n_rec];
    for (long long w = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < total; w += n_waves) {
        const long long i = item_record(item_off, n_rec, w);
        const long long q_lo = (w - item_off[i]) * COV_SLICE, q_hi = min((long long)M.l_seq[i], q_lo + COV_SLICE);
        int cur = -1;                                                  // the segment the lanes' counts belong to
        uint32_t acc = 0;
        auto flush = [&]() {
            long long sum = (long long)acc;
            for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
            if (cur >= 0 && lane == 0 && sum) atomicAdd(counts + cur, (unsigned long long)sum);
            acc = 0;
        };
        cov_walk(buf, M, S, (uint32_t)threshold, i, q_lo, q_hi, lane, [&](int t, long long) { if (t != cur) { flush(); cur = t; } },
                 [&](long long, uint32_t) { ++acc; });
        flush();
    }
}

// K_pileup (per_base of the request): k_bam_cov_count's work items and walk with the table sink: every counted base is one
// no-return 32-bit atomic at table[(seg_off[t] + x - lo[t]) * 4 + col].  There is nothing to reduce: the 64 lanes of a stride are
// 64 different positions, so a wave never collides with itself - only different records at the same position do.  One wave per
// workgroup (grid-stride), no LDS: it fits beside resident inflate waves.
__global__ __launch_bounds__(WAVE) void k_bam_pileup(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M, CovSegs S,
                                                     const long long *__restrict__ seg_off, int threshold,
                                                     const long long *__restrict__ item_off, uint32_t *__restrict__ table) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const long long q_lo = (w - item_off[i]) * COV_SLICE, q_hi = min((long long)M.l_seq[i], q_lo + COV_SLICE);
        long long row0 = 0;                                            // lo <= x < hi: 4 * x + row0 lies in the segment's rows
        cov_walk(buf, M, S, (uint32_t)threshold, i, q_lo, q_hi, lane, [&](int t, long long lo) { row0 = 4 * (seg_off[t] - lo); },
                 [&](long long x, uint32_t col) { atomicAdd(table + (row0 + 4 * x + col), 1u); });
    }
}

// ---- host side: the request's lifecycle (each_request in coral_bamgpu.hip, which calls all but open only when `active`) ---------
struct CovRequest {                  // window coverage; with per_base the table of a pileup request instead of the counters
    bool active = false;
    const CovTable *T = nullptr;     // the request's segments, threshold and callback (Request::cov)
    CovSegs segs{nullptr, nullptr, nullptr, 0};          // segments and counters in the workspace (n = 0: nothing to count)
    unsigned long long *counts = nullptr;
    long long *pile_off = nullptr;   // per_base: the segments' prefix offsets and the table [positions][4]
    uint32_t *pile = nullptr;
    int open(const Request &R, const Caps &, Decoded &, std::string &) { active = R.has_cov; T = &R.cov; return CORAL_OK; }
    void carve(Carver &take, const Caps &, const Decoded &) {
        const size_t n_seg = T->size();
        int32_t *seg = (int32_t *)take(3 * n_seg * 4);
        segs = CovSegs{seg, seg + n_seg, seg + 2 * n_seg, (int)n_seg};
        counts = (unsigned long long *)take(n_seg * 8);
        if (!T->per_base) return;
        pile_off = (long long *)take((n_seg + 1) * 8);
        pile = (uint32_t *)take((size_t)T->n_pos() * 16);
    }
    const char *start(const Decoded &, hipError_t &e) const {      // nullptr, or what failed with `e`
        if (segs.n == 0) return nullptr;
        const size_t b = T->size() * 4;
        if ((e = hipMemcpy((void *)segs.tid, T->tid.data(), b, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy((void *)segs.lo, T->lo.data(), b, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy((void *)segs.hi, T->hi.data(), b, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemset(counts, 0, 2 * b)) != hipSuccess)
            return "coverage request set-up";
        if (T->per_base && ((e = hipMemcpy(pile_off, T->seg_off.data(), (T->size() + 1) * 8, hipMemcpyHostToDevice)) != hipSuccess ||
                            (T->n_pos() > 0 && (e = hipMemset(pile, 0, (size_t)T->n_pos() * 16)) != hipSuccess)))
            return "pileup request set-up";
        return nullptr;
    }
    // queued before ev_parsed so that the slot is not inflated into while the kernels read its SEQ and QUAL
    bool batch(const Batch &B, Scratch S, std::string &err) const {
        const long long n = B.n_rec;
        if (n == 0 || segs.n == 0) return true;
        auto [items, item_off] = S.take<2>();
        hipLaunchKernelGGL(k_bam_cov_plan, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, B.stream, B.buf, n, B.M, B.end, segs, T->threshold,
                           (int)T->filter_all, items);
        if (!B.scan(items, item_off)) { err = "scan of the coverage work items failed"; return false; }
        const long long n_items = B.max_items(COV_SLICE);
        if (T->per_base)                 // one wave per workgroup, grid-stride beyond 32 per CU
            hipLaunchKernelGGL(k_bam_pileup, dim3((unsigned)std::min<long long>(n_items, 8192)), dim3(WAVE), 0, B.stream, B.buf, n, B.M, segs, pile_off,
                               T->threshold, item_off, pile);
        else                             // 4 waves per workgroup, grid-stride beyond
            hipLaunchKernelGGL(k_bam_cov_count, dim3((unsigned)std::min<long long>((n_items + 3) / 4, 8192)), dim3(256), 0, B.stream, B.buf, n, B.M, segs,
                               T->threshold, item_off, counts);
        return launched("window coverage", err);
    }
    bool finish(Decoded &D, int) const {
        if (!T->per_base) { D.cov.assign(T->size(), 0); return dev_get(D.cov.data(), counts, T->size() * 8); }
        D.pileup.assign((size_t)T->n_pos() * 4, 0);      // the table, and the counts per segment as its sums
        D.has_pileup = true;
        if (!dev_get(D.pileup.data(), pile, (size_t)T->n_pos() * 16)) return false;
        pileup_segment_sums(*T, D.pileup.data(), D.cov);
        return true;
    }
};
