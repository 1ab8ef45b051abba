// coral_bamgpu_depth.h — the binned-depth request of the GPU BAM decoder (depth_bin).
//   k_bam_depth     per record one walk of its CIGAR, one 64-bit atomic per run of lanes in the same bin
// Kernels, device structs and the host-side request in one place; included by coral_bamgpu.hip inside its anonymous namespace
// (once, behind coral_bamgpu_common.h), not a header of its own.

// ---------------------------------------------------------------------------------------------
// K_depth: whole-genome binned read depth (depth_bin of the request; the rules: DepthPartial in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
struct DepthDev {                        // device arrays of the request, carved from the caller's workspace
    long long *bin_off;                  // n_ref + 1: first bin of every contig
    int32_t *len;                        // n_ref: LN (>= 0)
    unsigned long long *bases, *reads;   // n_bins each
    int n_ref;
    uint32_t bin, min_mapq, exclude_flags;
    int count_deletions;
};

// `key` does not decrease from lane to lane: the sum of `v` over every run of equal keys, in the run's first lane (a segmented
// suffix sum by doubling; the other lanes of a run hold partial sums).
__device__ __forceinline__ uint32_t depth_run_sum(uint32_t key, uint32_t v, int lane) {
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t tv = __shfl_down(v, d), tk = __shfl_down(key, d);
        if (lane + d < WAVE && tk == key) v += tv;
    }
    return v;
}

// One wave per record (grid-stride), one-wave workgroups without LDS: it fits beside resident inflate waves.
// Only the fixed fields and the real CIGAR (M.cig_src / M.n_cigar: the CG tag is resolved) are read.  The wave takes 64 ops at a
// time; the wave prefix sum of the reference advance gives every lane its op's interval [a, e), clipped to the contig - so no bin
// at or behind ceil(LN / bin) is ever addressed.  Ops come in increasing reference order, hence the lanes' bins do not decrease:
//   first bin   every lane adds the part of its op inside the op's first bin b0; lanes with the same b0 are summed in the wave
//               (an op that is not counted joins the run with 0) and the run's first lane issues ONE no-return 64-bit atomic;
//   last bin    the same for the part inside the op's last bin b1, for the ops that cross a bin edge (rare unless bin is small);
//   in between  the whole bins b0 + 1 .. b1 - 1 of such an op get `bin` each, 64 bins per step of the wave.
// A run's sum fits 32 bits: the positions one record covers are disjoint, so a bin gets at most `bin` from it.
// Atomics per record: the bins it touches (at most twice each) plus its 64-op chunks - not its ops.
__global__ __launch_bounds__(WAVE) void k_bam_depth(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M, DepthDev X) {
    const int lane = threadIdx.x;
    const uint32_t bin = X.bin;
    for (long long i = blockIdx.x; i < n_rec; i += gridDim.x) {
        const int32_t tid = M.tid[i], pos = M.pos[i];
        const int n_ops = M.n_cigar[i];
        if (!depth_takes_part(tid, pos, (uint32_t)n_ops, (uint32_t)M.flag[i], (uint32_t)M.mapq[i], X.n_ref, X.exclude_flags, X.min_mapq)) continue;
        const long long ln = X.len[tid];
        if (pos >= ln) continue;                                       // (so ln >= 1 below)
        const long long bo = X.bin_off[tid];
        unsigned long long *bases = X.bases + bo;
        if (lane == 0) atomicAdd(X.reads + bo + (uint32_t)pos / bin, 1ull);
        const uint8_t *ops = buf + M.cig_src[i];
        long long r_base = pos;
        for (int c = 0; c < n_ops && r_base < ln; c += WAVE) {
            const int kk = c + lane;
            const uint32_t wd = kk < n_ops ? ld32(ops + 4ll * kk) : 15u;
            const uint32_t op = wd & 15u;
            const long long len = (long long)(wd >> 4);
            const long long ra = ((0x18Du >> op) & 1u) ? len : 0;     // M D N = X advance the reference
            long long rs = ra;
            for (int d = 1; d < WAVE; d <<= 1) {
                const long long t = __shfl_up(rs, d);
                if (lane >= d) rs += t;
            }
            const uint32_t a = (uint32_t)min(r_base + rs - ra, ln), e = (uint32_t)min(r_base + rs, ln);      // 0 <= a <= e <= LN
            const bool counted = depth_counts_op(op, X.count_deletions != 0) && e > a;
            const uint32_t b0 = min(a, (uint32_t)ln - 1u) / bin, b1 = (max(e, 1u) - 1u) / bin;               // counted: b0 <= b1 < the contig's bins
            const unsigned long long edge = ((unsigned long long)b0 + 1ull) * bin;
            const uint32_t first = counted ? (uint32_t)(min((unsigned long long)e, edge) - a) : 0u;
            const uint32_t last = counted && b1 > b0 ? (uint32_t)(e - (unsigned long long)b1 * bin) : 0u;
            {
                const uint32_t sum = depth_run_sum(b0, first, lane), prev = __shfl_up(b0, 1);
                if ((lane == 0 || prev != b0) && sum) atomicAdd(bases + b0, (unsigned long long)sum);
            }
            if (__ballot(last != 0u) != 0ull) {
                const uint32_t sum = depth_run_sum(b1, last, lane), prev = __shfl_up(b1, 1);
                if ((lane == 0 || prev != b1) && sum) atomicAdd(bases + b1, (unsigned long long)sum);
                unsigned long long m = __ballot(counted && b1 > b0 + 1u);
                while (m) {
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t k0 = __shfl(b0, j) + 1u, k1 = __shfl(b1, j);
                    for (uint32_t k = k0 + (uint32_t)lane; k < k1; k += WAVE) atomicAdd(bases + k, (unsigned long long)bin);
                }
            }
            r_base += __shfl(rs, WAVE - 1);
        }
    }
}

// ---- host side: the request's lifecycle (each_request in coral_bamgpu.hip, which calls all but open only when `active`) ---------
struct DepthRequest {                // binned depth: bin_off, the contig lengths and the two int64 tables in the workspace
    bool active = false;
    DepthDev X{};
    size_t n_bins = 0;
    // the rule that needs the header: at most 2^28 bins (refused here, nothing allocated)
    int open(const Request &R, const Caps &, Decoded &D, std::string &err) {
        active = R.depth_bin > 0;
        return !active || D.depth.init(R.depth_bin, R.depth_min_mapq, R.depth_exclude_flags, R.depth_count_deletions, D.ref_lens, err) ? CORAL_OK : CORAL_ERR_ARG;
    }
    void carve(Carver &take, const Caps &, const Decoded &D) {
        const DepthPartial &P = D.depth;
        const size_t n_ref = P.len.size();
        n_bins = (size_t)P.n_bins();
        X.bin_off = (long long *)take((n_ref + 1) * 8);
        X.len = (int32_t *)take(n_ref * 4);
        X.bases = (unsigned long long *)take(n_bins * 8);
        X.reads = (unsigned long long *)take(n_bins * 8);
        X.n_ref = (int)n_ref;
        X.bin = (uint32_t)P.bin; X.min_mapq = (uint32_t)P.min_mapq; X.exclude_flags = (uint32_t)P.exclude_flags;
        X.count_deletions = P.count_deletions ? 1 : 0;
    }
    const char *start(const Decoded &D, hipError_t &e) const {
        const size_t n_ref = (size_t)X.n_ref;
        const bool ok = (e = hipMemcpy(X.bin_off, D.depth.bin_off.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice)) == hipSuccess &&
                        (n_ref == 0 || (e = hipMemcpy(X.len, D.depth.len.data(), n_ref * 4, hipMemcpyHostToDevice)) == hipSuccess) &&
                        (n_bins == 0 || ((e = hipMemset(X.bases, 0, n_bins * 8)) == hipSuccess && (e = hipMemset(X.reads, 0, n_bins * 8)) == hipSuccess));
        return ok ? nullptr : "binned-depth request set-up";
    }
    bool batch(const Batch &B, Scratch, std::string &err) const {      // (no scratch: it reads the CIGAR bytes through M.cig_src)
        if (B.n_rec == 0 || n_bins == 0) return true;
        // one wave per workgroup, grid-stride beyond 32 per CU
        hipLaunchKernelGGL(k_bam_depth, dim3((unsigned)std::min<long long>(B.n_rec, 8192)), dim3(WAVE), 0, B.stream, B.buf, B.n_rec, B.M, X);
        return launched("binned depth", err);
    }
    bool finish(Decoded &D, int) const {
        D.depth.zero_tables();
        return dev_get(D.depth.bases.data(), X.bases, n_bins * 8) && dev_get(D.depth.reads.data(), X.reads, n_bins * 8);
    }
};
