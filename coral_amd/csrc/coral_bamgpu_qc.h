// coral_bamgpu_qc.h — the read-QC request of the GPU BAM decoder (want_qc).
//   k_bam_qc_plan + k_bam_qc           per read the sum of its QUAL bytes, and the 256-bin histogram of all of them
// Kernels, device structs and the host-side request in one place; included by coral_bamgpu.hip inside its anonymous namespace
// (once, behind coral_bamgpu_common.h), not a header of its own.

// ---------------------------------------------------------------------------------------------
// K_qc: per-read base-quality sums and the base-quality histogram (want_qc; the rules: QcPartial in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
#define QC_SLICE 16384ll                 // QUAL bytes per work item (as COV_SLICE: a 1 Mb read is 62 waves' work)
#ifndef QC_COPIES
#define QC_COPIES 4                      // copies of the 256-bin table per wave, interleaved: 4 KiB of LDS (a -DQC_COPIES=1 build is
#endif                                   // the single table to measure it against)

// One thread per record (one-wave workgroups): qual_sum[i] = 0 for a read with quality (k_bam_qc adds to it), -1 otherwise, and
// the number of work items its QUAL is cut into.  Slot n_rec gets 0 items (the scan's extra entry).
__global__ __launch_bounds__(WAVE) void k_bam_qc_plan(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                      MetaArrays M, long long *__restrict__ qual_sum, long long *__restrict__ n_items) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    long long cnt = 0;
    if (i < n_rec) {
        const uint32_t l_seq = (uint32_t)M.l_seq[i];
        bool counted = false;
        if (qc_is_read((uint32_t)M.flag[i], l_seq)) {
            const uint8_t *r = buf + rec_start[i];
            counted = qc_has_quality(r[qc_qual_offset(r[12], ld16(r + 16), l_seq)]);
        }
        if (counted) cnt = ((long long)l_seq + QC_SLICE - 1) / QC_SLICE;
        qual_sum[i] = counted ? 0 : -1;
    }
    n_items[i] = cnt;
}

// One wave per work item (one-wave workgroups, grid-stride): QUAL bytes [k * QC_SLICE, (k + 1) * QC_SLICE) of record i.
// QUAL begins at any byte address: the wave reads the 16-byte aligned chunks that cover its bytes, lane l the chunks l, l + 64,
// ... - one load instruction of the wave is 1 KiB of consecutive memory, every cache line is fetched once - and the bytes of the
// first and the last chunk that are not the item's are masked out.  Sum: v_sad_u8 per dword, reduced in the wave, ONE 64-bit
// atomic per item.  Histogram: COPIES copies of the 256 bins in LDS, interleaved (bin v of copy c at word v * COPIES + c, lane l
// uses copy l % COPIES): real QUAL sits on a few values, and lanes that add to the same word are serialised - with the copies
// side by side, lanes with the same value spread over COPIES words in COPIES different banks.  The workgroup adds its table to the
// device histogram once, at its end, with 64-bit atomics.  4 KiB of LDS (COPIES = 4): fits beside the inflate launch's 27 x 5.75 KiB
// of a CU's 160 KiB, as k_bgzf_crc's tables do.
__global__ __launch_bounds__(WAVE) void k_bam_qc(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                 MetaArrays M, const long long *__restrict__ item_off,
                                                 unsigned long long *__restrict__ qual_sum, unsigned long long *__restrict__ hist) {
    constexpr int COPIES = QC_COPIES;
    // (a 32-bit bin cannot overflow: the grid-stride loop gives a workgroup at most ceil(items / 2 048) work items of 16 KiB, and
    // CARRY_CAP + a batch stay below 4 GiB - under 2^21 bytes per workgroup and launch)
    __shared__ uint32_t H[256 * COPIES];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256 * COPIES; k += WAVE) H[k] = 0;
    __syncthreads();
    uint32_t *mine = H + (lane % COPIES);
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const uint32_t l_seq = (uint32_t)M.l_seq[i];
        const uint8_t *r = buf + rec_start[i];
        const long long q_lo = (w - item_off[i]) * QC_SLICE, q_hi = min((long long)l_seq, q_lo + QC_SLICE);
        const uint8_t *p = r + qc_qual_offset(r[12], ld16(r + 16), l_seq) + q_lo;
        const int n = (int)(q_hi - q_lo);                             // 1 .. QC_SLICE
        const int head = (int)((uintptr_t)p & 15u);
        const uint4 *chunks = reinterpret_cast<const uint4 *>(p - head);       // (inside the batch buffer: a record starts >= 36 bytes in front of its QUAL)
        const int n_chunks = (head + n + 15) >> 4;
        uint32_t acc = 0;
        for (int c = lane; c < n_chunks; c += WAVE) {
            const uint4 v = chunks[c];
            const uint32_t word[4] = {v.x, v.y, v.z, v.w};
            const int first = c * 16 - head;                          // item-relative index of the chunk's byte 0
            if (first >= 0 && first + 16 <= n) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const uint32_t x = word[d];
                    acc = __builtin_amdgcn_sad_u8(x, 0u, acc);
                    atomicAdd(mine + (x & 0xffu) * COPIES, 1u);
                    atomicAdd(mine + ((x >> 8) & 0xffu) * COPIES, 1u);
                    atomicAdd(mine + ((x >> 16) & 0xffu) * COPIES, 1u);
                    atomicAdd(mine + (x >> 24) * COPIES, 1u);
                }
            } else {                                                  // the item's first or last chunk: byte by byte
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t q = (word[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    if (first + j >= 0 && first + j < n) {
                        acc += q;
                        atomicAdd(mine + q * COPIES, 1u);
                    }
                }
            }
        }
        unsigned long long sum = acc;
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) atomicAdd(qual_sum + i, sum);
    }
    __syncthreads();
    for (int v = lane; v < 256; v += WAVE) {
        unsigned long long t = 0;
#pragma unroll
        for (int c = 0; c < COPIES; ++c) t += H[v * COPIES + c];
        if (t) atomicAdd(hist + v, t);
    }
}

// ---- host side: the request's lifecycle (each_request in coral_bamgpu.hip, which calls all but open only when `active`) ---------
struct QcRequest {
    bool active = false;
    long long *rows = nullptr;                // the batch's qual_sum rows: one array for all batches (collect)
    unsigned long long *hist = nullptr;       // the device histogram of the whole decode
    long long pending_n = 0;                  // records of the batch whose rows are still on the device
    int open(const Request &R, const Caps &, Decoded &D, std::string &) { if ((active = R.want_qc)) D.qc.init(); return CORAL_OK; }
    void carve(Carver &take, const Caps &C, const Decoded &) {
        rows = (long long *)take(C.rec_slots * 8);
        hist = (unsigned long long *)take(256 * 8);
    }
    const char *start(const Decoded &, hipError_t &e) const { return (e = hipMemset(hist, 0, 256 * 8)) != hipSuccess ? "read-QC request set-up" : nullptr; }
    // Nothing is waited for here: the rows are fetched with the next batch's host fields (behind that emit's stream
    // synchronisation, which any kernel queued here is in front of), or by coral_bamgpu_finish.
    bool batch(const Batch &B, Scratch S, std::string &err) {
        const long long n = B.n_rec;
        if (n == 0) return true;
        auto [items, item_off] = S.take<2>();
        hipLaunchKernelGGL(k_bam_qc_plan, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, B.stream, B.buf, B.rec_start, n, B.M, rows, items);
        if (!B.scan(items, item_off)) { err = "scan of the read-QC work items failed"; return false; }
        // one wave per workgroup, grid-stride beyond 8 per CU
        hipLaunchKernelGGL(k_bam_qc, dim3((unsigned)std::min<long long>(B.max_items(QC_SLICE), 2048)), dim3(WAVE), 0, B.stream, B.buf, B.rec_start, n, B.M, item_off,
                           (unsigned long long *)rows, hist);
        if (!launched("read-QC", err)) return false;
        pending_n = n;
        return true;
    }
    // The rows of the batch emitted last, if they are still on the device (the caller has synchronised the stream).  One array
    // for all batches: that holds only while every emit of a decode and the result call are given the SAME stream: the rows of
    // batch k-1 are complete once batch k's emit has waited for the stream that batch k-1's kernels were queued on, and batch
    // k's k_bam_qc_plan is queued only afterwards.
    bool collect(std::vector<int64_t> &v) { return collect_pending(v, rows, pending_n); }
    bool finish(Decoded &D, int) { return collect(D.qc.qual_sum) && dev_get(D.qc.hist, hist, 256 * 8); }
};
