// coral_bamgpu_index.h — the BAI-index request of the GPU BAM decoder (want_index).
//   k_bam_index + k_bam_index_compact  per record the virtual offset, the UCSC bin and the linear-index windows of a
//                   BAI index, per batch the heads of the runs of equal (tid, bin)
// Kernels, device structs and the host-side request in one place; included by coral_bamgpu.hip inside its anonymous namespace
// (once, behind coral_bamgpu_common.h), not a header of its own.

// ---------------------------------------------------------------------------------------------
// K_index: what a batch contributes to the BAI index of the file (want_index; IndexPartial in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
struct IndexDev {                        // device arrays of the request, carved from the caller's workspace
    unsigned long long *lin;             // linear index: smallest virtual offset per (contig, 16 384-base window), ~0 = none
    long long *lin_off;                  // n_ref + 1: first window of every contig
    unsigned long long *n_mapped, *n_unmapped, *n_no_coor;      // n_ref, n_ref, 1 counters
    unsigned long long *state;           // [2]: virtual offset of the position a batch ends at (read by the next batch: the
                                         // start of the record it carries in), alternating
    int32_t *unsorted;                   // set when a record sorts in front of its predecessor
    int n_ref;
};

// virtual offset of byte `rel` of the batch's inflated bytes: the block that holds it (the last one that starts at or in front
// of it: an empty block starts where its successor does); behind the batch's last byte the block that follows it (bgzf_tell)
__device__ __forceinline__ unsigned long long batch_voffset(const BlockDesc *__restrict__ desc, const uint32_t *__restrict__ boff, int n_blocks,
                                                            unsigned long long file_off, unsigned long long comp_bytes, long long rel,
                                                            long long infl_bytes) {
    if (rel < infl_bytes) {
        int a = 0, b = n_blocks;                                   // the last block with dst_off <= rel
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if ((long long)desc[m].dst_off <= rel) a = m; else b = m;
        }
        return ((file_off + boff[a]) << 16) | (unsigned long long)(rel - (long long)desc[a].dst_off);
    }
    int a = 0, b = n_blocks;                                       // the first block with dst_off >= rel
    while (a < b) {
        const int m = (a + b) >> 1;
        if ((long long)desc[m].dst_off < rel) a = m + 1; else b = m;
    }
    return (a < n_blocks ? file_off + boff[a] : file_off + comp_bytes) << 16;
}

__device__ __forceinline__ long long index_key(int32_t tid, int32_t pos, int32_t end, int n_ref, long long *beg_out, long long *end_out) {
    if (tid < 0 || tid >= n_ref) return -1;
    const long long b = pos < 0 ? 0 : pos, e = (long long)end > b ? (long long)end : b + 1, l = e - 1;
    *beg_out = b;
    *end_out = e;
    int bin = 0;
    if (b >> 14 == l >> 14) bin = (int)(4681 + (b >> 14));
    else if (b >> 17 == l >> 17) bin = (int)(585 + (b >> 17));
    else if (b >> 20 == l >> 20) bin = (int)(73 + (b >> 20));
    else if (b >> 23 == l >> 23) bin = (int)(9 + (b >> 23));
    else if (b >> 26 == l >> 26) bin = (int)(1 + (b >> 26));
    return (long long)tid * 65536 + bin;
}

__device__ __forceinline__ unsigned long long index_sort_word(int32_t tid, int32_t pos) {
    return tid < 0 ? ~0ull : ((unsigned long long)(uint32_t)tid << 32) | (uint32_t)(pos < 0 ? 0 : pos);
}

// One thread per record (one-wave workgroups: the kernel runs beside the next batch's inflate), thread n_rec for the batch's end.
// Record i: virtual offset of its first byte (a record carried in from the previous batch: where it STARTED, state[parity]),
// key = tid * 65536 + bin, head[i] = 1 when the key differs from its predecessor's (record 0 always: the host joins a run that
// goes on across batches), 64-bit atomicMin into every linear-index window it overlaps, the per-contig counters (one atomic per
// wave when the wave's records are on one contig), and the order check against its predecessor.
__global__ __launch_bounds__(WAVE) void k_bam_index(const long long *__restrict__ rec_start, long long n_rec, MetaArrays M,
                                                    const int32_t *__restrict__ end_in, const BlockDesc *__restrict__ desc,
                                                    const uint32_t *__restrict__ boff, int n_blocks, unsigned long long file_off,
                                                    unsigned long long comp_bytes, long long infl_bytes, long long carry_pos, int parity,
                                                    IndexDev X, unsigned long long *__restrict__ voff_out, long long *__restrict__ key_out,
                                                    long long *__restrict__ head_out) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == n_rec) {
        head_out[i] = 0;                                               // the scan's extra slot
        // where the batch ends: the start of the record that is carried into the next batch (or still the one carried into this
        // one: a record may span several batches), or the place just behind the batch's last record
        X.state[parity ^ 1] = carry_pos < CARRY_CAP ? X.state[parity]
                                                    : batch_voffset(desc, boff, n_blocks, file_off, comp_bytes, carry_pos - CARRY_CAP, infl_bytes);
    }
    const bool valid = i < n_rec;
    int32_t tid = -1, flag = 0;
    if (valid) {
        const long long x = rec_start[i];
        const unsigned long long voff = x < CARRY_CAP ? X.state[parity]
                                                      : batch_voffset(desc, boff, n_blocks, file_off, comp_bytes, x - CARRY_CAP, infl_bytes);
        tid = M.tid[i];
        flag = M.flag[i];
        const int32_t pos = M.pos[i];
        long long b = 0, e = 0;
        const long long key = index_key(tid, pos, end_in[i], X.n_ref, &b, &e);
        bool head = true;
        if (i > 0) {
            long long pb, pe;
            const int32_t ptid = M.tid[i - 1], ppos = M.pos[i - 1];
            head = index_key(ptid, ppos, end_in[i - 1], X.n_ref, &pb, &pe) != key;
            if (index_sort_word(tid, pos) < index_sort_word(ptid, ppos)) *X.unsorted = 1;
        }
        voff_out[i] = voff;
        key_out[i] = key;
        head_out[i] = head ? 1 : 0;
        if (key >= 0) {
            const long long w_first = X.lin_off[tid], nw = X.lin_off[tid + 1] - w_first;
            const long long w0 = min(b >> 14, nw - 1), w1 = min((e - 1) >> 14, nw - 1);
            for (long long w = w0; w <= w1; ++w) atomicMin(X.lin + w_first + w, voff);
        } else {
            tid = -1;
        }
    }
    // counters
    const unsigned long long act = __ballot(valid);
    if (act == 0ull) return;
    const int32_t t0 = __shfl(tid, (int)__builtin_ctzll(act));
    if (__ballot(valid && tid != t0) == 0ull) {
        const unsigned long long unm = __ballot(valid && (flag & 4));
        if (lane == (int)__builtin_ctzll(act)) {
            if (t0 < 0) atomicAdd(X.n_no_coor, (unsigned long long)__popcll(act));
            else {
                if (act & ~unm) atomicAdd(X.n_mapped + t0, (unsigned long long)__popcll(act & ~unm));
                if (unm) atomicAdd(X.n_unmapped + t0, (unsigned long long)__popcll(unm));
            }
        }
    } else if (valid) {
        atomicAdd(tid < 0 ? X.n_no_coor : (flag & 4) ? X.n_unmapped + tid : X.n_mapped + tid, 1ull);
    }
}

// the heads, compacted in file order: head_off = exclusive prefix sum of head
__global__ __launch_bounds__(WAVE) void k_bam_index_compact(long long n_rec, const long long *__restrict__ head, const long long *__restrict__ head_off,
                                                            const unsigned long long *__restrict__ voff, const long long *__restrict__ key,
                                                            unsigned long long *__restrict__ voff_out, long long *__restrict__ key_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec || !head[i]) return;
    voff_out[head_off[i]] = voff[i];
    key_out[head_off[i]] = key[i];
}

// ---- host side: the request's lifecycle (each_request in coral_bamgpu.hip, which calls all but open only when `active`) ---------
// Beside it, four hooks in the decoder behind idx.active: the staging of block offsets in the feeder, the two copies in
// launch_inflate, the first-record check in coral_bamgpu_next and the order note in coral_bamgpu_emit.
struct IndexRequest {
    bool active = false;
    IndexDev X{};
    uint32_t *boff[2] = {nullptr, nullptr};       // per block of the slot's batch: its file offset relative to the batch's
    BlockDesc *kept_desc[2] = {nullptr, nullptr}; // the slot's block table and offsets, kept for k_bam_index: the feeder re-stages
    uint32_t *kept_boff[2] = {nullptr, nullptr};  //   d_desc / boff for batch k + 2 while batch k is still being parsed
    int parity = 0;                               // which X.state the next batch reads
    int open(const Request &R, const Caps &, Decoded &D, std::string &) { if ((active = R.want_index)) D.idx.init(D.ref_lens); return CORAL_OK; }
    void carve(Carver &take, const Caps &C, const Decoded &D) {      // (everything per record comes from the batch's scratch)
        const size_t n_ref = D.idx.n_mapped.size();
        for (int i = 0; i < 2; ++i) {
            boff[i] = (uint32_t *)take(C.max_blocks * 4);
            kept_boff[i] = (uint32_t *)take(C.max_blocks * 4);
            kept_desc[i] = (BlockDesc *)take(C.max_blocks * sizeof(BlockDesc));
        }
        X.lin = (unsigned long long *)take(D.idx.lin.size() * 8); X.lin_off = (long long *)take((n_ref + 1) * 8);
        X.n_mapped = (unsigned long long *)take(n_ref * 8); X.n_unmapped = (unsigned long long *)take(n_ref * 8);
        X.n_no_coor = (unsigned long long *)take(8); X.state = (unsigned long long *)take(16); X.unsorted = (int32_t *)take(4);
        X.n_ref = (int)n_ref;
    }
    // with nothing in front of the first record (rank 0) the first batch's end state is never read; a later rank's first
    // record is found by search and must start inside its batch (checked in coral_bamgpu_next)
    const char *start(const Decoded &D, hipError_t &e) const {
        const size_t n_ref = (size_t)X.n_ref;
        const bool ok = (e = hipMemset(X.lin, 0xff, D.idx.lin.size() * 8)) == hipSuccess && (e = hipMemset(X.n_mapped, 0, n_ref * 8)) == hipSuccess &&
                                    (e = hipMemset(X.n_unmapped, 0, n_ref * 8)) == hipSuccess && (e = hipMemset(X.n_no_coor, 0, 8)) == hipSuccess &&
                                    (e = hipMemset(X.state, 0, 16)) == hipSuccess && (e = hipMemset(X.unsorted, 0, 4)) == hipSuccess &&
                                    (e = hipMemcpy(X.lin_off, D.idx.lin_off.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice)) == hipSuccess;
        return ok ? nullptr : "index request set-up";
    }
    // the batch's part of the index; also for a batch without records: the end state it leaves is the next batch's start
    bool batch(const Batch &B, Scratch S, std::string &err) {
        const long long n = B.n_rec;
        auto [voff_, out_voff_, key, head, head_off, out_key] = S.take<6>();
        unsigned long long *voff = (unsigned long long *)voff_, *out_voff = (unsigned long long *)out_voff_;
        hipLaunchKernelGGL(k_bam_index, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, B.stream, B.rec_start, n, B.M, B.end, kept_desc[B.slot],
                           kept_boff[B.slot], B.info.n_blocks, (unsigned long long)B.info.file_off, (unsigned long long)B.info.comp_bytes,
                           (long long)B.info.infl_bytes, B.carry_pos, parity, X, voff, key, head);
        parity ^= 1;
        long long n_heads = 0;
        if (n > 0) {
            if (!B.scan(head, head_off)) { err = "scan of the index run heads failed"; return false; }
            hipLaunchKernelGGL(k_bam_index_compact, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(WAVE), 0, B.stream, n, head, head_off, voff, key, out_voff, out_key);
            if (fetch_sync(B.stream, {{&n_heads, head_off + n, 8}}, nullptr, "index kernels", err) != CORAL_OK) return false;
            std::vector<long long> hk((size_t)n_heads);
            std::vector<unsigned long long> hv((size_t)n_heads);
            if (!dev_get(hk.data(), out_key, (size_t)n_heads * 8) || !dev_get(hv.data(), out_voff, (size_t)n_heads * 8)) {
                err = "copy of the index run heads failed";
                return false;
            }
            for (long long j = 0; j < n_heads; ++j) B.D.idx.add_head(hk[(size_t)j], hv[(size_t)j]);
        }
        return launched("index", err);
    }
    // false: a copy failed.  Sets D.idx.unsorted when the device saw the order broken; it stays set: no index can be built
    bool finish(Decoded &D, int) const {
        IndexPartial &P = D.idx;
        const size_t n_ref = (size_t)X.n_ref;
        unsigned long long state[2] = {0, 0}, no_coor = 0;
        int32_t dev_unsorted = 0;
        if (!(dev_get(P.lin.data(), X.lin, P.lin.size() * 8) && dev_get(P.n_mapped.data(), X.n_mapped, n_ref * 8) && dev_get(P.n_unmapped.data(), X.n_unmapped, n_ref * 8) &&
              dev_get(&no_coor, X.n_no_coor, 8) && dev_get(state, X.state, 16) && dev_get(&dev_unsorted, X.unsorted, 4)))
            return false;
        if (dev_unsorted) P.unsorted = true;
        if (!P.unsorted) { P.n_no_coor = (int64_t)no_coor; P.end_voff = state[parity]; }
        return true;
    }
};
