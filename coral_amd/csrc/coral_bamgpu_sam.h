// coral_bamgpu_sam.h - `import`: a mapper's SAM text as a BAM file, its records made ON THE GPU (included by coral_bamgpu.hip,
// behind coral_bamgpu_deflate.h: it needs BlockDesc, Carver and RecordSink of this translation unit).
//
//   k_sam_lines   newline positions -> line starts: per 1 024-byte tile a count, hipcub's scan over the tiles, then the same
//                 search again with every newline's rank
//   k_sam_size    one wave per line (coral_sam_core.h, the device backend): field boundaries, validation, the filter decision,
//                 the record's exact byte count; the lowest refused line through one atomicMin
//   k_sam_encode  one wave per line: the record at its offset of the scan, behind the sink's carried bytes; SEQ and QUAL in
//                 512-byte steps over the lanes, the CIGAR 64 bytes per step, names, numbers and tags as the tail
//   k_sam_fixup   the 'f' values the device does not convert exactly, converted by the host with strtof, scattered in
//
// The text goes up once, the record bytes are deflated where they stand (RecordSink) and only compressed bytes come back.
// Replaces `samtools view -bS` behind the mapper (/root/reference/scripts/align_nanopore_reads.sh:34-38).
#pragma once
// (coral_bamgpu.hip includes coral_sam_host.h and the system headers this file needs, outside its anonymous namespace)

#define SAM_GRID_CAP 2048                                            // one-wave workgroups, grid-stride, as the other side kernels
#define SAM_TILE 1024                                                // bytes of text per wave and step of k_sam_lines: 16 per lane
#define SAM_BATCH_DEFAULT (128ll << 20)
#define SAM_BATCH_MAX (1ll << 30)
#define SAM_TEXT_SLACK 256                                           // readable bytes behind the text (a tile is read whole)

struct SamFix { uint64_t text_off, out_off; };                       // a value for the host: where its text starts, where its 4 bytes go
struct SamStat { unsigned long long err, written, dropped; uint32_t n_fix, pad; };

// Backend of coral_sam::line for one wave.
struct SamWave {
    int lane;
    const uint8_t *text;
    uint8_t *out;
    SamFix *fix;
    uint32_t *n_fix, fix_cap;
    template <class F> __device__ __forceinline__ uint64_t ballot(F f) { return __ballot(f(lane)); }
    template <class F> __device__ __forceinline__ void each(F f) { f(lane); }
    template <class F> __device__ __forceinline__ uint64_t sum(F f) {
        unsigned long long v = f(lane);
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) v += __shfl_xor(v, d);
        return v;
    }
    __device__ __forceinline__ bool leader() const { return lane == 0; }
    __device__ __forceinline__ uint32_t uni(uint32_t x) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    __device__ __forceinline__ void slow_float(const uint8_t *at, uint32_t, uint8_t *dst) {
        if (lane != 0) return;
        const uint32_t k = atomicAdd(n_fix, 1u);
        if (k < fix_cap) fix[k] = SamFix{(uint64_t)(at - text), (uint64_t)(dst - out)};
    }
};

// Pass 1 (rank == nullptr): count[t] = newlines of tile t.  Pass 2: line_start[1 + r] = behind the newline of rank r, for
// r < line_cap.  The text is read in aligned 16-byte pieces, whole tiles: SAM_TEXT_SLACK bytes behind it are readable.
__global__ __launch_bounds__(WAVE) void k_sam_lines(const uint8_t *__restrict__ text, long long n, long long n_tiles, uint32_t *__restrict__ count,
                                                     const uint32_t *__restrict__ rank, uint32_t *__restrict__ line_start, uint32_t line_cap) {
    const int lane = threadIdx.x;
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long long at = t * SAM_TILE + 16 * lane;
        const uint4 v = *reinterpret_cast<const uint4 *>(text + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t mask = 0;                                           // bit k: byte at + k is a newline of the text
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (((w[k >> 2] >> (8 * (k & 3))) & 255u) == 10u && at + k < n) mask |= 1u << k;
        const uint32_t mine = (uint32_t)__popc(mask);
        uint32_t s = mine;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)s, d);
            if (lane >= d) s += u;
        }
        if (!rank) {
            if (lane == WAVE - 1) count[t] = s;
            continue;
        }
        uint32_t r = rank[t] + s - mine;
        for (uint32_t m = mask; m; m &= m - 1, ++r)
            if (r < line_cap) line_start[1 + r] = (uint32_t)(at + __builtin_ctz(m) + 1);
    }
}

// One wave per line, grid-stride.  size[i]: the record's bytes (0: dropped, or refused); size[n_lines] = 0 for the scan.
__global__ __launch_bounds__(WAVE) void k_sam_size(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start, long long n_lines, coral_sam::Contigs C,
                                                    coral_sam::Keep K, long long first_line, long long *__restrict__ size, SamStat *stat) {
    SamWave w{(int)threadIdx.x, text, nullptr, nullptr, nullptr, 0};
    unsigned long long written = 0, dropped = 0;
    for (long long i = blockIdx.x; i < n_lines; i += gridDim.x) {
        const uint32_t a = line_start[i], b = line_start[i + 1] - 1;  // (b: the line's '\n')
        uint32_t err;
        bool drop;
        const uint64_t bytes = coral_sam::line<SamWave, false>(w, text + a, b - a, C, K, nullptr, err, drop);
        if (w.lane == 0) {
            size[i] = (long long)bytes;
            if (err != coral_sam::F_NONE) atomicMin(&stat->err, ((unsigned long long)(first_line + i) << 8) | err);
        }
        written += bytes > 0;
        dropped += drop;
    }
    if (blockIdx.x == 0 && w.lane == 0) size[n_lines] = 0;
    if (w.lane == 0) {
        if (written) atomicAdd(&stat->written, written);
        if (dropped) atomicAdd(&stat->dropped, dropped);
    }
}

// One wave per written line, grid-stride: its record at out + off[i] (any alignment).
__global__ __launch_bounds__(WAVE) void k_sam_encode(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start, long long n_lines, coral_sam::Contigs C,
                                                      coral_sam::Keep K, const long long *__restrict__ off, uint8_t *__restrict__ out, SamFix *fix, SamStat *stat,
                                                      uint32_t fix_cap) {
    SamWave w{(int)threadIdx.x, text, out, fix, &stat->n_fix, fix_cap};
    for (long long i = blockIdx.x; i < n_lines; i += gridDim.x) {
        const long long o = off[i];
        if (off[i + 1] == o) continue;
        const uint32_t a = line_start[i], b = line_start[i + 1] - 1;
        uint32_t err;
        bool drop;
        coral_sam::line<SamWave, true>(w, text + a, b - a, C, K, out + o, err, drop);
    }
}

// fix[k] = (output offset, the value's bits): four bytes each, at any alignment
__global__ void k_sam_fixup(const SamFix *__restrict__ fix, uint32_t n, uint8_t *__restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) coral_sam::store32(out + fix[k].text_off, (uint32_t)fix[k].out_off);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// The workspace of coral_samgpu_import, carved in this order.  Sizes: a line is at least 16 bytes of text or refused, so a batch
// of B bytes has at most B / 16 + 2 lines the device needs room for (more: the host names the refused line); the records of a
// batch take at most coral_sam::record_bound bytes, and 0xff00 more for the sink's carried bytes stand in front.
struct SamWorkspace {
    uint8_t *text, *out, *names;
    uint32_t *tile_count, *tile_rank, *line_start, *slots;
    long long *size, *off;
    int64_t *name_off;
    SamFix *fix;
    SamStat *stat;
    void *tmp;
    size_t line_cap, n_tiles, out_cap, fix_cap, tmp_bytes, bytes;
    SamWorkspace(void *ws, size_t batch, RecordSink &sink, size_t n_ref, size_t n_slots, size_t names_bytes) {
        Carver take{(uintptr_t)ws};
        line_cap = batch / 16 + 2;
        n_tiles = (batch + 1 + SAM_TILE - 1) / SAM_TILE;
        out_cap = (size_t)coral_sam::record_bound(batch + 1, line_cap);
        fix_cap = batch / 64 + 16;
        text = (uint8_t *)take(n_tiles * SAM_TILE + SAM_TEXT_SLACK);
        tile_count = (uint32_t *)take((n_tiles + 1) * 4);
        tile_rank = (uint32_t *)take((n_tiles + 1) * 4);
        line_start = (uint32_t *)take((line_cap + 2) * 4);
        size = (long long *)take((line_cap + 2) * 8);
        off = (long long *)take((line_cap + 2) * 8);
        out = (uint8_t *)take((size_t)coral_deflate::BLOCK_MAX + out_cap + 256);
        fix = (SamFix *)take(fix_cap * sizeof(SamFix));
        stat = (SamStat *)take(sizeof(SamStat));
        names = (uint8_t *)take(names_bytes + 1);
        name_off = (int64_t *)take((n_ref + 1) * 8);
        slots = (uint32_t *)take((n_slots + 1) * 4);
        size_t t1 = 0, t2 = 0;
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(n_tiles + 1));
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (long long *)nullptr, (long long *)nullptr, (int)(line_cap + 1));
        tmp_bytes = std::max(t1, t2) + 256;
        tmp = take(tmp_bytes);
        sink.chunk = std::min(sink.chunk, ((size_t)coral_deflate::BLOCK_MAX + out_cap) / coral_deflate::BLOCK_MAX + 2);      // (no batch can fill more)
        sink.carve(take);
        bytes = take.used;
    }
};

inline int sam_fail(int code, const std::string &msg) { set_error(msg); return code; }
inline size_t sam_chunk(int32_t chunk_blocks) { return chunk_blocks > 0 ? (size_t)chunk_blocks : (size_t)DEFL_CHUNK_BLOCKS; }
inline size_t sam_batch(int64_t batch_bytes) { return batch_bytes > 0 ? (size_t)batch_bytes : (size_t)SAM_BATCH_DEFAULT; }

inline int64_t samgpu_workspace_bytes(int64_t batch_bytes, int32_t chunk_blocks, int32_t n_ref, int32_t n_slots, int64_t names_bytes) {
    if (batch_bytes < 0 || batch_bytes > SAM_BATCH_MAX || chunk_blocks < 0 || chunk_blocks > 16384 || n_ref < 0 || n_slots < 0 || names_bytes < 0) return CORAL_ERR_ARG;
    RecordSink sink;
    sink.chunk = sam_chunk(chunk_blocks);
    return (int64_t)SamWorkspace(nullptr, sam_batch(batch_bytes), sink, (size_t)n_ref, (size_t)n_slots, (size_t)names_bytes).bytes + 256;
}

// The feeder: a thread that reads lead ++ fd into two pinned buffers in turn, cuts each batch behind its last '\n' and moves the
// partial line to the front of the other buffer.  The text's last line gets its '\n' if it lacks one, so that every batch is
// whole '\n'-terminated lines.  A buffer is the consumer's from `take` to `release`.
struct SamFeeder {
    int fd = -1;
    const uint8_t *lead = nullptr;
    size_t lead_left = 0, cap = 0;
    uint8_t *buf[2] = {nullptr, nullptr};
    size_t n[2] = {0, 0};
    int state[2] = {0, 0};                   // 0: the feeder's, 1: a batch for the consumer
    bool last[2] = {false, false}, stop = false, too_long = false, io_failed = false, done = false;
    std::mutex mu;
    std::condition_variable cv;
    std::thread th;

    size_t pull(uint8_t *dst, size_t want) {                         // up to `want` bytes; 0: the end
        if (lead_left > 0) {
            const size_t k = std::min(want, lead_left);
            memcpy(dst, lead, k);
            lead += k;
            lead_left -= k;
            return k;
        }
        for (;;) {
            const ssize_t k = read(fd, dst, std::min<size_t>(want, 8u << 20));
            if (k >= 0) return (size_t)k;
            if (errno != EINTR) { io_failed = true; return 0; }
        }
    }
    void run() {
        size_t have = 0;                                             // bytes at the front of buf[k & 1]: the partial line
        for (size_t k = 0;; ++k) {
            const int s = (int)(k & 1);
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return state[s] == 0 || stop; });
                if (stop) break;
            }
            bool end = false;
            while (have < cap && !end) {
                const size_t got = pull(buf[s] + have, cap - have);
                end = got == 0;
                have += got;
                std::lock_guard<std::mutex> lk(mu);
                if (stop) break;
            }
            size_t whole = have, tail = 0;
            if (end) {
                if (have > 0 && buf[s][have - 1] != '\n') buf[s][have++] = '\n';      // (the buffers have room for it behind `cap` bytes)
                whole = have;
            } else {
                while (whole > 0 && buf[s][whole - 1] != '\n') --whole;
                tail = have - whole;
            }
            std::unique_lock<std::mutex> lk(mu);
            if (stop) break;
            if (!end && whole == 0) { too_long = true; done = true; cv.notify_all(); return; }
            if (io_failed) { done = true; cv.notify_all(); return; }
            if (tail > 0) {                                          // the partial line leads the next batch: the other buffer must be free
                cv.wait(lk, [&] { return state[s ^ 1] == 0 || stop; });
                if (stop) break;
                memcpy(buf[s ^ 1], buf[s] + whole, tail);
            }
            n[s] = whole;
            last[s] = end;
            state[s] = 1;
            have = tail;
            cv.notify_all();
            if (end) break;
        }
        std::lock_guard<std::mutex> lk(mu);
        done = true;
        cv.notify_all();
    }
    // batch k -> its buffer; false: none (the feeder failed, or stopped)
    bool take(size_t k, uint8_t *&data, size_t &bytes, bool &is_last) {
        std::unique_lock<std::mutex> lk(mu);
        const int s = (int)(k & 1);
        cv.wait(lk, [&] { return state[s] == 1 || done; });
        if (state[s] != 1) return false;
        data = buf[s];
        bytes = n[s];
        is_last = last[s];
        return true;
    }
    void release(size_t k) {
        std::lock_guard<std::mutex> lk(mu);
        state[k & 1] = 0;
        cv.notify_all();
    }
    void shut() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        if (th.joinable()) th.join();
    }
};

inline int samgpu_import(int32_t fd, const uint8_t *lead, int64_t lead_bytes, int64_t first_line, const char *out_path, const uint8_t *bam, int64_t bam_bytes,
                         const uint8_t *names, const int64_t *name_off, const uint32_t *slots, int32_t n_ref, int32_t n_slots, const int32_t *keep, int64_t batch_bytes,
                         int32_t chunk_blocks, void *workspace, int64_t workspace_bytes, hipStream_t stream, int64_t *stats, double *seconds) {
    const std::string me = "coral_samgpu_import: ";
    if (fd < 0 || lead_bytes < 0 || (lead_bytes > 0 && !lead) || !out_path || !bam || bam_bytes < 12 || !keep || !stats || !seconds)
        return sam_fail(CORAL_ERR_ARG, me + "a missing argument");
    if (n_ref < 0 || n_slots < 0 || (n_slots & (n_slots - 1)) || (n_ref > 0 && (!names || !name_off || !slots || n_slots < 2 * n_ref)))
        return sam_fail(CORAL_ERR_ARG, me + "the contig table: n_slots must be a power of two >= 2 n_ref, with its arrays");
    for (int k = 0; k < 4; ++k)
        if (keep[k] < 0) return sam_fail(CORAL_ERR_ARG, me + "record filter: negative value");
    const int64_t names_bytes = n_ref > 0 ? name_off[n_ref] : 0;
    const int64_t need = samgpu_workspace_bytes(batch_bytes, chunk_blocks, n_ref, n_slots, names_bytes);
    if (need < 0) return sam_fail(CORAL_ERR_ARG, me + "batch_bytes must be 0..2^30 and chunk_blocks 0..16384");
    if (!workspace || workspace_bytes < need) return sam_fail(CORAL_ERR_ARG, me + "the workspace is smaller than coral_samgpu_workspace_bytes");
    const size_t batch = sam_batch(batch_bytes);
    const auto t_all = std::chrono::steady_clock::now();

    RecordSink sink;
    sink.path = out_path;
    sink.header.assign(bam, bam + bam_bytes);
    sink.chunk = sam_chunk(chunk_blocks);
    const SamWorkspace W((void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255), batch, sink, (size_t)n_ref, (size_t)n_slots, (size_t)names_bytes);
    if (pack_tmp_bytes((int)sink.chunk) > DEFL_SCAN_TMP) return sam_fail(CORAL_ERR_HIP, me + "hipcub asks for more temporary storage than reserved");
    if (!(sink.fp = fopen(out_path, "wb"))) return sam_fail(CORAL_ERR_ARG, std::string("cannot create ") + out_path);

    int rc = CORAL_OK;
    std::string err;
    auto bad = [&](int code, const std::string &what) { if (rc == CORAL_OK) { rc = code; err = what; } return false; };
    auto hip_ok = [&](hipError_t e, const char *what) { return e == hipSuccess || bad(CORAL_ERR_HIP, me + what + ": " + hipGetErrorString(e)); };
    SamFeeder F;
    F.fd = fd;
    F.lead = lead;
    F.lead_left = (size_t)lead_bytes;
    F.cap = batch;
    SamStat *h_stat = nullptr;
    SamFix *h_fix = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool good = hip_ok(hipHostMalloc((void **)&h_stat, 256, hipHostMallocDefault), "hipHostMalloc") &&
                hip_ok(hipHostMalloc((void **)&h_fix, W.fix_cap * sizeof(SamFix), hipHostMallocDefault), "hipHostMalloc");
    for (int i = 0; i < 2 && good; ++i) good = hip_ok(hipHostMalloc((void **)&F.buf[i], batch + 16, hipHostMallocDefault), "hipHostMalloc");
    for (int i = 0; i < 4 && good; ++i) good = hip_ok(hipEventCreate(&ev[i]), "hipEventCreate");
    if (good && n_ref > 0)
        good = hip_ok(hipMemcpyAsync(W.names, names, (size_t)names_bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync") &&
               hip_ok(hipMemcpyAsync(W.name_off, name_off, ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, stream), "hipMemcpyAsync") &&
               hip_ok(hipMemcpyAsync(W.slots, slots, (size_t)n_slots * 4, hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
    good = good && hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize");
    if (good && !(sink.start() && sink.write_header(W.out, (size_t)coral_deflate::BLOCK_MAX + W.out_cap))) good = bad(CORAL_ERR_HIP, sink.error.empty() ? me + "record sink set-up" : sink.error);
    const coral_sam::Contigs C{W.names, W.name_off, W.slots, n_ref, (uint32_t)n_slots};
    const coral_sam::Keep K{(uint32_t)keep[0], (uint32_t)keep[1], (uint32_t)keep[2], (uint32_t)keep[3]};
    int64_t lines = 0, written = 0, dropped = 0, text_bytes = 0, batches = 0, fixups = 0;
    double wait_s = 0, size_s = 0, encode_s = 0;
    if (good) F.th = std::thread([&F] { F.run(); });

    for (size_t k = 0; good; ++k) {
        uint8_t *h_text = nullptr;
        size_t n = 0;
        bool is_last = false;
        const auto t0 = std::chrono::steady_clock::now();
        if (!F.take(k, h_text, n, is_last)) {
            if (F.too_long) bad(CORAL_ERR_CAPACITY, "SAM line " + std::to_string(first_line + lines) + " does not fit a batch of " + std::to_string(batch) + " bytes (batch_bytes)");
            else if (F.io_failed) bad(CORAL_ERR_FORMAT, me + "reading the text failed");
            else bad(CORAL_ERR_HIP, me + "the feeder stopped");
            break;
        }
        wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (n > 0) {
            ++batches;
            text_bytes += (int64_t)n;
            const long long n_tiles = (long long)((n + SAM_TILE - 1) / SAM_TILE);
            const unsigned tile_grid = (unsigned)std::min<long long>(n_tiles, SAM_GRID_CAP);
            size_t tmp = W.tmp_bytes;
            good = hip_ok(hipMemcpyAsync(W.text, h_text, n, hipMemcpyHostToDevice, stream), "hipMemcpyAsync") &&
                   hip_ok(hipMemsetAsync(W.stat, 0xff, 8, stream), "hipMemsetAsync") && hip_ok(hipMemsetAsync((uint8_t *)W.stat + 8, 0, sizeof(SamStat) - 8, stream), "hipMemsetAsync") &&
                   hip_ok(hipMemsetAsync(W.tile_count + n_tiles, 0, 4, stream), "hipMemsetAsync") && hip_ok(hipMemsetAsync(W.line_start, 0, 4, stream), "hipMemsetAsync");
            if (!good) break;
            hipLaunchKernelGGL(k_sam_lines, dim3(tile_grid), dim3(WAVE), 0, stream, W.text, (long long)n, n_tiles, W.tile_count, (const uint32_t *)nullptr, W.line_start, (uint32_t)W.line_cap);
            good = hip_ok(hipGetLastError(), "k_sam_lines") &&
                   hip_ok(hipcub::DeviceScan::ExclusiveSum(W.tmp, tmp, W.tile_count, W.tile_rank, (int)(n_tiles + 1), stream), "scan of the tiles' newlines");
            if (!good) break;
            hipLaunchKernelGGL(k_sam_lines, dim3(tile_grid), dim3(WAVE), 0, stream, W.text, (long long)n, n_tiles, W.tile_count, (const uint32_t *)W.tile_rank, W.line_start, (uint32_t)W.line_cap);
            uint32_t n_lines32 = 0;
            good = hip_ok(hipGetLastError(), "k_sam_lines") && hip_ok(hipMemcpyAsync(&h_stat->pad, W.tile_rank + n_tiles, 4, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync") &&
                   hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize");
            if (!good) break;
            n_lines32 = h_stat->pad;
            const long long n_lines = n_lines32;
            coral_sam::EncodeCounts X;
            auto host_refusal = [&]() {                              // the error path only: the host names the lowest refused line of the pinned text
                const coral_sam::Contigs HC{names, name_off, slots, n_ref, (uint32_t)n_slots};
                return coral_sam::encode_text(h_text, (int64_t)n, first_line + lines, HC, K, nullptr, 0, X) == 1;
            };
            if ((size_t)n_lines > W.line_cap) {                      // a line of fewer than 16 bytes: refused for certain
                if (host_refusal()) bad(CORAL_ERR_FORMAT, coral_sam::refusal_text(X.err_line, (uint32_t)X.err_field));
                else bad(CORAL_ERR_CAPACITY, me + "more lines in a batch than its arrays hold");
                break;
            }
            const unsigned line_grid = (unsigned)std::min<long long>(n_lines, SAM_GRID_CAP);
            tmp = W.tmp_bytes;
            good = hip_ok(hipEventRecord(ev[0], stream), "hipEventRecord");
            hipLaunchKernelGGL(k_sam_size, dim3(line_grid), dim3(WAVE), 0, stream, W.text, W.line_start, n_lines, C, K, (long long)(first_line + lines), W.size, W.stat);
            good = good && hip_ok(hipGetLastError(), "k_sam_size") && hip_ok(hipEventRecord(ev[1], stream), "hipEventRecord") &&
                   hip_ok(hipcub::DeviceScan::ExclusiveSum(W.tmp, tmp, W.size, W.off, (int)(n_lines + 1), stream), "scan of the record sizes") &&
                   hip_ok(hipMemcpyAsync(h_stat, W.stat, sizeof(SamStat), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync") &&
                   hip_ok(hipMemcpyAsync((uint8_t *)h_stat + 64, W.off + n_lines, 8, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync") &&
                   hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize");
            if (!good) break;
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) size_s += ms * 1e-3;
            if (h_stat->err != ~0ull) { bad(CORAL_ERR_FORMAT, coral_sam::refusal_text((int64_t)(h_stat->err >> 8), (uint32_t)(h_stat->err & 255))); break; }
            long long total = 0;
            memcpy(&total, (uint8_t *)h_stat + 64, 8);
            // the bound the buffer was sized by, asserted on the batch's own numbers
            if (total < 0 || (uint64_t)total > coral_sam::record_bound(n, (uint64_t)n_lines) || (size_t)total > W.out_cap) { bad(CORAL_ERR_CAPACITY, me + "the records of a batch exceed their bound"); break; }
            const long long n_written = (long long)h_stat->written;
            if (total > 0) {
                if (!sink.wait_moved(stream)) { bad(CORAL_ERR_HIP, sink.error); break; }
                uint8_t *dst = W.out + sink.carry;
                good = hip_ok(hipEventRecord(ev[2], stream), "hipEventRecord");
                hipLaunchKernelGGL(k_sam_encode, dim3(line_grid), dim3(WAVE), 0, stream, W.text, W.line_start, n_lines, C, K, W.off, dst, W.fix, W.stat, (uint32_t)W.fix_cap);
                good = good && hip_ok(hipGetLastError(), "k_sam_encode") && hip_ok(hipEventRecord(ev[3], stream), "hipEventRecord") &&
                       hip_ok(hipMemcpyAsync(h_stat, W.stat, sizeof(SamStat), hipMemcpyDeviceToHost, stream), "hipMemcpyAsync") &&
                       hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize");
                if (!good) break;
                if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) encode_s += ms * 1e-3;
                const uint32_t n_fix = h_stat->n_fix;
                if (n_fix > W.fix_cap) { bad(CORAL_ERR_CAPACITY, me + "more float values outside the exact path in a batch than batch_bytes / 64"); break; }
                if (n_fix > 0) {                                      // strtof of the pinned text, scattered in before the sink reads the bytes
                    good = hip_ok(hipMemcpy(h_fix, W.fix, n_fix * sizeof(SamFix), hipMemcpyDeviceToHost), "hipMemcpy");
                    for (uint32_t i = 0; i < n_fix && good; ++i) {
                        const uint64_t a = h_fix[i].text_off;
                        if (a >= n || h_fix[i].out_off + 4 > (uint64_t)total) { good = bad(CORAL_ERR_HIP, me + "a float fix-up outside the batch"); break; }
                        uint64_t b = a;
                        while (b < n && h_text[b] != ',' && h_text[b] != '\t' && h_text[b] != '\n') ++b;
                        h_fix[i] = SamFix{h_fix[i].out_off, coral_sam::HostLanes::strtof_bits(h_text + a, (uint32_t)(b - a))};
                    }
                    if (!good) break;
                    good = hip_ok(hipMemcpyAsync(W.fix, h_fix, n_fix * sizeof(SamFix), hipMemcpyHostToDevice, stream), "hipMemcpyAsync");
                    hipLaunchKernelGGL(k_sam_fixup, dim3((n_fix + 255) / 256), dim3(256), 0, stream, W.fix, n_fix, dst);
                    good = good && hip_ok(hipGetLastError(), "k_sam_fixup") && hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize");      // (h_fix is used again)
                    if (!good) break;
                    fixups += n_fix;
                }
                if (!sink.batch(W.out, total, n_written, stream)) { bad(CORAL_ERR_HIP, sink.error); break; }
            }
            lines += n_lines;
            written += n_written;
            dropped += (int64_t)h_stat->dropped;
        }
        // (the sink reads W.out on its own stream; W.text and the pinned text are free: every kernel that read them has been waited for)
        F.release(k);
        if (is_last) break;
    }
    good = rc == CORAL_OK;
    F.shut();
    if (good && !sink.finish(W.out)) bad(sink.error.find("writing") != std::string::npos ? CORAL_ERR_FORMAT : CORAL_ERR_HIP, sink.error);
    (void)hipStreamSynchronize(stream);                  // nothing of this call is left on the stream, whatever happened
    if (sink.s) (void)hipStreamSynchronize(sink.s);
    for (int i = 0; i < 2; ++i) if (F.buf[i]) (void)hipHostFree(F.buf[i]);
    if (h_stat) (void)hipHostFree(h_stat);
    if (h_fix) (void)hipHostFree(h_fix);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (rc != CORAL_OK) {
        if (sink.fp) { fclose(sink.fp); sink.fp = nullptr; }
        remove(out_path);
        return sam_fail(rc, err);
    }
    stats[0] = lines; stats[1] = written; stats[2] = dropped; stats[3] = text_bytes; stats[4] = sink.bytes; stats[5] = sink.file_bytes; stats[6] = sink.members;
    stats[7] = batches; stats[8] = fixups;
    seconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_all).count(); seconds[1] = wait_s; seconds[2] = size_s; seconds[3] = encode_s;
    return CORAL_OK;
}
