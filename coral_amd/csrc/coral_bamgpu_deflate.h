// coral_bamgpu_deflate.h - BGZF blocks made ON THE GPU (included by coral_bamgpu.hip, behind coral_bamgpu_reads.h): the writers
// behind bam.RecordBytes.write(device=...) and bam.sort_bam(write_device=...) deflate on the device instead of calling zlib on
// the host (coral_bgzf_write).  The writers touch nothing of the decode pipeline; RecordSink, at the end, is the one piece that
// does: the file a records request streams to (CORAL_SINK_BAM of coral_bamgpu_open_request), with its arrays in the decode's workspace.
//
//   k_bgzf_deflate  one wave per input block of at most 0xff00 bytes: one complete BGZF member (header with BSIZE, one dynamic or
//                   stored DEFLATE block, CRC-32, ISIZE) into the block's 64 KiB slot - coral_deflate_core.h, the device backend
//   k_bgzf_pack     hipcub's scan over the member lengths, then one wave per member: the fixed-stride slots gathered into one
//                   contiguous byte string with reads_window / reads_run (coral_bamgpu_reads.h)
//   k_bgzf_chunk_desc  the descriptors of a chunk of consecutive 0xff00-byte blocks, made on the device (RecordSink)
//
// Replaces what the reference's workflow gets from `samtools view -b` / `samtools sort` when they write their output
// (/root/reference/scripts/align_nanopore_reads.sh:44, :49: htslib's bgzf_write + zlib deflate).
#pragma once
#include "coral_deflate_core.h"

#define DEFL_GRID_CAP 2048                                           // one-wave workgroups, grid-stride, as the other side kernels
#define DEFL_TOKEN_BYTES ((size_t)coral_deflate::BLOCK_MAX * 4)      // per resident wave: at most one 32-bit token per input byte
#define DEFL_CHUNK_BLOCKS 1024                                       // blocks per chunk of coral_bgzf_write_gpu with the workspace it asks for
#define DEFL_SCAN_TMP (64u << 10)                                    // hipcub's temporary storage for a scan over one chunk's lengths

// Backend of coral_deflate::Deflater for one wave.  LDS accesses of one wave are executed in order, so a fence is a compiler
// barrier with the wave's memory counters drained; the tokens in global memory are written and read back by the same wave.
struct DeflWave {
    int lane;
    unsigned long long votes;
    uint32_t total;
    __device__ __forceinline__ uint32_t uni(uint32_t x) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    __device__ __forceinline__ void fence() {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void add_count(uint32_t *c) { atomicAdd(c, 1u); }
    __device__ __forceinline__ void or_bits(uint32_t *p, uint32_t v) { atomicOr(p, v); }
    // The largest value of the lanes that name the same slot: every lane stores, the losers that hold a larger value store again.
    // Which lane's store lands last in a round does not matter - a slot only ever grows and ends at the maximum.
    __device__ __forceinline__ void store_max16(uint16_t *p, uint32_t v) {
        volatile uint16_t *q = p;
        for (;;) {
            const bool need = (uint32_t)*q < v;
            if (__ballot(need) == 0ull) break;
            if (need) *q = (uint16_t)v;
            fence();
        }
    }
    __device__ __forceinline__ void vote(int, bool p) { votes = __ballot(p); }
    __device__ __forceinline__ unsigned long long vote_mask() const { return votes; }
    __device__ __forceinline__ uint32_t scan_excl(uint32_t x) {
        uint32_t s = x;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)s, d);
            if (lane >= d) s += t;
        }
        total = (uint32_t)__builtin_amdgcn_readlane((int)s, WAVE - 1);
        return s - x;
    }
    __device__ __forceinline__ uint32_t scan_total() const { return total; }
};

// One wave per block, in one-wave workgroups, grid-stride.  desc[b] = {src_off, src_len <= 0xff00, dst_off (a multiple of 4), 0};
// the member goes to out + dst_off (a slot of 64 KiB), its length to member_bytes[b] (0 for a block that is too long: nothing is
// written).  LDS: coral_deflate::State, 22 528 bytes per wave (the 8 192 x 16-bit hash table is 16 KiB of it) -> 7 waves per CU.
// `tokens`: DEFL_TOKEN_BYTES per workgroup of the launch.
__global__ __launch_bounds__(WAVE) void k_bgzf_deflate(const uint8_t *__restrict__ in, const BlockDesc *__restrict__ desc, int n_blocks,
                                                        uint8_t *__restrict__ out, uint32_t *__restrict__ member_bytes, uint32_t *tokens) {
    __shared__ coral_deflate::State S;
    const int lane = threadIdx.x;
    uint32_t *tok = tokens + (size_t)blockIdx.x * coral_deflate::BLOCK_MAX;
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const BlockDesc d = desc[b];
        if (d.src_len > (uint32_t)coral_deflate::BLOCK_MAX || (d.dst_off & 3u)) {
            if (lane == 0) member_bytes[b] = 0;
            continue;
        }
        DeflWave w;
        w.lane = lane;
        w.votes = 0;
        w.total = 0;
        coral_deflate::Deflater<DeflWave> D(w, &S, in + d.src_off, d.src_len, reinterpret_cast<uint32_t *>(out + d.dst_off), tok);
        const uint32_t bytes = D.run();
        if (lane == 0) member_bytes[b] = bytes;
    }
}

// One wave per member, grid-stride: member b, member_bytes[b] bytes at slots + b * 64 KiB, goes to packed + off[b] (off: the
// exclusive scan of the lengths).  Source and destination have byte alignments of their own: reads_run stores aligned 16-byte
// chunks of the OUTPUT (a member's first and last chunk byte by byte, only its own bytes), each filled by reads_window from the
// two aligned source chunks that cover it.  Every output byte has one writer: no atomics.
__global__ __launch_bounds__(WAVE) void k_bgzf_pack(const uint8_t *__restrict__ slots, int n_blocks, const uint32_t *__restrict__ member_bytes,
                                                     const uint32_t *__restrict__ off, uint8_t *__restrict__ packed) {
    const int lane = threadIdx.x;
    const long long slots_bytes = (long long)n_blocks * coral_deflate::SLOT_BYTES;
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const long long from = (long long)b * coral_deflate::SLOT_BYTES, bytes = member_bytes[b];
        if (bytes > 0) reads_run(packed, (long long)off[b], 0, bytes, lane, [&](long long j0) { return reads_window(slots, from + j0, slots_bytes); });
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
inline size_t deflate_scratch_bytes(long long n_blocks) { return (size_t)std::min<long long>(std::max<long long>(n_blocks, 0), DEFL_GRID_CAP) * DEFL_TOKEN_BYTES; }

inline hipError_t launch_deflate(const uint8_t *in, const uint32_t *desc, int n_blocks, uint8_t *out, uint32_t *member_bytes, void *scratch, hipStream_t stream) {
    hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)std::min(n_blocks, DEFL_GRID_CAP)), dim3(WAVE), 0, stream, in, (const BlockDesc *)desc, n_blocks, out,
                       member_bytes, (uint32_t *)scratch);
    return hipGetLastError();
}

// off[0 .. n_blocks] = where each member starts in `packed` (off[n_blocks]: all bytes; the caller keeps them below 2^32), then the gather.
inline hipError_t launch_pack(const uint8_t *slots, const uint32_t *member_bytes, int n_blocks, uint8_t *packed, uint32_t *off, void *tmp, size_t tmp_bytes,
                              hipStream_t stream) {
    hipError_t e = hipMemsetAsync(off, 0, 4, stream);
    if (e != hipSuccess) return e;
    if ((e = hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, member_bytes, off + 1, n_blocks, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)std::min(n_blocks, DEFL_GRID_CAP)), dim3(WAVE), 0, stream, slots, n_blocks, member_bytes, off, packed);
    return hipGetLastError();
}

inline size_t pack_tmp_bytes(int n_blocks) {
    size_t tmp = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, tmp, (const uint32_t *)nullptr, (uint32_t *)nullptr, std::max(n_blocks, 1));
    return tmp;
}

// The workspace of coral_bgzf_write_gpu for chunks of `blocks` blocks, carved in this order (every piece a multiple of 256 bytes)
struct DeflateWorkspace {
    uint8_t *in, *slots, *packed;
    uint32_t *desc, *member, *off;
    void *tokens, *tmp;
    size_t bytes;
    DeflateWorkspace(void *ws, size_t blocks) {
        Carver take{(uintptr_t)ws};
        in = (uint8_t *)take(blocks * coral_deflate::BLOCK_MAX);
        slots = (uint8_t *)take(blocks * coral_deflate::SLOT_BYTES);
        packed = (uint8_t *)take(blocks * coral_deflate::SLOT_BYTES);
        desc = (uint32_t *)take(blocks * sizeof(BlockDesc));
        member = (uint32_t *)take(blocks * 4);
        off = (uint32_t *)take((blocks + 1) * 4);
        tokens = take(deflate_scratch_bytes((long long)blocks));
        tmp = take(DEFL_SCAN_TMP);
        bytes = take.used;
    }
};

inline size_t write_gpu_workspace_bytes(size_t blocks) { return DeflateWorkspace(nullptr, blocks).bytes + 256; }      // (+ 256: the caller's pointer need not be aligned)

// coral_bgzf_write_gpu (include/coral_hip.h).  The blocks are those of coral_bgzf_write; chunks of consecutive blocks go up
// through two pinned buffers (chunk k + 1 is gathered on the host while chunk k is deflated), each chunk is deflated and packed,
// and only its packed bytes come back, to be written while the next chunk is on the device.  A member is a function of its
// block alone, so the file does not depend on how many blocks the workspace lets a chunk have.
inline int bgzf_write_gpu(const char *path, const uint8_t *const *parts, const int64_t *part_bytes, int32_t n_parts, void *workspace, int64_t workspace_bytes,
                          hipStream_t stream) {
    using coral_deflate::BLOCK_MAX;
    using coral_deflate::SLOT_BYTES;
    const char *me = "coral_bgzf_write_gpu: ";
    if (!path) { set_error(std::string(me) + "no path"); return CORAL_ERR_ARG; }
    if (n_parts < 0 || (n_parts > 0 && (!parts || !part_bytes))) { set_error(std::string(me) + "n_parts must be >= 0, with the parts and their sizes"); return CORAL_ERR_ARG; }
    struct Block { const uint8_t *p; uint32_t n; };
    std::vector<Block> blocks;
    for (int32_t k = 0; k < n_parts; ++k) {
        if (part_bytes[k] < 0 || (part_bytes[k] > 0 && !parts[k])) { set_error(std::string(me) + "bad part"); return CORAL_ERR_ARG; }
        for (size_t at = 0, n = (size_t)part_bytes[k]; at < n; at += BLOCK_MAX) blocks.push_back(Block{parts[k] + at, (uint32_t)std::min<size_t>(BLOCK_MAX, n - at)});
    }
    if (!workspace || workspace_bytes < (int64_t)write_gpu_workspace_bytes(1)) { set_error(std::string(me) + "no workspace, or one too small for a single block"); return CORAL_ERR_ARG; }
    uint8_t *base = (uint8_t *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const size_t usable = (size_t)workspace_bytes - (size_t)(base - (uint8_t *)workspace);
    size_t chunk = 1;                                   // the largest chunk (at most 16 384 blocks: its packed bytes stay below 2^32) that fits
    for (size_t lo = 1, hi = 16384; lo <= hi;) {
        const size_t mid = (lo + hi) / 2;
        if (DeflateWorkspace(nullptr, mid).bytes <= usable) { chunk = mid; lo = mid + 1; }
        else hi = mid - 1;
    }
    if (DeflateWorkspace(nullptr, chunk).bytes > usable) { set_error(std::string(me) + "workspace too small"); return CORAL_ERR_ARG; }
    if (pack_tmp_bytes((int)chunk) > DEFL_SCAN_TMP) { set_error(std::string(me) + "hipcub asks for more temporary storage than reserved"); return CORAL_ERR_HIP; }
    chunk = std::min(chunk, std::max<size_t>(blocks.size(), 1));
    const DeflateWorkspace W(base, chunk);
    FILE *fp = fopen(path, "wb");
    if (!fp) { set_error(std::string("cannot create ") + path); return CORAL_ERR_ARG; }

    uint8_t *h_in[2] = {nullptr, nullptr}, *h_out = nullptr;
    uint32_t *h_desc[2] = {nullptr, nullptr}, *h_total = nullptr;
    hipEvent_t ev_out = nullptr;
    std::string err;
    bool io_ok = true;
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && err.empty()) err = std::string(me) + what + ": " + hipGetErrorString(e);
        return e == hipSuccess;
    };
    const size_t n_chunks = (blocks.size() + chunk - 1) / chunk;
    auto chunk_blocks = [&](size_t k) { return std::min(chunk, blocks.size() - k * chunk); };
    auto fill = [&](size_t k) {                         // the chunk's blocks at a fixed stride, and their descriptors
        const size_t nb = chunk_blocks(k);
        for (size_t i = 0; i < nb; ++i) {
            const Block &b = blocks[k * chunk + i];
            memcpy(h_in[k & 1] + i * BLOCK_MAX, b.p, b.n);
            uint32_t *d = h_desc[k & 1] + 4 * i;
            d[0] = (uint32_t)(i * BLOCK_MAX); d[1] = b.n; d[2] = (uint32_t)(i * SLOT_BYTES); d[3] = 0;
        }
    };
    auto launch = [&](size_t k) {
        const size_t nb = chunk_blocks(k);
        const size_t in_bytes = (nb - 1) * BLOCK_MAX + blocks[k * chunk + nb - 1].n;
        return hip_ok(hipMemcpyAsync(W.in, h_in[k & 1], in_bytes, hipMemcpyHostToDevice, stream), "hipMemcpyAsync") &&
               hip_ok(hipMemcpyAsync(W.desc, h_desc[k & 1], nb * sizeof(BlockDesc), hipMemcpyHostToDevice, stream), "hipMemcpyAsync") &&
               hip_ok(launch_deflate(W.in, W.desc, (int)nb, W.slots, W.member, W.tokens, stream), "k_bgzf_deflate") &&
               hip_ok(launch_pack(W.slots, W.member, (int)nb, W.packed, W.off, W.tmp, DEFL_SCAN_TMP, stream), "k_bgzf_pack") &&
               hip_ok(hipMemcpyAsync(h_total, W.off + nb, 4, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
    };
    if (n_chunks > 0) {
        bool ok = hip_ok(hipHostMalloc((void **)&h_out, chunk * SLOT_BYTES, hipHostMallocDefault), "hipHostMalloc") &&
                  hip_ok(hipHostMalloc((void **)&h_total, 256, hipHostMallocDefault), "hipHostMalloc") &&
                  hip_ok(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming), "hipEventCreate");
        for (int i = 0; i < 2 && ok; ++i)
            ok = hip_ok(hipHostMalloc((void **)&h_in[i], chunk * BLOCK_MAX, hipHostMallocDefault), "hipHostMalloc") &&
                 hip_ok(hipHostMalloc((void **)&h_desc[i], chunk * sizeof(BlockDesc), hipHostMallocDefault), "hipHostMalloc");
        if (ok) {
            fill(0);
            ok = launch(0);
        }
        for (size_t k = 0; k < n_chunks && ok && io_ok; ++k) {
            if (k + 1 < n_chunks) fill(k + 1);                                      // (beside chunk k on the device)
            if (!(ok = hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize"))) break;
            const size_t total = *h_total, nb = chunk_blocks(k);
            if (total < nb * 26 || total > nb * (size_t)coral_deflate::MEMBER_MAX) { err = std::string(me) + "the packed chunk has an impossible size"; ok = false; break; }
            ok = hip_ok(hipMemcpyAsync(h_out, W.packed, total, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync") && hip_ok(hipEventRecord(ev_out, stream), "hipEventRecord");
            if (ok && k + 1 < n_chunks) ok = launch(k + 1);                         // (behind the copy: `packed` is free again)
            ok = ok && hip_ok(hipEventSynchronize(ev_out), "hipEventSynchronize");
            if (ok) io_ok = fwrite(h_out, 1, total, fp) == total;                   // (beside chunk k + 1 on the device)
        }
        (void)hipStreamSynchronize(stream);             // nothing of this call is left on the stream, whatever happened
        for (int i = 0; i < 2; ++i) {
            if (h_in[i]) (void)hipHostFree(h_in[i]);
            if (h_desc[i]) (void)hipHostFree(h_desc[i]);
        }
        if (h_out) (void)hipHostFree(h_out);
        if (h_total) (void)hipHostFree(h_total);
        if (ev_out) (void)hipEventDestroy(ev_out);
    }
    static const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    io_ok = io_ok && fwrite(EOF_BLOCK, 1, 28, fp) == 28;
    io_ok = (fclose(fp) == 0) && io_ok;
    if (!err.empty()) { set_error(err); return CORAL_ERR_HIP; }
    if (!io_ok) { set_error(std::string("writing ") + path + " failed"); return CORAL_ERR_FORMAT; }
    return CORAL_OK;
}

// ---- the file sink of a records request (CORAL_SINK_BAM; ReadsRequest in coral_bamgpu_reads.h) -----------------------------------
// The descriptors of one chunk, made where they are read: block k of n_blocks is in[k * 0xff00 ..) with 0xff00 bytes (the last
// one: last_len), its member goes to slot k.
__global__ __launch_bounds__(WAVE) void k_bgzf_chunk_desc(BlockDesc *__restrict__ desc, int n_blocks, uint32_t last_len) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_blocks) return;
    desc[k] = BlockDesc{(uint32_t)k * (uint32_t)coral_deflate::BLOCK_MAX, k == n_blocks - 1 ? last_len : (uint32_t)coral_deflate::BLOCK_MAX,
                        (uint32_t)k * (uint32_t)coral_deflate::SLOT_BYTES, 0u};
}

// A BGZF file that grows while the decode runs: the header at `start`, per batch the full 0xff00-byte blocks of the records
// written so far (the rest, the carry, waits at the front of the request's buffer for the next batch), at `finish` the carry, if
// any, and the EOF block.  The cuts run through the concatenation of all batches, so the file is coral_bgzf_write_gpu's of the
// two parts (header, all record bytes).  Chunks of at most `chunk` blocks go through k_bgzf_chunk_desc, k_bgzf_deflate and
// k_bgzf_pack on the sink's own stream; a chunk's total comes back first (4 bytes), then exactly its packed bytes into one of two
// pinned buffers, and it is written while the chunk behind it is on the device.  A chunk that was launched last stays in flight
// when a batch ends: it is taken in by the next batch's first chunk, or by `finish`.
// A failure leaves the file without the EOF block (readers see it truncated); the destructor closes it.
struct RecordSink {
    std::string path, error;
    std::vector<uint8_t> header;
    size_t chunk = DEFL_CHUNK_BLOCKS;
    FILE *fp = nullptr;
    // device memory (carved by the request) and what the sink owns: its stream, events and pinned buffers
    uint8_t *slots = nullptr, *packed = nullptr;
    BlockDesc *desc = nullptr;
    uint32_t *member = nullptr, *off = nullptr;
    void *tokens = nullptr, *tmp = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev_copied = nullptr, ev_moved = nullptr, ev_total = nullptr, ev_out = nullptr;
    uint8_t *h_out[2] = {nullptr, nullptr};
    uint32_t *h_total = nullptr;
    bool moved = false;                  // ev_moved has been recorded: the next batch's copy waits for it
    long long carry = 0;                 // bytes at the front of the buffer that belong to the next block
    int launched_blocks = 0;             // blocks of the chunk in flight (0: none)
    size_t n_chunks = 0;                 // chunks launched so far (chunk c comes back through h_out[c & 1])
    int64_t records = 0, bytes = 0, file_bytes = 0, members = 0;

    bool fail(const std::string &what) { if (error.empty()) error = "record sink: " + what; return false; }
    bool ok(hipError_t e, const char *what) { return e == hipSuccess || fail(std::string(what) + ": " + hipGetErrorString(e)); }

    void carve(Carver &take) {
        slots = (uint8_t *)take(chunk * coral_deflate::SLOT_BYTES);
        packed = (uint8_t *)take(chunk * coral_deflate::SLOT_BYTES);
        desc = (BlockDesc *)take(chunk * sizeof(BlockDesc));
        member = (uint32_t *)take(chunk * 4);
        off = (uint32_t *)take((chunk + 1) * 4);
        tokens = take(deflate_scratch_bytes((long long)chunk));
        tmp = take(DEFL_SCAN_TMP);
    }
    bool start() {
        bool good = ok(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate") &&
                    ok(hipHostMalloc((void **)&h_total, 256, hipHostMallocDefault), "hipHostMalloc");
        for (hipEvent_t *e : {&ev_copied, &ev_moved, &ev_total, &ev_out}) good = good && ok(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate");
        for (int i = 0; i < 2 && good; ++i) good = ok(hipHostMalloc((void **)&h_out[i], chunk * coral_deflate::SLOT_BYTES, hipHostMallocDefault), "hipHostMalloc");
        return good;
    }
    // The chunk in flight: its total, then its packed bytes into its pinned buffer.  n = 0: there is none.
    bool take_in(uint8_t *&data, size_t &n) {
        n = 0;
        if (launched_blocks == 0) return true;
        const size_t nb = (size_t)launched_blocks;
        launched_blocks = 0;
        if (!ok(hipEventSynchronize(ev_total), "hipEventSynchronize")) return false;
        const size_t total = *h_total;
        if (total < nb * 26 || total > nb * (size_t)coral_deflate::MEMBER_MAX) return fail("the packed chunk has an impossible size");
        data = h_out[(n_chunks - 1) & 1];
        if (!ok(hipMemcpyAsync(data, packed, total, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") || !ok(hipEventRecord(ev_out, s), "hipEventRecord")) return false;
        n = total;
        members += (int64_t)nb;
        return true;
    }
    bool write_out(const uint8_t *data, size_t n) {      // (behind take_in: the bytes are on their way)
        if (n == 0) return true;
        if (!ok(hipEventSynchronize(ev_out), "hipEventSynchronize")) return false;
        if (fwrite(data, 1, n, fp) != n) return fail("writing " + path + " failed");
        file_bytes += (int64_t)n;
        return true;
    }
    // n_blocks <= chunk blocks at `in` (device; the last one last_len bytes), queued on the sink's stream behind what is there; the
    // chunk in front comes back and is written while this one runs.
    bool submit(const uint8_t *in, int n_blocks, uint32_t last_len) {
        uint8_t *data = nullptr;
        size_t n = 0;
        if (!take_in(data, n)) return false;                         // (its copy is queued in front of this chunk's pack: `packed` is free)
        hipLaunchKernelGGL(k_bgzf_chunk_desc, dim3((unsigned)((n_blocks + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, desc, n_blocks, last_len);
        if (!ok(hipGetLastError(), "k_bgzf_chunk_desc") ||
            !ok(launch_deflate(in, (const uint32_t *)desc, n_blocks, slots, member, tokens, s), "k_bgzf_deflate") ||
            !ok(launch_pack(slots, member, n_blocks, packed, off, tmp, DEFL_SCAN_TMP, s), "k_bgzf_pack") ||
            !ok(hipMemcpyAsync(h_total, off + n_blocks, 4, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") || !ok(hipEventRecord(ev_total, s), "hipEventRecord"))
            return false;
        launched_blocks = n_blocks;
        ++n_chunks;
        return write_out(data, n);
    }
    // `n` bytes at `in` as whole blocks, the last one shorter when n is no multiple of 0xff00, in chunks
    bool submit_all(const uint8_t *in, size_t n) {
        const size_t nb = (n + coral_deflate::BLOCK_MAX - 1) / coral_deflate::BLOCK_MAX;
        for (size_t c0 = 0; c0 < nb; c0 += chunk) {
            const size_t k = std::min(chunk, nb - c0);
            const size_t last = c0 + k == nb ? n - (nb - 1) * coral_deflate::BLOCK_MAX : (size_t)coral_deflate::BLOCK_MAX;
            if (!submit(in + c0 * coral_deflate::BLOCK_MAX, (int)k, (uint32_t)last)) return false;
        }
        return true;
    }
    // The header, through `buf` (the request's buffer, cap bytes; nothing else uses it yet): it ends a block.
    bool write_header(uint8_t *buf, size_t cap) {
        const size_t piece = std::min(chunk, cap / coral_deflate::BLOCK_MAX) * coral_deflate::BLOCK_MAX;
        for (size_t at = 0; at < header.size(); at += piece) {
            const size_t n = std::min(piece, header.size() - at);
            if (!ok(hipMemcpyAsync(buf, header.data() + at, n, hipMemcpyHostToDevice, s), "hipMemcpyAsync") || !submit_all(buf, n)) return false;
        }
        moved = true;                                // (the first batch's copy waits for the header's deflate, which reads `buf`)
        return ok(hipEventRecord(ev_moved, s), "hipEventRecord");
    }
    // One batch: `n` new bytes stand at buf + carry, written by a kernel on `stream`.  Its full blocks are deflated, the rest moves
    // to the front (source and destination cannot overlap: the tail is shorter than one block, and at least one block lies in
    // front of it).
    bool batch(uint8_t *buf, long long n, long long n_records, hipStream_t stream) {
        if (!ok(hipEventRecord(ev_copied, stream), "hipEventRecord") || !ok(hipStreamWaitEvent(s, ev_copied, 0), "hipStreamWaitEvent")) return false;
        const long long total = carry + n, n_full = total / coral_deflate::BLOCK_MAX, tail = total - n_full * coral_deflate::BLOCK_MAX;
        if (n_full > 0 && !submit_all(buf, (size_t)(n_full * coral_deflate::BLOCK_MAX))) return false;
        if (n_full > 0 && tail > 0 && !ok(hipMemcpyAsync(buf, buf + n_full * coral_deflate::BLOCK_MAX, (size_t)tail, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync")) return false;
        if (!ok(hipEventRecord(ev_moved, s), "hipEventRecord")) return false;
        moved = true;
        carry = tail;
        records += n_records;
        bytes += n;
        return true;
    }
    // One sorted run of a spill file (CORAL_SINK_RUNS): `n` bytes stand at buf, offset 0, written by a kernel on
    // `stream`.  ALL of them are deflated now, a short last block included: a run is a whole number of members and shares none.
    bool run(uint8_t *buf, long long n, long long n_records, hipStream_t stream) {
        if (!ok(hipEventRecord(ev_copied, stream), "hipEventRecord") || !ok(hipStreamWaitEvent(s, ev_copied, 0), "hipStreamWaitEvent")) return false;
        if (n > 0 && !submit_all(buf, (size_t)n)) return false;
        if (!ok(hipEventRecord(ev_moved, s), "hipEventRecord")) return false;
        moved = true;
        records += n_records;
        bytes += n;
        return true;
    }
    // The chunk in flight, if any, comes back and is written: file_bytes is then where the next member will start.
    bool flush() {
        uint8_t *data = nullptr;
        size_t n = 0;
        return take_in(data, n) && write_out(data, n);
    }
    // The end of a file without an EOF block (a spill file is members only).
    bool close_plain() {
        if (!flush()) return false;
        const bool good = fclose(fp) == 0;
        fp = nullptr;
        return good || fail("writing " + path + " failed");
    }
    // The next batch's copy kernel on `stream` writes behind the carry: behind the tail move, and behind the deflate that read the buffer.
    bool wait_moved(hipStream_t stream) { return !moved || ok(hipStreamWaitEvent(stream, ev_moved, 0), "hipStreamWaitEvent"); }
    bool finish(uint8_t *buf) {
        if (carry > 0 && !submit_all(buf, (size_t)carry)) return false;
        carry = 0;
        uint8_t *data = nullptr;
        size_t n = 0;
        if (!take_in(data, n) || !write_out(data, n)) return false;
        static const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        bool good = fwrite(EOF_BLOCK, 1, 28, fp) == 28;
        good = (fclose(fp) == 0) && good;
        fp = nullptr;
        if (!good) return fail("writing " + path + " failed");
        file_bytes += 28;
        ++members;
        return true;
    }
    ~RecordSink() {
        if (s) (void)hipStreamSynchronize(s);        // (its kernels work in the caller's workspace, which is about to be released)
        if (fp) fclose(fp);
        for (hipEvent_t e : {ev_copied, ev_moved, ev_total, ev_out}) if (e) (void)hipEventDestroy(e);
        for (int i = 0; i < 2; ++i) if (h_out[i]) (void)hipHostFree(h_out[i]);
        if (h_total) (void)hipHostFree(h_total);
        if (s) (void)hipStreamDestroy(s);
    }
};
