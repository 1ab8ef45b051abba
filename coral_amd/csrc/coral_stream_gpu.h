// coral_stream_gpu.h - what the device sessions that stream text in pieces share (FASTA: coral_kmer.hip, coral_comp.hip; FASTQ:
// coral_fastq.hip, the first whose per-piece results come down again, through `retired`): the double-buffered staging of the
// pieces and the scan that gives every kept byte of a FASTA piece its ordinal; and, for every session that carves a caller's
// workspace (coral_cngpu.hip too), up256 and the typed Carver.
//
// A PieceStager owns two pinned buffers, a non-blocking copy stream and five events a buffer.  Per piece, with no host wait but the
// one for the buffer's earlier use:
//   acquire   the next buffer; its earlier piece is retired first (wait for EV_DONE, add its three stage times, call `retired`)
//   (caller)  fills pinned[b]
//   upload    EV_UP0, the copy on the copy stream, EV_UP1, the caller's stream waits for it, EV_K0; the buffer is the device's now
//   (caller)  first stage kernels; mark_k1; second stage kernels
//   done      EV_DONE, whenever the buffer is the device's
// so that an upload runs beside the kernels of the piece before.  seconds[0..2] = upload, first stage, second stage; seconds[3]
// is the caller's.
#ifndef CORAL_STREAM_GPU_H
#define CORAL_STREAM_GPU_H

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <functional>
#include <string>

#include "coral_fasta_core.h"

namespace coral_stream {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {                      // hands the workspace out in 256-byte steps (p == 0: only the size is counted)
    uintptr_t p;
    size_t used = 0;
    template <class T> T *take(size_t n) { used += up256(n * sizeof(T)); return (T *)(p + used - up256(n * sizeof(T))); }
};

inline bool hip_ok(hipError_t e, const char *what, std::string &err) {
    if (e == hipSuccess) return true;
    if (err.empty()) err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

// exclusive sums of the keep flags (a byte that is not '\n' / '\r'), read straight from the bytes
inline hipError_t keep_scan(void *tmp, size_t &tmp_bytes, const uint8_t *text, uint32_t *pos, int64_t n, hipStream_t stream) {
    using KeepIter = hipcub::TransformInputIterator<uint32_t, coral_fasta::KeepOp, const uint8_t *>;
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, KeepIter(text, coral_fasta::KeepOp()), pos, (int)n, stream);
}

inline size_t keep_scan_tmp_bytes(int64_t n) {
    size_t b = 0;
    return keep_scan(nullptr, b, nullptr, nullptr, n, nullptr) == hipSuccess ? b : 0;
}

// The body of a scatter kernel (k_kmer_scatter, k_sketch_scatter): four bytes a thread, the kept bytes' symbols to dense[pos];
// the thread of the last byte leaves the number of kept symbols in *m.  `symbol`: byte -> symbol, `skip` the symbol of a byte that
// is not kept.
template <int BLOCK, class Symbol>
__device__ __forceinline__ void scatter_symbols(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ pos, uint32_t n, uint8_t *__restrict__ dense, uint32_t *__restrict__ m,
                                                const Symbol &symbol, uint8_t skip) {
    const uint32_t words = (n + 3) / 4;
    for (uint32_t w = blockIdx.x * BLOCK + threadIdx.x; w < words; w += gridDim.x * BLOCK) {
        const uint32_t bytes = ((const uint32_t *)raw)[w];           // (both arrays are allocated in whole words of four)
        const uint4 p = ((const uint4 *)pos)[w];
        const uint32_t at[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = w * 4 + j;
            if (i >= n) break;
            const uint8_t sym = symbol((uint8_t)(bytes >> (8 * j)));
            if (sym != skip) dense[at[j]] = sym;
            if (i == n - 1) *m = at[j] + (sym != skip);
        }
    }
}

// In front of a piece's bytes, in the pinned buffer and on the device, for the sessions that follow the contigs (coral_comp.hip,
// coral_sketch.hip): the header lines that open in the piece, at most MAX_BOUND of them (a piece with more is fed as several).
constexpr int MAX_BOUND = 1024;
struct PieceHead {
    uint32_t n_bytes, n_bounds, open_before, pad;
    uint32_t bounds[MAX_BOUND];                  // byte offsets of the header lines that open in the piece, rising
};
constexpr size_t HEAD_BYTES = (sizeof(PieceHead) + 255) & ~(size_t)255;

enum { EV_UP0, EV_UP1, EV_K0, EV_K1, EV_DONE, N_EV };

struct PieceStager {
    hipStream_t stream = nullptr, copy = nullptr;        // the caller's; the session's own
    uint8_t *pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2][N_EV] = {};
    bool used[2] = {false, false};
    int next = 0;
    double seconds[4] = {0, 0, 0, 0};
    std::function<void(int)> retired;                    // (optional) takes what the piece of a buffer brought down, when that piece is through

    // after what the caller queued on `stream_` to prepare its workspace
    bool open(hipStream_t stream_, size_t pinned_bytes, std::string &err) {
        stream = stream_;
        bool good = hip_ok(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking), "hipStreamCreateWithFlags", err);
        for (int b = 0; b < 2 && good; ++b) {
            good = hip_ok(hipHostMalloc((void **)&pinned[b], pinned_bytes, hipHostMallocDefault), "hipHostMalloc", err);
            for (int e = 0; e < N_EV && good; ++e) good = hip_ok(hipEventCreate(&ev[b][e]), "hipEventCreate", err);
        }
        return good && hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize", err);      // (the copy stream writes into the workspace: nothing earlier may still use it)
    }

    void close() {
        if (copy) (void)hipStreamSynchronize(copy);
        (void)hipStreamSynchronize(stream);
        for (int b = 0; b < 2; ++b) {
            for (hipEvent_t e : ev[b]) if (e) (void)hipEventDestroy(e);
            if (pinned[b]) (void)hipHostFree(pinned[b]);
        }
        if (copy) (void)hipStreamDestroy(copy);
    }

    // the buffer's earlier piece is through: its stage times are read
    bool retire(int b, std::string &err) {
        if (!used[b]) return true;
        if (!hip_ok(hipEventSynchronize(ev[b][EV_DONE]), "hipEventSynchronize", err)) return false;
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[b][EV_UP0], ev[b][EV_UP1]) == hipSuccess) seconds[0] += ms * 1e-3;
        if (hipEventElapsedTime(&ms, ev[b][EV_K0], ev[b][EV_K1]) == hipSuccess) seconds[1] += ms * 1e-3;
        if (hipEventElapsedTime(&ms, ev[b][EV_K1], ev[b][EV_DONE]) == hipSuccess) seconds[2] += ms * 1e-3;
        if (retired) retired(b);
        used[b] = false;
        return true;
    }

    // the buffer of the next piece, or -1
    int acquire(std::string &err) {
        const int b = next;
        next ^= 1;
        return retire(b, err) ? b : -1;
    }

    // both buffers, the older piece first
    bool drain(std::string &err) { return retire(next, err) && retire(next ^ 1, err); }

    bool upload(int b, void *dst, size_t bytes, std::string &err) {
        const bool good = hip_ok(hipEventRecord(ev[b][EV_UP0], copy), "hipEventRecord", err) &&
                          hip_ok(hipMemcpyAsync(dst, pinned[b], bytes, hipMemcpyHostToDevice, copy), "hipMemcpyAsync", err) &&
                          hip_ok(hipEventRecord(ev[b][EV_UP1], copy), "hipEventRecord", err) && hip_ok(hipStreamWaitEvent(stream, ev[b][EV_UP1], 0), "hipStreamWaitEvent", err) &&
                          hip_ok(hipEventRecord(ev[b][EV_K0], stream), "hipEventRecord", err);
        if (good) used[b] = true;                            // (from here on the buffer is the device's until EV_DONE)
        return good;
    }

    bool mark_k1(int b, std::string &err) { return hip_ok(hipEventRecord(ev[b][EV_K1], stream), "hipEventRecord", err); }

    // the event goes in whatever happened, so that the buffer's next use (or close) has something to wait for
    bool done(int b, bool good, std::string &err) {
        if (used[b]) good = hip_ok(hipEventRecord(ev[b][EV_DONE], stream), "hipEventRecord", err) && good;
        return good;
    }
};

}  // namespace coral_stream
#endif /* CORAL_STREAM_GPU_H */
