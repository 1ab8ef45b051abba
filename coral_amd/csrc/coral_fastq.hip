// coral_fastq.hip - the device backend of the read QC and the read filter on FASTQ text: the kernels behind coral_fastq_open ..
// coral_fastq_close (include/coral_hip.h) for a device session.  The rule is coral_fastq_core.h's, the same functions the host
// backend (coral_fastq_host.h) loops over.  The histogram and the workspace are the caller's; the staging of the pieces is
// coral_stream_gpu.h's PieceStager.  It stands in for the reference's scripts/report_nanopore_qc.py:35-48.
//
// Per fed piece of at most `staging` bytes that closes at most MAX_REC records (a piece with more is fed as several), stream-ordered,
// no host wait but the one for the staging buffer's earlier use:
//   host            record_ends counts the '\n' bytes of the caller's bytes (memchr), so that the records the piece closes and where
//                   each ends are known before any kernel runs; the piece is copied into a pinned buffer
//   copy stream     the piece goes up into one of two raw buffers, so that an upload runs beside the kernels of the piece before
//   (scan)          exclusive sums of the is-newline flags: every byte's line within the piece; the host passes the lines in front
//   k_fastq_accum   each thread takes ACC_SPT consecutive bytes in aligned 16-byte loads and classifies them by their line's phase:
//                   bases and quality characters add into piece-local record rows, a row a thread leaves gets its sums at once,
//                   its last row is left to the wave: lanes in the same record are neighbours, the run's first lane issues one
//                   no-return atomicAdd per column.  Quality characters count into a 256-bin LDS table that is flushed with one
//                   atomic per non-zero bin.  Wrong first bytes and quality characters out of range leave the smallest stream
//                   offset (atomicMin).
//   k_fastq_walk    one workgroup: the records the piece closes get the carried sums, are checked (quality count against length)
//                   and written out; the open record's sums move into the carry (Carry) for the next piece; the rows are zeroed
// The closed records' rows and the offending offset come down behind k_fastq_walk, into the piece's pinned buffer, and are taken
// when that buffer is next used (PieceStager::retired) - where the kept records' bytes are still at hand for the writer.
// Plain C++ atomics and vector stores only.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_fastq_gpu.h"
#include "coral_stream_gpu.h"

namespace {

using namespace coral_fastq;
using namespace coral_stream;

constexpr int WAVE = 64;
constexpr int ACC_SPT = 64;                      // bytes per thread of k_fastq_accum: four 16-byte loads
constexpr int ACC_BLOCK = 256;
constexpr int ACC_TILE = ACC_SPT * ACC_BLOCK;
constexpr int MAX_REC = 1024;                    // records one piece closes
constexpr int ROWS = MAX_REC + 1;                // and the one that stays open
constexpr int WALK_BLOCK = 256;
constexpr int64_t MIN_STAGING = 16, MAX_STAGING = (int64_t)1 << 30;
constexpr uint32_t NO_ROW = 0xffffffffu;

struct RowTable {                                // piece-local sums; zero between the pieces
    uint32_t len[ROWS], qcnt[ROWS], close_at[ROWS];      // bases, quality characters, the byte of the '\n' that closes the record
    unsigned long long qsum[ROWS];
};

struct Carry {                                   // what stays in device memory between the pieces: the open record, the first refusal
    unsigned long long len, qcnt, qsum, bad;
};

struct Closed {                                  // a closed record as it comes down
    unsigned long long qual_sum;
    uint32_t length, pad;
};

struct Down {                                    // what a piece brings down
    unsigned long long bad, pad;
    Closed rows[MAX_REC];
};

inline hipError_t newline_scan(void *tmp, size_t &tmp_bytes, const uint8_t *text, uint32_t *pos, int64_t n, hipStream_t stream) {
    using Iter = hipcub::TransformInputIterator<uint32_t, NewlineOp, const uint8_t *>;
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, Iter(text, NewlineOp()), pos, (int)n, stream);
}

inline size_t newline_scan_tmp_bytes(int64_t n) {
    size_t b = 0;
    return newline_scan(nullptr, b, nullptr, nullptr, n, nullptr) == hipSuccess ? b : 0;
}

// `key` does not decrease over the lanes: the sum of `v` over every run of equal keys, in the run's first lane
__device__ __forceinline__ uint32_t run_sum(uint32_t key, uint32_t v, int lane) {
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t tv = __shfl_down(v, d), tk = __shfl_down(key, d);
        if (lane + d < WAVE && tk == key) v += tv;
    }
    return v;
}

// n bytes at `raw`, byte i in line pos[i] of the piece; the piece starts `off0` bytes into the stream in a line of phase `phase0`
// (first0: at its first byte) and holds the rows 0 .. max_row
__global__ __launch_bounds__(ACC_BLOCK) void k_fastq_accum(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ pos, uint32_t n, uint32_t phase0, uint32_t first0,
                                                            unsigned long long off0, uint32_t max_row, RowTable *__restrict__ R, unsigned long long *__restrict__ hist,
                                                            Carry *__restrict__ C) {
    __shared__ uint32_t bins[256];
    static_assert(ACC_BLOCK == 256, "one bin a thread");
    bins[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long start = ((unsigned long long)blockIdx.x * ACC_BLOCK + threadIdx.x) * ACC_SPT;
    uint32_t a_len = 0, a_cnt = 0, a_sum = 0, key = NO_ROW;
    unsigned long long bad = NO_OFFSET;
    if (start < n) {
        const uint32_t b0 = (uint32_t)start;
        uint32_t line = pos[b0];
        bool first = b0 ? is_newline(raw[b0 - 1]) : first0 != 0;
        uint32_t row = row_of(phase0, line);
        auto flush = [&]() {
            if (row <= max_row) {
                if (a_len) atomicAdd(&R->len[row], a_len);
                if (a_cnt) { atomicAdd(&R->qcnt[row], a_cnt); atomicAdd(&R->qsum[row], (unsigned long long)a_sum); }
            }
            a_len = 0; a_cnt = 0; a_sum = 0;
        };
#pragma unroll
        for (int v = 0; v < ACC_SPT / 16; ++v) {
            const uint32_t base = b0 + 16u * v;
            if (base >= n) continue;
            const uint4 q = *(const uint4 *)(raw + base);             // (the buffer holds whole 16-byte words)
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t i = base + e;
                if (i >= n) continue;
                const uint8_t c = (uint8_t)(w[e / 4] >> (8 * (e % 4)));
                const uint32_t phase = (phase0 + line) & 3u;
                const Byte b = classify(phase, first, c);
                first = false;
                if (b == BYTE_BASE) ++a_len;
                else if (b == BYTE_QUAL) { ++a_cnt; a_sum += c - QUAL_BASE; atomicAdd(&bins[c - QUAL_BASE], 1u); }
                else if (b == BYTE_BAD && bad == NO_OFFSET) bad = off0 + i;
                if (is_newline(c)) {                                  // (a refused one too: the lines stay the scan's)
                    if (phase == 3) {
                        if (row <= max_row) R->close_at[row] = i;
                        flush();
                        ++row;
                    }
                    ++line;
                    first = true;
                }
            }
        }
        // a thread without a counted byte keeps its key: the keys must not decrease from lane to lane, or a run would be split
        if (row <= max_row) key = row;
        else { a_len = 0; a_cnt = 0; a_sum = 0; }
    }
    {                                                                 // the thread's last row: one atomic per run of lanes and column
        const int lane = threadIdx.x & (WAVE - 1);
        const uint32_t prev = __shfl_up(key, 1);
        const uint32_t s_len = run_sum(key, a_len, lane), s_cnt = run_sum(key, a_cnt, lane), s_sum = run_sum(key, a_sum, lane);
        if (key != NO_ROW && (lane == 0 || prev != key)) {
            if (s_len) atomicAdd(&R->len[key], s_len);
            if (s_cnt) { atomicAdd(&R->qcnt[key], s_cnt); atomicAdd(&R->qsum[key], (unsigned long long)s_sum); }
        }
    }
    if (bad != NO_OFFSET) atomicMin(&C->bad, bad);
    __syncthreads();
    const uint32_t mine = bins[threadIdx.x];
    if (mine) atomicAdd(&hist[threadIdx.x], (unsigned long long)mine);
}

// the piece closed n_closed records (rows 0 .. n_closed - 1); row n_closed stays open
__global__ __launch_bounds__(WALK_BLOCK) void k_fastq_walk(RowTable *__restrict__ R, uint32_t n_closed, unsigned long long off0, Carry *__restrict__ C, Down *__restrict__ D) {
    const unsigned long long c_len = C->len, c_cnt = C->qcnt, c_sum = C->qsum;
    __syncthreads();                                                  // (every thread has read the carry)
    const uint32_t rows = min(n_closed, (uint32_t)MAX_REC);
    for (uint32_t j = threadIdx.x; j <= rows; j += WALK_BLOCK) {
        unsigned long long len = R->len[j], cnt = R->qcnt[j], sum = R->qsum[j];
        const uint32_t at = R->close_at[j];
        R->len[j] = 0; R->qcnt[j] = 0; R->qsum[j] = 0; R->close_at[j] = 0;
        if (j == 0) { len += c_len; cnt += c_cnt; sum += c_sum; }
        if (j < rows) {
            if (!record_ok(len, cnt)) atomicMin(&C->bad, off0 + at);
            Closed out;
            out.qual_sum = sum; out.length = (uint32_t)min(len, (unsigned long long)0xffffffffu); out.pad = 0;
            D->rows[j] = out;
        } else { C->len = len; C->qcnt = cnt; C->qsum = sum; }
    }
    __syncthreads();
    if (threadIdx.x == 0) { D->bad = atomicMin(&C->bad, NO_OFFSET); D->pad = 0; }      // (read where the atomics of both kernels went)
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct Workspace {
    uint8_t *raw[2];
    uint32_t *pos;
    RowTable *rows;
    Carry *carry;
    Down *down;
    void *tmp;
    size_t tmp_bytes, bytes;
    Workspace(void *base, int64_t staging, size_t cub_bytes) {
        Carver cv{(uintptr_t)base};
        const size_t S = ((size_t)staging + 15) & ~(size_t)15;
        raw[0] = cv.take<uint8_t>(S); raw[1] = cv.take<uint8_t>(S);
        pos = cv.take<uint32_t>(S);
        rows = cv.take<RowTable>(1);
        carry = cv.take<Carry>(1);
        down = cv.take<Down>(1);
        tmp = cv.take<uint8_t>(cub_bytes);
        tmp_bytes = cub_bytes;
        bytes = cv.used;
    }
};

}  // namespace

namespace coral_fastq_gpu {

struct Device {
    int device = 0;
    bool finished = false;
    uint64_t bad = NO_OFFSET;                    // the first refusal that came down
    unsigned long long *hist = nullptr;
    int64_t staging = 0;
    Workspace W{nullptr, 16, 0};
    PieceStager st;                              // a pinned buffer: the piece, and from down_at on what comes down (Down)
    hipEvent_t ev_walk[2] = {nullptr, nullptr};  // between k_fastq_accum and k_fastq_walk
    double walk_seconds = 0;
    size_t down_at = 0;
    uint32_t n_bytes[2] = {0, 0};
    std::vector<uint32_t> ends[2];               // behind the '\n' bytes that close the records of the buffer's piece
    std::vector<uint8_t> kept;
    uint64_t lines = 0, offset = 0;              // '\n' bytes and bytes fed so far
    bool first = true;
    Rows rows;
    RecordWriter out;
    std::string write_error;
};

int64_t workspace_bytes(int64_t staging_bytes) {
    if (staging_bytes < MIN_STAGING || staging_bytes > MAX_STAGING) return CORAL_ERR_ARG;
    const Workspace W(nullptr, staging_bytes, newline_scan_tmp_bytes(staging_bytes) + 256);
    return (int64_t)W.bytes + 256;
}

void geometry(int32_t *out) {
    const int32_t g[8] = {ACC_SPT, ACC_BLOCK, WAVE, MAX_REC, (int32_t)MIN_STAGING, 16, WALK_BLOCK, 0};
    for (int i = 0; i < 8; ++i) out[i] = g[i];
}

const Rows &rows(const Device *d) { return d->rows; }

void close(Device *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    d->st.close();
    for (hipEvent_t e : d->ev_walk) if (e) (void)hipEventDestroy(e);
    delete d;
}

// a piece that is through: the refusal, or the rows of the records it closed and the kept ones' bytes
static void take_down(Device *d, int b) {
    const Down *down = (const Down *)(d->st.pinned[b] + d->down_at);
    float ms = 0;
    if (hipEventElapsedTime(&ms, d->ev_walk[b], d->st.ev[b][EV_DONE]) == hipSuccess) d->walk_seconds += ms * 1e-3;
    if (down->bad != NO_OFFSET && d->bad == NO_OFFSET) d->bad = down->bad;
    if (d->bad == NO_OFFSET && d->write_error.empty()) {
        const size_t k = d->ends[b].size();
        d->kept.resize(k);
        for (size_t j = 0; j < k; ++j) d->kept[j] = d->rows.close(down->rows[j].length, down->rows[j].qual_sum) ? 1 : 0;
        if (!d->out.piece(d->st.pinned[b], d->n_bytes[b], d->ends[b].data(), d->kept.data(), k)) d->write_error = d->out.error;
    }
    d->ends[b].clear();
    d->n_bytes[b] = 0;
}

static std::string refusal(uint64_t at) { return "the text is no four-line FASTQ at byte " + std::to_string(at); }

int open(int device, const Thresholds &thr, int fd, int64_t staging_bytes, void *hist, void *workspace, int64_t ws_bytes, void *stream, Device **out, std::string &err) {
    if (!hist || !out || staging_bytes < MIN_STAGING || staging_bytes > MAX_STAGING || device < 0) {
        err = "no histogram, a staging size outside 16 .. 2^30 or a bad device";
        return CORAL_ERR_ARG;
    }
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    const size_t cub_bytes = newline_scan_tmp_bytes(staging_bytes) + 256;
    const Workspace sized(nullptr, staging_bytes, cub_bytes);
    if (!workspace || ws_bytes < (int64_t)sized.bytes + 256) { err = "the workspace is smaller than coral_fastq_workspace_bytes"; return CORAL_ERR_ARG; }
    Device *d = new Device();
    d->device = device; d->hist = (unsigned long long *)hist; d->staging = staging_bytes;
    d->rows.thr = thr; d->out.fd = fd;
    d->W = Workspace((void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255), staging_bytes, cub_bytes);
    d->down_at = up256((size_t)staging_bytes);
    d->st.retired = [d](int b) { take_down(d, b); };
    Carry zero{0, 0, 0, NO_OFFSET};
    bool good = hip_ok(hipMemsetAsync(d->W.rows, 0, sizeof(RowTable), (hipStream_t)stream), "hipMemsetAsync", err) &&
                hip_ok(hipMemcpyAsync(d->W.carry, &zero, sizeof(zero), hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync", err) &&
                hip_ok(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize", err);      // (`zero` is this frame's)
    for (int b = 0; b < 2 && good; ++b) good = hip_ok(hipEventCreate(&d->ev_walk[b]), "hipEventCreate", err);
    good = good && d->st.open((hipStream_t)stream, d->down_at + sizeof(Down), err);
    if (!good) { close(d); return CORAL_ERR_HIP; }
    *out = d;
    return CORAL_OK;
}

static int failed(Device *d, std::string &err) {
    if (d->bad != NO_OFFSET) { err = refusal(d->bad); return CORAL_ERR_FORMAT; }
    if (!d->write_error.empty()) { err = d->write_error; return CORAL_ERR_ARG; }
    return CORAL_OK;
}

// the next piece: at most `n` bytes of it; *taken = how many it was
static int feed_piece(Device *d, const uint8_t *bytes, uint32_t n, uint32_t *taken, std::string &err) {
    PieceStager &st = d->st;
    const int b = st.acquire(err);
    if (b < 0) return CORAL_ERR_HIP;
    if (const int rc = failed(d, err)) return rc;
    const uint32_t phase0 = phase_of(d->lines), first0 = d->first ? 1u : 0u;
    const uint64_t off0 = d->offset;
    const uint32_t m = (uint32_t)record_ends(d->lines, d->first, bytes, n, MAX_REC, d->ends[b]);
    const uint32_t n_closed = (uint32_t)d->ends[b].size();
    *taken = m;
    d->offset += m;
    d->n_bytes[b] = m;
    memcpy(st.pinned[b], bytes, m);
    const Workspace &W = d->W;
    bool good = st.upload(b, W.raw[b], m, err);
    if (good) {
        size_t tb = W.tmp_bytes;
        good = hip_ok(newline_scan(W.tmp, tb, W.raw[b], W.pos, m, st.stream), "scan of the newline flags", err) && st.mark_k1(b, err);
    }
    if (good) {
        const unsigned blocks = (unsigned)(((long long)m + ACC_TILE - 1) / ACC_TILE);
        hipLaunchKernelGGL(k_fastq_accum, dim3(blocks), dim3(ACC_BLOCK), 0, st.stream, W.raw[b], W.pos, m, phase0, first0, (unsigned long long)off0, n_closed, W.rows, d->hist, W.carry);
        good = hip_ok(hipGetLastError(), "k_fastq_accum", err) && hip_ok(hipEventRecord(d->ev_walk[b], st.stream), "hipEventRecord", err);
    }
    if (good) {
        hipLaunchKernelGGL(k_fastq_walk, dim3(1), dim3(WALK_BLOCK), 0, st.stream, W.rows, n_closed, (unsigned long long)off0, W.carry, W.down);
        good = hip_ok(hipGetLastError(), "k_fastq_walk", err) &&
               hip_ok(hipMemcpyAsync(st.pinned[b] + d->down_at, W.down, 16 + (size_t)n_closed * sizeof(Closed), hipMemcpyDeviceToHost, st.stream), "hipMemcpyAsync", err);
    }
    return st.done(b, good, err) ? CORAL_OK : CORAL_ERR_HIP;
}

int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err) {
    if (!d || d->finished || n < 0 || (n > 0 && !bytes)) { err = "no session, a finished one, or no bytes"; return CORAL_ERR_ARG; }
    if (const int rc = failed(d, err)) return rc;
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    for (int64_t at = 0; at < n;) {
        uint32_t taken = 0;
        const int rc = feed_piece(d, bytes + at, (uint32_t)std::min<int64_t>(d->staging, n - at), &taken, err);
        if (rc != CORAL_OK) return rc;
        at += taken;
    }
    return CORAL_OK;
}

int finish(Device *d, double *seconds, std::string &err) {
    if (!d || d->finished) { err = "no session, or a finished one"; return CORAL_ERR_ARG; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    d->finished = true;
    if (!d->st.drain(err)) return CORAL_ERR_HIP;          // (the older piece first: its records come first)
    Carry c{};
    if (!hip_ok(hipMemcpyAsync(&c, d->W.carry, sizeof(c), hipMemcpyDeviceToHost, d->st.stream), "hipMemcpyAsync", err) || !hip_ok(hipStreamSynchronize(d->st.stream), "hipStreamSynchronize", err))
        return CORAL_ERR_HIP;
    if (seconds) {
        seconds[0] = d->st.seconds[0]; seconds[1] = d->st.seconds[1] + d->walk_seconds; seconds[2] = std::max(0.0, d->st.seconds[2] - d->walk_seconds);
        seconds[3] = d->out.seconds;
    }
    if (d->bad == NO_OFFSET && c.bad != NO_OFFSET) d->bad = c.bad;
    if (d->bad == NO_OFFSET && d->write_error.empty()) {
        const End e = end_of_stream(d->lines, d->first);
        bool k = false;
        if (e == END_BAD || (e == END_CLOSES && !record_ok(c.len, c.qcnt))) d->bad = d->offset;
        else if (e == END_CLOSES) k = d->rows.close(c.len, c.qsum);
        if (d->bad == NO_OFFSET && !d->out.finish(e == END_CLOSES, k)) d->write_error = d->out.error;
        if (seconds) seconds[3] = d->out.seconds;
    }
    d->rows.st.bad_offset = d->bad;
    return failed(d, err);
}

}  // namespace coral_fastq_gpu
