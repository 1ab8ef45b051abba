// coral_comp.hip - the device backend of `composition`: the kernels behind coral_comp_open .. coral_comp_close (include/coral_hip.h)
// for a device session.  The rule is coral_comp_core.h's, the same functions the host backend (coral_comp_host.h) loops over.  The
// three tables and the workspace are the caller's; the staging of the pieces is coral_stream_gpu.h's PieceStager.  It
// stands in for the GC and repeat-mask columns of the reference table of the reference's scripts/call_cnvs.sh:12-17.
//
// Per fed piece of at most `staging` bytes and at most MAX_BOUND header lines (a piece with more is fed as several), stream-ordered,
// no host wait but the one for the staging buffer's earlier use:
//   host            scan_piece finds the header lines in the caller's bytes and takes the names; the piece is copied into a pinned
//                   buffer behind a PieceHead with the headers' byte offsets, and every header line is blanked to '\n'
//   copy stream     head and piece go up into one of two raw buffers, so that an upload runs beside the kernels of the piece before
//   (scan)          exclusive sums of the is-position flags (a byte that is not '\n' / '\r'): every byte's ordinal in the piece
//   k_comp_walk     one workgroup: the contigs that the piece's headers close get their lengths (carried positions + ordinals),
//                   every stretch between two headers its first bin; the carry (Carry) moves on to the next piece
//   k_comp_count    each thread takes COUNT_SPT consecutive bytes in aligned 16-byte loads, finds its stretch by a search in the
//                   headers' offsets, sums runs of equal bin and leaves its last bin to the wave: lanes with the same bin are
//                   neighbours (positions ascend), the run's first lane issues one no-return atomicAdd per table
// The closed contigs' lengths come down behind k_comp_walk, into the piece's pinned buffer, and are read when it is next used.
// Plain C++ atomics and vector stores only.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_comp_gpu.h"
#include "coral_stream_gpu.h"

namespace {

using namespace coral_comp;
using namespace coral_stream;

constexpr int WAVE = 64;
constexpr int COUNT_SPT = 64;                    // bytes per thread of k_comp_count: four 16-byte loads
constexpr int COUNT_BLOCK = 256;
constexpr int COUNT_TILE = COUNT_SPT * COUNT_BLOCK;
constexpr int WALK_BLOCK = 256;                  // (MAX_BOUND, the header lines of one piece, and PieceHead are coral_stream_gpu.h's)
constexpr int WALK_ITEMS = MAX_BOUND / WALK_BLOCK;
constexpr int64_t MIN_STAGING = 16, MAX_STAGING = (int64_t)1 << 30;
constexpr uint32_t NO_BIN = 0xffffffffu;

struct Carry {                                   // what stays in device memory between the pieces
    unsigned long long cur_len, bin_base;        // the open contig's positions so far; the bins in front of it
    unsigned long long positions, gc, at, masked;
};

struct Segs {                                    // a piece's stretches: stretch 0 belongs to the carried contig, stretch j + 1 starts at bounds[j]
    unsigned long long pos0;                     // the contig position of stretch 0's first position (the others start at 0)
    uint32_t n_seg, n_bytes;
    uint32_t start[MAX_BOUND + 1], ord[MAX_BOUND + 1];      // first byte; the ordinal of that byte
    unsigned long long bin[MAX_BOUND + 1];       // the first bin of the stretch's contig
};

__global__ __launch_bounds__(WALK_BLOCK) void k_comp_walk(const PieceHead *__restrict__ H, const uint8_t *__restrict__ raw, const uint32_t *__restrict__ pos,
                                                           unsigned long long bin_size, Carry *__restrict__ C, Segs *__restrict__ S, unsigned long long *__restrict__ closed) {
    using Scan = hipcub::BlockScan<unsigned long long, WALK_BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    const uint32_t n = H->n_bytes, nb = min(H->n_bounds, (uint32_t)MAX_BOUND);
    const unsigned long long carry_len = C->cur_len, carry_bin = C->bin_base;
    unsigned long long bins[WALK_ITEMS], lens[WALK_ITEMS], sum = 0;
    uint32_t at[WALK_ITEMS], ords[WALK_ITEMS];
#pragma unroll
    for (int k = 0; k < WALK_ITEMS; ++k) {
        const uint32_t j = threadIdx.x * WALK_ITEMS + k;
        bins[k] = 0; lens[k] = 0; at[k] = 0; ords[k] = 0;
        if (j < nb) {
            at[k] = min(H->bounds[j], n - 1);
            ords[k] = pos[at[k]];
            const uint32_t before = j ? pos[min(H->bounds[j - 1], n - 1)] : 0u;
            lens[k] = (unsigned long long)(ords[k] - before) + (j ? 0ull : carry_len);
            bins[k] = bins_of(lens[k], bin_size);
        }
        sum += bins[k];
    }
    unsigned long long excl, all;
    Scan(tmp).ExclusiveSum(sum, excl, all);
    unsigned long long run = carry_bin + excl;
#pragma unroll
    for (int k = 0; k < WALK_ITEMS; ++k) {
        const uint32_t j = threadIdx.x * WALK_ITEMS + k;
        if (j < nb) {
            run += bins[k];
            S->start[j + 1] = at[k]; S->ord[j + 1] = ords[k]; S->bin[j + 1] = run;
            closed[j] = lens[k];
        }
    }
    __syncthreads();                                                  // (every thread has read the carry)
    if (threadIdx.x == 0) {
        S->pos0 = carry_len; S->n_seg = nb + 1; S->n_bytes = n;
        S->start[0] = 0; S->ord[0] = 0; S->bin[0] = carry_bin;
        const unsigned long long total = (unsigned long long)pos[n - 1] + (is_position(raw[n - 1]) ? 1u : 0u);
        if (nb) { C->cur_len = total - pos[min(H->bounds[nb - 1], n - 1)]; C->bin_base = carry_bin + all; }
        else C->cur_len = carry_len + total;
        C->positions += total;
    }
}

// `key` does not decrease over the lanes that hold one: the sum of `v` over every run of equal keys, in the run's first lane
__device__ __forceinline__ uint32_t run_sum(uint32_t key, uint32_t v, int lane) {
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t tv = __shfl_down(v, d), tk = __shfl_down(key, d);
        if (lane + d < WAVE && tk == key) v += tv;
    }
    return v;
}

__global__ __launch_bounds__(COUNT_BLOCK) void k_comp_count(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ pos, const Segs *__restrict__ S, unsigned long long bin_size,
                                                             unsigned long long capacity, uint32_t *__restrict__ gc, uint32_t *__restrict__ at, uint32_t *__restrict__ masked,
                                                             Carry *__restrict__ C) {
    using Reduce = hipcub::BlockReduce<uint32_t, COUNT_BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const uint32_t n = S->n_bytes, n_seg = S->n_seg;
    const unsigned long long first = ((unsigned long long)blockIdx.x * COUNT_BLOCK + threadIdx.x) * COUNT_SPT;
    uint32_t a_gc = 0, a_at = 0, a_mk = 0, t_gc = 0, t_at = 0, t_mk = 0, key = NO_BIN;
    if (first < n) {
        const uint32_t b0 = (uint32_t)first;
        uint32_t lo = 0, hi = n_seg;                                  // the last stretch that starts at or in front of b0
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (S->start[mid] <= b0) lo = mid; else hi = mid;
        }
        uint32_t j = lo;
        const unsigned long long p = (j ? 0ull : S->pos0) + (pos[b0] - S->ord[j]);
        unsigned long long bin = S->bin[j] + p / bin_size, left = bin_size - p % bin_size;
        uint32_t next = j + 1 < n_seg ? S->start[j + 1] : NO_BIN;
        auto flush = [&]() {
            if (bin < capacity) {
                if (a_gc) atomicAdd(gc + bin, a_gc);
                if (a_at) atomicAdd(at + bin, a_at);
                if (a_mk) atomicAdd(masked + bin, a_mk);
            }
            t_gc += a_gc; t_at += a_at; t_mk += a_mk;
            a_gc = 0; a_at = 0; a_mk = 0;
        };
#pragma unroll
        for (int v = 0; v < COUNT_SPT / 16; ++v) {
            const uint32_t base = b0 + 16u * v;
            if (base >= n) break;
            const uint4 q = *(const uint4 *)(raw + base);             // (the buffer holds whole 16-byte words)
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t i = base + e;
                if (i >= n) break;
                if (i == next) {
                    flush();
                    ++j;
                    bin = S->bin[j]; left = bin_size;
                    next = j + 1 < n_seg ? S->start[j + 1] : NO_BIN;
                }
                const uint8_t c = (uint8_t)(w[e / 4] >> (8 * (e % 4)));
                if (!is_position(c)) continue;
                if (left == 0) { flush(); ++bin; left = bin_size; }
                const uint32_t cls = classes(c);
                a_gc += cls & CLS_GC ? 1u : 0u; a_at += cls & CLS_AT ? 1u : 0u; a_mk += cls & CLS_MASKED ? 1u : 0u;
                --left;
            }
        }
        t_gc += a_gc; t_at += a_at; t_mk += a_mk;
        // a thread without a counted base keeps its key: the keys must not decrease from lane to lane, or a run would be split
        if (bin < capacity) key = (uint32_t)bin;                                  // (capacity <= 2^28)
        else { a_gc = 0; a_at = 0; a_mk = 0; }
    }
    {                                                                 // the thread's last bin: one atomic per run of lanes and table
        const int lane = threadIdx.x & (WAVE - 1);
        const uint32_t prev = __shfl_up(key, 1);
        const uint32_t s_gc = run_sum(key, a_gc, lane), s_at = run_sum(key, a_at, lane), s_mk = run_sum(key, a_mk, lane);
        if (key != NO_BIN && (lane == 0 || prev != key)) {
            if (s_gc) atomicAdd(gc + key, s_gc);
            if (s_at) atomicAdd(at + key, s_at);
            if (s_mk) atomicAdd(masked + key, s_mk);
        }
    }
    const uint32_t b_gc = Reduce(tmp).Sum(t_gc);
    __syncthreads();
    const uint32_t b_at = Reduce(tmp).Sum(t_at);
    __syncthreads();
    const uint32_t b_mk = Reduce(tmp).Sum(t_mk);
    if (threadIdx.x == 0) {
        if (b_gc) atomicAdd(&C->gc, (unsigned long long)b_gc);
        if (b_at) atomicAdd(&C->at, (unsigned long long)b_at);
        if (b_mk) atomicAdd(&C->masked, (unsigned long long)b_mk);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct Workspace {
    uint8_t *raw[2];                 // PieceHead (HEAD_BYTES), then the piece
    uint32_t *pos;
    Segs *segs;
    unsigned long long *closed;
    Carry *carry;
    void *tmp;
    size_t tmp_bytes, bytes;
    Workspace(void *base, int64_t staging, size_t cub_bytes) {
        Carver cv{(uintptr_t)base};
        const size_t S = ((size_t)staging + 15) & ~(size_t)15;
        raw[0] = cv.take<uint8_t>(HEAD_BYTES + S); raw[1] = cv.take<uint8_t>(HEAD_BYTES + S);
        pos = cv.take<uint32_t>(S);
        segs = cv.take<Segs>(1);
        closed = cv.take<unsigned long long>(MAX_BOUND);
        carry = cv.take<Carry>(1);
        tmp = cv.take<uint8_t>(cub_bytes);
        tmp_bytes = cub_bytes;
        bytes = cv.used;
    }
};

}  // namespace

namespace coral_comp_gpu {

struct Device {
    int device = 0;
    bool finished = false, started = false;
    int format_error = COMP_OK;
    uint64_t bin_size = 0, capacity = 0;
    uint32_t *gc = nullptr, *at = nullptr, *masked = nullptr;
    int64_t staging = 0;
    Workspace W{nullptr, 16, 0};
    PieceStager st;                  // a pinned buffer: PieceHead (HEAD_BYTES), the piece, and from closed_at on the lengths that come down
    size_t closed_at = 0;
    uint32_t n_closed[2] = {0, 0};
    bool open_before[2] = {false, false};
    LineState line;
    Names names;
    std::vector<int64_t> lengths;
    std::vector<uint32_t> bounds;
    std::vector<std::pair<uint32_t, uint32_t>> blanks;
};

int64_t workspace_bytes(int64_t staging_bytes) {
    if (staging_bytes < MIN_STAGING || staging_bytes > MAX_STAGING) return CORAL_ERR_ARG;
    const Workspace W(nullptr, staging_bytes, keep_scan_tmp_bytes(staging_bytes) + 256);
    return (int64_t)W.bytes + 256;
}

void geometry(int32_t *out) {
    const int32_t g[8] = {COUNT_SPT, COUNT_BLOCK, WAVE, MAX_BOUND, WALK_BLOCK, (int32_t)MIN_STAGING, 16, 0};
    for (int i = 0; i < 8; ++i) out[i] = g[i];
}

void close(Device *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    d->st.close();
    delete d;
}

int open(int64_t bin_size, int device, uint32_t *gc, uint32_t *at, uint32_t *masked, int64_t capacity, int64_t staging_bytes, void *workspace, int64_t ws_bytes, void *stream,
         Device **out, std::string &err) {
    if (!bin_size_ok(bin_size) || !gc || !at || !masked || !out || capacity < 1 || capacity > MAX_BINS || staging_bytes < MIN_STAGING || staging_bytes > MAX_STAGING || device < 0) {
        err = "bin_size outside 1 .. 2^31 - 1, a missing table, a capacity outside 1 .. 2^28, a staging size outside 16 .. 2^30 or a bad device";
        return CORAL_ERR_ARG;
    }
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    const size_t cub_bytes = keep_scan_tmp_bytes(staging_bytes) + 256;
    const Workspace sized(nullptr, staging_bytes, cub_bytes);
    if (!workspace || ws_bytes < (int64_t)sized.bytes + 256) { err = "the workspace is smaller than coral_comp_workspace_bytes"; return CORAL_ERR_ARG; }
    Device *d = new Device();
    d->device = device; d->bin_size = (uint64_t)bin_size; d->capacity = (uint64_t)capacity; d->gc = gc; d->at = at; d->masked = masked; d->staging = staging_bytes;
    d->W = Workspace((void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255), staging_bytes, cub_bytes);
    d->closed_at = up256(HEAD_BYTES + (size_t)staging_bytes);
    d->st.retired = [d](int b) {                         // a piece that is through leaves the lengths of the contigs it closed
        const unsigned long long *closed = (const unsigned long long *)(d->st.pinned[b] + d->closed_at);
        for (uint32_t j = d->open_before[b] ? 0 : 1; j < d->n_closed[b]; ++j) d->lengths.push_back((int64_t)closed[j]);
        d->n_closed[b] = 0;
    };
    const bool good = hip_ok(hipMemsetAsync(d->W.carry, 0, sizeof(Carry), (hipStream_t)stream), "hipMemsetAsync", err) &&
                      d->st.open((hipStream_t)stream, d->closed_at + (size_t)MAX_BOUND * 8, err);
    if (!good) { close(d); return CORAL_ERR_HIP; }
    *out = d;
    return CORAL_OK;
}

// the next piece: at most `n` bytes of it; *taken = how many it was
static int feed_piece(Device *d, const uint8_t *bytes, uint32_t n, uint32_t *taken, std::string &err) {
    PieceStager &st = d->st;
    const int b = st.acquire(err);
    if (b < 0) return CORAL_ERR_HIP;
    const bool open_before = d->started;
    int fe = COMP_OK;
    const uint32_t m = (uint32_t)scan_piece(d->line, d->names, d->started, bytes, n, MAX_BOUND, d->bounds, d->blanks, &fe);
    if (fe != COMP_OK) { d->format_error = fe; err = format_text(fe); return CORAL_ERR_FORMAT; }
    *taken = m;
    PieceHead *head = (PieceHead *)st.pinned[b];
    uint8_t *text = st.pinned[b] + HEAD_BYTES;
    const uint32_t nb = (uint32_t)d->bounds.size();
    head->n_bytes = m; head->n_bounds = nb; head->open_before = open_before; head->pad = 0;
    if (nb) memcpy(head->bounds, d->bounds.data(), (size_t)nb * 4);
    memcpy(text, bytes, m);
    for (const auto &r : d->blanks) memset(text + r.first, '\n', r.second - r.first);
    const Workspace &W = d->W;
    const PieceHead *dev_head = (const PieceHead *)W.raw[b];
    const uint8_t *dev_text = W.raw[b] + HEAD_BYTES;
    bool good = st.upload(b, W.raw[b], HEAD_BYTES + m, err);
    if (good) {
        size_t tb = W.tmp_bytes;
        good = hip_ok(keep_scan(W.tmp, tb, dev_text, W.pos, m, st.stream), "scan of the position flags", err);
    }
    if (good) {
        hipLaunchKernelGGL(k_comp_walk, dim3(1), dim3(WALK_BLOCK), 0, st.stream, dev_head, dev_text, W.pos, (unsigned long long)d->bin_size, W.carry, W.segs, W.closed);
        good = hip_ok(hipGetLastError(), "k_comp_walk", err);
        if (good && nb) {
            good = hip_ok(hipMemcpyAsync(st.pinned[b] + d->closed_at, W.closed, (size_t)nb * 8, hipMemcpyDeviceToHost, st.stream), "hipMemcpyAsync", err);
            if (good) { d->n_closed[b] = nb; d->open_before[b] = open_before; }
        }
        good = good && st.mark_k1(b, err);
    }
    if (good) {
        const unsigned blocks = (unsigned)(((long long)m + COUNT_TILE - 1) / COUNT_TILE);
        hipLaunchKernelGGL(k_comp_count, dim3(blocks), dim3(COUNT_BLOCK), 0, st.stream, dev_text, W.pos, W.segs, (unsigned long long)d->bin_size, (unsigned long long)d->capacity, d->gc,
                           d->at, d->masked, W.carry);
        good = hip_ok(hipGetLastError(), "k_comp_count", err);
    }
    return st.done(b, good, err) ? CORAL_OK : CORAL_ERR_HIP;
}

int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err) {
    if (!d || d->finished || n < 0 || (n > 0 && !bytes)) { err = "no session, a finished one, or no bytes"; return CORAL_ERR_ARG; }
    if (d->format_error != COMP_OK) { err = format_text(d->format_error); return CORAL_ERR_FORMAT; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    for (int64_t at = 0; at < n;) {
        uint32_t taken = 0;
        const int rc = feed_piece(d, bytes + at, (uint32_t)std::min<int64_t>(d->staging, n - at), &taken, err);
        if (rc != CORAL_OK) return rc;
        at += taken;
    }
    return CORAL_OK;
}

int finish(Device *d, coral_comp::Stats &st, std::vector<int64_t> &lengths, coral_comp::Names &names, double *seconds, std::string &err) {
    if (!d || d->finished) { err = "no session, or a finished one"; return CORAL_ERR_ARG; }
    if (d->format_error != COMP_OK) { err = format_text(d->format_error); return CORAL_ERR_FORMAT; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    d->finished = true;
    if (!d->st.drain(err)) return CORAL_ERR_HIP;          // (the older piece first: its contigs come first)
    Carry c{};
    if (!hip_ok(hipMemcpyAsync(&c, d->W.carry, sizeof(c), hipMemcpyDeviceToHost, d->st.stream), "hipMemcpyAsync", err) || !hip_ok(hipStreamSynchronize(d->st.stream), "hipStreamSynchronize", err))
        return CORAL_ERR_HIP;
    if (d->names.in_line && !d->names.close_line()) { d->format_error = COMP_FORMAT_EMPTY_NAME; err = format_text(d->format_error); return CORAL_ERR_FORMAT; }
    st = coral_comp::Stats();
    st.bins = c.bin_base;
    if (d->started) { d->lengths.push_back((int64_t)c.cur_len); st.bins += bins_of(c.cur_len, d->bin_size); }
    st.n_contigs = d->lengths.size();
    st.positions = c.positions; st.gc = c.gc; st.at = c.at; st.masked = c.masked;
    lengths = d->lengths;
    names = d->names;
    if (seconds) for (int i = 0; i < 4; ++i) seconds[i] = d->st.seconds[i];
    return CORAL_OK;
}

}  // namespace coral_comp_gpu
