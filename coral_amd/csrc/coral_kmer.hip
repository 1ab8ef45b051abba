// coral_kmer.hip - the device backend of `kmers`: the kernels behind coral_kmer_open .. coral_kmer_close (include/coral_hip.h) for a
// device session.  The rule is coral_kmer_core.h's, the same functions the host backend (coral_kmer_host.h) loops over.  The table
// (4^k uint32) and the workspace are the caller's; the staging of the pieces is coral_stream_gpu.h's PieceStager.
//
// Per fed piece of at most `staging` bytes, stream-ordered, no host wait but the one for the staging buffer's earlier use:
//   host            copy into a pinned buffer; mask_headers turns every header line's body into '\n' (the '>' stays: one break)
//   copy stream     the piece goes up into one of two raw buffers, so that an upload runs beside the kernels of the piece before
//   (scan)          exclusive sums of the keep flags (a byte that is not '\n' / '\r'), read straight from the bytes
//   k_kmer_scatter  the kept bytes' symbols (base 0..3, break) back to back behind the 16 symbols carried from the piece before
//   k_kmer_count    each thread takes COUNT_SPT consecutive symbols, warms its rolling words on the k-1 symbols in front of them and
//                   issues one no-return atomicAdd per run of equal indices
//   k_kmer_carry    the last 16 symbols move to the front for the next piece
// After the last piece:
//   k_kmer_stats    distinct and the histogram of the counts below 65 536 (below 8 192 in LDS, flushed once per workgroup)
//   k_kmer_sel_count, (scan), k_kmer_sel_write: the entries above a threshold in table order - a count per tile of the table,
//                   the tiles' offsets, then every tile ranks its own entries; used for the counts of 65 536 and more (at most 65 535
//                   entries: the histogram's tail, added on the host) and for coral_kmer_select
//   k_kmer_lookup   the counts of a list of indices
// Plain C++ atomics and vector stores only.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_kmer_gpu.h"
#include "coral_stream_gpu.h"

namespace {

using namespace coral_kmer;
using namespace coral_stream;

constexpr int PRE = 16;                          // symbols carried in front of a piece's (>= MAX_K - 1, and keeps the runs 16-byte aligned)
constexpr int COUNT_SPT = 32;                    // symbols per thread of k_kmer_count
constexpr int COUNT_BLOCK = 256;
constexpr int COUNT_TILE = COUNT_SPT * COUNT_BLOCK;
constexpr int SCATTER_BLOCK = 256;
constexpr int TABLE_BLOCK = 256;                 // k_kmer_stats and k_kmer_sel_*: 16 entries (four uint4) per thread
constexpr int TABLE_ITEMS = 16;
constexpr int TABLE_TILE = TABLE_BLOCK * TABLE_ITEMS;
constexpr uint32_t LDS_BINS = 8192;
constexpr long long GRID_CAP = 4096;
constexpr int64_t MAX_STAGING = (int64_t)1 << 30;
constexpr int64_t TAIL_CAP = 65536;

struct Scalars {                                 // what stays in device memory between the kernels
    unsigned long long n_bases, total, distinct;
    uint32_t m, pad;                             // kept symbols of the current piece
};

// four bytes a thread: symbols to dense[pos]; the thread of the last byte leaves the number of kept symbols
__global__ __launch_bounds__(SCATTER_BLOCK) void k_kmer_scatter(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ pos, uint32_t n, uint8_t *__restrict__ dense,
                                                                 Scalars *__restrict__ S) {
    scatter_symbols<SCATTER_BLOCK>(raw, pos, n, dense, &S->m, [](uint8_t c) { return classify(c); }, SYM_SKIP);
}

// `dense` starts at the PRE carried symbols; the piece's m symbols follow
__global__ __launch_bounds__(COUNT_BLOCK) void k_kmer_count(const uint8_t *__restrict__ dense, Scalars *__restrict__ S, int k, int canonical, uint32_t *__restrict__ table) {
    using Reduce = hipcub::BlockReduce<unsigned long long, COUNT_BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const uint32_t m = S->m;
    const unsigned long long start = ((unsigned long long)blockIdx.x * COUNT_BLOCK + threadIdx.x) * COUNT_SPT;
    unsigned long long bases = 0, kmers = 0;
    if (start < m) {
        const uint8_t *run = dense + PRE + start;
        Roll r;
        for (int j = k - 1; j >= 1; --j) roll_push(r, run[-j], k);      // (at most k-1 bases: no window completes here)
        uint32_t sym[COUNT_SPT / 4];
        for (int v = 0; v < COUNT_SPT / 16; ++v) {
            const uint4 q = ((const uint4 *)run)[v];
            sym[4 * v] = q.x; sym[4 * v + 1] = q.y; sym[4 * v + 2] = q.z; sym[4 * v + 3] = q.w;
        }
        const uint32_t left = m - (uint32_t)start < (uint32_t)COUNT_SPT ? m - (uint32_t)start : (uint32_t)COUNT_SPT;
        uint64_t pending = 0;
        uint32_t pending_n = 0;
#pragma unroll
        for (int j = 0; j < COUNT_SPT; ++j) {
            if ((uint32_t)j < left) {
                const uint8_t s = (uint8_t)(sym[j / 4] >> (8 * (j % 4)));
                bases += s < 4;
                if (roll_push(r, s, k)) {
                    const uint64_t idx = roll_index(r, canonical != 0);
                    ++kmers;
                    if (pending_n && idx == pending) ++pending_n;
                    else {
                        if (pending_n) atomicAdd(table + pending, pending_n);
                        pending = idx;
                        pending_n = 1;
                    }
                }
            }
        }
        if (pending_n) atomicAdd(table + pending, pending_n);
    }
    const unsigned long long b = Reduce(tmp).Sum(bases);
    __syncthreads();
    const unsigned long long t = Reduce(tmp).Sum(kmers);
    if (threadIdx.x == 0) {
        if (b) atomicAdd(&S->n_bases, b);
        if (t) atomicAdd(&S->total, t);
    }
}

__global__ void k_kmer_carry(uint8_t *__restrict__ dense, const Scalars *__restrict__ S) {
    const uint32_t m = S->m;
    uint8_t v = 0;
    if (threadIdx.x < PRE) v = dense[m + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < PRE) dense[threadIdx.x] = v;
}

// n4 = entries / 4 (4^k is a multiple of four)
__global__ __launch_bounds__(TABLE_BLOCK) void k_kmer_stats(const uint32_t *__restrict__ table, unsigned long long n4, long long n_tiles, uint32_t *__restrict__ hist,
                                                             Scalars *__restrict__ S) {
    using Reduce = hipcub::BlockReduce<unsigned long long, TABLE_BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    __shared__ uint32_t bins[LDS_BINS];
    for (uint32_t b = threadIdx.x; b < LDS_BINS; b += TABLE_BLOCK) bins[b] = 0;
    __syncthreads();
    unsigned long long distinct = 0, ones = 0;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        for (int j = 0; j < TABLE_ITEMS / 4; ++j) {
            const unsigned long long v = (unsigned long long)tile * (TABLE_TILE / 4) + (unsigned long long)j * TABLE_BLOCK + threadIdx.x;
            if (v >= n4) continue;
            const uint4 q = ((const uint4 *)table)[v];
            const uint32_t c4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t c = c4[e];
                if (!c) continue;
                ++distinct;
                if (c == 1) ++ones;
                else if (c < LDS_BINS) atomicAdd(&bins[c], 1u);
                else if (c < HIST_DIRECT) atomicAdd(&hist[c], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < LDS_BINS; b += TABLE_BLOCK)
        if (bins[b]) atomicAdd(&hist[b], bins[b]);
    const unsigned long long d = Reduce(tmp).Sum(distinct);
    __syncthreads();
    const unsigned long long o = Reduce(tmp).Sum(ones);
    if (threadIdx.x == 0) {
        if (d) atomicAdd(&S->distinct, d);
        if (o) atomicAdd(&hist[1], (uint32_t)o);
    }
}

// thread t of a tile owns its entries 16 t .. 16 t + 15: how many of them lie above the threshold, and which
__device__ __forceinline__ uint32_t tile_entries(const uint32_t *__restrict__ table, unsigned long long n4, long long tile, uint32_t greater_than, uint32_t c[TABLE_ITEMS]) {
    uint32_t hits = 0;
#pragma unroll
    for (int j = 0; j < TABLE_ITEMS / 4; ++j) {
        const unsigned long long v = (unsigned long long)tile * (TABLE_TILE / 4) + (unsigned long long)threadIdx.x * (TABLE_ITEMS / 4) + j;
        uint4 q = {0, 0, 0, 0};
        if (v < n4) q = ((const uint4 *)table)[v];
        c[4 * j] = q.x; c[4 * j + 1] = q.y; c[4 * j + 2] = q.z; c[4 * j + 3] = q.w;
    }
#pragma unroll
    for (int e = 0; e < TABLE_ITEMS; ++e) hits += c[e] > greater_than;       // (an entry past the table reads 0: never above)
    return hits;
}

__global__ __launch_bounds__(TABLE_BLOCK) void k_kmer_sel_count(const uint32_t *__restrict__ table, unsigned long long n4, long long n_tiles, uint32_t greater_than,
                                                                 unsigned long long *__restrict__ tile_cnt) {
    using Reduce = hipcub::BlockReduce<uint32_t, TABLE_BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t c[TABLE_ITEMS];
        const uint32_t sum = Reduce(tmp).Sum(tile_entries(table, n4, tile, greater_than, c));
        if (threadIdx.x == 0) tile_cnt[tile] = sum;
        __syncthreads();
    }
}

__global__ __launch_bounds__(TABLE_BLOCK) void k_kmer_sel_write(const uint32_t *__restrict__ table, unsigned long long n4, long long n_tiles, uint32_t greater_than,
                                                                 const unsigned long long *__restrict__ tile_off, unsigned long long capacity, uint64_t *__restrict__ kmers,
                                                                 uint32_t *__restrict__ counts) {
    using Scan = hipcub::BlockScan<uint32_t, TABLE_BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const unsigned long long first = tile_off[tile];
        if (tile_off[tile + 1] == first || first >= capacity) continue;          // (the same for every thread of the workgroup)
        uint32_t c[TABLE_ITEMS], rank;
        const uint32_t hits = tile_entries(table, n4, tile, greater_than, c);
        Scan(tmp).ExclusiveSum(hits, rank);
        unsigned long long at = first + rank;
        const uint64_t entry = (uint64_t)tile * TABLE_TILE + (uint64_t)threadIdx.x * TABLE_ITEMS;
#pragma unroll
        for (int e = 0; e < TABLE_ITEMS; ++e) {
            if (c[e] > greater_than) {
                if (at < capacity) { kmers[at] = entry + e; counts[at] = c[e]; }
                ++at;
            }
        }
        __syncthreads();
    }
}

__global__ void k_kmer_lookup(const uint32_t *__restrict__ table, unsigned long long entries, const uint64_t *__restrict__ idx, long long n, uint32_t *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = idx[i] < entries ? table[idx[i]] : 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
long long table_tiles(int k) { return (long long)((table_entries(k) + TABLE_TILE - 1) / TABLE_TILE); }

size_t cub_tmp_bytes(int k, int64_t staging) {
    size_t need = keep_scan_tmp_bytes(staging), b = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(table_tiles(k) + 1)) == hipSuccess) need = std::max(need, b);
    return need + 256;
}

struct Workspace {
    uint8_t *raw[2], *dense;
    uint32_t *pos, *hist, *tail_counts;
    uint64_t *tail_kmers;
    unsigned long long *tile_cnt, *tile_off;
    Scalars *scal;
    void *tmp;
    size_t tmp_bytes, bytes;
    Workspace(void *base, int k, int64_t staging, size_t cub_bytes) {
        Carver cv{(uintptr_t)base};
        const size_t S = ((size_t)staging + 3) & ~(size_t)3, T = (size_t)table_tiles(k) + 1;
        raw[0] = cv.take<uint8_t>(S); raw[1] = cv.take<uint8_t>(S);
        pos = cv.take<uint32_t>(S);
        dense = cv.take<uint8_t>(PRE + S + COUNT_SPT + PRE);        // (a thread's last run is read whole; the carry reads PRE behind m)
        hist = cv.take<uint32_t>(HIST_DIRECT);
        tail_kmers = cv.take<uint64_t>(TAIL_CAP); tail_counts = cv.take<uint32_t>(TAIL_CAP);
        tile_cnt = cv.take<unsigned long long>(T); tile_off = cv.take<unsigned long long>(T);
        scal = cv.take<Scalars>(1);
        tmp = cv.take<uint8_t>(cub_bytes);
        tmp_bytes = cub_bytes;
        bytes = cv.used;
    }
};

unsigned grid_of(long long items, int per_block) { return (unsigned)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, GRID_CAP)); }

}  // namespace

namespace coral_kmer_gpu {

struct Device {
    int k = 0, device = 0;
    bool canonical = true, finished = false;
    uint32_t *table = nullptr;
    int64_t staging = 0;
    uint64_t bases_before = 0;
    Workspace W{nullptr, 1, 16, 0};
    PieceStager st;
    LineState line;
    uint64_t n_sequences = 0;
};

int64_t workspace_bytes(int k, int64_t staging_bytes) {
    if (!k_ok(k) || staging_bytes < 16 || staging_bytes > MAX_STAGING) return CORAL_ERR_ARG;
    const Workspace W(nullptr, k, staging_bytes, cub_tmp_bytes(k, staging_bytes));
    return (int64_t)W.bytes + 256;
}

void geometry(int32_t *out) {
    const int32_t g[8] = {COUNT_SPT, COUNT_BLOCK, TABLE_TILE, TABLE_BLOCK, PRE, SCATTER_BLOCK * 4, (int32_t)LDS_BINS, (int32_t)HIST_DIRECT};
    for (int i = 0; i < 8; ++i) out[i] = g[i];
}

void close(Device *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    d->st.close();
    delete d;
}

int open(int k, bool canonical, int device, uint32_t *table, int64_t staging_bytes, void *workspace, int64_t ws_bytes, void *stream, uint64_t bases_before, Device **out,
         std::string &err) {
    if (!k_ok(k) || !table || !out || staging_bytes < 16 || staging_bytes > MAX_STAGING || device < 0) { err = "k outside 1..16, no table, a staging size outside 16 .. 2^30 or a bad device"; return CORAL_ERR_ARG; }
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    const size_t cub_bytes = cub_tmp_bytes(k, staging_bytes);
    const Workspace sized(nullptr, k, staging_bytes, cub_bytes);
    if (!workspace || ws_bytes < (int64_t)sized.bytes + 256) { err = "the workspace is smaller than coral_kmer_workspace_bytes"; return CORAL_ERR_ARG; }
    Device *d = new Device();
    d->k = k; d->device = device; d->canonical = canonical; d->table = table; d->staging = staging_bytes; d->bases_before = bases_before;
    d->W = Workspace((void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255), k, staging_bytes, cub_bytes);
    const hipStream_t s = (hipStream_t)stream;
    const bool good = hip_ok(hipMemsetAsync(d->W.dense, SYM_BREAK, PRE, s), "hipMemsetAsync", err) && hip_ok(hipMemsetAsync(d->W.scal, 0, sizeof(Scalars), s), "hipMemsetAsync", err) &&
                      d->st.open(s, (size_t)staging_bytes, err);
    if (!good) { close(d); return CORAL_ERR_HIP; }
    *out = d;
    return CORAL_OK;
}

static int feed_piece(Device *d, const uint8_t *bytes, uint32_t n, std::string &err) {
    PieceStager &st = d->st;
    const int b = st.acquire(err);
    if (b < 0) return CORAL_ERR_HIP;
    memcpy(st.pinned[b], bytes, n);
    d->n_sequences += mask_headers(d->line, st.pinned[b], n);
    const Workspace &W = d->W;
    bool good = st.upload(b, W.raw[b], n, err);
    if (good) {
        size_t tb = W.tmp_bytes;
        good = hip_ok(keep_scan(W.tmp, tb, W.raw[b], W.pos, n, st.stream), "scan of the keep flags", err);
    }
    if (good) {
        hipLaunchKernelGGL(k_kmer_scatter, dim3(grid_of(((long long)n + 3) / 4, SCATTER_BLOCK)), dim3(SCATTER_BLOCK), 0, st.stream, W.raw[b], W.pos, n, W.dense + PRE, W.scal);
        good = hip_ok(hipGetLastError(), "k_kmer_scatter", err) && st.mark_k1(b, err);
    }
    if (good) {
        const unsigned blocks = (unsigned)(((long long)n + COUNT_TILE - 1) / COUNT_TILE);      // (enough for n kept symbols; a thread past m leaves)
        hipLaunchKernelGGL(k_kmer_count, dim3(blocks), dim3(COUNT_BLOCK), 0, st.stream, W.dense, W.scal, d->k, (int)d->canonical, d->table);
        hipLaunchKernelGGL(k_kmer_carry, dim3(1), dim3(64), 0, st.stream, W.dense, W.scal);
        good = hip_ok(hipGetLastError(), "k_kmer_count", err);
    }
    return st.done(b, good, err) ? CORAL_OK : CORAL_ERR_HIP;
}

int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err) {
    if (!d || d->finished || n < 0 || (n > 0 && !bytes)) { err = "no session, a finished one, or no bytes"; return CORAL_ERR_ARG; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    for (int64_t at = 0; at < n; at += d->staging) {
        const int rc = feed_piece(d, bytes + at, (uint32_t)std::min<int64_t>(d->staging, n - at), err);
        if (rc != CORAL_OK) return rc;
    }
    return CORAL_OK;
}

// the entries above the threshold into device arrays; *n = how many there are
static bool select_pass(Device *d, uint64_t greater_than, int64_t capacity, uint64_t *kmers, uint32_t *counts, int64_t *n, std::string &err) {
    const Workspace &W = d->W;
    const long long tiles = table_tiles(d->k);
    const unsigned long long n4 = table_entries(d->k) / 4;
    if (greater_than >= 0xffffffffull) { *n = 0; return true; }      // (no uint32 is above)
    const uint32_t t = (uint32_t)greater_than;
    const unsigned grid = grid_of(tiles, 1);
    bool good = hip_ok(hipMemsetAsync(W.tile_cnt + tiles, 0, 8, d->st.stream), "hipMemsetAsync", err);
    if (!good) return false;
    hipLaunchKernelGGL(k_kmer_sel_count, dim3(grid), dim3(TABLE_BLOCK), 0, d->st.stream, d->table, n4, tiles, t, W.tile_cnt);
    size_t tb = W.tmp_bytes;
    good = hip_ok(hipGetLastError(), "k_kmer_sel_count", err) && hip_ok(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.tile_cnt, W.tile_off, (int)(tiles + 1), d->st.stream), "scan of the tiles", err);
    if (!good) return false;
    if (capacity > 0) {
        hipLaunchKernelGGL(k_kmer_sel_write, dim3(grid), dim3(TABLE_BLOCK), 0, d->st.stream, d->table, n4, tiles, t, W.tile_off, (unsigned long long)capacity, kmers, counts);
        if (!hip_ok(hipGetLastError(), "k_kmer_sel_write", err)) return false;
    }
    unsigned long long total = 0;
    good = hip_ok(hipMemcpyAsync(&total, W.tile_off + tiles, 8, hipMemcpyDeviceToHost, d->st.stream), "hipMemcpyAsync", err) && hip_ok(hipStreamSynchronize(d->st.stream), "hipStreamSynchronize", err);
    *n = (int64_t)total;
    return good;
}

int finish(Device *d, coral_kmer::Stats &st, std::map<uint64_t, uint64_t> &hist, double *seconds, std::string &err) {
    if (!d || d->finished) { err = "no session, or a finished one"; return CORAL_ERR_ARG; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    d->finished = true;
    const Workspace &W = d->W;
    if (!d->st.drain(err) || !hip_ok(hipStreamSynchronize(d->st.stream), "hipStreamSynchronize", err)) return CORAL_ERR_HIP;
    Scalars s{};
    hipEvent_t *ev = d->st.ev[0];                        // (both buffers are retired: their events are free)
    bool good = hip_ok(hipMemcpyAsync(&s, W.scal, sizeof(s), hipMemcpyDeviceToHost, d->st.stream), "hipMemcpyAsync", err) && hip_ok(hipStreamSynchronize(d->st.stream), "hipStreamSynchronize", err);
    if (!good) return CORAL_ERR_HIP;
    st = coral_kmer::Stats();
    st.n_sequences = d->n_sequences;
    st.n_bases = d->bases_before + s.n_bases;
    st.total = s.total;
    if (st.n_bases >= MAX_BASES) { err = "the stream has 2^32 bases or more: a counter may have wrapped"; return CORAL_ERR_CAPACITY; }
    const long long tiles = table_tiles(d->k);
    good = hip_ok(hipEventRecord(ev[EV_K0], d->st.stream), "hipEventRecord", err) && hip_ok(hipMemsetAsync(W.hist, 0, (size_t)HIST_DIRECT * 4, d->st.stream), "hipMemsetAsync", err);
    if (!good) return CORAL_ERR_HIP;
    hipLaunchKernelGGL(k_kmer_stats, dim3(grid_of(tiles, 1)), dim3(TABLE_BLOCK), 0, d->st.stream, d->table, (unsigned long long)(table_entries(d->k) / 4), tiles, W.hist, W.scal);
    if (!hip_ok(hipGetLastError(), "k_kmer_stats", err)) return CORAL_ERR_HIP;
    int64_t n_tail = 0;
    if (!select_pass(d, HIST_DIRECT - 1, TAIL_CAP, W.tail_kmers, W.tail_counts, &n_tail, err)) return CORAL_ERR_HIP;
    if (n_tail >= TAIL_CAP) { err = "more than 65 535 counts of 65 536 and more"; return CORAL_ERR_HIP; }
    std::vector<uint32_t> direct(HIST_DIRECT), tail((size_t)n_tail);
    good = hip_ok(hipMemcpyAsync(direct.data(), W.hist, (size_t)HIST_DIRECT * 4, hipMemcpyDeviceToHost, d->st.stream), "hipMemcpyAsync", err) &&
           (n_tail == 0 || hip_ok(hipMemcpyAsync(tail.data(), W.tail_counts, (size_t)n_tail * 4, hipMemcpyDeviceToHost, d->st.stream), "hipMemcpyAsync", err)) &&
           hip_ok(hipMemcpyAsync(&s, W.scal, sizeof(s), hipMemcpyDeviceToHost, d->st.stream), "hipMemcpyAsync", err) && hip_ok(hipEventRecord(ev[EV_K1], d->st.stream), "hipEventRecord", err) &&
           hip_ok(hipStreamSynchronize(d->st.stream), "hipStreamSynchronize", err);
    if (!good) return CORAL_ERR_HIP;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[EV_K0], ev[EV_K1]) == hipSuccess) d->st.seconds[3] = ms * 1e-3;
    st.distinct = s.distinct;
    hist.clear();
    for (uint32_t c = 1; c < HIST_DIRECT; ++c) if (direct[c]) { hist[c] = direct[c]; st.max_count = c; }
    for (uint32_t c : tail) { ++hist[c]; if (c > st.max_count) st.max_count = c; }
    if (seconds) for (int i = 0; i < 4; ++i) seconds[i] = d->st.seconds[i];
    return CORAL_OK;
}

int select(Device *d, uint64_t greater_than, int64_t capacity, uint64_t *kmers, uint32_t *counts, int64_t *n, std::string &err) {
    if (!d || !d->finished || capacity < 0 || !n || (capacity > 0 && (!kmers || !counts))) { err = "no finished session, or a missing array"; return CORAL_ERR_ARG; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    if (!select_pass(d, greater_than, capacity, kmers, counts, n, err)) return CORAL_ERR_HIP;
    if (*n > capacity) { err = "more selected k-mers than the capacity"; return CORAL_ERR_CAPACITY; }
    return CORAL_OK;
}

int lookup(Device *d, const uint64_t *indices, int64_t n, uint32_t *counts, std::string &err) {
    if (!d || !d->finished || n < 0 || (n > 0 && (!indices || !counts))) { err = "no finished session, or a missing array"; return CORAL_ERR_ARG; }
    if (n == 0) return CORAL_OK;
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    hipLaunchKernelGGL(k_kmer_lookup, dim3(grid_of(n, 256)), dim3(256), 0, d->st.stream, d->table, (unsigned long long)table_entries(d->k), indices, (long long)n, counts);
    const bool good = hip_ok(hipGetLastError(), "k_kmer_lookup", err) && hip_ok(hipStreamSynchronize(d->st.stream), "hipStreamSynchronize", err);
    return good ? CORAL_OK : CORAL_ERR_HIP;
}

}  // namespace coral_kmer_gpu
