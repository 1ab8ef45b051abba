// coral_sketch.hip - the device backend of `sketch`: the kernels behind coral_sketch_open .. coral_sketch_close and the seed index
// (coral_sketch_sort, _lookup, _anchors of include/coral_hip.h).  The rule is coral_sketch_core.h's, the same functions the host
// backend (coral_sketch_host.h) loops over.  The output arrays, the weights' bitmap and the workspace are the caller's; the staging
// of the pieces is coral_stream_gpu.h's PieceStager, the piece's head (its header lines) PieceHead as in coral_comp.hip.
//
// The symbols of the stream stand in one buffer: CARRY symbols kept from the pieces before, then the piece's.  A table of contig
// starts - the buffer index of every contig's boundary symbol, negative for a contig that opened before the buffer - gives every
// position its contig and its place in it.  Per fed piece of at most `staging` bytes and MAX_BOUND header lines, stream-ordered, no
// host wait but the one for the staging buffer's earlier use:
//   host             scan_piece finds the header lines and takes the names; the piece is copied into a pinned buffer behind a
//                    PieceHead, every header line is blanked to '\n' but for its '>', every other '>' becomes a plain non-base
//   copy stream      head and piece go up into one of two raw buffers, beside the kernels of the piece before
//   (scan)           exclusive sums of the keep flags
//   k_sketch_scatter the kept bytes' symbols (base, non-base, contig boundary) behind the carried ones
//   k_sketch_walk    one workgroup: the piece's contig starts join the table, the contigs they close get their lengths, and the
//                    positions that can be decided are set: all of a closed contig, else those with w - 1 k-mers to their right
//   k_sketch_tile    twice (count, write), a workgroup per tile of TILE positions: 16-byte loads of the symbols with their halos
//                    into LDS, rolling fwd / rev per thread for a run of keys, the keys in LDS with w - 1 halos on each side, the
//                    two sliding passes (window minima, then the largest minimum over the windows of a position), ranks by
//                    ballot in position order; between the two a scan of the tiles' counts
//   k_sketch_carry   the last CARRY symbols and their contig starts move to the front; the output count moves on
// CARRY = 528 >= 2 (w - 1) + (k - 1) for every w <= 256 and k <= 16: the undecided tail and the halo in front of it always fit.
// The index: one hipcub radix sort of the pairs over the key's 2k + 1 bits (stable), a binary-search kernel, and count / scan /
// write for the anchors.  Plain C++ and vector stores only.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_sketch_gpu.h"
#include "coral_stream_gpu.h"

namespace {

using namespace coral_sketch;
using namespace coral_stream;

constexpr int CARRY = 528;                       // symbols kept in front of a piece's (a multiple of 16)
constexpr int BLOCK = 256;
constexpr int ITEMS = 8;                         // positions per thread of k_sketch_tile
constexpr int TILE = BLOCK * ITEMS;
constexpr int WAVES = BLOCK / 64;
constexpr int HALO = MAX_W - 1;
constexpr int KEYS_LDS = TILE + 2 * HALO;        // keys of a tile with both halos
constexpr int MINS_LDS = TILE + HALO;            // window minima: the windows that start in the left halo or in the tile
constexpr int SYMS_LDS = ((KEYS_LDS + 2 * (MAX_K - 1) + 15 + 15) / 16 + 1) * 16;
constexpr int TABLE_CAP = 2048;                  // contig starts: 1 + CARRY carried, MAX_BOUND of the piece
constexpr int SCATTER_BLOCK = 256;
constexpr int64_t MIN_STAGING = 16, MAX_STAGING = (int64_t)1 << 30;
static_assert(CARRY >= 2 * (MAX_W - 1) + (MAX_K - 1) && CARRY % 16 == 0, "the carry holds the undecided tail and its halo");
static_assert(1 + CARRY + MAX_BOUND <= TABLE_CAP, "the table holds the carried and the piece's contig starts");
static_assert(TABLE_CAP % BLOCK == 0 && CARRY <= 3 * BLOCK, "k_sketch_carry's registers");

struct State {                                   // what stays in device memory between the kernels
    long long hi, u, u_next;                     // symbols in the buffer; the first undecided position; the first one left undecided
    long long base_id, last_len;                 // contig of table entry 0; the open contig's positions at the end of the stream
    unsigned long long total;                    // minimizers of the pieces before
    uint32_t m, n_entries;                       // kept symbols of the current piece; table entries
};

__global__ __launch_bounds__(SCATTER_BLOCK) void k_sketch_scatter(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ pos, uint32_t n, uint8_t *__restrict__ dense,
                                                                   State *__restrict__ S) {
    scatter_symbols<SCATTER_BLOCK>(raw, pos, n, dense, &S->m, [](uint8_t c) { return dense_symbol(c); }, SYM_SKIP);
}

__global__ __launch_bounds__(BLOCK) void k_sketch_walk(const PieceHead *__restrict__ H, const uint32_t *__restrict__ pos, State *__restrict__ S, long long *__restrict__ starts,
                                                        long long *__restrict__ closed, int k, int w, int finished) {
    const uint32_t n = finished ? 0u : H->n_bytes, nb = finished ? 0u : min(H->n_bounds, (uint32_t)MAX_BOUND), nc = S->n_entries;
    const long long hi = CARRY + (finished ? 0ll : (long long)S->m);
    for (uint32_t j = threadIdx.x; j < nb; j += BLOCK) {
        const long long at = CARRY + (long long)pos[min(H->bounds[j], n - 1)];
        const long long before = j ? CARRY + (long long)pos[min(H->bounds[j - 1], n - 1)] : starts[nc - 1];
        starts[nc + j] = at;
        closed[j] = at - before - 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long last = starts[nc + nb - 1], u = S->u;
        long long next = hi;
        if (!finished) {
            next = hi - (w + k - 2);                                   // p + (w - 1) + (k - 1) <= hi - 1 for every decided p of the open contig
            next = next < last + 1 ? last + 1 : next;
            next = next < u ? u : next;
        }
        S->n_entries = nc + nb; S->hi = hi; S->u_next = next;
        if (finished) S->last_len = hi - last - 1;
    }
}

// the last table entry that starts at or in front of x, among lo .. hi
__device__ __forceinline__ int entry_of(const long long *__restrict__ starts, int lo, int hi, long long x) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (starts[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_sketch_tile(const uint8_t *__restrict__ dense, const State *__restrict__ S, const long long *__restrict__ starts, int k, int w,
                                                        const uint32_t *__restrict__ bitmap, unsigned long long *__restrict__ tile_cnt, const unsigned long long *__restrict__ tile_off,
                                                        unsigned long long capacity, uint64_t *__restrict__ out_key, uint64_t *__restrict__ out_value) {
    __shared__ uint64_t keys[KEYS_LDS];
    __shared__ uint64_t mins[MINS_LDS];
    __shared__ uint4 syms4[SYMS_LDS / 16];
    __shared__ uint8_t strands[KEYS_LDS];
    __shared__ uint32_t row_cnt[ITEMS * WAVES];
    __shared__ int ent[2];
    const uint8_t *syms = (const uint8_t *)syms4;
    const int tid = threadIdx.x;
    const long long hi = S->hi, t0 = (long long)blockIdx.x * TILE;
    const long long p_lo = t0 > S->u ? t0 : S->u, p_hi = t0 + TILE < S->u_next ? t0 + TILE : S->u_next;
    const int n_ent = (int)S->n_entries;
    if (p_lo >= p_hi) {                                               // (the same for every thread of the workgroup)
        if (!WRITE && tid == 0) tile_cnt[blockIdx.x] = 0;
        return;
    }
    unsigned long long first = 0;
    if (WRITE) {
        first = S->total + tile_off[blockIdx.x];
        if (tile_off[blockIdx.x + 1] == tile_off[blockIdx.x] || first >= capacity) return;
    }
    // key positions k_lo .. k_end - 1 have a slot; those from k_hi on lack a symbol and are invalid
    const long long k_lo = p_lo - (w - 1) > 0 ? p_lo - (w - 1) : 0, k_end = p_hi + (w - 1);
    const long long k_hi = k_end < hi - k + 1 ? k_end : hi - k + 1;
    const long long s_base = (k_lo - (k - 1)) & ~(long long)15;       // (rounds down, below zero too)
    const long long s_end = k_hi + k - 1;                             // <= hi
    const int n_words = s_end > s_base ? (int)((s_end - s_base + 15) / 16) : 0;
    for (int v = tid; v < n_words && v < SYMS_LDS / 16; v += BLOCK) {
        const long long g = s_base + 16ll * v;
        uint4 q = {0x06060606u, 0x06060606u, 0x06060606u, 0x06060606u};      // SYM_CONTIG in front of the buffer
        if (g >= 0 && g < hi) q = *(const uint4 *)(dense + g);        // (the buffer is allocated 16 bytes past its last symbol)
        syms4[v] = q;
    }
    __syncthreads();
    {                                                                 // a run of consecutive keys a thread: the rolling words are warmed on k - 1 symbols
        const int n_keys = (int)(k_end - k_lo), per = (n_keys + BLOCK - 1) / BLOCK;
        const long long q0 = k_lo + (long long)tid * per;
        Roll r;
        if (q0 < k_hi)
            for (int j = 0; j < k - 1; ++j) roll_push(r, syms[q0 + j - s_base], k);
        for (int i = 0; i < per; ++i) {
            const long long q = q0 + i;
            if (q >= k_end) break;
            uint64_t key = KEY_INVALID;
            uint32_t strand = 0;
            if (q < k_hi && roll_push(r, syms[q + k - 1 - s_base], k)) key = kmer_key(r, k, bitmap, &strand);
            keys[q - k_lo] = key;
            strands[q - k_lo] = (uint8_t)strand;
        }
    }
    if (tid == 0) {
        ent[0] = entry_of(starts, 0, n_ent - 1, k_lo);
        ent[1] = entry_of(starts, ent[0], n_ent - 1, k_end);
    }
    __syncthreads();
    const int e_lo = ent[0], e_hi = ent[1];
    // the contig of a position: its table entry and the windows over its k-mer positions a .. b (b < a: it has none)
    const auto contig_of = [&](long long x, int *e) {
        *e = e_lo == e_hi ? e_lo : entry_of(starts, e_lo, e_hi, x);
        const long long a = starts[*e] + 1, end = *e + 1 < n_ent ? starts[*e + 1] : hi;
        return Windows(a, end - k, w);
    };
    const auto key_at = [&](long long x) { return x >= k_lo && x < k_end ? keys[x - k_lo] : KEY_INVALID; };
    const auto min_at = [&](long long j) { return j >= k_lo && j < p_hi ? mins[j - k_lo] : (uint64_t)0; };
    for (long long j = k_lo + tid; j < p_hi; j += BLOCK) {            // the first pass: the minimum of every window that lies inside its contig
        int e;
        const Windows W = contig_of(j, &e);
        mins[j - k_lo] = W.b >= W.a && W.is_start(j) ? window_min(key_at, j, W.ww) : (uint64_t)0;
    }
    __syncthreads();
    uint32_t sel = 0;                                                 // the second: bit i = position t0 + i * BLOCK + tid is a minimizer
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const long long p = t0 + (long long)i * BLOCK + tid;
        bool s = false;
        if (p >= p_lo && p < p_hi) {
            const uint64_t mine = keys[p - k_lo];
            if (mine != KEY_INVALID) {
                int e;
                const Windows W = contig_of(p, &e);
                s = W.b >= W.a && p >= W.a && p <= W.b && is_minimizer(min_at, W, p, mine);
            }
        }
        const unsigned long long ballot = __ballot(s);
        if (lane == 0) row_cnt[i * WAVES + wave] = (uint32_t)__popcll(ballot);
        if (s) sel |= 1u << i;
    }
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) {
            unsigned long long sum = 0;
            for (int c = 0; c < ITEMS * WAVES; ++c) sum += row_cnt[c];
            tile_cnt[blockIdx.x] = sum;
        }
        return;
    }
    const long long base_id = S->base_id;
    unsigned long long row_first = first;                             // position order: row i of BLOCK positions, wave by wave, lane by lane
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const bool s = sel >> i & 1u;
        const unsigned long long ballot = __ballot(s);
        unsigned long long at = row_first;
        for (int v = 0; v < wave; ++v) at += row_cnt[i * WAVES + v];
        at += (unsigned long long)__popcll(ballot & ((1ull << lane) - 1));
        if (s && at < capacity) {
            const long long p = t0 + (long long)i * BLOCK + tid;
            int e;
            const Windows W = contig_of(p, &e);
            out_key[at] = keys[p - k_lo];
            out_value[at] = pack_value((uint64_t)(base_id + e), (uint64_t)(p - W.a), strands[p - k_lo]);
        }
        for (int v = 0; v < WAVES; ++v) row_first += row_cnt[i * WAVES + v];
    }
}

// one workgroup: the last CARRY symbols and the contig starts at or behind the one that is open at them move to the front
__global__ __launch_bounds__(BLOCK) void k_sketch_carry(uint8_t *__restrict__ dense, State *__restrict__ S, long long *__restrict__ starts, const unsigned long long *__restrict__ tile_off,
                                                         int n_tiles) {
    __shared__ int before;
    const long long shift = S->hi - CARRY;
    const int n_ent = (int)S->n_entries;
    if (threadIdx.x == 0) before = 0;
    __syncthreads();
    uint8_t sym[3];
    long long st[TABLE_CAP / BLOCK];
    int mine = 0;
    for (int i = 0; i < 3; ++i) { const int x = threadIdx.x + i * BLOCK; sym[i] = x < CARRY ? dense[x + shift] : 0; }
    for (int i = 0; i < TABLE_CAP / BLOCK; ++i) {
        const int e = threadIdx.x + i * BLOCK;
        st[i] = e < n_ent ? starts[e] : 0;
        mine += e < n_ent && st[i] < shift;
    }
    if (mine) atomicAdd(&before, mine);
    __syncthreads();                                                  // (everything is read)
    const int drop = before - 1;                                      // entry 0 starts in front of the buffer: before >= 1
    for (int i = 0; i < 3; ++i) { const int x = threadIdx.x + i * BLOCK; if (x < CARRY) dense[x] = sym[i]; }
    for (int i = 0; i < TABLE_CAP / BLOCK; ++i) {
        const int e = threadIdx.x + i * BLOCK;
        if (e < n_ent && e >= drop) starts[e - drop] = st[i] - shift;
    }
    if (threadIdx.x == 0) {
        S->base_id += drop; S->n_entries = (uint32_t)(n_ent - drop);
        S->u = S->u_next - shift;
        S->total += tile_off[n_tiles];
    }
}

// ---- the index -------------------------------------------------------------------------------------------------------------------
__global__ void k_sketch_lookup(const uint64_t *__restrict__ sorted, long long n, const uint64_t *__restrict__ qkey, long long nq, long long max_occ, int64_t *__restrict__ first,
                                int64_t *__restrict__ count, unsigned long long *__restrict__ emit) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long long)gridDim.x * blockDim.x) {
        int64_t f, c;
        find_entries(sorted, n, qkey[i], &f, &c);
        first[i] = f; count[i] = c;
        if (emit) emit[i] = c > max_occ ? 0ull : (unsigned long long)c;
    }
}

__global__ void k_sketch_anchor_write(const uint64_t *__restrict__ values, const uint32_t *__restrict__ query, const uint32_t *__restrict__ qpos, const uint8_t *__restrict__ qstrand,
                                      long long nq, const int64_t *__restrict__ first, const unsigned long long *__restrict__ emit, const unsigned long long *__restrict__ off,
                                      unsigned long long capacity, uint64_t *__restrict__ a_query, uint64_t *__restrict__ a_ref) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long c = emit[i], at = off[i];
        const uint64_t q = anchor_query(query[i], qpos[i]);
        for (unsigned long long e = 0; e < c && at + e < capacity; ++e) {
            a_query[at + e] = q;
            a_ref[at + e] = anchor_ref(values[first[i] + (int64_t)e], qstrand[i]);
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
long long tiles_of(int64_t n) { return ((long long)CARRY + n + TILE - 1) / TILE; }

size_t cub_tmp_bytes(int64_t staging) {
    size_t need = keep_scan_tmp_bytes(staging), b = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(tiles_of(staging) + 1)) == hipSuccess) need = std::max(need, b);
    return need + 256;
}

struct Workspace {
    uint8_t *raw[2], *dense;         // PieceHead (HEAD_BYTES), then the piece; the symbols
    uint32_t *pos;
    long long *starts, *closed;
    unsigned long long *tile_cnt, *tile_off;
    State *state;
    void *tmp;
    size_t tmp_bytes, bytes;
    Workspace(void *base, int64_t staging, size_t cub_bytes) {
        Carver cv{(uintptr_t)base};
        const size_t S = ((size_t)staging + 15) & ~(size_t)15, T = (size_t)tiles_of(staging) + 1;
        raw[0] = cv.take<uint8_t>(HEAD_BYTES + S); raw[1] = cv.take<uint8_t>(HEAD_BYTES + S);
        pos = cv.take<uint32_t>(S);
        dense = cv.take<uint8_t>(CARRY + S + 32);                    // (a tile's last 16-byte load may reach past the last symbol)
        starts = cv.take<long long>(TABLE_CAP); closed = cv.take<long long>(MAX_BOUND);
        tile_cnt = cv.take<unsigned long long>(T); tile_off = cv.take<unsigned long long>(T);
        state = cv.take<State>(1);
        tmp = cv.take<uint8_t>(cub_bytes);
        tmp_bytes = cub_bytes;
        bytes = cv.used;
    }
};

unsigned grid_of(long long items, int per_block) { return (unsigned)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, 4096)); }

}  // namespace

namespace coral_sketch_gpu {

struct Device {
    int k = 0, w = 0, device = 0;
    bool finished = false, started = false;
    int format_error = SKETCH_OK;
    const uint32_t *bitmap = nullptr;
    uint64_t *out_key = nullptr, *out_value = nullptr;
    uint64_t capacity = 0;
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
    const Workspace W(nullptr, staging_bytes, cub_tmp_bytes(staging_bytes));
    return (int64_t)W.bytes + 256;
}

void geometry(int32_t *out) {
    const int32_t g[8] = {TILE, CARRY, BLOCK, ITEMS, MAX_BOUND, TABLE_CAP, (int32_t)MIN_STAGING, MAX_W};
    for (int i = 0; i < 8; ++i) out[i] = g[i];
}

void close(Device *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    d->st.close();
    delete d;
}

int open(int k, int w, int device, const uint32_t *bitmap, uint64_t *out_key, uint64_t *out_value, int64_t capacity, int64_t staging_bytes, void *workspace, int64_t ws_bytes, void *stream,
         Device **out, std::string &err) {
    if (!k_ok(k) || !w_ok(w) || !out || capacity < 0 || (capacity > 0 && (!out_key || !out_value)) || staging_bytes < MIN_STAGING || staging_bytes > MAX_STAGING || device < 0) {
        err = "k outside 1..16, w outside 1..256, a missing output array, a staging size outside 16 .. 2^30 or a bad device";
        return CORAL_ERR_ARG;
    }
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    const size_t cub_bytes = cub_tmp_bytes(staging_bytes);
    const Workspace sized(nullptr, staging_bytes, cub_bytes);
    if (!workspace || ws_bytes < (int64_t)sized.bytes + 256) { err = "the workspace is smaller than coral_sketch_workspace_bytes"; return CORAL_ERR_ARG; }
    Device *d = new Device();
    d->k = k; d->w = w; d->device = device; d->bitmap = bitmap; d->out_key = out_key; d->out_value = out_value; d->capacity = (uint64_t)capacity; d->staging = staging_bytes;
    d->W = Workspace((void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255), staging_bytes, cub_bytes);
    d->closed_at = up256(HEAD_BYTES + (size_t)staging_bytes);
    d->st.retired = [d](int b) {                         // a piece that is through leaves the lengths of the contigs it closed
        const long long *closed = (const long long *)(d->st.pinned[b] + d->closed_at);
        for (uint32_t j = d->open_before[b] ? 0 : 1; j < d->n_closed[b]; ++j) d->lengths.push_back((int64_t)closed[j]);
        d->n_closed[b] = 0;
    };
    // an empty buffer: CARRY boundary symbols, which no k-mer holds, under a table entry of no contig (id -1) that starts in front
    State s0{};
    s0.hi = CARRY; s0.u = 0; s0.u_next = 0; s0.base_id = -1; s0.n_entries = 1;
    const long long start0 = -1;
    const hipStream_t s = (hipStream_t)stream;
    const bool good = hip_ok(hipMemsetAsync(d->W.dense, SYM_CONTIG, CARRY, s), "hipMemsetAsync", err) &&
                      hip_ok(hipMemcpyAsync(d->W.state, &s0, sizeof(s0), hipMemcpyHostToDevice, s), "hipMemcpyAsync", err) &&
                      hip_ok(hipMemcpyAsync(d->W.starts, &start0, sizeof(start0), hipMemcpyHostToDevice, s), "hipMemcpyAsync", err) &&
                      hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize", err) && d->st.open(s, d->closed_at + (size_t)MAX_BOUND * 8, err);
    if (!good) { close(d); return CORAL_ERR_HIP; }
    *out = d;
    return CORAL_OK;
}

// the decided positions of the buffer: count, scan, write, then the carry
static bool sketch_buffer(Device *d, int64_t n, std::string &err) {
    const Workspace &W = d->W;
    const hipStream_t s = d->st.stream;
    const long long tiles = tiles_of(n);
    if (!hip_ok(hipMemsetAsync(W.tile_cnt + tiles, 0, 8, s), "hipMemsetAsync", err)) return false;
    hipLaunchKernelGGL(k_sketch_tile<false>, dim3((unsigned)tiles), dim3(BLOCK), 0, s, W.dense, W.state, W.starts, d->k, d->w, d->bitmap, W.tile_cnt, W.tile_off,
                       (unsigned long long)d->capacity, d->out_key, d->out_value);
    size_t tb = W.tmp_bytes;
    if (!hip_ok(hipGetLastError(), "k_sketch_tile", err) || !hip_ok(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, W.tile_cnt, W.tile_off, (int)(tiles + 1), s), "scan of the tiles", err)) return false;
    hipLaunchKernelGGL(k_sketch_tile<true>, dim3((unsigned)tiles), dim3(BLOCK), 0, s, W.dense, W.state, W.starts, d->k, d->w, d->bitmap, W.tile_cnt, W.tile_off,
                       (unsigned long long)d->capacity, d->out_key, d->out_value);
    hipLaunchKernelGGL(k_sketch_carry, dim3(1), dim3(BLOCK), 0, s, W.dense, W.state, W.starts, W.tile_off, (int)tiles);
    return hip_ok(hipGetLastError(), "k_sketch_carry", err);
}

// the next piece: at most `n` bytes of it; *taken = how many it was
static int feed_piece(Device *d, const uint8_t *bytes, uint32_t n, uint32_t *taken, std::string &err) {
    PieceStager &st = d->st;
    const int b = st.acquire(err);
    if (b < 0) return CORAL_ERR_HIP;
    const bool open_before = d->started;
    int fe = SKETCH_OK;
    const uint32_t m = (uint32_t)coral_comp::scan_piece(d->line, d->names, d->started, bytes, n, MAX_BOUND, d->bounds, d->blanks, &fe);
    if (fe != SKETCH_OK) { d->format_error = fe; err = refusal_text(fe); return CORAL_ERR_FORMAT; }
    *taken = m;
    PieceHead *head = (PieceHead *)st.pinned[b];
    uint8_t *text = st.pinned[b] + HEAD_BYTES;
    const uint32_t nb = (uint32_t)d->bounds.size();
    head->n_bytes = m; head->n_bounds = nb; head->open_before = open_before; head->pad = 0;
    if (nb) memcpy(head->bounds, d->bounds.data(), (size_t)nb * 4);
    memcpy(text, bytes, m);
    for (const auto &r : d->blanks) memset(text + r.first, '\n', r.second - r.first);
    mark_contigs(text, m, d->bounds);
    const Workspace &W = d->W;
    const PieceHead *dev_head = (const PieceHead *)W.raw[b];
    const uint8_t *dev_text = W.raw[b] + HEAD_BYTES;
    bool good = st.upload(b, W.raw[b], HEAD_BYTES + m, err);
    if (good) {
        size_t tb = W.tmp_bytes;
        good = hip_ok(keep_scan(W.tmp, tb, dev_text, W.pos, m, st.stream), "scan of the keep flags", err);
    }
    if (good) {
        hipLaunchKernelGGL(k_sketch_scatter, dim3(grid_of(((long long)m + 3) / 4, SCATTER_BLOCK)), dim3(SCATTER_BLOCK), 0, st.stream, dev_text, W.pos, m, W.dense + CARRY, W.state);
        hipLaunchKernelGGL(k_sketch_walk, dim3(1), dim3(BLOCK), 0, st.stream, dev_head, W.pos, W.state, W.starts, W.closed, d->k, d->w, 0);
        good = hip_ok(hipGetLastError(), "k_sketch_walk", err);
        if (good && nb) {
            good = hip_ok(hipMemcpyAsync(st.pinned[b] + d->closed_at, W.closed, (size_t)nb * 8, hipMemcpyDeviceToHost, st.stream), "hipMemcpyAsync", err);
            if (good) { d->n_closed[b] = nb; d->open_before[b] = open_before; }
        }
        good = good && st.mark_k1(b, err);
    }
    good = good && sketch_buffer(d, m, err);
    return st.done(b, good, err) ? CORAL_OK : CORAL_ERR_HIP;
}

int feed(Device *d, const uint8_t *bytes, int64_t n, std::string &err) {
    if (!d || d->finished || n < 0 || (n > 0 && !bytes)) { err = "no session, a finished one, or no bytes"; return CORAL_ERR_ARG; }
    if (d->format_error != SKETCH_OK) { err = refusal_text(d->format_error); return CORAL_ERR_FORMAT; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    for (int64_t at = 0; at < n;) {
        uint32_t taken = 0;
        const int rc = feed_piece(d, bytes + at, (uint32_t)std::min<int64_t>(d->staging, n - at), &taken, err);
        if (rc != CORAL_OK) return rc;
        at += taken;
    }
    return CORAL_OK;
}

int finish(Device *d, uint64_t *n_out, std::vector<int64_t> &lengths, Names &names, double *seconds, std::string &err) {
    if (!d || d->finished) { err = "no session, or a finished one"; return CORAL_ERR_ARG; }
    if (d->format_error != SKETCH_OK) { err = refusal_text(d->format_error); return CORAL_ERR_FORMAT; }
    if (!hip_ok(hipSetDevice(d->device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    d->finished = true;
    if (!d->st.drain(err)) return CORAL_ERR_HIP;          // (the older piece first: its contigs come first)
    const Workspace &W = d->W;
    const hipStream_t s = d->st.stream;
    hipEvent_t *ev = d->st.ev[0];                        // (both buffers are retired: their events are free)
    if (!hip_ok(hipEventRecord(ev[EV_K0], s), "hipEventRecord", err)) return CORAL_ERR_HIP;
    hipLaunchKernelGGL(k_sketch_walk, dim3(1), dim3(BLOCK), 0, s, (const PieceHead *)nullptr, W.pos, W.state, W.starts, W.closed, d->k, d->w, 1);
    if (!hip_ok(hipGetLastError(), "k_sketch_walk", err) || !sketch_buffer(d, 0, err)) return CORAL_ERR_HIP;
    State st{};
    if (!hip_ok(hipMemcpyAsync(&st, W.state, sizeof(st), hipMemcpyDeviceToHost, s), "hipMemcpyAsync", err) || !hip_ok(hipEventRecord(ev[EV_K1], s), "hipEventRecord", err) ||
        !hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize", err))
        return CORAL_ERR_HIP;
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[EV_K0], ev[EV_K1]) == hipSuccess) d->st.seconds[3] = ms * 1e-3;
    if (d->names.in_line && !d->names.close_line()) { d->format_error = SKETCH_FORMAT_EMPTY_NAME; err = refusal_text(d->format_error); return CORAL_ERR_FORMAT; }
    if (d->started) d->lengths.push_back((int64_t)st.last_len);
    *n_out = st.total;
    lengths = d->lengths;
    names = d->names;
    if (seconds) for (int i = 0; i < 4; ++i) seconds[i] = d->st.seconds[i];
    return CORAL_OK;
}

// ---- the index -------------------------------------------------------------------------------------------------------------------
static size_t sort_tmp_bytes(int64_t n) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0, 64, (hipStream_t) nullptr);
    return b + 256;
}

int64_t sort_workspace_bytes(int64_t n) {
    if (n < 0 || n > 0x7fffffff) return CORAL_ERR_ARG;
    return (int64_t)(2 * up256((size_t)n * 8) + up256(sort_tmp_bytes(n)) + 256);
}

int sort(int device, uint64_t *keys, uint64_t *values, int64_t n, int k, void *workspace, int64_t ws_bytes, void *stream, std::string &err) {
    if (device < 0 || !k_ok(k) || n < 0 || n > 0x7fffffff || (n > 0 && (!keys || !values))) { err = "a bad device, k outside 1..16, or a missing array"; return CORAL_ERR_ARG; }
    if (n == 0) return CORAL_OK;
    if (!workspace || ws_bytes < sort_workspace_bytes(n)) { err = "the workspace is smaller than coral_sketch_sort_workspace_bytes"; return CORAL_ERR_ARG; }
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    Carver cv{((uintptr_t)workspace + 255) & ~(uintptr_t)255};
    uint64_t *k2 = cv.take<uint64_t>((size_t)n), *v2 = cv.take<uint64_t>((size_t)n);
    size_t tb = sort_tmp_bytes(n);
    void *tmp = cv.take<uint8_t>(tb);
    const hipStream_t s = (hipStream_t)stream;
    const bool good = hip_ok(hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const uint64_t *)keys, k2, (const uint64_t *)values, v2, (int)n, 0, 2 * k + 1, s), "radix sort", err) &&
                      hip_ok(hipMemcpyAsync(keys, k2, (size_t)n * 8, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync", err) &&
                      hip_ok(hipMemcpyAsync(values, v2, (size_t)n * 8, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync", err) && hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize", err);
    return good ? CORAL_OK : CORAL_ERR_HIP;
}

int lookup(int device, const uint64_t *sorted, int64_t n, const uint64_t *qkey, int64_t nq, int64_t *first, int64_t *count, void *stream, std::string &err) {
    if (device < 0 || n < 0 || nq < 0 || (n > 0 && !sorted) || (nq > 0 && (!qkey || !first || !count))) { err = "a bad device or a missing array"; return CORAL_ERR_ARG; }
    if (nq == 0) return CORAL_OK;
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sketch_lookup, dim3(grid_of(nq, 256)), dim3(256), 0, s, sorted, (long long)n, qkey, (long long)nq, 0ll, first, count, (unsigned long long *)nullptr);
    return hip_ok(hipGetLastError(), "k_sketch_lookup", err) && hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize", err) ? CORAL_OK : CORAL_ERR_HIP;
}

static size_t anchors_tmp_bytes(int64_t nq) {
    size_t b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(nq + 1));
    return b + 256;
}

int64_t anchors_workspace_bytes(int64_t nq) {
    if (nq < 0 || nq >= 0x7fffffff) return CORAL_ERR_ARG;
    return (int64_t)(4 * up256((size_t)(nq + 1) * 8) + up256(anchors_tmp_bytes(nq)) + 256);
}

int anchors(int device, const uint64_t *sorted, const uint64_t *values, int64_t n, const uint32_t *query, const uint32_t *qpos, const uint8_t *qstrand, const uint64_t *qkey, int64_t nq,
            int64_t max_occ, int64_t capacity, uint64_t *a_query, uint64_t *a_ref, void *workspace, int64_t ws_bytes, void *stream, int64_t *n_out, std::string &err) {
    if (device < 0 || n < 0 || nq < 0 || nq >= 0x7fffffff || max_occ < 0 || capacity < 0 || !n_out || (n > 0 && (!sorted || !values)) || (nq > 0 && (!query || !qpos || !qstrand || !qkey)) ||
        (capacity > 0 && (!a_query || !a_ref))) { err = "a bad device, a negative size or a missing array"; return CORAL_ERR_ARG; }
    *n_out = 0;
    if (nq == 0) return CORAL_OK;
    if (!workspace || ws_bytes < anchors_workspace_bytes(nq)) { err = "the workspace is smaller than coral_sketch_anchors_workspace_bytes"; return CORAL_ERR_ARG; }
    if (!hip_ok(hipSetDevice(device), "hipSetDevice", err)) return CORAL_ERR_HIP;
    Carver cv{((uintptr_t)workspace + 255) & ~(uintptr_t)255};
    int64_t *first = cv.take<int64_t>((size_t)nq + 1), *count = cv.take<int64_t>((size_t)nq + 1);
    unsigned long long *emit = cv.take<unsigned long long>((size_t)nq + 1), *off = cv.take<unsigned long long>((size_t)nq + 1);
    size_t tb = anchors_tmp_bytes(nq);
    void *tmp = cv.take<uint8_t>(tb);
    const hipStream_t s = (hipStream_t)stream;
    if (!hip_ok(hipMemsetAsync(emit + nq, 0, 8, s), "hipMemsetAsync", err)) return CORAL_ERR_HIP;
    hipLaunchKernelGGL(k_sketch_lookup, dim3(grid_of(nq, 256)), dim3(256), 0, s, sorted, (long long)n, qkey, (long long)nq, (long long)max_occ, first, count, emit);
    if (!hip_ok(hipGetLastError(), "k_sketch_lookup", err) || !hip_ok(hipcub::DeviceScan::ExclusiveSum(tmp, tb, emit, off, (int)(nq + 1), s), "scan of the counts", err)) return CORAL_ERR_HIP;
    if (capacity > 0) {
        hipLaunchKernelGGL(k_sketch_anchor_write, dim3(grid_of(nq, 256)), dim3(256), 0, s, values, query, qpos, qstrand, (long long)nq, first, emit, off, (unsigned long long)capacity, a_query, a_ref);
        if (!hip_ok(hipGetLastError(), "k_sketch_anchor_write", err)) return CORAL_ERR_HIP;
    }
    unsigned long long total = 0;
    if (!hip_ok(hipMemcpyAsync(&total, off + nq, 8, hipMemcpyDeviceToHost, s), "hipMemcpyAsync", err) || !hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize", err)) return CORAL_ERR_HIP;
    *n_out = (int64_t)total;
    if (*n_out > capacity) { err = "more anchors than the capacity"; return CORAL_ERR_CAPACITY; }
    return CORAL_OK;
}

}  // namespace coral_sketch_gpu
