// coral_bamgpu_merge.h — the streamed coordinate sort of the GPU BAM decoder (the CORAL_SINK_RUNS sink of
// coral_bamgpu_open_request, coral_bamgpu_merge_runs; bam.sort_bam_stream): sorted runs spilled to disk while the decode runs, merged on the device.
// In both phases uncompressed record bytes exist only in HBM.
//   phase 1   ReadsRequest (coral_bamgpu_reads.h) with dest = CORAL_SINK_RUNS: every batch is sorted as for reads_order = 1, its sorted copy
//             goes to offset 0 of the sink's buffer and ALL of it is deflated (RecordSink::run): one run of the spill file, a
//             whole number of BGZF members, every one but the run's last of 0xff00 bytes.  No header, no EOF block.  What comes
//             back per written record: its 8-byte key and its length - MergeRuns below, 12 bytes per record.
//   phase 2   MergeRuns::merge.  Once: the keys go up in run-major order, ONE stable hipcub radix sort of (key, global ordinal)
//             - a tie goes to the earlier run, inside a run to the earlier record: coral_bam_records_merge's rule -,
//             k_bam_merge_lens + three scans, and the order comes back (perm, 4 bytes per record).  The host plans steps
//             (coral_merge_plan.h); per step the touched runs' members go spill file -> pinned -> device -> k_bgzf_inflate +
//             k_bgzf_crc into the staging buffer, and
//   k_bam_merge_copy   gathers the step's records, in final order, behind the carry of a second RecordSink, which cuts the
//             concatenation of all steps at 0xff00 bytes, deflates and writes: the file is coral_bgzf_write_gpu's of (sorted
//             header, all records in order).
// Host memory: 12 bytes per written record from phase 1 (16 while the keys go up: the order's 4 join them, then the keys are
// freed), the two pinned chunks of the sink and two pinned pieces of compressed spill bytes - not the records.
// Limits: fewer than 2^31 records; 52 bytes of device memory per record for the order (two key and two ordinal buffers, the
// lengths, their scan, and the two output scans; the permuted lengths and item counts live in the key buffers once the sort is
// done); the spill file is about as large as the output.  The reader is synchronous: read, upload, inflate, wait for the status
// words, copy, next step; the sink deflates and writes a step's blocks beside the next step's read and inflate.
// Kernels, device structs and the host-side struct in one place; included by coral_bamgpu_reads.h (behind RecordSink), not a
// header of its own.
#pragma once
#include "coral_merge_plan.h"

static_assert(coral_merge::BLOCK == coral_deflate::BLOCK_MAX, "the planner cuts runs where the sink did");

#define MERGE_PIN_BYTES (32ull << 20)          // one pinned piece of compressed spill bytes (two of them, used alternately)
#define MERGE_STAGE_MAX 0xf0000000ll           // BlockDesc::dst_off is 32 bits

struct U32AsI64 {
    __host__ __device__ __forceinline__ long long operator()(uint32_t x) const { return (long long)x; }
};

// One thread per sorted position j (one-wave workgroups, as every side kernel): the length of the record that sorts there and
// its work items of READS_COPY_SLICE bytes; slot n, the scans' extra entry, is 0.
__global__ __launch_bounds__(WAVE) void k_bam_merge_lens(long long n, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ len,
                                                         long long *__restrict__ sorted_len, long long *__restrict__ sorted_items) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    const long long bytes = j < n ? (long long)len[perm[j]] : 0;
    sorted_len[j] = bytes;
    sorted_items[j] = (bytes + READS_COPY_SLICE - 1) / READS_COPY_SLICE;
}

struct MergeOrder {                      // the device arrays of the order, the same for every step
    const uint32_t *perm;                // sorted position -> run-major ordinal
    const long long *src_pos;            // run-major ordinal -> its first byte in the concatenation of all runs
    const long long *run_first;          // n_runs + 1: the first ordinal of every run
    const long long *delta;              // per run, of the step: staging base - first staged byte of the run in that concatenation
    const long long *item_off, *out_off; // the scans over the sorted positions (n + 1 entries)
    int n_runs;
};

// k_bam_reads_copy_sorted's launch shape (one wave per work item, one-wave workgroups, grid-stride, no LDS): the step's work
// items are those of the sorted positions [j0, j1).  Work item w belongs to position j; its record is g = perm[j] of run r (the
// last run that begins at or in front of g: empty runs share their first ordinal with the run behind them); the bytes come from
// stage + src_pos[g] + delta[r] and go to origin carry + out_off[j] - out_off[j0] of `out`, the sink's buffer.  A lane takes an
// aligned 16-byte chunk of the OUTPUT, filled from the two aligned source chunks that cover it (reads_window: stage_bytes is
// what is allocated, a guard of 16 bytes and more behind the staged ones); an item's edge chunks are stored byte by byte
// (reads_run).  Every output byte has one writer: no atomics.
__global__ __launch_bounds__(WAVE) void k_bam_merge_copy(const uint8_t *__restrict__ stage, long long stage_bytes, MergeOrder O, long long j0, long long j1,
                                                         long long carry, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long w0 = O.item_off[j0], total = O.item_off[j1] - w0, base = carry - O.out_off[j0];
    for (long long k = blockIdx.x; k < total; k += gridDim.x) {
        const long long w = w0 + k;
        const long long j = j0 + item_record(O.item_off + j0, j1 - j0, w);
        const long long g = (long long)O.perm[j];
        int r = 0, e = O.n_runs;
        while (e - r > 1) {
            const int m = (r + e) >> 1;
            if (O.run_first[m] <= g) r = m; else e = m;
        }
        const long long src = O.src_pos[g] + O.delta[r], at = O.out_off[j], bytes = O.out_off[j + 1] - at;
        const long long a = (w - O.item_off[j]) * READS_COPY_SLICE, b = min(bytes, a + READS_COPY_SLICE);
        reads_run(out, base + at, a, b, lane, [&](long long q) { return reads_window(stage, src + q, stage_bytes); });
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
struct MergeRuns {
    struct Run { int64_t first = 0, n = 0, bytes = 0, file_off = 0; };
    std::string spill_path, error;
    size_t chunk = DEFL_CHUNK_BLOCKS;
    int64_t default_stage = 0;               // one batch's capacity: no record of a run is longer
    std::vector<Run> runs;                   // phase 1: one per batch, in batch order
    std::vector<unsigned long long> keys;    // per written record, run-major (freed once they are on the device)
    std::vector<uint32_t> lens;
    int64_t spill_bytes = 0;
    bool merged = false, out_created = false;
    // what the merge did (coral_bamgpu_merge_stats)
    int64_t steps = 0, blocks = 0, blocks_twice = 0, out_records = 0, out_bytes = 0, out_file_bytes = 0, out_members = 0;
    double t_total = 0, t_order = 0, t_read = 0, t_inflate_wait = 0, t_inflate_gpu = 0, t_copy_gpu = 0, t_sink = 0;

    int64_t n_records() const { return (int64_t)lens.size(); }
    int64_t stage_of(int64_t stage_bytes) const { return stage_bytes > 0 ? stage_bytes : default_stage; }

    // phase 1, per batch: the written records of the batch's sorted positions
    bool add_run(const std::vector<long long> &off, const std::vector<unsigned long long> &sorted_keys, long long n, int64_t file_off) {
        Run R;
        R.first = n_records();
        R.file_off = file_off;
        for (long long i = 0; i < n; ++i) {
            const long long l = off[(size_t)i + 1] - off[(size_t)i];
            if (l <= 0) continue;
            keys.push_back(sorted_keys[(size_t)i]);
            lens.push_back((uint32_t)l);
            R.bytes += l;
        }
        R.n = n_records() - R.first;
        runs.push_back(R);
        if (n_records() >= ((int64_t)1 << 31)) { error = "streamed sort: 2^31 records or more"; return false; }
        return true;
    }

    // The second workspace, carved in this order (p == 0: only the size is counted)
    struct Dev {
        unsigned long long *key[2];
        uint32_t *ord[2], *len;
        long long *src_pos, *out_off, *item_off, *run_first, *delta;
        void *sort_tmp, *scan_tmp;
        size_t sort_tmp_bytes, scan_tmp_bytes;
        uint8_t *stage, *comp, *out;
        BlockDesc *desc;
        uint32_t *crc;
        int32_t *status;
        size_t stage_alloc, comp_cap, out_cap, max_blocks, bytes;
        RecordSink *sink;
    };
    bool carve(uintptr_t p, int64_t stage, RecordSink *sink, Dev &W, std::string &err) const {
        Carver take{p};
        const size_t n = (size_t)n_records(), nr = runs.size();
        for (int i = 0; i < 2; ++i) { W.key[i] = (unsigned long long *)take((n + 1) * 8); W.ord[i] = (uint32_t *)take(n * 4); }
        W.len = (uint32_t *)take(n * 4);
        W.src_pos = (long long *)take(n * 8);
        W.out_off = (long long *)take((n + 1) * 8);
        W.item_off = (long long *)take((n + 1) * 8);
        W.run_first = (long long *)take((nr + 1) * 8);
        W.delta = (long long *)take((nr + 1) * 8);
        W.sort_tmp_bytes = W.scan_tmp_bytes = 0;
        hipcub::DoubleBuffer<unsigned long long> keys_(nullptr, nullptr);
        hipcub::DoubleBuffer<uint32_t> ords_(nullptr, nullptr);
        if (hipcub::DeviceRadixSort::SortPairs(nullptr, W.sort_tmp_bytes, keys_, ords_, (int)std::max<size_t>(n, 1), 0, 64) != hipSuccess ||
            hipcub::DeviceScan::ExclusiveSum(nullptr, W.scan_tmp_bytes, (long long *)nullptr, (long long *)nullptr, (int)(n + 1)) != hipSuccess) {
            err = "coral_bamgpu_merge: the size of hipcub's temporary storage could not be queried";
            return false;
        }
        W.sort_tmp_bytes += 256;
        W.scan_tmp_bytes += 256;
        W.sort_tmp = take(W.sort_tmp_bytes);
        W.scan_tmp = take(W.scan_tmp_bytes);
        W.stage_alloc = up256((size_t)stage + 32);                 // (reads_window's guard behind the staged bytes)
        W.stage = (uint8_t *)take(W.stage_alloc);
        W.max_blocks = (size_t)stage / coral_deflate::BLOCK_MAX + nr + 1;      // full blocks, and one short last block per run
        W.comp_cap = W.max_blocks * coral_deflate::SLOT_BYTES;      // (BSIZE is 16 bits: no member is longer than a slot)
        W.comp = (uint8_t *)take(W.comp_cap + COMP_SLACK);
        W.desc = (BlockDesc *)take(W.max_blocks * sizeof(BlockDesc));
        W.crc = (uint32_t *)take(W.max_blocks * 4);
        W.status = (int32_t *)take(W.max_blocks * 4);
        W.out_cap = (size_t)stage + 256;                           // a step's records are a part of what it staged
        W.out = (uint8_t *)take(W.out_cap + coral_deflate::BLOCK_MAX);       // + the carry in front
        W.sink = sink;
        if (sink) sink->carve(take);
        else { RecordSink probe; probe.chunk = sink_chunk(stage); probe.carve(take); }
        W.bytes = take.used;
        return true;
    }
    size_t sink_chunk(int64_t stage) const { return std::min(chunk, (size_t)stage / coral_deflate::BLOCK_MAX + 2); }      // (no step can fill more)

    int64_t workspace_bytes(int64_t stage_bytes, std::string &err) const {
        const int64_t stage = stage_of(stage_bytes);
        if (stage <= 0 || stage > MERGE_STAGE_MAX) { err = "coral_bamgpu_merge_workspace_bytes: stage_bytes must be 0 (one batch's capacity) .. 0xf0000000"; return CORAL_ERR_ARG; }
        Dev W;
        if (!carve(0, stage, nullptr, W, err)) return CORAL_ERR_HIP;
        return (int64_t)W.bytes + 256;
    }

    // what the merge owns besides the workspace
    struct Host {
        uint8_t *pin[2] = {nullptr, nullptr};
        BlockDesc *desc = nullptr;           // (pinned; the blocks' trailer CRCs follow the table in the same buffer)
        int32_t *status = nullptr;
        long long *delta = nullptr;
        hipEvent_t ev_pin[2] = {nullptr, nullptr}, ev_stage_free = nullptr, ev_t[4] = {nullptr, nullptr, nullptr, nullptr};
        bool pin_used[2] = {false, false};
        FILE *fp = nullptr;
        hipStream_t stream = nullptr;
        ~Host() {
            (void)hipStreamSynchronize(stream);      // (an error may leave uploads from the pinned buffers in flight)
            if (fp) fclose(fp);
            for (int i = 0; i < 2; ++i) { if (pin[i]) (void)hipHostFree(pin[i]); if (ev_pin[i]) (void)hipEventDestroy(ev_pin[i]); }
            if (desc) (void)hipHostFree(desc);
            if (status) (void)hipHostFree(status);
            if (delta) (void)hipHostFree(delta);
            if (ev_stage_free) (void)hipEventDestroy(ev_stage_free);
            for (hipEvent_t e : ev_t) if (e) (void)hipEventDestroy(e);
        }
    };

    int bad(int code, const std::string &what) { if (error.empty()) error = "coral_bamgpu_merge_runs: " + what; return code; }

    int merge(const char *out_path, const uint8_t *header, int64_t header_bytes, void *workspace, int64_t workspace_bytes_, int64_t stage_bytes, hipStream_t stream) {
        error.clear();
        out_created = false;
        const auto t0 = std::chrono::steady_clock::now();
        int rc;
        {
            RecordSink out;                  // (destroyed - its stream drained, its file closed - before a failed output is removed)
            rc = merge_into(out, out_path, header, header_bytes, workspace, workspace_bytes_, stage_bytes, stream);
            (void)hipStreamSynchronize(stream);      // nothing of this call is left on the stream, whatever happened
            if (rc != CORAL_OK && error.empty()) error = out.error;
            if (rc == CORAL_OK) { out_records = out.records; out_bytes = out.bytes; out_file_bytes = out.file_bytes; out_members = out.members; }
        }
        if (rc != CORAL_OK && out_created) (void)remove(out_path);      // (a refusal in front of the file's creation leaves what was there)
        merged = rc == CORAL_OK;
        t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return rc;
    }

    int merge_into(RecordSink &out, const char *out_path, const uint8_t *header, int64_t header_bytes, void *workspace, int64_t workspace_bytes_, int64_t stage_bytes,
                   hipStream_t stream) {
        using clock = std::chrono::steady_clock;
        auto since = [](clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); };
        const int64_t stage = stage_of(stage_bytes), n = n_records();
        const size_t nr = runs.size();
        if (stage <= 0 || stage > MERGE_STAGE_MAX) return bad(CORAL_ERR_ARG, "stage_bytes must be 0 (one batch's capacity) .. 0xf0000000");
        if (!workspace || (((uintptr_t)workspace) & 255)) return bad(CORAL_ERR_ARG, "no workspace, or one that is not 256-byte aligned");
        Dev W;
        std::string err;
        out.chunk = sink_chunk(stage);
        if (!carve((uintptr_t)workspace, stage, &out, W, err)) return bad(CORAL_ERR_HIP, err);
        if ((int64_t)W.bytes > workspace_bytes_) return bad(CORAL_ERR_ARG, "the workspace is smaller than coral_bamgpu_merge_workspace_bytes says");
        if (pack_tmp_bytes((int)out.chunk) > DEFL_SCAN_TMP) return bad(CORAL_ERR_HIP, "hipcub asks for more temporary storage than reserved");
        auto hip = [&](hipError_t e, const char *what) {
            if (e != hipSuccess && error.empty()) error = std::string("coral_bamgpu_merge_runs: ") + what + ": " + hipGetErrorString(e);
            return e == hipSuccess;
        };
        steps = blocks = blocks_twice = 0;
        t_order = t_read = t_inflate_wait = t_inflate_gpu = t_copy_gpu = t_sink = 0;

        // ---- the order, once -----------------------------------------------------------------------------------------------------
        const auto t_order0 = clock::now();
        std::vector<uint32_t> perm((size_t)n);
        std::vector<long long> run_first(nr + 1, 0), run_byte0(nr + 1, 0);
        std::vector<int64_t> run_records(nr);
        for (size_t r = 0; r < nr; ++r) {
            run_first[r] = runs[r].first;
            run_records[r] = runs[r].n;
            run_byte0[r + 1] = run_byte0[r] + runs[r].bytes;
        }
        run_first[nr] = n;
        MergeOrder O{nullptr, W.src_pos, W.run_first, W.delta, W.item_off, W.out_off, (int)nr};
        if (n > 0) {
            if ((int64_t)keys.size() != n) return bad(CORAL_ERR_ARG, "a merge of these runs has been started already: their keys are gone");
            for (int64_t g = 0; g < n; ++g) perm[(size_t)g] = (uint32_t)g;
            if (!hip(hipMemcpyAsync(W.key[0], keys.data(), (size_t)n * 8, hipMemcpyHostToDevice, stream), "upload of the keys") ||
                !hip(hipMemcpyAsync(W.ord[0], perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream), "upload of the ordinals") ||
                !hip(hipMemcpyAsync(W.len, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream), "upload of the lengths") ||
                !hip(hipMemcpyAsync(W.run_first, run_first.data(), (nr + 1) * 8, hipMemcpyHostToDevice, stream), "upload of the run table") ||
                !hip(hipStreamSynchronize(stream), "hipStreamSynchronize"))
                return CORAL_ERR_HIP;
            hipcub::DoubleBuffer<unsigned long long> kb(W.key[0], W.key[1]);
            hipcub::DoubleBuffer<uint32_t> ob(W.ord[0], W.ord[1]);
            size_t tmp = W.sort_tmp_bytes;
            if (!hip(hipcub::DeviceRadixSort::SortPairs(W.sort_tmp, tmp, kb, ob, (int)n, 0, 64, stream), "sort of the keys")) return CORAL_ERR_HIP;
            O.perm = ob.Current();
            long long *sorted_len = (long long *)W.key[0], *sorted_items = (long long *)W.key[1];      // (the keys are dead: n + 1 entries each)
            hipLaunchKernelGGL(k_bam_merge_lens, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, (long long)n, O.perm, W.len, sorted_len, sorted_items);
            if (!hip(hipGetLastError(), "k_bam_merge_lens")) return CORAL_ERR_HIP;
            size_t t1 = W.scan_tmp_bytes, t2 = W.scan_tmp_bytes, t3 = W.scan_tmp_bytes;
            hipcub::TransformInputIterator<long long, U32AsI64, const uint32_t *> wide(W.len, U32AsI64());
            if (!hip(hipcub::DeviceScan::ExclusiveSum(W.scan_tmp, t1, sorted_len, W.out_off, (int)(n + 1), stream), "scan of the lengths") ||
                !hip(hipcub::DeviceScan::ExclusiveSum(W.scan_tmp, t2, sorted_items, W.item_off, (int)(n + 1), stream), "scan of the work items") ||
                !hip(hipcub::DeviceScan::ExclusiveSum(W.scan_tmp, t3, wide, W.src_pos, (int)n, stream), "scan of the source positions") ||
                !hip(hipMemcpyAsync(perm.data(), O.perm, (size_t)n * 4, hipMemcpyDeviceToHost, stream), "copy of the order") ||
                !hip(hipStreamSynchronize(stream), "hipStreamSynchronize"))
                return CORAL_ERR_HIP;
        }
        coral_merge::Plan plan;
        if (const int prc = coral_merge::plan_steps((int64_t)nr, run_records.data(), lens.data(), perm.data(), stage, plan, err)) return bad(prc, err);
        std::vector<unsigned long long>().swap(keys);              // (a refusal above can be answered with a larger stage; from here the host keeps lengths and order)
        t_order = since(t_order0);

        // ---- the output: header first, in blocks of its own ----------------------------------------------------------------------------
        out.path = out_path;
        out.header.assign(header, header + header_bytes);
        if (!(out.fp = fopen(out_path, "wb"))) return bad(CORAL_ERR_ARG, std::string("cannot create ") + out_path);
        out_created = true;
        if (!(out.start() && out.write_header(W.out, W.out_cap + coral_deflate::BLOCK_MAX))) return CORAL_ERR_HIP;

        Host H;
        H.stream = stream;
        const size_t pin_bytes = std::min<size_t>(MERGE_PIN_BYTES, W.comp_cap);
        if (plan.n_steps() > 0) {
            if (!(H.fp = fopen(spill_path.c_str(), "rb"))) return bad(CORAL_ERR_FORMAT, "cannot open the spill file " + spill_path);
            bool good = hip(hipHostMalloc((void **)&H.desc, up256(W.max_blocks * (sizeof(BlockDesc) + 4)), hipHostMallocDefault), "hipHostMalloc") &&
                        hip(hipHostMalloc((void **)&H.status, up256(W.max_blocks * 4), hipHostMallocDefault), "hipHostMalloc") &&
                        hip(hipHostMalloc((void **)&H.delta, up256((nr + 1) * 8), hipHostMallocDefault), "hipHostMalloc") &&
                        hip(hipEventCreateWithFlags(&H.ev_stage_free, hipEventDisableTiming), "hipEventCreate");
            for (int i = 0; i < 2 && good; ++i)
                good = hip(hipHostMalloc((void **)&H.pin[i], pin_bytes, hipHostMallocDefault), "hipHostMalloc") &&
                       hip(hipEventCreateWithFlags(&H.ev_pin[i], hipEventDisableTiming), "hipEventCreate");
            for (int i = 0; i < 4 && good; ++i) good = hip(hipEventCreate(&H.ev_t[i]), "hipEventCreate");
            if (!good) return CORAL_ERR_HIP;
        }
        std::vector<coral_merge::RunExtent> extent(nr);
        std::vector<coral_merge::RunCursor> cursor(nr);
        for (size_t r = 0; r < nr; ++r) {
            extent[r].file_off = runs[r].file_off;
            extent[r].file_end = r + 1 < nr ? runs[r + 1].file_off : spill_bytes;
            extent[r].bytes = runs[r].bytes;
            cursor[r].off = runs[r].file_off;
        }
        auto elapsed = [&](int a, double &t) {      // (behind a wait for the stream: both events have fired)
            float ms = 0;
            if (hipEventElapsedTime(&ms, H.ev_t[a], H.ev_t[a + 1]) == hipSuccess) t += ms * 1e-3;
        };
        std::vector<long long> delta(nr + 1, 0);
        std::vector<coral_merge::Member> members;
        uint32_t *h_crc = nullptr;
        int piece = 0;
        for (int64_t s = 0; s < plan.n_steps(); ++s) {
            const int64_t j0 = plan.step_j[(size_t)s], j1 = plan.step_j[(size_t)s + 1];
            h_crc = reinterpret_cast<uint32_t *>(H.desc + W.max_blocks);
            // the staging buffer is refilled behind the copy kernel that read it
            if (s > 0 && !hip(hipStreamWaitEvent(stream, H.ev_stage_free, 0), "hipStreamWaitEvent")) return CORAL_ERR_HIP;
            size_t n_blocks = 0, comp_used = 0;
            std::fill(delta.begin(), delta.end(), 0);
            for (int64_t p = plan.step_part[(size_t)s]; p < plan.step_part[(size_t)s + 1]; ++p) {
                const coral_merge::Part &P = plan.parts[(size_t)p];
                const size_t r = (size_t)P.run;
                delta[r] = P.stage_base - P.first_block * coral_merge::BLOCK - run_byte0[r];
                if (P.n_blocks > 0 && P.first_block == cursor[r].block - 1) ++blocks_twice;
                for (int64_t b = P.first_block, end = P.first_block + P.n_blocks; b < end;) {
                    const int pi = piece++ & 1;
                    // a pinned buffer is rewritten only after its upload has completed
                    if (H.pin_used[pi] && !hip(hipEventSynchronize(H.ev_pin[pi]), "hipEventSynchronize")) return CORAL_ERR_HIP;
                    if (n_blocks + (size_t)(end - b) > W.max_blocks) return bad(CORAL_ERR_HIP, "a step has more blocks than its tables");
                    const auto t_read0 = clock::now();
                    int64_t got = 0;
                    size_t used = 0;
                    members.clear();
                    const int rrc = coral_merge::read_members(H.fp, extent[r], cursor[r], b, end - b, H.pin[pi], std::min(pin_bytes, W.comp_cap - comp_used), members, &got,
                                                              &used, err);
                    t_read += since(t_read0);
                    if (rrc != coral_merge::PLAN_OK) return bad(rrc == coral_merge::PLAN_ERR_FORMAT ? CORAL_ERR_FORMAT : CORAL_ERR_HIP, err);
                    for (int64_t m = 0; m < got; ++m) {
                        const coral_merge::Member &M = members[(size_t)m];
                        H.desc[n_blocks] = BlockDesc{(uint32_t)(comp_used + M.src_off), M.src_len, (uint32_t)(P.stage_base + (b + m - P.first_block) * coral_merge::BLOCK), M.isize};
                        h_crc[n_blocks] = M.crc;
                        ++n_blocks;
                    }
                    if (!hip(hipMemcpyAsync(W.comp + comp_used, H.pin[pi], used, hipMemcpyHostToDevice, stream), "upload of the spill's members") ||
                        !hip(hipEventRecord(H.ev_pin[pi], stream), "hipEventRecord"))
                        return CORAL_ERR_HIP;
                    H.pin_used[pi] = true;
                    comp_used += used;
                    b += got;
                }
            }
            // inflate + checksums into the staging buffer (the launch code of coral_bgzf_inflate and of the decoder), then the status words
            const auto t_wait0 = clock::now();
            if (n_blocks > 0) {
                if (!hip(hipMemcpyAsync(W.desc, H.desc, n_blocks * sizeof(BlockDesc), hipMemcpyHostToDevice, stream), "upload of the block table") ||
                    !hip(hipMemcpyAsync(W.crc, h_crc, n_blocks * 4, hipMemcpyHostToDevice, stream), "upload of the checksums"))
                    return CORAL_ERR_HIP;
                (void)hipEventRecord(H.ev_t[0], stream);
                hipLaunchKernelGGL(k_bgzf_inflate<0>, dim3((unsigned)((n_blocks + INFL_WAVES - 1) / INFL_WAVES)), dim3(INFL_WAVES * WAVE), 0, stream, W.comp, W.desc, (int)n_blocks,
                                   W.stage, W.status);
                if (!hip(hipGetLastError(), "k_bgzf_inflate")) return CORAL_ERR_HIP;
                hipLaunchKernelGGL(k_bgzf_crc, dim3((unsigned)n_blocks), dim3(WAVE), 0, stream, W.stage, W.desc, W.crc, (int)n_blocks, W.status);
                if (!hip(hipGetLastError(), "k_bgzf_crc")) return CORAL_ERR_HIP;
                (void)hipEventRecord(H.ev_t[1], stream);
                if (!hip(hipMemcpyAsync(H.status, W.status, n_blocks * 4, hipMemcpyDeviceToHost, stream), "copy of the status words")) return CORAL_ERR_HIP;
            }
            if (!hip(hipStreamSynchronize(stream), "hipStreamSynchronize")) return CORAL_ERR_HIP;
            t_inflate_wait += since(t_wait0);
            if (n_blocks > 0) elapsed(0, t_inflate_gpu);
            if (s > 0) elapsed(2, t_copy_gpu);                     // (of the step in front)
            for (size_t b = 0; b < n_blocks; ++b)
                if (H.status[b] != 0) {
                    char msg[160];
                    snprintf(msg, sizeof msg, "block %zu of step %lld of the spill file does not inflate (%s %d)", b, (long long)s, H.status[b] == ERR_CRC ? "checksum, status" : "status",
                             (int)H.status[b]);
                    return bad(CORAL_ERR_FORMAT, msg);
                }
            blocks += (int64_t)n_blocks;
            // the copy: behind the sink's tail move and the deflate that read its buffer
            long long bytes = 0, items = 0;
            for (int64_t j = j0; j < j1; ++j) {
                const long long l = lens[perm[(size_t)j]];
                bytes += l;
                items += (l + READS_COPY_SLICE - 1) / READS_COPY_SLICE;
            }
            if ((size_t)bytes > W.out_cap) return bad(CORAL_ERR_HIP, "a step's records do not fit the sink's buffer");
            const auto t_sink0 = clock::now();
            memcpy(H.delta, delta.data(), (nr + 1) * 8);          // (its last upload lies in front of the wait above)
            if (!hip(hipMemcpyAsync(W.delta, H.delta, (nr + 1) * 8, hipMemcpyHostToDevice, stream), "upload of the step's run words")) return CORAL_ERR_HIP;
            if (!out.wait_moved(stream)) return CORAL_ERR_HIP;
            (void)hipEventRecord(H.ev_t[2], stream);
            if (items > 0) {
                hipLaunchKernelGGL(k_bam_merge_copy, dim3((unsigned)std::min<long long>(items, 2048)), dim3(WAVE), 0, stream, W.stage, (long long)W.stage_alloc, O, (long long)j0,
                                   (long long)j1, out.carry, W.out);
                if (!hip(hipGetLastError(), "k_bam_merge_copy")) return CORAL_ERR_HIP;
            }
            (void)hipEventRecord(H.ev_t[3], stream);
            if (!hip(hipEventRecord(H.ev_stage_free, stream), "hipEventRecord")) return CORAL_ERR_HIP;
            if (!out.batch(W.out, bytes, j1 - j0, stream)) return CORAL_ERR_HIP;
            t_sink += since(t_sink0);
            ++steps;
        }
        if (!hip(hipStreamSynchronize(stream), "hipStreamSynchronize")) return CORAL_ERR_HIP;
        if (plan.n_steps() > 0) elapsed(2, t_copy_gpu);
        const auto t_fin0 = clock::now();
        if (!out.finish(W.out)) return CORAL_ERR_HIP;
        t_sink += since(t_fin0);
        return CORAL_OK;
    }
};
