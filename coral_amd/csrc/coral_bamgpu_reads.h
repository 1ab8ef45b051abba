// coral_bamgpu_reads.h — the reads request of the GPU BAM decoder (want_reads: FASTQ text, record bytes, coordinate order).
//   k_bam_reads_plan + k_bam_reads_emit   the selected records as FASTQ text (nibbles -> ASCII, reverse strand mirrored
//                   and complemented), scattered to scanned offsets of a per-batch buffer the host collects one batch later
//   k_bam_reads_copy   want_reads = 2: the selected records' own bytes, gathered to the same scanned offsets
//   k_bam_reads_copy_shifted   the same into a buffer whose head holds bytes carried over: a request that writes to a file
//                   (RecordSink in coral_bamgpu_deflate.h; TextSink, below, is the plain file of a FASTQ request)
//   k_bam_sort_keys + k_bam_sort_permute + k_bam_reads_copy_sorted   reads_order = 1: the same bytes in coordinate order
//                   (with MergeRuns, coral_bamgpu_merge.h: every batch's sorted run goes to a spill file, merged on the device later)
// Kernels, device structs and the host-side request in one place; included by coral_bamgpu.hip inside its anonymous namespace
// (once, behind coral_bamgpu_common.h), not a header of its own.

// ---------------------------------------------------------------------------------------------
// K_reads: the selected records as FASTQ text (want_reads; the rules: ReadsRule and reads_* in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
struct ReadsDev {                        // the request's device arrays, carved from the caller's workspace
    const int32_t *tid, *lo, *hi;        // the segments (n_seg = 0: no region limit)
    const uint8_t *names;                // the sorted names as one blob and n_names + 1 offsets (n_names = 0: no name limit)
    const int64_t *name_off;
    int n_seg;
    long long n_names;
    uint32_t exclude_flags;
    int mode;                            // READS_AS_FASTQ or READS_AS_RECORDS
};

// One thread per record (one-wave workgroups: they run beside the inflate launch): the rule, from the fixed
// fields k_bam_meta left, the end position k_bam_emit left and the name behind the record's fixed fields.  out_len[i] = bytes of
// the record's text, n_items[i] = its work items of READS_SLICE bases; both 0 when the record is not written, and in slot n_rec
// (the scans' extra entry).  In mode READS_AS_RECORDS a record without SEQ takes part too, out_len[i] is the record's own size,
// 4 + block_size, and its work items are slices of READS_COPY_SLICE of those bytes.
__global__ __launch_bounds__(WAVE) void k_bam_reads_plan(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                         MetaArrays M, const int32_t *__restrict__ end_in, ReadsDev X,
                                                         long long *__restrict__ out_len, long long *__restrict__ n_items) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    long long bytes = 0, items = 0;
    if (i < n_rec) {
        const uint32_t l_seq = (uint32_t)M.l_seq[i];
        const uint8_t *r = buf + rec_start[i];
        const uint32_t l_read_name = r[12];
        bool w = l_read_name > 0 && reads_takes_part((uint32_t)M.flag[i], l_seq, X.exclude_flags, X.mode);
        if (w && X.n_seg > 0) w = reads_meets_segment(X.tid, X.lo, X.hi, X.n_seg, M.tid[i], M.pos[i], end_in[i]);
        if (w && X.n_names > 0) w = reads_name_listed(X.names, X.name_off, X.n_names, r + 36, l_read_name - 1u);
        if (w && X.mode == READS_AS_RECORDS) {
            bytes = reads_record_bytes(ld32(r));
            items = (bytes + READS_COPY_SLICE - 1) / READS_COPY_SLICE;
        } else if (w) {
            bytes = reads_text_bytes(l_seq, l_read_name);
            items = ((long long)l_seq + READS_SLICE - 1) / READS_SLICE;
        }
    }
    out_len[i] = bytes;
    n_items[i] = items;
}

// The 16 bytes buf[p .. p + 16) for any p, from the two aligned 16-byte chunks that cover them (the second one is the first one
// of the lane that makes the next 16 characters: the same or the next cache line, served by the L1).  A chunk that does not lie
// inside [0, buf_bytes) reads as zeros: only the windows of an item's edge chunks reach outside the record, with bytes that are
// not used.
__device__ __forceinline__ uint4 reads_window(const uint8_t *__restrict__ buf, long long p, long long buf_bytes) {
    const long long base = p & ~15ll;
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
    if (base >= 0 && base + 16 <= buf_bytes) lo = *reinterpret_cast<const uint4 *>(buf + base);
    if (base + 16 >= 0 && base + 32 <= buf_bytes) hi = *reinterpret_cast<const uint4 *>(buf + base + 16);
    const uint32_t sh = (uint32_t)(p & 15);
    uint32_t d0 = lo.x, d1 = lo.y, d2 = lo.z, d3 = lo.w, d4 = hi.x, d5 = hi.y, d6 = hi.z, d7 = hi.w;
    if (sh & 8u) { d0 = d2; d1 = d3; d2 = d4; d3 = d5; d4 = d6; d5 = d7; }
    if (sh & 4u) { d0 = d1; d1 = d2; d2 = d3; d3 = d4; d4 = d5; }
    const uint32_t bs = (sh & 3u) * 8u;
    return make_uint4(__builtin_amdgcn_alignbit(d1, d0, bs), __builtin_amdgcn_alignbit(d2, d1, bs), __builtin_amdgcn_alignbit(d3, d2, bs),
                      __builtin_amdgcn_alignbit(d4, d3, bs));
}

__device__ __forceinline__ uint4 reads_mirror(uint4 v) {      // the 16 bytes in reverse order
    return make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
}

// 16 characters of SEQ.  Forward: of the bases s0 .. s0 + 15, in that order; reverse: of the same bases from s0 + 15 down to s0,
// complemented.  The nine bytes that hold the bases are read as one big-endian number N whose nibble k (from the top) is base
// s0 + k - shifted by one nibble when s0 is odd -, so that character t is the table entry of nibble t (forward) or 15 - t
// (reverse): mirroring the indices is all a reverse-strand record costs.  s0 may be negative or reach behind l_seq in an item's
// edge chunks; those characters are not stored.
template <bool REV>
__device__ __forceinline__ uint4 reads_seq_chunk(const uint8_t *__restrict__ buf, long long seq_at, long long s0, long long buf_bytes) {
    constexpr unsigned long long T_LO = reads_char_table(0, REV), T_HI = reads_char_table(1, REV);
    const uint4 v = reads_window(buf, seq_at + (s0 >> 1), buf_bytes);
    unsigned long long N = ((unsigned long long)__builtin_bswap32(v.x) << 32) | __builtin_bswap32(v.y);
    if (s0 & 1) N = (N << 4) | ((v.z & 0xffu) >> 4);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t code = (uint32_t)(N >> (REV ? 4 * t : 60 - 4 * t)) & 15u;
        const uint32_t c = (uint32_t)(((code & 8u) ? T_HI : T_LO) >> ((code & 7u) * 8u)) & 0xffu;
        w[t >> 2] |= c << (8 * (t & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t reads_qual_word(uint32_t x) {      // min(q, 93) + 33 on each of the four bytes
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= (uint32_t)reads_qual_char((x >> (8 * k)) & 0xffu) << (8 * k);
    return r;
}

// One run of an item's output: the characters [a, b) of a field (SEQ or QUAL) whose character 0 lies at out[origin].  Lane l takes
// the 16-byte aligned chunks l, l + 64, ... of the output that the run touches: one store instruction of the wave is 1 KiB of
// consecutive memory.  A chunk that lies inside the run is ONE aligned 16-byte store; the run's first and last chunk, which it may
// share with a neighbouring item or field, are stored byte by byte, only the run's own bytes.  make(j0) gives the characters
// j0 .. j0 + 15 of the field.
template <class Make>
__device__ __forceinline__ void reads_run(uint8_t *__restrict__ out, long long origin, long long a, long long b, int lane, Make make) {
    const long long c0 = (origin + a) >> 4, c1 = (origin + b - 1) >> 4;
    for (long long c = c0 + lane; c <= c1; c += WAVE) {
        const long long j0 = 16 * c - origin;
        const uint4 v = make(j0);
        if (j0 >= a && j0 + 16 <= b) {
            *reinterpret_cast<uint4 *>(out + 16 * c) = v;
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (j0 + t >= a && j0 + t < b) out[16 * c + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
        }
    }
}

// One wave per work item (one-wave workgroups, grid-stride, no LDS): the bases [k * READS_SLICE, (k + 1) * READS_SLICE) of a
// written record - their SEQ characters and their QUAL characters, two runs of the record's text at out_off[i].  Item 0 also
// writes what is not a base: `@`, the name, and the three line ends.  With flag 0x10 character j of either field comes from base
// l_seq - 1 - j: the source window of a chunk is the mirrored one, read once - no second pass.  Every output byte has exactly
// one writer (the items of a record split [0, l_seq), the records split the text): no atomics.
__global__ __launch_bounds__(WAVE) void k_bam_reads_emit(const uint8_t *__restrict__ buf, long long buf_bytes, const long long *__restrict__ rec_start,
                                                         long long n_rec, MetaArrays M, const long long *__restrict__ item_off,
                                                         const long long *__restrict__ out_off, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const long long l_seq = (long long)(uint32_t)M.l_seq[i];
        const long long rs = rec_start[i];
        const uint8_t *r = buf + rs;
        const long long l_read_name = r[12];
        const bool rev = (ld16(r + 18) & 0x10u) != 0;
        const long long seq_at = M.seq_src[i], qual_at = seq_at + (l_seq + 1) / 2;
        const bool has_qual = buf[qual_at] != 0xff;
        const long long at = out_off[i];
        const long long seq_origin = at + l_read_name + 1, qual_origin = seq_origin + l_seq + 3;
        const long long k = w - item_off[i], a = k * READS_SLICE, b = min(l_seq, a + READS_SLICE);
        if (k == 0) {
            uint8_t *o = out + at;
            for (long long j = lane; j < l_read_name - 1; j += WAVE) o[1 + j] = r[36 + j];
            if (lane == 0) {
                o[0] = '@';
                o[l_read_name] = '\n';
                out[seq_origin + l_seq] = '\n'; out[seq_origin + l_seq + 1] = '+'; out[seq_origin + l_seq + 2] = '\n';
                out[qual_origin + l_seq] = '\n';
            }
        }
        if (rev) reads_run(out, seq_origin, a, b, lane, [&](long long j0) { return reads_seq_chunk<true>(buf, seq_at, l_seq - 16 - j0, buf_bytes); });
        else reads_run(out, seq_origin, a, b, lane, [&](long long j0) { return reads_seq_chunk<false>(buf, seq_at, j0, buf_bytes); });
        reads_run(out, qual_origin, a, b, lane, [&](long long j0) {
            if (!has_qual) return make_uint4(0x22222222u, 0x22222222u, 0x22222222u, 0x22222222u);
            uint4 v = reads_window(buf, qual_at + (rev ? l_seq - 16 - j0 : j0), buf_bytes);
            if (rev) v = reads_mirror(v);
            return make_uint4(reads_qual_word(v.x), reads_qual_word(v.y), reads_qual_word(v.z), reads_qual_word(v.w));
        });
    }
}

// One wave per work item (one-wave workgroups, grid-stride, no LDS), mode READS_AS_RECORDS: the bytes [k * READS_COPY_SLICE,
// (k + 1) * READS_COPY_SLICE) of a written record - block_size word first - go from buf + rec_start[i] to out + out_off[i] as
// they stand.  Source and destination have byte alignments of their own: a lane takes an aligned 16-byte chunk of the OUTPUT,
// filled from the two aligned source chunks that cover it (reads_window) and stored as one uint4; the item's first and last
// chunk, which it may share with the neighbouring item or record, are stored byte by byte, only the item's own bytes
// (reads_run).  Every output byte has exactly one writer (the items split the record, the records split the output): no atomics.
__global__ __launch_bounds__(WAVE) void k_bam_reads_copy(const uint8_t *__restrict__ buf, long long buf_bytes, const long long *__restrict__ rec_start,
                                                         long long n_rec, const long long *__restrict__ item_off,
                                                         const long long *__restrict__ out_off, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const long long rs = rec_start[i], at = out_off[i], bytes = out_off[i + 1] - at;
        const long long a = (w - item_off[i]) * READS_COPY_SLICE, b = min(bytes, a + READS_COPY_SLICE);
        reads_run(out, at, a, b, lane, [&](long long j0) { return reads_window(buf, rs + j0, buf_bytes); });
    }
}

// k_bam_reads_copy for a request that writes to a file (RecordSink): the batch's records land `shift` bytes into `out`, behind the
// bytes the batch in front left for this one's first block.  The shift goes into the origin, not into the pointer: reads_run
// stores aligned 16-byte chunks relative to `out`, which stays 16-byte aligned; the chunk the carried bytes share with the
// batch's first record is one of reads_run's edge chunks, stored byte by byte.
__global__ __launch_bounds__(WAVE) void k_bam_reads_copy_shifted(const uint8_t *__restrict__ buf, long long buf_bytes, const long long *__restrict__ rec_start,
                                                                 long long n_rec, const long long *__restrict__ item_off,
                                                                 const long long *__restrict__ out_off, long long shift, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const long long rs = rec_start[i], at = out_off[i], bytes = out_off[i + 1] - at;
        const long long a = (w - item_off[i]) * READS_COPY_SLICE, b = min(bytes, a + READS_COPY_SLICE);
        reads_run(out, at + shift, a, b, lane, [&](long long j0) { return reads_window(buf, rs + j0, buf_bytes); });
    }
}

// Coordinate order (reads_order = 1 of a records request): between the plan and the scans the batch's records are sorted by
// reads_sort_key - hipcub's radix sort of (key, ordinal), stable, so records with equal keys keep their file order - and
// everything behind works on sorted positions: position j holds record ord[j].  All three kernels are one-wave workgroups
// (DESIGN.md §10 (vi)).
// One thread per record: its key from the fixed fields k_bam_meta left, and its ordinal.
__global__ __launch_bounds__(WAVE) void k_bam_sort_keys(long long n_rec, MetaArrays M, unsigned long long *__restrict__ key, uint32_t *__restrict__ ord) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    key[i] = reads_sort_key(M.tid[i], M.pos[i], (uint32_t)M.flag[i]);
    ord[i] = (uint32_t)i;
}

// One thread per sorted position: the plan's out_len / n_items of the record that sorts there (0 for a record that is not
// written, wherever it sorts); slot n_rec, the scans' extra entry, is 0.
__global__ __launch_bounds__(WAVE) void k_bam_sort_permute(long long n_rec, const uint32_t *__restrict__ ord, const long long *__restrict__ out_len,
                                                           const long long *__restrict__ n_items, long long *__restrict__ sorted_len,
                                                           long long *__restrict__ sorted_items) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_rec) return;
    const long long i = j < n_rec ? (long long)ord[j] : n_rec;
    sorted_len[j] = j < n_rec ? out_len[i] : 0;
    sorted_items[j] = j < n_rec ? n_items[i] : 0;
}

// k_bam_reads_copy for sorted positions (same launch shape, same work items of READS_COPY_SLICE bytes): item_off / out_off are
// the scans over the PERMUTED arrays, so work item w belongs to sorted position j, whose bytes come from record ord[j].  Every
// output byte still has exactly one writer (the items split the record, the sorted positions split the output): no atomics.
__global__ __launch_bounds__(WAVE) void k_bam_reads_copy_sorted(const uint8_t *__restrict__ buf, long long buf_bytes, const long long *__restrict__ rec_start,
                                                                long long n_rec, const uint32_t *__restrict__ ord,
                                                                const long long *__restrict__ item_off, const long long *__restrict__ out_off,
                                                                uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long j = item_record(item_off, n_rec, w);
        const long long rs = rec_start[ord[j]], at = out_off[j], bytes = out_off[j + 1] - at;
        const long long a = (w - item_off[j]) * READS_COPY_SLICE, b = min(bytes, a + READS_COPY_SLICE);
        reads_run(out, at, a, b, lane, [&](long long j0) { return reads_window(buf, rs + j0, buf_bytes); });
    }
}

#include "coral_bamgpu_deflate.h"      // RecordSink; its kernels use reads_window / reads_run above
#include "coral_bamgpu_merge.h"        // MergeRuns: the streamed coordinate sort (sorted runs to a spill file, merged on the device)

// ---- host side: the request's lifecycle (each_request in coral_bamgpu.hip, which calls all but open only when `active`) ---------
// The plain file a FASTQ request writes to (CORAL_SINK_TEXT): each batch's text goes there where `collect` would
// append it to the host-side result - no compression, no carry.  A failure leaves what was written; the destructor closes the file.
struct TextSink {
    std::string path;
    FILE *fp = nullptr;
    std::vector<uint8_t> host;           // one batch's text on its way to the file
    int64_t records = 0, bytes = 0;
    bool write(const void *dev, long long &pending) {
        host.resize((size_t)pending);
        const bool ok = dev_get(host.data(), dev, host.size()) && fwrite(host.data(), 1, host.size(), fp) == host.size();
        bytes += pending;
        pending = 0;
        return ok;
    }
    bool finish() {
        const bool ok = fclose(fp) == 0;
        fp = nullptr;
        return ok;
    }
    ~TextSink() { if (fp) fclose(fp); }
};

struct ReadsRequest {                // FASTQ text, or the own bytes (R->mode), of the selected records
    bool active = false;
    int dest = CORAL_SINK_HOST;      // where the result goes (coral_bam_sink_t::kind, set by the open call): the host-side result, or
    TextSink text_sink;              //   CORAL_SINK_TEXT: the FASTQ text goes to a plain file
    RecordSink sink;                 //   CORAL_SINK_BAM: the records go to a BGZF file; CORAL_SINK_RUNS: to the spill file, where
    MergeRuns merge;                 //   every batch's sorted run is kept track of for the merge
    const ReadsRule *R = nullptr;    // the request (Request::reads)
    ReadsDev X{};
    uint8_t *text = nullptr;         // the batch's text: one buffer for all batches (collect)
    size_t text_cap = 0, buf_bytes = 0;
    long long pending_bytes = 0;     // text of the batch emitted last that is still on the device
    // coordinate order (R->order): the sort's double buffers of keys and ordinals, the permuted plan arrays and hipcub's
    // temporary storage - carved only for such a request
    unsigned long long *sort_key[2] = {nullptr, nullptr};
    uint32_t *sort_ord[2] = {nullptr, nullptr};
    long long *sorted_len = nullptr, *sorted_items = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    bool ordered() const { return active && R->order == READS_ORDER_COORDINATE; }
    bool deflates() const { return dest == CORAL_SINK_BAM || dest == CORAL_SINK_RUNS; }      // `sink` is in use
    // What went to the file so far - records, their bytes, the file's bytes, its BGZF members (a text file: its bytes are the
    // text's, and it has no members) -, and why the sink failed, if it did.
    std::array<int64_t, 4> file_counts() const {
        if (dest == CORAL_SINK_TEXT) return {text_sink.records, text_sink.bytes, text_sink.bytes, 0};
        return {sink.records, sink.bytes, sink.file_bytes, sink.members};
    }
    const std::string &sink_error() const { return sink.error; }
    int open(const Request &Q, const Caps &C, Decoded &, std::string &err) {
        active = Q.reads.on;
        R = &Q.reads;
        if (deflates()) {
            sink.chunk = std::min(sink.chunk, C.batch_cap / coral_deflate::BLOCK_MAX + 2);      // (no batch can fill more)
            if (pack_tmp_bytes((int)sink.chunk) > DEFL_SCAN_TMP) { err = "coral_bamgpu_open_request (file sink): hipcub asks for more temporary storage than reserved"; return CORAL_ERR_HIP; }
        }
        if (!ordered()) return CORAL_OK;
        // the sort's temporary storage, queried once for the largest batch, as the scan's is
        hipcub::DoubleBuffer<unsigned long long> keys(nullptr, nullptr);
        hipcub::DoubleBuffer<uint32_t> ords(nullptr, nullptr);
        if (hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp_bytes, keys, ords, (int)std::min<size_t>(C.rec_slots, 0x7fffffff), 0, 64) != hipSuccess) {
            err = "coral_bamgpu_open_request (reads_order = 1): the size of the sort's temporary storage could not be queried";
            return CORAL_ERR_HIP;
        }
        sort_tmp_bytes += 256;
        return CORAL_OK;
    }
    // The output buffer is sized by a bound, not by a count: a record of l bases and a name field of n bytes (NUL included) takes
    // at least 36 + n + 1.5 l bytes of the batch (block_size, the fixed fields, the name, SEQ, QUAL) and its text 2 l + n + 5, and
    // 2 l + n + 5 <= 4/3 (36 + n + 1.5 l) = 48 + 4/3 n + 2 l.  So the text of all records of a batch fits 4/3 of the batch's bytes,
    // the carried ones included (+ 256: the division's remainder and room to spare).  In mode READS_AS_RECORDS the written bytes
    // are a part of the batch's own: one batch's capacity + 256.  With a sink: + 0xff00 for the bytes carried in front, and the
    // sink's own arrays - only then.
    void carve(Carver &take, const Caps &C, const Decoded &) {
        if (ordered()) {
            for (int i = 0; i < 2; ++i) { sort_key[i] = (unsigned long long *)take(C.rec_slots * 8); sort_ord[i] = (uint32_t *)take(C.rec_slots * 4); }
            sorted_len = (long long *)take(C.rec_slots * 8); sorted_items = (long long *)take(C.rec_slots * 8);
            sort_tmp = take(sort_tmp_bytes);
        }
        buf_bytes = up256(C.batch_cap + COMP_SLACK);               // (what d_infl[slot] really has: reads_window's guard)
        const size_t n_seg = R->tid.size(), n_names = (size_t)R->n_names();
        int32_t *seg = (int32_t *)take(3 * n_seg * 4);
        uint8_t *names = (uint8_t *)take(R->names.size());
        int64_t *off = (int64_t *)take((n_names + 1) * 8);
        X = ReadsDev{seg, seg + n_seg, seg + 2 * n_seg, names, off, (int)n_seg, (long long)n_names, R->exclude_flags, R->mode};
        text_cap = (R->mode == READS_AS_RECORDS ? C.batch_cap : C.batch_cap / 3 * 4) + 256;
        text = (uint8_t *)take(text_cap + (deflates() ? (size_t)coral_deflate::BLOCK_MAX : 0));
        if (deflates()) sink.carve(take);
    }
    const char *start(const Decoded &, hipError_t &e) {
        const size_t b = (size_t)X.n_seg * 4;
        const bool ok = (b == 0 || ((e = hipMemcpy((void *)X.tid, R->tid.data(), b, hipMemcpyHostToDevice)) == hipSuccess &&
                                    (e = hipMemcpy((void *)X.lo, R->lo.data(), b, hipMemcpyHostToDevice)) == hipSuccess &&
                                    (e = hipMemcpy((void *)X.hi, R->hi.data(), b, hipMemcpyHostToDevice)) == hipSuccess)) &&
                        (X.n_names == 0 || ((e = hipMemcpy((void *)X.names, R->names.data(), R->names.size(), hipMemcpyHostToDevice)) == hipSuccess &&
                                            (e = hipMemcpy((void *)X.name_off, R->name_off.data(), R->name_off.size() * 8, hipMemcpyHostToDevice)) == hipSuccess));
        if (!ok) return "reads request set-up";
        if (deflates() && !(sink.start() && (dest == CORAL_SINK_RUNS || sink.write_header(text, text_cap)))) { e = hipGetLastError(); return "record sink set-up"; }      // (a spill file has no header)
        return nullptr;
    }
    // It waits for its own totals (16 bytes: no read-back of the batch lies behind these kernels, so they are a small copy of their
    // own, as k_bam_keep_compact's count is).  The text itself is not waited for (collect).
    // The kernels take a record's l_read_name from its bytes, not from M.name_len: that array is one of the scratch pool.
    bool batch(const Batch &B, Scratch S, std::string &err) {
        if (!collect(B.D)) { err = "copy of the reads text failed"; return false; }      // (of the batch in front: its kernels have run, ours are not queued yet)
        const long long n = B.n_rec;
        if (n == 0) return dest != CORAL_SINK_RUNS || spill_run(B, {0}, {}, 0, 0, 0, nullptr, nullptr, nullptr, err);      // (an empty run)
        auto [out_len, n_items, out_off, item_off] = S.take<4>();
        hipLaunchKernelGGL(k_bam_reads_plan, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, B.stream, B.buf, B.rec_start, n, B.M, B.end, X, out_len, n_items);
        const uint32_t *ord = nullptr;                   // coordinate order: sorted position -> record of the batch
        const unsigned long long *sorted_key = nullptr;  // and the keys in that order
        if (ordered()) {
            hipLaunchKernelGGL(k_bam_sort_keys, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(WAVE), 0, B.stream, n, B.M, sort_key[0], sort_ord[0]);
            hipcub::DoubleBuffer<unsigned long long> keys(sort_key[0], sort_key[1]);
            hipcub::DoubleBuffer<uint32_t> ords(sort_ord[0], sort_ord[1]);
            size_t need = 0, tmp = sort_tmp_bytes;           // (the storage was sized for the largest batch: checked, not assumed)
            if (hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys, ords, (int)n, 0, 64, B.stream) != hipSuccess || need > sort_tmp_bytes ||
                hipcub::DeviceRadixSort::SortPairs(sort_tmp, tmp, keys, ords, (int)n, 0, 64, B.stream) != hipSuccess) {
                err = "sort of the reads keys failed";
                return false;
            }
            ord = ords.Current();
            sorted_key = keys.Current();
            hipLaunchKernelGGL(k_bam_sort_permute, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, B.stream, n, ord, out_len, n_items, sorted_len, sorted_items);
            if (!B.scan(sorted_len, out_off) || !B.scan(sorted_items, item_off)) { err = "scan of the sorted reads work items failed"; return false; }
            B.D.reads_runs.push_back((int64_t)B.D.reads_off.size() - 1);      // this batch's run begins behind what is written
        } else if (!B.scan(out_len, out_off) || !B.scan(n_items, item_off)) { err = "scan of the reads work items failed"; return false; }
        std::vector<long long> off((size_t)n + 1);
        std::vector<unsigned long long> run_keys(dest == CORAL_SINK_RUNS ? (size_t)n : 0);      // a run of the spill file: the sorted keys come with the offsets
        long long items = 0;
        const int rc = dest == CORAL_SINK_RUNS
            ? fetch_sync(B.stream, {{off.data(), out_off, (size_t)(n + 1) * 8}, {&items, item_off + n, 8}, {run_keys.data(), sorted_key, (size_t)n * 8}}, nullptr, "reads plan", err)
            : fetch_sync(B.stream, {{off.data(), out_off, (size_t)(n + 1) * 8}, {&items, item_off + n, 8}}, nullptr, "reads plan", err);
        if (rc != CORAL_OK) return false;
        const long long bytes = off[(size_t)n];
        if (bytes < 0 || (size_t)bytes > text_cap || items < 0) { err = "reads request: the batch's text does not fit its buffer"; return false; }
        if (dest == CORAL_SINK_RUNS) return spill_run(B, off, run_keys, n, bytes, items, ord, item_off, out_off, err);
        if (bytes == 0) return true;                     // no record of the batch is written: nothing more is queued
        if (dest == CORAL_SINK_BAM) {                    // to the file: behind the carried bytes, and nothing for the host-side result
            long long written = 0;
            for (long long i = 0; i < n; ++i) written += off[(size_t)i + 1] > off[(size_t)i];
            if (!sink.wait_moved(B.stream)) { err = sink.error; return false; }
            hipLaunchKernelGGL(k_bam_reads_copy_shifted, dim3((unsigned)std::min<long long>(items, 2048)), dim3(WAVE), 0, B.stream, B.buf, (long long)buf_bytes,
                               B.rec_start, n, item_off, out_off, sink.carry, text);
            if (!launched("reads", err)) return false;
            if (!sink.batch(text, bytes, written, B.stream)) { err = sink.error; return false; }
            return true;
        }
        const int64_t base = B.D.reads_off.back();
        for (long long i = 0; i < n; ++i)
            if (off[(size_t)i + 1] > off[(size_t)i]) {
                if (dest == CORAL_SINK_TEXT) ++text_sink.records;
                else B.D.reads_off.push_back(base + off[(size_t)i + 1]);
            }
        // one wave per workgroup, grid-stride beyond 8 per CU
        const dim3 grid((unsigned)std::min<long long>(items, 2048));
        if (ord)
            hipLaunchKernelGGL(k_bam_reads_copy_sorted, grid, dim3(WAVE), 0, B.stream, B.buf, (long long)buf_bytes, B.rec_start, n, ord, item_off, out_off, text);
        else if (X.mode == READS_AS_RECORDS)
            hipLaunchKernelGGL(k_bam_reads_copy, grid, dim3(WAVE), 0, B.stream, B.buf, (long long)buf_bytes, B.rec_start, n, item_off, out_off, text);
        else
            hipLaunchKernelGGL(k_bam_reads_emit, grid, dim3(WAVE), 0, B.stream, B.buf, (long long)buf_bytes, B.rec_start, n, B.M, item_off, out_off, text);
        if (!launched("reads", err)) return false;
        pending_bytes = bytes;
        return true;
    }
    // One batch of a streamed sort: the sorted copy at offset 0 of the sink's buffer - a run never shares a block with another -,
    // all of its blocks deflated right away, and what the merge needs of it kept (MergeRuns::add_run).  The chunk in flight is
    // written first, so that the file's size is where the run begins.
    bool spill_run(const Batch &B, const std::vector<long long> &off, const std::vector<unsigned long long> &run_keys, long long n, long long bytes, long long items,
                   const uint32_t *ord, const long long *item_off, const long long *out_off, std::string &err) {
        if (!sink.flush()) { err = sink.error; return false; }
        if (!merge.add_run(off, run_keys, n, sink.file_bytes)) { err = merge.error; return false; }
        if (bytes == 0) return true;
        if (!sink.wait_moved(B.stream)) { err = sink.error; return false; }
        hipLaunchKernelGGL(k_bam_reads_copy_sorted, dim3((unsigned)std::min<long long>(items, 2048)), dim3(WAVE), 0, B.stream, B.buf, (long long)buf_bytes, B.rec_start, n, ord,
                           item_off, out_off, text);
        if (!launched("reads", err)) return false;
        if (!sink.run(text, bytes, merge.runs.back().n, B.stream)) { err = sink.error; return false; }
        return true;
    }
    // The text of the batch emitted last, if it is still on the device (the caller has synchronised the stream).  One buffer for
    // all batches: QcRequest::collect's argument, under the same condition - every emit of a decode and the result call are
    // given the SAME stream.
    bool collect(Decoded &D) { return dest == CORAL_SINK_TEXT ? text_sink.write(text, pending_bytes) : collect_pending(D.reads_text, text, pending_bytes); }
    // A file is closed in its own way; what all three leave in the host-side result is the same.
    bool finish(Decoded &D, int n_threads) {
        D.has_reads = true;
        switch (dest) {
        case CORAL_SINK_RUNS:            // the spill file ends with its last run's last member: no EOF block
            if (!sink.close_plain()) return false;
            merge.spill_bytes = sink.file_bytes;
            break;
        case CORAL_SINK_BAM:
            if (!sink.finish(text)) return false;
            break;
        case CORAL_SINK_TEXT:
            if (!collect(D) || !text_sink.finish()) return false;
            break;
        default:
            return collect(D) && merge_host_runs(D, n_threads);
        }
        D.reads_in_file = true;          // nothing is kept here but the number of records and their inflated bytes
        D.reads_file_records = file_counts()[0];
        D.reads_file_bytes = file_counts()[1];
        return true;
    }
    // Coordinate order: every batch left one sorted run (D.reads_runs: the written record it begins at); more than one run goes
    // through the host's stable k-way merge, run order = batch order, and the runs are freed.
    bool merge_host_runs(Decoded &D, int n_threads) {
        if (!ordered() || D.reads_runs.size() < 2) return true;
        const size_t n_runs = D.reads_runs.size(), n_rec = D.reads_off.size() - 1;
        std::vector<const uint8_t *> data(n_runs, D.reads_text.data());
        std::vector<const int64_t *> off(n_runs);
        std::vector<int64_t> n(n_runs);
        for (size_t r = 0; r < n_runs; ++r) {
            off[r] = D.reads_off.data() + D.reads_runs[r];
            n[r] = (r + 1 < n_runs ? D.reads_runs[r + 1] : (int64_t)n_rec) - D.reads_runs[r];
        }
        std::vector<uint8_t> text(D.reads_text.size());
        std::vector<int64_t> merged(n_rec + 1);
        if (coral_bam_records_merge((int32_t)n_runs, data.data(), off.data(), n.data(), text.data(), merged.data(), n_threads) != CORAL_OK) return false;
        D.reads_text.swap(text);
        D.reads_off.swap(merged);
        D.reads_runs.assign(1, 0);
        return true;
    }
};
