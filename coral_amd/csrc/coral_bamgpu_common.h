// coral_bamgpu_common.h — what the GPU BAM decoder (coral_bamgpu.hip) shares with the requests that ride along it, one header
// each (coral_bamgpu_reads.h, _cov.h, _qc.h, _depth.h, _index.h): a few device helpers and the parse's per-record arrays, and the
// host-side pieces of a request's lifecycle - the workspace carver, the view of a batch, the scratch pool, the mid-batch
// read-back.  Included by coral_bamgpu.hip inside its anonymous namespace, behind its constants; not a header of its own.

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

struct MetaArrays {                                                // what k_bam_meta leaves per record
    int32_t *tid, *pos, *flag, *mapq, *l_seq, *nm, *n_cigar;       // what the host mirrors need (+ end, qlen from k_bam_emit)
    long long *cig_src, *seq_src, *sa_src;                         // buffer offsets
    long long *pad_ops, *name_len, *sa_len;                        // scan inputs (n + 1 entries, the last one 0)
};

// the record of work item w: the last i with item_off[i] <= w (item_off: the exclusive sums of n_rec + 1 item counts)
__device__ __forceinline__ long long item_record(const long long *__restrict__ item_off, long long n_rec, long long w) {
    long long a = 0, b = n_rec;
    while (b - a > 1) {
        const long long m = (a + b) >> 1;
        if (item_off[m] <= w) a = m; else b = m;
    }
    return a;
}

// what k_bam_keep and k_bam_meta leave in the parse's error word
enum { REC_ERR_SHORT = 1, REC_ERR_FIELDS = 2, REC_ERR_TAG_B = 3, REC_ERR_TAG_TYPE = 4, REC_ERR_TAG_OVERRUN = 5 };

// ---- host side ----------------------------------------------------------------------------------------------------------------
inline const char *rec_error_text(int e) {
    switch (e) {
        case REC_ERR_SHORT: return "record shorter than its fixed fields";
        case REC_ERR_FIELDS: return "record fields overrun the record";
        case REC_ERR_TAG_B: return "truncated B tag";
        case REC_ERR_TAG_TYPE: return "unknown tag type";
        case REC_ERR_TAG_OVERRUN: return "tag overruns the record";
    }
    return "malformed record";
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct BatchInfo {
    int n_blocks = 0;
    uint64_t file_off = 0, comp_bytes = 0, infl_bytes = 0;
    uint64_t ubase = 0;              // offset of the batch's first inflated byte in this range's uncompressed stream
    bool has_limit = false;          // the next byte range begins at or in front of this batch's end:
    long long limit_rel = 0;         //   at this offset from the batch's first inflated byte (negative: in an earlier batch)
    bool last = false;               // nothing follows (in this span)
    int span = 0;                    // span decode: which span the batch belongs to, whether it is the span's first batch and
    bool span_first = false;         //   where in its first block the span's first record starts
    uint32_t start_off = 0;
    bool span_tail = false;          // span decode: the batch ends with the span's last own block; what lies behind is only staged
                                     //   when the parse of this batch says that the span's last record goes on (span_verdict)
};

struct Carver {                      // hands the workspace out in 256-byte steps (p == 0: only the size is counted)
    uintptr_t p;
    size_t used = 0;
    void *operator()(size_t n) { used += up256(n); return (void *)(p + used - up256(n)); }
};

// the capacities a request sizes its part of the workspace by: BGZF blocks of a batch, its records + 1, its bytes with the carried ones
struct Caps { size_t max_blocks, rec_slots, batch_cap; };

inline bool dev_get(void *dst, const void *src, size_t bytes) { return bytes == 0 || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; }

// A request's result of the batch emitted last: appends the `pending` elements still waiting in a device buffer to v.
template <class T>
bool collect_pending(std::vector<T> &v, const void *src, long long &pending) {
    const size_t base = v.size();
    v.resize(base + (size_t)pending);
    const bool ok = dev_get(v.data() + base, src, (size_t)pending * sizeof(T));
    pending = 0;
    return ok;
}

inline bool launched(const char *what, std::string &err) {      // behind a request's launches
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = std::string(what) + " launch failed: " + hipGetErrorString(e);
    return e == hipSuccess;
}

// The one read-back in the middle of a batch: queues the copies (with d_error, also that of the parse's error word), waits for the
// stream and says what went wrong: CORAL_ERR_HIP with "`what` failed: ...", or CORAL_ERR_FORMAT with the record error's text.
struct Fetch { void *dst; const void *src; size_t bytes; };
inline int fetch_sync(hipStream_t stream, std::initializer_list<Fetch> list, const int32_t *d_error, const char *what, std::string &err) {
    int32_t rec_err = 0;
    bool ok = true;
    for (const Fetch &f : list) ok = ok && hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyDeviceToHost, stream) == hipSuccess;
    ok = ok && (!d_error || hipMemcpyAsync(&rec_err, d_error, 4, hipMemcpyDeviceToHost, stream) == hipSuccess);
    if (!ok || hipStreamSynchronize(stream) != hipSuccess) { err = std::string(what) + " failed: " + hipGetErrorString(hipGetLastError()); return CORAL_ERR_HIP; }
    if (rec_err) { err = rec_error_text(rec_err); return CORAL_ERR_FORMAT; }
    return CORAL_OK;
}

// The per-record scratch of the parse that a request may overwrite, handed to each request's batch() afresh: seven arrays of
// Caps::rec_slots 8-byte entries, of which a request takes the K it needs.
// - They are free because the batch's host copies synchronised the stream behind k_bam_emit, their last reader.
// - The next batch's k_bam_meta and scans refill them on the same stream, behind ev_parsed.
struct Scratch {
    static constexpr int N = 7;
    long long *a[N];
    template <int K>
    std::array<long long *, K> take() const {      // the first K: which ones a request gets does not matter
        static_assert(K <= N, "a request takes more scratch arrays than the parse leaves");
        std::array<long long *, K> r;
        std::copy(a, a + K, r.begin());
        return r;
    }
};

struct Batch {                       // the batch between coral_bamgpu_next and the end of coral_bamgpu_emit, as a request sees it
    hipStream_t stream;
    int slot;
    const uint8_t *buf;              // the slot's buffer: CARRY_CAP bytes for what was carried, then the batch's inflated bytes
    const long long *rec_start;      // the (kept) records' starts in buf
    long long n_rec;
    MetaArrays M;
    const int32_t *end;              // bam_endpos per record (k_bam_emit)
    const BatchInfo &info;
    long long carry_pos;             // where the batch's last whole record ends
    void *scan_tmp;                  // hipcub's temporary storage, sized for Caps::rec_slots counts
    size_t scan_tmp_bytes;
    Decoded &D;                      // the host-side result
    // exclusive sums of the batch's n_rec + 1 per-record counts (scan inputs, work items, run heads)
    bool scan(long long *in, long long *out) const {
        size_t tmp = scan_tmp_bytes;
        return hipcub::DeviceScan::ExclusiveSum(scan_tmp, tmp, in, out, (int)(n_rec + 1), stream) == hipSuccess;
    }
    // work items of `slice` bytes: at most one per record plus one per slice
    long long max_items(long long slice) const { return n_rec + ((long long)CARRY_CAP + (long long)info.infl_bytes) / slice + 1; }
};
