// coral_sketch.cpp - the minimizer sketch's C ABI (coral_sketch_* of include/coral_hip.h): a session that is either the host backend
// (coral_sketch_host.h over coral_sketch_core.h, one thread: what the kernels are compared against, and `device="cpu"` of
// coral_amd/minimizers.py) or a device session of coral_sketch.hip; and the seed index over two arrays, host (device < 0) or
// device.  It is the first stage of `winnowmap -W repetitive_k15.txt -ax map-ont` of the reference's
// scripts/align_nanopore_reads.sh, line 34.
#include <hip/hip_runtime.h>      // (the core's host / device markers: hipcc compiles every source as HIP)

#include <chrono>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_sketch_gpu.h"

namespace coral_bam { void set_error(const std::string &msg); }      // coral_bam_last_error() of the calling thread (coral_bam.cpp)

using namespace coral_sketch;

namespace {

struct Session {
    bool finished = false;
    uint64_t capacity = 0;
    HostSketcher *host = nullptr;
    coral_sketch_gpu::Device *dev = nullptr;
    std::vector<int64_t> lengths;
    Names names;
    double host_seconds = 0;
};

int fail(int rc, const char *who, const std::string &msg) { coral_bam::set_error(std::string(who) + ": " + msg); return rc; }
int refused(const char *who, int e) { return fail(e == SKETCH_TOO_LONG ? CORAL_ERR_CAPACITY : CORAL_ERR_FORMAT, who, refusal_text(e)); }

}  // namespace

extern "C" int64_t coral_sketch_bitmap_bytes(int32_t k) { return k_ok(k) ? (int64_t)(bitmap_words(k) * 4) : CORAL_ERR_ARG; }

extern "C" int64_t coral_sketch_workspace_bytes(int64_t staging_bytes) { return coral_sketch_gpu::workspace_bytes(staging_bytes); }

extern "C" int coral_sketch_geometry(int32_t *geometry) {
    if (!geometry) return CORAL_ERR_ARG;
    coral_sketch_gpu::geometry(geometry);
    return CORAL_OK;
}

extern "C" int coral_sketch_open(int32_t k, int32_t w, int32_t device, const void *weights, void *keys, void *values, int64_t capacity, int64_t staging_bytes, void *workspace,
                                 int64_t workspace_bytes, void *stream, void **handle) {
    const char *me = "coral_sketch_open";
    if (!handle) return fail(CORAL_ERR_ARG, me, "no handle");
    *handle = nullptr;
    if (!k_ok(k) || !w_ok(w) || capacity < 0 || (capacity > 0 && (!keys || !values))) return fail(CORAL_ERR_ARG, me, "k outside 1..16, w outside 1..256, or a missing output array");
    Session *s = new Session();
    s->capacity = (uint64_t)capacity;
    if (device < 0) s->host = new HostSketcher(k, w, (const uint32_t *)weights, (uint64_t *)keys, (uint64_t *)values, capacity);
    else {
        std::string err;
        const int rc = coral_sketch_gpu::open(k, w, device, (const uint32_t *)weights, (uint64_t *)keys, (uint64_t *)values, capacity, staging_bytes, workspace, workspace_bytes, stream, &s->dev, err);
        if (rc != CORAL_OK) { delete s; return fail(rc, me, err); }
    }
    *handle = s;
    return CORAL_OK;
}

extern "C" int coral_sketch_feed(void *handle, const uint8_t *bytes, int64_t n) {
    const char *me = "coral_sketch_feed";
    Session *s = (Session *)handle;
    if (!s || s->finished || n < 0 || (n > 0 && !bytes)) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no bytes");
    if (s->host) {
        const auto t0 = std::chrono::steady_clock::now();
        const int e = s->host->feed(bytes, (size_t)n);
        s->host_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return e == SKETCH_OK ? CORAL_OK : refused(me, e);
    }
    std::string err;
    const int rc = coral_sketch_gpu::feed(s->dev, bytes, n, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int coral_sketch_finish(void *handle, int64_t *stats, double *seconds) {
    const char *me = "coral_sketch_finish";
    Session *s = (Session *)handle;
    if (!s || s->finished || !stats) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no stats");
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (seconds) for (int i = 0; i < 4; ++i) seconds[i] = 0;
    uint64_t n_out = 0;
    if (s->host) {
        const auto t0 = std::chrono::steady_clock::now();
        const int e = s->host->finish();
        if (e != SKETCH_OK) return refused(me, e);
        n_out = s->host->n_out;
        s->lengths = s->host->lengths;
        s->names = s->host->names;
        if (seconds) { seconds[2] = s->host_seconds; seconds[3] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    } else {
        std::string err;
        const int rc = coral_sketch_gpu::finish(s->dev, &n_out, s->lengths, s->names, seconds, err);
        if (rc != CORAL_OK) return fail(rc, me, err);
        if (!contigs_fit(s->lengths)) return refused(me, SKETCH_TOO_LONG);
    }
    s->finished = true;
    int64_t positions = 0;
    for (int64_t l : s->lengths) positions += l;
    stats[0] = (int64_t)s->lengths.size(); stats[1] = positions; stats[2] = (int64_t)n_out; stats[3] = (int64_t)std::min<uint64_t>(n_out, s->capacity);
    stats[6] = (int64_t)s->names.blob.size();
    if (n_out > s->capacity) return fail(CORAL_ERR_CAPACITY, me, "more minimizers than the capacity (stats[2] suffices)");
    return CORAL_OK;
}

extern "C" int coral_sketch_contigs(void *handle, int64_t n_contigs, int64_t *lengths, int64_t names_capacity, uint8_t *names, int64_t *name_off) {
    const char *me = "coral_sketch_contigs";
    Session *s = (Session *)handle;
    if (!s || !s->finished || n_contigs < 0 || names_capacity < 0 || (n_contigs > 0 && !lengths) || !name_off || (names_capacity > 0 && !names))
        return fail(CORAL_ERR_ARG, me, "no finished session, or a missing array");
    if ((int64_t)s->lengths.size() > n_contigs || (int64_t)s->names.blob.size() > names_capacity)
        return fail(CORAL_ERR_CAPACITY, me, "more contigs or name bytes than the capacities (stats[0] and stats[6] of coral_sketch_finish)");
    for (size_t c = 0; c < s->lengths.size(); ++c) lengths[c] = s->lengths[c];
    for (size_t c = 0; c <= s->lengths.size(); ++c) name_off[c] = s->names.off[c];
    if (!s->names.blob.empty()) memcpy(names, s->names.blob.data(), s->names.blob.size());
    return CORAL_OK;
}

extern "C" int coral_sketch_close(void *handle) {
    Session *s = (Session *)handle;
    if (!s) return CORAL_OK;
    delete s->host;
    coral_sketch_gpu::close(s->dev);
    delete s;
    return CORAL_OK;
}

// ---- the index ---------------------------------------------------------------------------------------------------------------------
extern "C" int64_t coral_sketch_sort_workspace_bytes(int64_t n) { return coral_sketch_gpu::sort_workspace_bytes(n); }

extern "C" int coral_sketch_sort(int32_t device, void *keys, void *values, int64_t n, int32_t k, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *me = "coral_sketch_sort";
    if (device < 0) {
        if (n < 0 || (n > 0 && (!keys || !values))) return fail(CORAL_ERR_ARG, me, "a missing array");
        sort_pairs((uint64_t *)keys, (uint64_t *)values, (size_t)n);
        return CORAL_OK;
    }
    std::string err;
    const int rc = coral_sketch_gpu::sort(device, (uint64_t *)keys, (uint64_t *)values, n, k, workspace, workspace_bytes, stream, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int coral_sketch_lookup(int32_t device, const void *sorted_keys, int64_t n, const void *query_keys, int64_t n_queries, int64_t *first, int64_t *count, void *stream) {
    const char *me = "coral_sketch_lookup";
    if (device < 0) {
        if (n < 0 || n_queries < 0 || (n > 0 && !sorted_keys) || (n_queries > 0 && (!query_keys || !first || !count))) return fail(CORAL_ERR_ARG, me, "a missing array");
        for (int64_t i = 0; i < n_queries; ++i) find_entries((const uint64_t *)sorted_keys, n, ((const uint64_t *)query_keys)[i], first + i, count + i);
        return CORAL_OK;
    }
    std::string err;
    const int rc = coral_sketch_gpu::lookup(device, (const uint64_t *)sorted_keys, n, (const uint64_t *)query_keys, n_queries, first, count, stream, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int64_t coral_sketch_anchors_workspace_bytes(int64_t n_queries) { return coral_sketch_gpu::anchors_workspace_bytes(n_queries); }

extern "C" int coral_sketch_anchors(int32_t device, const void *sorted_keys, const void *values, int64_t n, const uint32_t *query, const uint32_t *qpos, const uint8_t *qstrand,
                                    const void *qkey, int64_t n_queries, int64_t max_occ, int64_t capacity, void *anchor_query, void *anchor_ref, void *workspace, int64_t workspace_bytes,
                                    void *stream, int64_t *n_anchors) {
    const char *me = "coral_sketch_anchors";
    if (device < 0) {
        if (n < 0 || n_queries < 0 || max_occ < 0 || capacity < 0 || !n_anchors || (n > 0 && (!sorted_keys || !values)) || (n_queries > 0 && (!query || !qpos || !qstrand || !qkey)) ||
            (capacity > 0 && (!anchor_query || !anchor_ref)))
            return fail(CORAL_ERR_ARG, me, "a negative size or a missing array");
        *n_anchors = expand_anchors((const uint64_t *)sorted_keys, (const uint64_t *)values, n, query, qpos, qstrand, (const uint64_t *)qkey, n_queries, max_occ, capacity,
                                    (uint64_t *)anchor_query, (uint64_t *)anchor_ref);
        return *n_anchors > capacity ? fail(CORAL_ERR_CAPACITY, me, "more anchors than the capacity") : CORAL_OK;
    }
    std::string err;
    const int rc = coral_sketch_gpu::anchors(device, (const uint64_t *)sorted_keys, (const uint64_t *)values, n, query, qpos, qstrand, (const uint64_t *)qkey, n_queries, max_occ, capacity,
                                             (uint64_t *)anchor_query, (uint64_t *)anchor_ref, workspace, workspace_bytes, stream, n_anchors, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}
