// coral_kmer.cpp - the k-mer counter's C ABI (coral_kmer_* of include/coral_hip.h): a session that is either the host backend
// (coral_kmer_host.h over coral_kmer_core.h, one thread: what the kernels are compared against, and `device="cpu"` of
// coral_amd/kmers.py) or a device session of coral_kmer.hip.  It stands in for `meryl count k=15` and `meryl print greater-than
// distinct=0.9998` of the reference's scripts/align_nanopore_reads.sh, lines 29-30.
#include <hip/hip_runtime.h>      // (the core's host / device markers: hipcc compiles every source as HIP)

#include <chrono>
#include <map>
#include <string>

#include "../../include/coral_hip.h"
#include "coral_kmer_gpu.h"

namespace coral_bam { void set_error(const std::string &msg); }      // coral_bam_last_error() of the calling thread (coral_bam.cpp)

using namespace coral_kmer;

namespace {

struct Session {
    int k = 0;
    bool finished = false, refused = false;
    HostCounter *host = nullptr;
    coral_kmer_gpu::Device *dev = nullptr;
    Stats st;
    std::map<uint64_t, uint64_t> hist;
    double host_seconds = 0;
};

int fail(int rc, const char *who, const std::string &msg) { coral_bam::set_error(std::string(who) + ": " + msg); return rc; }

}  // namespace

extern "C" int64_t coral_kmer_table_bytes(int32_t k) { return k_ok(k) ? (int64_t)(table_entries(k) * 4) : CORAL_ERR_ARG; }

extern "C" int64_t coral_kmer_workspace_bytes(int32_t k, int64_t staging_bytes) { return coral_kmer_gpu::workspace_bytes(k, staging_bytes); }

extern "C" int coral_kmer_geometry(int32_t *geometry) {
    if (!geometry) return CORAL_ERR_ARG;
    coral_kmer_gpu::geometry(geometry);
    return CORAL_OK;
}

extern "C" int coral_kmer_open(int32_t k, int32_t canonical, int32_t device, void *table, int64_t staging_bytes, void *workspace, int64_t workspace_bytes, void *stream,
                               int64_t bases_before, void **handle) {
    const char *me = "coral_kmer_open";
    if (!handle) return fail(CORAL_ERR_ARG, me, "no handle");
    *handle = nullptr;
    if (!k_ok(k) || !table || bases_before < 0 || (uint64_t)bases_before >= MAX_BASES) return fail(CORAL_ERR_ARG, me, "k outside 1..16, no table, or bases_before outside 0 .. 2^32 - 1");
    Session *s = new Session();
    s->k = k;
    if (device < 0) s->host = new HostCounter(k, canonical != 0, (uint32_t *)table, (uint64_t)bases_before);
    else {
        std::string err;
        const int rc = coral_kmer_gpu::open(k, canonical != 0, device, (uint32_t *)table, staging_bytes, workspace, workspace_bytes, stream, (uint64_t)bases_before, &s->dev, err);
        if (rc != CORAL_OK) { delete s; return fail(rc, me, err); }
    }
    *handle = s;
    return CORAL_OK;
}

extern "C" int coral_kmer_feed(void *handle, const uint8_t *bytes, int64_t n) {
    const char *me = "coral_kmer_feed";
    Session *s = (Session *)handle;
    if (!s || s->finished || n < 0 || (n > 0 && !bytes)) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no bytes");
    if (s->host) {
        if (s->refused) return fail(CORAL_ERR_CAPACITY, me, "the stream has 2^32 bases or more");
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = s->host->feed(bytes, (size_t)n);
        s->host_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!ok) { s->refused = true; return fail(CORAL_ERR_CAPACITY, me, "the stream has 2^32 bases or more"); }
        return CORAL_OK;
    }
    std::string err;
    const int rc = coral_kmer_gpu::feed(s->dev, bytes, n, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int coral_kmer_finish(void *handle, int64_t *stats, double *seconds) {
    const char *me = "coral_kmer_finish";
    Session *s = (Session *)handle;
    if (!s || s->finished || !stats) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no stats");
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (seconds) for (int i = 0; i < 4; ++i) seconds[i] = 0;
    if (s->host) {
        if (s->refused) return fail(CORAL_ERR_CAPACITY, me, "the stream has 2^32 bases or more");
        const auto t0 = std::chrono::steady_clock::now();
        s->st = s->host->st;
        table_histogram(s->host->table, s->k, s->st, s->hist);
        if (seconds) { seconds[2] = s->host_seconds; seconds[3] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    } else {
        std::string err;
        const int rc = coral_kmer_gpu::finish(s->dev, s->st, s->hist, seconds, err);
        if (rc != CORAL_OK) return fail(rc, me, err);
    }
    s->finished = true;
    stats[0] = (int64_t)s->st.n_sequences; stats[1] = (int64_t)s->st.n_bases; stats[2] = (int64_t)s->st.total; stats[3] = (int64_t)s->st.distinct;
    stats[4] = (int64_t)s->hist.size(); stats[5] = (int64_t)s->st.max_count;
    return CORAL_OK;
}

extern "C" int coral_kmer_histogram(void *handle, int64_t capacity, int64_t *values, int64_t *numbers) {
    const char *me = "coral_kmer_histogram";
    Session *s = (Session *)handle;
    if (!s || !s->finished || capacity < 0 || (capacity > 0 && (!values || !numbers))) return fail(CORAL_ERR_ARG, me, "no finished session, or a missing array");
    if ((int64_t)s->hist.size() > capacity) return fail(CORAL_ERR_CAPACITY, me, "more count values than the capacity (stats[4] of coral_kmer_finish)");
    int64_t i = 0;
    for (const auto &kv : s->hist) { values[i] = (int64_t)kv.first; numbers[i] = (int64_t)kv.second; ++i; }
    return CORAL_OK;
}

extern "C" int coral_kmer_select(void *handle, int64_t greater_than, int64_t capacity, uint64_t *kmers, uint32_t *counts, int64_t *n) {
    const char *me = "coral_kmer_select";
    Session *s = (Session *)handle;
    if (!s || !s->finished || greater_than < 0 || capacity < 0 || !n || (capacity > 0 && (!kmers || !counts))) return fail(CORAL_ERR_ARG, me, "no finished session, a negative threshold or a missing array");
    if (s->host) {
        *n = (int64_t)table_select(s->host->table, s->k, (uint64_t)greater_than, (uint64_t)capacity, kmers, counts);
        return *n > capacity ? fail(CORAL_ERR_CAPACITY, me, "more selected k-mers than the capacity") : CORAL_OK;
    }
    std::string err;
    const int rc = coral_kmer_gpu::select(s->dev, (uint64_t)greater_than, capacity, kmers, counts, n, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int coral_kmer_lookup(void *handle, const uint64_t *indices, int64_t n, uint32_t *counts) {
    const char *me = "coral_kmer_lookup";
    Session *s = (Session *)handle;
    if (!s || !s->finished || n < 0 || (n > 0 && (!indices || !counts))) return fail(CORAL_ERR_ARG, me, "no finished session, or a missing array");
    if (s->host) {
        const uint64_t entries = table_entries(s->k);
        for (int64_t i = 0; i < n; ++i) counts[i] = indices[i] < entries ? s->host->table[indices[i]] : 0;
        return CORAL_OK;
    }
    std::string err;
    const int rc = coral_kmer_gpu::lookup(s->dev, indices, n, counts, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int coral_kmer_close(void *handle) {
    Session *s = (Session *)handle;
    if (!s) return CORAL_OK;
    delete s->host;
    coral_kmer_gpu::close(s->dev);
    delete s;
    return CORAL_OK;
}
