// coral_comp.cpp - the C ABI of the reference's per-bin composition (coral_comp_* of include/coral_hip.h): a session that is either
// the host backend (coral_comp_host.h over coral_comp_core.h, one thread: what the kernels are compared against, and
// `device="cpu"` of coral_amd/composition.py) or a device session of coral_comp.hip.  It stands in for the GC and repeat-mask
// columns of the reference table that the reference's scripts/call_cnvs.sh:12-17 hands to `cnvkit.py batch --reference`.
#include <hip/hip_runtime.h>      // (the core's host / device markers: hipcc compiles every source as HIP)

#include <chrono>
#include <string>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_comp_gpu.h"

namespace coral_bam { void set_error(const std::string &msg); }      // coral_bam_last_error() of the calling thread (coral_bam.cpp)

using namespace coral_comp;

namespace {

struct Session {
    bool finished = false;
    uint64_t capacity = 0;
    HostComposer *host = nullptr;
    coral_comp_gpu::Device *dev = nullptr;
    Stats st;
    std::vector<int64_t> lengths;
    Names names;
    double host_seconds = 0;
};

int fail(int rc, const char *who, const std::string &msg) { coral_bam::set_error(std::string(who) + ": " + msg); return rc; }

}  // namespace

extern "C" int64_t coral_comp_workspace_bytes(int64_t staging_bytes) { return coral_comp_gpu::workspace_bytes(staging_bytes); }

extern "C" int coral_comp_geometry(int32_t *geometry) {
    if (!geometry) return CORAL_ERR_ARG;
    coral_comp_gpu::geometry(geometry);
    return CORAL_OK;
}

extern "C" int coral_comp_open(int64_t bin_size, int32_t device, void *gc, void *at, void *masked, int64_t capacity, int64_t staging_bytes, void *workspace,
                               int64_t workspace_bytes, void *stream, void **handle) {
    const char *me = "coral_comp_open";
    if (!handle) return fail(CORAL_ERR_ARG, me, "no handle");
    *handle = nullptr;
    if (!bin_size_ok(bin_size) || !gc || !at || !masked || capacity < 1 || capacity > MAX_BINS)
        return fail(CORAL_ERR_ARG, me, "bin_size outside 1 .. 2^31 - 1, a missing table, or a capacity outside 1 .. 2^28");
    Session *s = new Session();
    s->capacity = (uint64_t)capacity;
    if (device < 0) s->host = new HostComposer(bin_size, (uint32_t *)gc, (uint32_t *)at, (uint32_t *)masked, capacity);
    else {
        std::string err;
        const int rc = coral_comp_gpu::open(bin_size, device, (uint32_t *)gc, (uint32_t *)at, (uint32_t *)masked, capacity, staging_bytes, workspace, workspace_bytes, stream, &s->dev, err);
        if (rc != CORAL_OK) { delete s; return fail(rc, me, err); }
    }
    *handle = s;
    return CORAL_OK;
}

extern "C" int coral_comp_feed(void *handle, const uint8_t *bytes, int64_t n) {
    const char *me = "coral_comp_feed";
    Session *s = (Session *)handle;
    if (!s || s->finished || n < 0 || (n > 0 && !bytes)) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no bytes");
    if (s->host) {
        const auto t0 = std::chrono::steady_clock::now();
        const int e = s->host->feed(bytes, (size_t)n);
        s->host_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return e == COMP_OK ? CORAL_OK : fail(CORAL_ERR_FORMAT, me, format_text(e));
    }
    std::string err;
    const int rc = coral_comp_gpu::feed(s->dev, bytes, n, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int coral_comp_finish(void *handle, int64_t *stats, double *seconds) {
    const char *me = "coral_comp_finish";
    Session *s = (Session *)handle;
    if (!s || s->finished || !stats) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no stats");
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    if (seconds) for (int i = 0; i < 4; ++i) seconds[i] = 0;
    if (s->host) {
        const int e = s->host->finish();
        if (e != COMP_OK) return fail(CORAL_ERR_FORMAT, me, format_text(e));
        s->st = s->host->st;
        s->lengths = s->host->lengths;
        s->names = s->host->names;
        if (seconds) seconds[2] = s->host_seconds;
    } else {
        std::string err;
        const int rc = coral_comp_gpu::finish(s->dev, s->st, s->lengths, s->names, seconds, err);
        if (rc != CORAL_OK) return fail(rc, me, err);
    }
    s->finished = true;
    stats[0] = (int64_t)s->st.n_contigs; stats[1] = (int64_t)s->st.positions; stats[2] = (int64_t)s->st.bins; stats[3] = (int64_t)s->st.gc; stats[4] = (int64_t)s->st.at;
    stats[5] = (int64_t)s->st.masked; stats[6] = (int64_t)s->names.blob.size();
    if (s->st.bins > s->capacity) return fail(CORAL_ERR_CAPACITY, me, s->st.bins > (uint64_t)MAX_BINS ? "more than 2^28 bins: choose a larger bin_size" : "more bins than the capacity (stats[2] suffices)");
    return CORAL_OK;
}

extern "C" int coral_comp_contigs(void *handle, int64_t n_contigs, int64_t *lengths, int64_t names_capacity, uint8_t *names, int64_t *name_off) {
    const char *me = "coral_comp_contigs";
    Session *s = (Session *)handle;
    if (!s || !s->finished || n_contigs < 0 || names_capacity < 0 || (n_contigs > 0 && !lengths) || !name_off || (names_capacity > 0 && !names))
        return fail(CORAL_ERR_ARG, me, "no finished session, or a missing array");
    if ((int64_t)s->lengths.size() > n_contigs || (int64_t)s->names.blob.size() > names_capacity)
        return fail(CORAL_ERR_CAPACITY, me, "more contigs or name bytes than the capacities (stats[0] and stats[6] of coral_comp_finish)");
    for (size_t c = 0; c < s->lengths.size(); ++c) lengths[c] = s->lengths[c];
    for (size_t c = 0; c <= s->lengths.size(); ++c) name_off[c] = s->names.off[c];
    if (!s->names.blob.empty()) memcpy(names, s->names.blob.data(), s->names.blob.size());
    return CORAL_OK;
}

extern "C" int coral_comp_close(void *handle) {
    Session *s = (Session *)handle;
    if (!s) return CORAL_OK;
    delete s->host;
    coral_comp_gpu::close(s->dev);
    delete s;
    return CORAL_OK;
}
