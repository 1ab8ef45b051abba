// coral_fastq.cpp - the C ABI of the read QC and the read filter on FASTQ text (coral_fastq_* of include/coral_hip.h): a session that is
// either the host backend (coral_fastq_host.h over coral_fastq_core.h, one thread: what the kernels are compared against, and
// `device="cpu"` of coral_amd/fastq.py) or a device session of coral_fastq.hip.  It stands in for the reference's
// scripts/report_nanopore_qc.py:35-48.
#include <hip/hip_runtime.h>      // (the core's host / device markers: hipcc compiles every source as HIP)

#include <chrono>
#include <string>

#include "../../include/coral_hip.h"
#include "coral_fastq_gpu.h"

namespace coral_bam { void set_error(const std::string &msg); }      // coral_bam_last_error() of the calling thread (coral_bam.cpp)

using namespace coral_fastq;

namespace {

struct Session {
    bool finished = false;
    HostFastq *host = nullptr;
    coral_fastq_gpu::Device *dev = nullptr;
    double host_seconds = 0;
};

int fail(int rc, const char *who, const std::string &msg) { coral_bam::set_error(std::string(who) + ": " + msg); return rc; }

int host_code(const HostFastq &h) { return h.error == FASTQ_FORMAT ? CORAL_ERR_FORMAT : CORAL_ERR_ARG; }

}  // namespace

extern "C" int64_t coral_fastq_workspace_bytes(int64_t staging_bytes) { return coral_fastq_gpu::workspace_bytes(staging_bytes); }

extern "C" int coral_fastq_geometry(int32_t *geometry) {
    if (!geometry) return CORAL_ERR_ARG;
    coral_fastq_gpu::geometry(geometry);
    return CORAL_OK;
}

extern "C" int coral_fastq_open(int32_t device, int64_t min_length, int64_t max_length, int64_t min_mean_q100, int32_t output_fd, int64_t staging_bytes, void *hist,
                                void *workspace, int64_t workspace_bytes, void *stream, void **handle) {
    const char *me = "coral_fastq_open";
    if (!handle) return fail(CORAL_ERR_ARG, me, "no handle");
    *handle = nullptr;
    if (!hist || !thresholds_ok(min_length, max_length, min_mean_q100))
        return fail(CORAL_ERR_ARG, me, "no histogram, a length threshold outside 0 .. 2^31 - 1, max_length below min_length, or min_mean_q100 outside 0 .. 9300");
    Thresholds thr;
    thr.min_length = (uint64_t)min_length; thr.max_length = (uint64_t)max_length; thr.min_mean_q100 = (uint64_t)min_mean_q100;
    Session *s = new Session();
    if (device < 0) s->host = new HostFastq(thr, output_fd, (uint64_t *)hist);
    else {
        std::string err;
        const int rc = coral_fastq_gpu::open(device, thr, output_fd, staging_bytes, hist, workspace, workspace_bytes, stream, &s->dev, err);
        if (rc != CORAL_OK) { delete s; return fail(rc, me, err); }
    }
    *handle = s;
    return CORAL_OK;
}

extern "C" int coral_fastq_feed(void *handle, const uint8_t *bytes, int64_t n) {
    const char *me = "coral_fastq_feed";
    Session *s = (Session *)handle;
    if (!s || s->finished || n < 0 || (n > 0 && !bytes)) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no bytes");
    if (s->host) {
        const auto t0 = std::chrono::steady_clock::now();
        const int e = s->host->feed(bytes, (size_t)n);
        s->host_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return e == FASTQ_OK ? CORAL_OK : fail(host_code(*s->host), me, s->host->error_text);
    }
    std::string err;
    const int rc = coral_fastq_gpu::feed(s->dev, bytes, n, err);
    return rc == CORAL_OK ? rc : fail(rc, me, err);
}

extern "C" int coral_fastq_finish(void *handle, int64_t *stats, double *seconds) {
    const char *me = "coral_fastq_finish";
    Session *s = (Session *)handle;
    if (!s || s->finished || !stats) return fail(CORAL_ERR_ARG, me, "no session, a finished one, or no stats");
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    stats[6] = -1;
    if (seconds) for (int i = 0; i < 4; ++i) seconds[i] = 0;
    s->finished = true;
    int rc = CORAL_OK;
    std::string err;
    if (s->host) {
        const auto t0 = std::chrono::steady_clock::now();
        const int e = s->host->finish();
        s->host_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (e != FASTQ_OK) { rc = host_code(*s->host); err = s->host->error_text; }
        if (seconds) { seconds[2] = s->host_seconds - s->host->out.seconds; seconds[3] = s->host->out.seconds; }
    } else rc = coral_fastq_gpu::finish(s->dev, seconds, err);
    const Stats &st = s->host ? s->host->rows.st : coral_fastq_gpu::rows(s->dev).st;
    if (st.bad_offset != NO_OFFSET) stats[6] = (int64_t)st.bad_offset;
    if (rc != CORAL_OK) return fail(rc, me, err);
    stats[0] = (int64_t)st.records; stats[1] = (int64_t)st.reads; stats[2] = (int64_t)st.no_seq; stats[3] = (int64_t)st.bases; stats[4] = (int64_t)st.kept;
    stats[5] = (int64_t)st.kept_bases;
    return CORAL_OK;
}

extern "C" int coral_fastq_rows(void *handle, int64_t n_reads, int32_t *length, int64_t *qual_sum, uint8_t *kept) {
    const char *me = "coral_fastq_rows";
    Session *s = (Session *)handle;
    if (!s || !s->finished || n_reads < 0 || (n_reads > 0 && (!length || !qual_sum || !kept))) return fail(CORAL_ERR_ARG, me, "no finished session, or a missing array");
    const Rows &r = s->host ? s->host->rows : coral_fastq_gpu::rows(s->dev);
    if (r.st.bad_offset != NO_OFFSET) return fail(CORAL_ERR_FORMAT, me, "the text was refused");
    if ((int64_t)r.length.size() > n_reads) return fail(CORAL_ERR_CAPACITY, me, "more reads than the capacity (stats[1] of coral_fastq_finish)");
    if (!r.length.empty()) {
        memcpy(length, r.length.data(), r.length.size() * sizeof(int32_t));
        memcpy(qual_sum, r.qual_sum.data(), r.qual_sum.size() * sizeof(int64_t));
        memcpy(kept, r.kept.data(), r.kept.size());
    }
    return CORAL_OK;
}

extern "C" int coral_fastq_close(void *handle) {
    Session *s = (Session *)handle;
    if (!s) return CORAL_OK;
    delete s->host;
    coral_fastq_gpu::close(s->dev);
    delete s;
    return CORAL_OK;
}
