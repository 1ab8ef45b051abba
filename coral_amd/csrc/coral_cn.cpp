// coral_cn.cpp - the host side of `cnv`: coral_cn_segment_host, coral_cn_log2_q16 and coral_cn_fdr_cut (include/coral_hip.h), the
// host build of coral_cn_core.h.  One thread: this is what the device path (coral_cngpu.hip) is compared against, and
// cnv.segment_depth with device "cpu"; it stands in for the segmentation of `cnvkit.py batch` (the reference's scripts/call_cnvs.sh).
#include <hip/hip_runtime.h>      // (the core's host / device markers: hipcc compiles every source as HIP)

#include <string.h>

#include <string>

#include "../../include/coral_hip.h"
#include "coral_cn_host.h"

namespace coral_bam { void set_error(const std::string &msg); }      // coral_bam_last_error() of the calling thread (coral_bam.cpp)

using namespace coral_cn;

extern "C" int32_t coral_cn_log2_q16(uint64_t x) { return x ? log2_q16(x) : -1; }

extern "C" int64_t coral_cn_fdr_cut(const int64_t *mags_desc, int64_t n_peaks, int64_t h, double sigma, double q) { return fdr_cut(mags_desc, n_peaks, h, sigma, q); }

extern "C" int coral_cn_segment_host(int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases, const int64_t *ref_bases,
                                     const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end,
                                     int64_t *row_probes, int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts) {
    const char *me = "coral_cn_segment_host: ";
    const Table T{n_contigs, bin_off, lengths, bin_size, bases, ref_bases, centre};
    if (!counts || row_cap < 0 || !table_ok(T, levels, fdr_q)) {
        coral_bam::set_error(std::string(me) + "a missing array, bins that do not fit the contigs, more than 2^28 bins, levels outside 1..20 or fdr_q outside (0, 1)");
        return CORAL_ERR_ARG;
    }
    Rows R;
    Counts X;
    segment_host(T, levels, fdr_q, R, X);
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    counts[0] = X.rows; counts[1] = X.kept; counts[2] = X.centre; counts[3] = X.ref_centre; counts[4] = X.breakpoints;
    if (X.rows > row_cap) { coral_bam::set_error(std::string(me) + "more rows than row_cap"); return CORAL_ERR_CAPACITY; }
    if (X.rows > 0 && (!row_contig || !row_start || !row_end || !row_probes || !row_sum_s || !row_sum_bases)) { coral_bam::set_error(std::string(me) + "a missing row array"); return CORAL_ERR_ARG; }
    const size_t n = (size_t)X.rows;
    if (n) {
        memcpy(row_contig, R.contig.data(), n * 4);
        memcpy(row_start, R.start.data(), n * 8);
        memcpy(row_end, R.end.data(), n * 8);
        memcpy(row_probes, R.probes.data(), n * 8);
        memcpy(row_sum_s, R.sum_s.data(), n * 8);
        memcpy(row_sum_bases, R.sum_bases.data(), n * 8);
    }
    return CORAL_OK;
}
