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

extern "C" int coral_cn_segment_gc_host(int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases, const int64_t *ref_bases,
                                        const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end,
                                        int64_t *row_probes, int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts, const uint32_t *gc, const uint32_t *at,
                                        int32_t gc_strata, int64_t gc_min_bins, int32_t min_called_permille, int64_t *bias, int64_t *stratum_bins) {
    const char *me = gc ? "coral_cn_segment_gc_host: " : "coral_cn_segment_host: ";
    Table T{n_contigs, bin_off, lengths, bin_size, bases, ref_bases, centre};
    T.gc = gc; T.at = at;
    if (gc) { T.gc_strata = gc_strata; T.gc_min_bins = gc_min_bins; T.min_called_permille = min_called_permille; }
    if (!counts || row_cap < 0 || !table_ok(T, levels, fdr_q) || (gc && (!bias || !stratum_bins))) {
        coral_bam::set_error(std::string(me) + "a missing array, bins that do not fit the contigs, more than 2^28 bins, levels outside 1..20, fdr_q outside (0, 1), gc_strata outside "
                                               "1..1000, gc_min_bins below 1 or min_called_permille outside 0..1000");
        return CORAL_ERR_ARG;
    }
    Rows R;
    Counts X;
    GcBias G;
    segment_host(T, levels, fdr_q, R, X, &G);
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    counts[0] = X.rows; counts[1] = X.kept; counts[2] = X.centre; counts[3] = X.ref_centre; counts[4] = X.breakpoints; counts[5] = X.uncalled;
    if (gc) for (int32_t g = 0; g <= gc_strata; ++g) { bias[g] = G.bias[(size_t)g]; stratum_bins[g] = G.stratum_bins[(size_t)g]; }
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

extern "C" int coral_cn_segment_host(int32_t n_contigs, const int64_t *bin_off, const int64_t *lengths, int64_t bin_size, const int64_t *bases, const int64_t *ref_bases,
                                     const uint8_t *centre, int32_t levels, double fdr_q, int64_t row_cap, int32_t *row_contig, int64_t *row_start, int64_t *row_end,
                                     int64_t *row_probes, int64_t *row_sum_s, int64_t *row_sum_bases, int64_t *counts) {
    return coral_cn_segment_gc_host(n_contigs, bin_off, lengths, bin_size, bases, ref_bases, centre, levels, fdr_q, row_cap, row_contig, row_start, row_end, row_probes, row_sum_s,
                                    row_sum_bases, counts, nullptr, nullptr, 0, 0, 0, nullptr, nullptr);
}
