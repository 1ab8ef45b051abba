// coral_sam.cpp - the host side of `import`: coral_sam_header and coral_sam_encode (include/coral_hip.h), the host build of
// coral_sam_core.h.  One thread: this is what the device path (coral_bamgpu_sam.h) is compared against, and bam.import_sam with
// device "cpu"; it replaces the parse of `samtools view -bS` (/root/reference/scripts/align_nanopore_reads.sh:34-38).
#include <hip/hip_runtime.h>      // (the core's host / device markers: hipcc compiles every source as HIP)

#include <string>

#include "../../include/coral_hip.h"
#include "coral_sam_host.h"

namespace coral_bam { void set_error(const std::string &msg); }      // coral_bam_last_error() of the calling thread (coral_bam.cpp)

using namespace coral_sam;

extern "C" int coral_sam_header(const uint8_t *text, int64_t text_bytes, int64_t *sizes, uint8_t *bam, uint8_t *names, int64_t *name_off, uint32_t *slots) {
    if (text_bytes < 0 || (text_bytes > 0 && !text) || !sizes) { coral_bam::set_error("coral_sam_header: no text, or no sizes"); return CORAL_ERR_ARG; }
    Header H;
    std::string err;
    if (!parse_header(text, text_bytes, H, err)) { coral_bam::set_error("SAM header, " + err); return CORAL_ERR_FORMAT; }
    const int64_t n_ref = (int64_t)H.name_off.size() - 1;
    sizes[0] = (int64_t)H.bam.size(); sizes[1] = n_ref; sizes[2] = H.name_off.back(); sizes[3] = (int64_t)H.slots.size(); sizes[4] = H.text_bytes; sizes[5] = H.n_lines;
    if (!bam && !names && !name_off && !slots) return CORAL_OK;
    if (!bam || !names || !name_off || !slots) { coral_bam::set_error("coral_sam_header: all four output arrays, or none"); return CORAL_ERR_ARG; }
    memcpy(bam, H.bam.data(), H.bam.size());
    memcpy(names, H.names.data(), (size_t)H.name_off.back());
    memcpy(name_off, H.name_off.data(), H.name_off.size() * 8);
    memcpy(slots, H.slots.data(), H.slots.size() * 4);
    return CORAL_OK;
}

extern "C" int coral_sam_encode(const uint8_t *text, int64_t text_bytes, int64_t first_line, const uint8_t *names, const int64_t *name_off, const uint32_t *slots, int32_t n_ref,
                                int32_t n_slots, const int32_t *keep, uint8_t *out, int64_t out_cap, int64_t *counts) {
    const char *me = "coral_sam_encode: ";
    if (text_bytes < 0 || (text_bytes > 0 && !text) || !counts || !keep || out_cap < 0) { coral_bam::set_error(std::string(me) + "a missing array"); return CORAL_ERR_ARG; }
    if (n_ref < 0 || n_slots < 0 || (n_slots & (n_slots - 1)) || (n_ref > 0 && (!names || !name_off || !slots || n_slots < 2 * n_ref))) {
        coral_bam::set_error(std::string(me) + "the contig table: n_slots must be a power of two >= 2 n_ref, with its arrays");
        return CORAL_ERR_ARG;
    }
    for (int k = 0; k < 4; ++k)
        if (keep[k] < 0) { coral_bam::set_error(std::string(me) + "record filter: negative value"); return CORAL_ERR_ARG; }
    const Contigs C{names, name_off, slots, n_ref, (uint32_t)n_slots};
    const Keep K{(uint32_t)keep[0], (uint32_t)keep[1], (uint32_t)keep[2], (uint32_t)keep[3]};
    EncodeCounts X;
    const int rc = encode_text(text, text_bytes, first_line, C, K, out, out_cap, X);
    counts[0] = X.lines; counts[1] = X.written; counts[2] = X.dropped; counts[3] = X.out_bytes; counts[4] = X.err_line; counts[5] = X.err_field;
    if (rc == 1) { coral_bam::set_error(refusal_text(X.err_line, (uint32_t)X.err_field)); return CORAL_ERR_FORMAT; }
    if (rc == 2) { coral_bam::set_error(std::string(me) + "out is too short"); return CORAL_ERR_CAPACITY; }
    return CORAL_OK;
}
