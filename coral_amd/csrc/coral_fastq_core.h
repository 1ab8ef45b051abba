// coral_fastq_core.h - the rule of the read QC and the read filter on FASTQ text (`qc --fastq`, `filter`), written once: small inline
// functions that the host backend (coral_fastq_host.h, coral_fastq.cpp) and the kernels (coral_fastq.hip) both call, so that both give
// the same rows, the same histogram and the same refusals.  It stands in for the reference's scripts/report_nanopore_qc.py:35-48
// (`pysam.FastxFile`, `len(sequence)`, `np.mean(quality)` of every record that has a sequence); DESIGN.md §4 states the rule in words.
//
//   - a line starts at the first byte of the stream and behind every '\n'; line k (from 0) has phase k mod 4; four lines are one
//     record: name, sequence, separator, quality.
//   - a phase-0 line must start with '@', a phase-2 line with '+'; the rest of either is not looked at.
//   - '\r' is skipped wherever it stands in a phase-1 or phase-3 line; every other byte of a phase-1 line is one base (`length`,
//     at most 2^31 - 1), every other byte of a phase-3 line one quality character q, 33 <= q <= 126, that adds q - 33 to the
//     record's `qual_sum` and 1 to the histogram's bin q - 33.  A record's quality count must equal its length.
//   - the stream may end at a record boundary, inside a phase-3 line or right behind the '\n' of a phase-2 line (either closes the
//     record); everything else is refused, at the stream offset of the first offending byte: a wrong first byte or a quality
//     character out of range at that byte, a record whose counts differ (or whose length is too large) at the byte that closes it
//     (its quality line's '\n', or the end of the stream), a stream that ends inside lines 0-2 at its end.
//   - a record is kept iff length >= min_length, (max_length == 0 or length <= max_length) and 100 * qual_sum >= min_mean_q100 *
//     length, in 64-bit integers: the arithmetic mean of the Phred values in hundredths, not a mean of error probabilities.
// No HIP in this header beyond the host / device markers.
#ifndef CORAL_FASTQ_CORE_H
#define CORAL_FASTQ_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CORAL_FASTQ_HD __host__ __device__ inline
#else
#define CORAL_FASTQ_HD inline
#endif

namespace coral_fastq {

constexpr uint64_t MAX_LENGTH = 0x7fffffffull;
constexpr int64_t MAX_MEAN_Q100 = 9300;              // '~' is 93
constexpr uint32_t QUAL_BASE = 33, QUAL_TOP = 126;
constexpr uint64_t NO_OFFSET = ~0ull;

struct Thresholds {
    uint64_t min_length = 0, max_length = 0, min_mean_q100 = 0;
};

// what the next byte of the stream is, from the phase of its line and whether it is the line's first byte
enum Byte : uint8_t {
    BYTE_NAME,       // of a name or separator line: not looked at
    BYTE_SKIP,       // '\r' of a sequence or quality line
    BYTE_BASE,       // one base
    BYTE_QUAL,       // one quality character
    BYTE_END_LINE,   // the '\n' of a line of phase 0-2
    BYTE_CLOSE,      // the '\n' of a quality line: it closes the record
    BYTE_BAD         // refused at this byte
};

CORAL_FASTQ_HD bool is_newline(uint8_t c) { return c == '\n'; }
CORAL_FASTQ_HD uint32_t phase_of(uint64_t line) { return (uint32_t)(line & 3); }
CORAL_FASTQ_HD bool quality_ok(uint8_t c) { return c >= QUAL_BASE && c <= QUAL_TOP; }

CORAL_FASTQ_HD Byte classify(uint32_t phase, bool first, uint8_t c) {
    if (first && ((phase == 0 && c != '@') || (phase == 2 && c != '+'))) return BYTE_BAD;
    if (c == '\n') return phase == 3 ? BYTE_CLOSE : BYTE_END_LINE;
    if (phase == 0 || phase == 2) return BYTE_NAME;
    if (c == '\r') return BYTE_SKIP;
    if (phase == 1) return BYTE_BASE;
    return quality_ok(c) ? BYTE_QUAL : BYTE_BAD;
}

// of a record at the byte that closes it
CORAL_FASTQ_HD bool record_ok(uint64_t length, uint64_t qual_count) { return qual_count == length && length <= MAX_LENGTH; }

// where the stream ends: `lines` '\n' bytes were read, `first`: the last one was the last byte (or the stream is empty)
enum End : uint8_t { END_BOUNDARY, END_CLOSES, END_BAD };
CORAL_FASTQ_HD End end_of_stream(uint64_t lines, bool first) {
    const uint32_t phase = phase_of(lines);
    return phase == 3 ? END_CLOSES : phase == 0 && first ? END_BOUNDARY : END_BAD;
}

CORAL_FASTQ_HD bool thresholds_ok(int64_t min_length, int64_t max_length, int64_t min_mean_q100) {
    return min_length >= 0 && min_length <= (int64_t)MAX_LENGTH && max_length >= 0 && max_length <= (int64_t)MAX_LENGTH && (max_length == 0 || max_length >= min_length) &&
           min_mean_q100 >= 0 && min_mean_q100 <= MAX_MEAN_Q100;
}

CORAL_FASTQ_HD bool keeps(const Thresholds &t, uint64_t length, uint64_t qual_sum) {
    return length >= t.min_length && (t.max_length == 0 || length <= t.max_length) && 100 * qual_sum >= t.min_mean_q100 * length;
}

// the piece-local row of a byte: `phase0` is the phase of the line the piece starts in, `line` the '\n' bytes of the piece in
// front of the byte.  Row 0 is the record that is open where the piece starts (or the first one that starts in it).
CORAL_FASTQ_HD uint32_t row_of(uint32_t phase0, uint32_t line) { return (phase0 + line) >> 2; }

// the flags of a scan that gives every byte of a piece its line
struct NewlineOp {
    CORAL_FASTQ_HD uint32_t operator()(const uint8_t &c) const { return is_newline(c); }
};

}  // namespace coral_fastq
#endif /* CORAL_FASTQ_CORE_H */
