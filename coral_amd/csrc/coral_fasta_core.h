// coral_fasta_core.h - the lines of FASTA text, written once for every consumer of a reference genome (`kmers`: coral_kmer_core.h,
// `composition`: coral_comp_core.h), host and device alike; DESIGN.md §4 states the rule in words.
//
//   - FASTA text is a stream of bytes.  A line starts at the stream's first byte and behind every '\n'.  A line whose first byte
//     is '>' is a header line; it runs up to and including its '\n'.
//   - '\n' and '\r' are skipped wherever they stand: every other byte of a line that is no header is kept.
// No HIP in this header beyond the host / device markers.
#ifndef CORAL_FASTA_CORE_H
#define CORAL_FASTA_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CORAL_FASTA_HD __host__ __device__ inline
#else
#define CORAL_FASTA_HD inline
#endif

namespace coral_fasta {

// where the stream stands between two bytes
struct LineState {
    uint8_t line_start = 1, in_header = 0;
};

enum Line : uint8_t { LINE_OPEN, LINE_HEADER, LINE_TEXT };      // a header's '>', the rest of its line ('\n' included), any other byte

// of a byte outside a header line
CORAL_FASTA_HD bool kept(uint8_t c) { return c != '\n' && c != '\r'; }

// the next byte of the stream -> where it stands
CORAL_FASTA_HD Line line_step(LineState &s, uint8_t c) {
    if (s.in_header) {
        if (c == '\n') { s.in_header = 0; s.line_start = 1; }
        return LINE_HEADER;
    }
    const bool first = s.line_start != 0;
    s.line_start = c == '\n';
    if (first && c == '>') { s.in_header = 1; return LINE_OPEN; }
    return LINE_TEXT;
}

// the keep flags of a piece whose header lines are blanked to '\n', for a scan that gives every kept byte its ordinal
struct KeepOp {
    CORAL_FASTA_HD uint32_t operator()(const uint8_t &c) const { return kept(c); }
};

}  // namespace coral_fasta
#endif /* CORAL_FASTA_CORE_H */
