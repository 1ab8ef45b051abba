// coral_comp_core.h - the rule of the reference's per-bin composition (`composition`), written once: small inline functions that the
// host backend (coral_comp_host.h, coral_comp.cpp) and the kernels (coral_comp.hip) both call, so that both give the same tables.
// It stands in for the GC and repeat-mask columns of the reference table that the reference's scripts/call_cnvs.sh:12-17 hands to
// `cnvkit.py batch --reference hg38full_ref_5k.cnn`; DESIGN.md §4 states the rule in words.
//
//   - lines are coral_fasta_core.h's; a header line starts a contig; '\n' and '\r' are skipped wherever they stand.
//   - every other byte of a line that is no header is one position of the current contig (`samtools faidx` coordinates: N,
//     IUPAC codes, '*' and '-' are positions too).
//   - a position is gc (GCgc), at (ATat) or neither (uncalled), and masked when its byte is a..z.
//   - contig c of length len[c] has ceil(len[c] / bin_size) bins, the last one short; bins follow in file order; three uint32
//     counters a bin: gc, at, masked.  1 <= bin_size <= 2^31 - 1, so no counter wraps; at most 2^28 bins.
// No HIP in this header beyond the host / device markers.
#ifndef CORAL_COMP_CORE_H
#define CORAL_COMP_CORE_H

#include <stdint.h>

#include "coral_fasta_core.h"

namespace coral_comp {

using namespace coral_fasta;

constexpr int64_t MAX_BIN_SIZE = 0x7fffffff;
constexpr int64_t MAX_BINS = (int64_t)1 << 28;
constexpr uint32_t CLS_GC = 1, CLS_AT = 2, CLS_MASKED = 4;
enum Kind : uint8_t { KIND_OPEN, KIND_HEADER, KIND_SKIP, KIND_POSITION };      // a header's '>', the rest of its line, '\n' / '\r', a position

CORAL_FASTA_HD bool bin_size_ok(int64_t bin_size) { return bin_size >= 1 && bin_size <= MAX_BIN_SIZE; }
CORAL_FASTA_HD bool is_position(uint8_t c) { return kept(c); }                    // of a byte outside a header line

// the classes of a position's byte
CORAL_FASTA_HD uint32_t classes(uint8_t c) {
    const uint32_t masked = c >= 'a' && c <= 'z' ? CLS_MASKED : 0;
    switch (c | 0x20) {                                // (only a letter's two cases map onto it)
        case 'g': case 'c': return CLS_GC | masked;
        case 'a': case 't': return CLS_AT | masked;
        default: return masked;
    }
}

// the next byte of the stream -> what it is
CORAL_FASTA_HD Kind next_kind(LineState &s, uint8_t c) {
    const Line l = line_step(s, c);
    return l == LINE_OPEN ? KIND_OPEN : l == LINE_HEADER ? KIND_HEADER : is_position(c) ? KIND_POSITION : KIND_SKIP;
}

CORAL_FASTA_HD uint64_t bins_of(uint64_t length, uint64_t bin_size) { return (length + bin_size - 1) / bin_size; }

// a byte that ends a contig's name inside its header line
CORAL_FASTA_HD bool ends_name(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

}  // namespace coral_comp
#endif /* CORAL_COMP_CORE_H */
