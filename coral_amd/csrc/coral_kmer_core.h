// coral_kmer_core.h - the k-mer counter's rule, written once: small inline functions that the host backend (coral_kmer_host.h,
// coral_kmer.cpp) and the kernels (coral_kmer.hip) both call, so that `kmers` gives the same table on either.  It stands in for
// lines 29-30 of the reference's scripts/align_nanopore_reads.sh (`meryl count k=15`, `meryl print greater-than distinct=0.9998`);
// DESIGN.md §4 states the rule in words and says what is not pinned against meryl.
//
//   - lines are coral_fasta_core.h's.  A header line's '>' is one break, the rest of it up to and including its '\n' is skipped.
//   - '\n' and '\r' are skipped wherever they stand; A C G T a c g t are the bases 0..3; every other byte is a break.
//   - a k-mer is a window of k consecutive bases without a break, 1 <= k <= 16, as a 2k-bit integer, first base in the top bits;
//     canonical: the smaller of the window and its reverse complement.
//   - counts are uint32 in one table of 4^k entries, index = the k-mer; fewer than 2^32 bases in all, so no counter wraps.
// No HIP in this header beyond the host / device markers.
#ifndef CORAL_KMER_CORE_H
#define CORAL_KMER_CORE_H

#include <stdint.h>

#include "coral_fasta_core.h"

namespace coral_kmer {

using namespace coral_fasta;

constexpr int MAX_K = 16;
constexpr uint64_t MAX_BASES = (uint64_t)1 << 32;      // a stream with this many bases or more is refused
constexpr uint32_t HIST_DIRECT = 65536;                // counts below it have a histogram bin of their own; the others are listed
constexpr uint8_t SYM_BREAK = 4, SYM_SKIP = 5;         // beside the bases 0..3

CORAL_FASTA_HD bool k_ok(int k) { return k >= 1 && k <= MAX_K; }
CORAL_FASTA_HD uint64_t table_entries(int k) { return (uint64_t)1 << (2 * k); }

// a byte of a sequence line (or a header's '>') -> base, break or skip
CORAL_FASTA_HD uint8_t classify(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        case '\n': case '\r': return SYM_SKIP;
        default: return SYM_BREAK;
    }
}

// the next byte of the stream -> its symbol; *header is set when the byte opens a header line
CORAL_FASTA_HD uint8_t next_symbol(LineState &s, uint8_t c, bool *header) {
    const Line l = line_step(s, c);
    *header = l == LINE_OPEN;
    return l == LINE_OPEN ? SYM_BREAK : l == LINE_HEADER ? SYM_SKIP : classify(c);
}

// the rolling window: the last min(run, k) bases, forward and as the reverse complement
struct Roll {
    uint64_t fwd = 0, rev = 0;
    uint32_t run = 0;                // bases since the last break, capped at k
};

// pushes a kept symbol (a base or a break); true when a window of k bases is complete
CORAL_FASTA_HD bool roll_push(Roll &r, uint8_t sym, int k) {
    if (sym > 3) { r.run = 0; r.fwd = 0; r.rev = 0; return false; }
    const uint64_t mask = table_entries(k) - 1;
    r.fwd = ((r.fwd << 2) | sym) & mask;
    r.rev = (r.rev >> 2) | ((uint64_t)(3 - sym) << (2 * (k - 1)));
    if (r.run < (uint32_t)k) ++r.run;
    return r.run == (uint32_t)k;
}

CORAL_FASTA_HD uint64_t roll_index(const Roll &r, bool canonical) { return canonical && r.rev < r.fwd ? r.rev : r.fwd; }

CORAL_FASTA_HD uint64_t reverse_complement(uint64_t kmer, int k) {
    uint64_t out = 0;
    for (int i = 0; i < k; ++i) { out = (out << 2) | (3 - (kmer & 3)); kmer >>= 2; }
    return out;
}

}  // namespace coral_kmer
#endif /* CORAL_KMER_CORE_H */
