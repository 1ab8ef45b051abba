// coral_sketch_core.h - the minimizer sketch's rule, written once: small inline functions that the host backend
// (coral_sketch_host.h, coral_sketch.cpp) and the kernels (coral_sketch.hip) both call, so that `sketch` gives the same seed index
// on either.  It is the first stage of the mapper of the reference's scripts/align_nanopore_reads.sh, line 34 (`winnowmap -W
// repetitive_k15.txt -ax map-ont`); DESIGN.md §4 states the rule in words and says what is not pinned against winnowmap.
//
//   - lines are coral_fasta_core.h's; a header line ends a contig and opens the next; '\n' and '\r' are skipped wherever they stand.
//   - every other byte of a sequence line is one position of its contig: A C G T a c g t are the bases 0..3, anything else (N, an
//     IUPAC code) is a non-base that stays in its place.
//   - the k-mer at position p is the k bases from p on, 1 <= k <= 16; fwd / rev as coral_kmer::Roll.  It is invalid when it holds a
//     non-base or when fwd == rev.  Else strand = rev < fwd, canon = min(fwd, rev) and
//     key = hash64(canon, 4^k - 1) | repetitive(canon) << 2k: a repetitive k-mer loses to every other one.
//   - a contig with n >= 1 k-mer positions has the windows of ww = min(w, n) consecutive positions inside it, 1 <= w <= 256.  An
//     invalid k-mer has the key +infinity and keeps its place.  Position p is a minimizer iff its k-mer is valid and its key is
//     the minimum of at least one window that holds p; all tied minima count.  With M[j] the minimum of window j that is: key[p]
//     == max(M[j] for the windows j that hold p).
//   - output: key, and value = contig << 32 | pos << 1 | strand, in (contig, pos) order; then sorted by key, stably.
// No HIP in this header beyond the host / device markers.
#ifndef CORAL_SKETCH_CORE_H
#define CORAL_SKETCH_CORE_H

#include <stdint.h>

#include "coral_kmer_core.h"

namespace coral_sketch {

using namespace coral_kmer;

constexpr int MAX_W = 256;
constexpr uint8_t SYM_CONTIG = 6;                      // beside the bases 0..3 and SYM_BREAK (a non-base in its place)
constexpr uint64_t KEY_INVALID = ~(uint64_t)0;         // +infinity
constexpr int64_t MAX_CONTIG_POSITIONS = (int64_t)1 << 31;
constexpr int64_t MAX_CONTIGS = (int64_t)1 << 32;

CORAL_FASTA_HD bool w_ok(int w) { return w >= 1 && w <= MAX_W; }
CORAL_FASTA_HD uint64_t kmer_mask(int k) { return table_entries(k) - 1; }
CORAL_FASTA_HD uint64_t bitmap_words(int k) { return (table_entries(k) + 31) / 32; }      // uint32 words of the weights' bitmap

// the usual invertible integer hash, every step taken & mask: a permutation of 0 .. mask
CORAL_FASTA_HD uint64_t hash64(uint64_t x, uint64_t mask) {
    x = (~x + (x << 21)) & mask;
    x = x ^ x >> 24;
    x = (x + (x << 3) + (x << 8)) & mask;
    x = x ^ x >> 14;
    x = (x + (x << 2) + (x << 4)) & mask;
    x = x ^ x >> 28;
    x = (x + (x << 31)) & mask;
    return x;
}

CORAL_FASTA_HD bool repetitive(const uint32_t *bitmap, uint64_t canon) { return bitmap && (bitmap[canon >> 5] >> (canon & 31) & 1u); }

// a byte of a piece whose header lines are blanked but for their '>' and that holds no other '>' -> its symbol
CORAL_FASTA_HD uint8_t dense_symbol(uint8_t c) { return c == '>' ? SYM_CONTIG : classify(c); }

// the key of a complete window (r.run == k) and its strand; KEY_INVALID for a k-mer that is its own reverse complement
CORAL_FASTA_HD uint64_t kmer_key(const Roll &r, int k, const uint32_t *bitmap, uint32_t *strand) {
    if (r.fwd == r.rev) { *strand = 0; return KEY_INVALID; }
    *strand = r.rev < r.fwd;
    const uint64_t canon = *strand ? r.rev : r.fwd;
    return hash64(canon, kmer_mask(k)) | (uint64_t)repetitive(bitmap, canon) << (2 * k);
}

CORAL_FASTA_HD uint64_t pack_value(uint64_t contig, uint64_t pos, uint32_t strand) { return contig << 32 | pos << 1 | strand; }

// The windows of a contig whose k-mer positions are a .. b (n = b - a + 1 >= 1).
struct Windows {
    int64_t a, b;
    int ww;
    CORAL_FASTA_HD Windows(int64_t a_, int64_t b_, int w) : a(a_), b(b_), ww(b_ - a_ + 1 < w ? (int)(b_ - a_ + 1) : w) {}
    CORAL_FASTA_HD bool is_start(int64_t j) const { return j >= a && j + ww - 1 <= b; }      // window j lies inside the contig
    CORAL_FASTA_HD int64_t first_of(int64_t p) const { return p - ww + 1 > a ? p - ww + 1 : a; }      // the windows that hold p
    CORAL_FASTA_HD int64_t last_of(int64_t p) const { return p < b - ww + 1 ? p : b - ww + 1; }
};

// the first sliding pass: the minimum of window j (`key`: position -> key)
template <class Key> CORAL_FASTA_HD uint64_t window_min(const Key &key, int64_t j, int ww) {
    uint64_t m = KEY_INVALID;
    for (int i = 0; i < ww; ++i) { const uint64_t v = key(j + i); m = v < m ? v : m; }
    return m;
}

// the second: is the valid key `mine` of position p the largest minimum of the windows that hold p (`wmin`: window -> minimum)
template <class Min> CORAL_FASTA_HD bool is_minimizer(const Min &wmin, const Windows &W, int64_t p, uint64_t mine) {
    uint64_t m = 0;
    for (int64_t j = W.first_of(p); j <= W.last_of(p); ++j) { const uint64_t v = wmin(j); m = v > m ? v : m; }
    return m == mine;
}

}  // namespace coral_sketch
#endif /* CORAL_SKETCH_CORE_H */
