// coral_kmer_host.h - the k-mer counter's host backend: a straight loop over coral_kmer_core.h with a small state carried between
// feeds, and the same table layout as the device.  It is what the kernels (coral_kmer.hip) are compared against and `device="cpu"`
// of coral_amd/kmers.py.  mask_headers is the host's share of the device path: it blanks the header lines of a piece, which
// coral_fasta_host.h finds.  No HIP: g++ alone builds it (tests/native/kmer_host.cpp).
#ifndef CORAL_KMER_HOST_H
#define CORAL_KMER_HOST_H

#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "coral_fasta_host.h"
#include "coral_kmer_core.h"

namespace coral_kmer {

struct Stats {
    uint64_t n_sequences = 0, n_bases = 0, total = 0, distinct = 0, max_count = 0;
};

// One pass, one thread.  `table`: 4^k zeroed (or earlier) counters, the caller's.
struct HostCounter {
    int k;
    bool canonical;
    uint32_t *table;
    LineState line;
    Roll roll;
    Stats st;
    HostCounter(int k_, bool canonical_, uint32_t *table_, uint64_t bases_before) : k(k_), canonical(canonical_), table(table_) { st.n_bases = bases_before; }

    // false: the stream reached 2^32 bases (nothing more is counted)
    bool feed(const uint8_t *bytes, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            bool header;
            const uint8_t sym = next_symbol(line, bytes[i], &header);
            st.n_sequences += header;
            if (sym == SYM_SKIP) continue;
            if (sym < 4 && ++st.n_bases >= MAX_BASES) return false;
            if (roll_push(roll, sym, k)) { ++table[roll_index(roll, canonical)]; ++st.total; }
        }
        return true;
    }
};

// The header lines of a piece, for a consumer that classifies byte by byte (coral_kmer_core.h's classify): every byte of a header
// line behind its '>' becomes '\n' in place, so that the '>' is the one break and the rest is skipped.  `s` is the state in front
// of the piece and becomes the one behind it; returns the number of header lines that open in the piece.
inline uint64_t mask_headers(LineState &s, uint8_t *buf, size_t n) {
    uint64_t opened = 0;
    size_t pos = 0;
    for (HeaderLine h; next_header_line(s, buf, n, pos, h);) {
        opened += !h.carried;
        memset(buf + h.body, '\n', h.end - h.body);
    }
    return opened;
}

// four entries at once (4^k is a multiple of four)
inline bool four_zeros(const uint32_t *p) {
    uint64_t a, b;
    memcpy(&a, p, 8);
    memcpy(&b, p + 2, 8);
    return (a | b) == 0;
}

// distinct, the largest count and the exact histogram (count value -> k-mers with it) of a table
inline void table_histogram(const uint32_t *table, int k, Stats &st, std::map<uint64_t, uint64_t> &hist) {
    const uint64_t n = table_entries(k);
    std::vector<uint64_t> direct(HIST_DIRECT, 0);
    hist.clear();
    st.distinct = 0;
    st.max_count = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if ((i & 3) == 0 && four_zeros(table + i)) { i += 3; continue; }      // (most of a large table is empty)
        const uint32_t c = table[i];
        if (!c) continue;
        ++st.distinct;
        if (c > st.max_count) st.max_count = c;
        if (c < HIST_DIRECT) ++direct[c]; else ++hist[c];
    }
    for (uint32_t c = 1; c < HIST_DIRECT; ++c) if (direct[c]) hist[c] = direct[c];
}

// the entries with a count above `greater_than`, in table order; returns how many there are (the first `capacity` are written)
inline uint64_t table_select(const uint32_t *table, int k, uint64_t greater_than, uint64_t capacity, uint64_t *kmers, uint32_t *counts) {
    const uint64_t n = table_entries(k);
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if ((i & 3) == 0 && four_zeros(table + i)) { i += 3; continue; }
        if (table[i] <= greater_than) continue;
        if (m < capacity) { kmers[m] = i; counts[m] = table[i]; }
        ++m;
    }
    return m;
}

}  // namespace coral_kmer
#endif /* CORAL_KMER_HOST_H */
