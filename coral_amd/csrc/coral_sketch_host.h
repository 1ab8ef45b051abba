// coral_sketch_host.h - the minimizer sketch's host backend: a straight loop over coral_sketch_core.h with the open contig's keys
// carried between feeds, and the same two output arrays as the device.  It is what the kernels (coral_sketch.hip) are compared
// against and `device="cpu"` of coral_amd/minimizers.py; one thread, O(n w).  The sorted index, its lookup and the expansion into
// anchors have their host forms here too.  mark_contigs is the host's share of the device path.  Names and the refusals of a text
// are the composition session's (coral_comp_host.h).  No HIP: g++ alone builds it.
#ifndef CORAL_SKETCH_HOST_H
#define CORAL_SKETCH_HOST_H

#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "coral_comp_host.h"
#include "coral_sketch_core.h"

namespace coral_sketch {

using coral_comp::Names;
enum { SKETCH_OK = 0, SKETCH_FORMAT_BEFORE_HEADER = coral_comp::COMP_FORMAT_BEFORE_HEADER, SKETCH_FORMAT_EMPTY_NAME = coral_comp::COMP_FORMAT_EMPTY_NAME, SKETCH_TOO_LONG = 3 };

inline const char *refusal_text(int e) {
    return e == SKETCH_TOO_LONG ? "a contig of 2^31 positions or more, or 2^32 contigs or more" : coral_comp::format_text(e);
}

// true when the contigs fit the value's fields
inline bool contigs_fit(const std::vector<int64_t> &lengths) {
    if ((int64_t)lengths.size() >= MAX_CONTIGS) return false;
    for (int64_t l : lengths) if (l >= MAX_CONTIG_POSITIONS) return false;
    return true;
}

// One pass, one thread.  `out_key` / `out_value` hold `capacity` entries, the caller's; minimizers behind the capacity are counted
// (n_out) and not written.
struct HostSketcher {
    static constexpr size_t BLOCK = 1 << 16;           // undecided k-mer positions kept before a prefix of them is decided
    int k, w;
    const uint32_t *bitmap;
    uint64_t *out_key, *out_value, capacity, n_out = 0, positions = 0;
    LineState line;
    Names names;
    std::vector<int64_t> lengths;
    bool started = false;
    int error = SKETCH_OK;
    Roll roll;
    uint64_t cur_len = 0;                              // of the open contig: its positions so far,
    int64_t base = 0, decided = 0;                     // the k-mer position of keys[0], the first undecided one,
    std::vector<uint64_t> keys, mins;                  // the keys from `base` on
    std::vector<uint8_t> strands;

    HostSketcher(int k_, int w_, const uint32_t *bitmap_, uint64_t *out_key_, uint64_t *out_value_, int64_t capacity_)
        : k(k_), w(w_), bitmap(bitmap_), out_key(out_key_), out_value(out_value_), capacity((uint64_t)capacity_) {}

    // the positions that can be decided: all of a closed contig, else those with w - 1 k-mer positions to their right
    void decide(bool closed) {
        const int64_t n = base + (int64_t)keys.size();
        const int64_t limit = closed ? n : n - (w - 1);
        if (limit > decided) {
            const Windows W(0, n - 1, w);
            const auto key = [&](int64_t p) { return keys[(size_t)(p - base)]; };
            const int64_t j0 = W.first_of(decided), j1 = W.last_of(limit - 1);
            mins.resize((size_t)(j1 - j0 + 1));
            for (int64_t j = j0; j <= j1; ++j) mins[(size_t)(j - j0)] = window_min(key, j, W.ww);
            const auto wmin = [&](int64_t j) { return mins[(size_t)(j - j0)]; };
            for (int64_t p = decided; p < limit; ++p) {
                const uint64_t mine = key(p);
                if (mine == KEY_INVALID || !is_minimizer(wmin, W, p, mine)) continue;
                if (n_out < capacity) { out_key[n_out] = mine; out_value[n_out] = pack_value(lengths.size(), (uint64_t)p, strands[(size_t)(p - base)]); }
                ++n_out;
            }
            decided = limit;
        }
        const int64_t keep_from = std::max(base, decided - (w - 1));
        keys.erase(keys.begin(), keys.begin() + (keep_from - base));
        strands.erase(strands.begin(), strands.begin() + (keep_from - base));
        base = keep_from;
    }

    void close_contig() {
        if (!started) return;
        decide(true);
        if ((int64_t)cur_len >= MAX_CONTIG_POSITIONS || (int64_t)lengths.size() + 1 >= MAX_CONTIGS) error = SKETCH_TOO_LONG;
        lengths.push_back((int64_t)cur_len);
        keys.clear(); strands.clear();
        base = 0; decided = 0; cur_len = 0;
        roll = Roll();
    }

    int feed(const uint8_t *bytes, size_t n) {
        for (size_t i = 0; i < n && error == SKETCH_OK; ++i) {
            const uint8_t c = bytes[i];
            switch (coral_comp::next_kind(line, c)) {
                case coral_comp::KIND_OPEN:
                    close_contig();
                    started = true;
                    names.open();
                    break;
                case coral_comp::KIND_HEADER:
                    if (c == '\n') { if (!names.close_line()) error = SKETCH_FORMAT_EMPTY_NAME; }
                    else if (!names.bytes(&c, 1)) error = SKETCH_FORMAT_EMPTY_NAME;
                    break;
                case coral_comp::KIND_SKIP: break;
                case coral_comp::KIND_POSITION: {
                    if (!started) { error = SKETCH_FORMAT_BEFORE_HEADER; break; }
                    const bool complete = roll_push(roll, classify(c), k);
                    ++cur_len; ++positions;
                    if (cur_len < (uint64_t)k) break;
                    uint32_t strand = 0;
                    keys.push_back(complete ? kmer_key(roll, k, bitmap, &strand) : KEY_INVALID);
                    strands.push_back((uint8_t)strand);
                    if (keys.size() >= BLOCK + 2 * (size_t)w) decide(false);
                    break;
                }
            }
        }
        return error;
    }

    // the end of the stream: the open contig and an open header line are closed
    int finish() {
        if (error != SKETCH_OK) return error;
        if (names.in_line && !names.close_line()) return error = SKETCH_FORMAT_EMPTY_NAME;
        close_contig();
        started = false;
        return error;
    }
};

// The host's share of the device path, on a piece in its staging buffer whose header lines coral_comp::scan_piece has found and
// blanked: every other '>' of the piece is a non-base like any ('N' stands for it), and the header lines get their '>' back, so
// that dense_symbol finds the contig boundaries.
inline void mark_contigs(uint8_t *text, size_t n, const std::vector<uint32_t> &bounds) {
    for (uint8_t *p = text; (p = (uint8_t *)memchr(p, '>', (size_t)(text + n - p))) != nullptr; ++p) *p = 'N';
    for (uint32_t b : bounds) text[b] = '>';
}

// ---- the index ---------------------------------------------------------------------------------------------------------------------
// stable by key: ties keep their (contig, pos) order
inline void sort_pairs(uint64_t *keys, uint64_t *values, size_t n) {
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return keys[x] < keys[y]; });
    std::vector<uint64_t> k2(n), v2(n);
    for (size_t i = 0; i < n; ++i) { k2[i] = keys[order[i]]; v2[i] = values[order[i]]; }
    if (n) { memcpy(keys, k2.data(), n * 8); memcpy(values, v2.data(), n * 8); }
}

// the entries of `key` in the sorted keys: the first one and how many (first = the insertion point when there is none)
CORAL_FASTA_HD void find_entries(const uint64_t *sorted, int64_t n, uint64_t key, int64_t *first, int64_t *count) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (sorted[mid] < key) lo = mid + 1; else hi = mid; }
    int64_t lo2 = lo, hi2 = n;
    while (lo2 < hi2) { const int64_t mid = lo2 + (hi2 - lo2) / 2; if (sorted[mid] <= key) lo2 = mid + 1; else hi2 = mid; }
    *first = lo; *count = lo2 - lo;
}

// an anchor's two words: query << 32 | qpos, and the index entry's value with the strands combined
CORAL_FASTA_HD uint64_t anchor_query(uint64_t query, uint64_t qpos) { return query << 32 | qpos; }
CORAL_FASTA_HD uint64_t anchor_ref(uint64_t value, uint32_t qstrand) { return value ^ (uint64_t)(qstrand & 1u); }

// every query minimizer whose key has at most max_occ entries gives one anchor per entry: query order, then index order; returns
// how many there are (the first `capacity` are written)
inline int64_t expand_anchors(const uint64_t *sorted, const uint64_t *values, int64_t n, const uint32_t *query, const uint32_t *qpos, const uint8_t *qstrand, const uint64_t *qkey,
                              int64_t nq, int64_t max_occ, int64_t capacity, uint64_t *a_query, uint64_t *a_ref) {
    int64_t m = 0;
    for (int64_t i = 0; i < nq; ++i) {
        int64_t first, count;
        find_entries(sorted, n, qkey[i], &first, &count);
        if (count > max_occ) continue;
        for (int64_t e = first; e < first + count; ++e, ++m)
            if (m < capacity) { a_query[m] = anchor_query(query[i], qpos[i]); a_ref[m] = anchor_ref(values[e], qstrand[i]); }
    }
    return m;
}

}  // namespace coral_sketch
#endif /* CORAL_SKETCH_HOST_H */
