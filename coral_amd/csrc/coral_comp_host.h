// coral_comp_host.h - the host backend of the reference's per-bin composition: a straight loop over coral_comp_core.h with a small
// state carried between feeds, and the same tables as the device.  It is what the kernels (coral_comp.hip) are compared against
// and `device="cpu"` of coral_amd/composition.py.  scan_piece is the host's share of the device path: it takes the contigs'
// names from the header lines of a piece, which coral_fasta_host.h finds, and says what to blank.  It stands in for the GC and repeat-mask columns of the reference table of
// the reference's scripts/call_cnvs.sh:12-17.  No HIP: g++ alone builds it (tests/native/comp_host.cpp).
#ifndef CORAL_COMP_HOST_H
#define CORAL_COMP_HOST_H

#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "coral_comp_core.h"
#include "coral_fasta_host.h"

namespace coral_comp {

enum { COMP_OK = 0, COMP_FORMAT_BEFORE_HEADER = 1, COMP_FORMAT_EMPTY_NAME = 2 };

inline const char *format_text(int e) {
    return e == COMP_FORMAT_BEFORE_HEADER ? "a sequence byte stands in front of the first header line" : "a header line without a name";
}

struct Stats {
    uint64_t n_contigs = 0, positions = 0, bins = 0, gc = 0, at = 0, masked = 0;
};

// The contigs' names: the bytes behind a header's '>' up to the first blank, tab, '\r' or '\n'.
struct Names {
    std::string blob;
    std::vector<int64_t> off{0};
    bool taking = false, in_line = false;              // the name is still growing; a header line is open
    void open() { taking = true; in_line = true; }
    // bytes of the open header line behind its '>' (without the line's '\n'); false: the name ended empty
    bool bytes(const uint8_t *p, size_t n) {
        if (!taking) return true;
        size_t m = 0;
        while (m < n && !ends_name(p[m])) ++m;
        blob.append((const char *)p, m);
        if (m < n) return end_name();
        return true;
    }
    bool end_name() {
        if (!taking) return true;
        taking = false;
        const bool filled = (int64_t)blob.size() > off.back();
        off.push_back((int64_t)blob.size());
        return filled;
    }
    // the header line's '\n', or the end of the stream inside it
    bool close_line() { in_line = false; return end_name(); }
};

// One pass, one thread.  The three tables hold `capacity` zeroed counters each, the caller's; bins behind the capacity are counted
// (st.bins) and not written.
struct HostComposer {
    uint64_t bin_size, capacity;
    uint32_t *gc, *at, *masked;
    LineState line;
    Names names;
    std::vector<int64_t> lengths;
    Stats st;
    bool started = false;
    int error = COMP_OK;
    uint64_t cur_len = 0, bin = 0, left = 0;           // of the open contig: its positions, the bin of the next one, that bin's room

    HostComposer(int64_t bin_size_, uint32_t *gc_, uint32_t *at_, uint32_t *masked_, int64_t capacity_)
        : bin_size((uint64_t)bin_size_), capacity((uint64_t)capacity_), gc(gc_), at(at_), masked(masked_) {}

    void close_contig() {
        if (!started) return;
        lengths.push_back((int64_t)cur_len);
        st.bins += bins_of(cur_len, bin_size);
    }

    int feed(const uint8_t *bytes, size_t n) {
        for (size_t i = 0; i < n && error == COMP_OK; ++i) {
            const uint8_t c = bytes[i];
            switch (next_kind(line, c)) {
                case KIND_OPEN:
                    close_contig();
                    started = true;
                    cur_len = 0; bin = st.bins; left = bin_size;
                    names.open();
                    break;
                case KIND_HEADER:
                    if (c == '\n') { if (!names.close_line()) error = COMP_FORMAT_EMPTY_NAME; }
                    else if (!names.bytes(&c, 1)) error = COMP_FORMAT_EMPTY_NAME;
                    break;
                case KIND_SKIP: break;
                case KIND_POSITION: {
                    if (!started) { error = COMP_FORMAT_BEFORE_HEADER; break; }
                    if (left == 0) { ++bin; left = bin_size; }
                    const uint32_t cls = classes(c);
                    if (bin < capacity) { gc[bin] += cls & CLS_GC ? 1 : 0; at[bin] += cls & CLS_AT ? 1 : 0; masked[bin] += cls & CLS_MASKED ? 1 : 0; }
                    st.gc += cls & CLS_GC ? 1 : 0; st.at += cls & CLS_AT ? 1 : 0; st.masked += cls & CLS_MASKED ? 1 : 0;
                    --left; ++cur_len; ++st.positions;
                    break;
                }
            }
        }
        return error;
    }

    // the end of the stream: the open contig and an open header line are closed
    int finish() {
        if (error != COMP_OK) return error;
        if (names.in_line && !names.close_line()) return error = COMP_FORMAT_EMPTY_NAME;
        close_contig();
        started = false;
        st.n_contigs = lengths.size();
        return COMP_OK;
    }
};

// The header lines of the next piece of the stream, found before the piece is copied: `bounds` gets the byte offset of
// every header line that opens in the piece (its '>'), `blanks` the ranges [a, b) of header bytes ('>' included, the line's '\n'
// not) for the caller to overwrite with '\n', `names` the contigs' names.  At most max_bounds headers are taken: the piece ends in
// front of the next one.  `s` and `started` (a header line has been seen) are the state in front of the piece and become the
// state behind what was taken.  Returns the bytes taken (> 0 for n > 0); *error is a COMP_FORMAT_* when the text is refused.
inline size_t scan_piece(LineState &s, Names &names, bool &started, const uint8_t *src, size_t n, size_t max_bounds, std::vector<uint32_t> &bounds,
                         std::vector<std::pair<uint32_t, uint32_t>> &blanks, int *error) {
    bounds.clear();
    blanks.clear();
    *error = COMP_OK;
    if (!started) {                                      // only '\n' and '\r' may stand in front of the first header line (none is open yet)
        size_t i = 0;
        while (i < n && !is_position(src[i])) ++i;
        if (i < n && (src[i] != '>' || !(i == 0 ? s.line_start != 0 : src[i - 1] == '\n'))) { *error = COMP_FORMAT_BEFORE_HEADER; return n; }
    }
    size_t pos = 0;
    for (HeaderLine h; next_header_line(s, src, n, pos, h);) {
        if (!h.carried) {
            if (bounds.size() == max_bounds) { s.in_header = 0; s.line_start = 1; return h.begin; }      // the piece ends in front of this line
            bounds.push_back((uint32_t)h.begin);
            started = true;
            names.open();
        }
        if (h.end > h.begin) blanks.emplace_back((uint32_t)h.begin, (uint32_t)h.end);
        if (!names.bytes(src + h.body, h.end - h.body) || (h.closed && !names.close_line())) { *error = COMP_FORMAT_EMPTY_NAME; return n; }
    }
    return n;
}

}  // namespace coral_comp
#endif /* CORAL_COMP_HOST_H */
