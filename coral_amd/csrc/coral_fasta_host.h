// coral_fasta_host.h - the host's share of every device path that streams FASTA text in pieces: the header lines of a piece, found
// with memchr instead of byte by byte (coral_fasta_core.h's line_step is the rule; tests/native/kmer_host.cpp and comp_host.cpp
// hold its two callers, mask_headers and scan_piece, against that rule).  Headers are few, so this costs little beside the copy
// into a staging buffer.  No HIP: g++ alone builds it.
#ifndef CORAL_FASTA_HOST_H
#define CORAL_FASTA_HOST_H

#include <stddef.h>
#include <string.h>

#include "coral_fasta_core.h"

namespace coral_fasta {

// One header line as far as it lies in a piece of n bytes.
struct HeaderLine {
    bool carried;                    // it was open in front of the piece: its '>' is not here
    bool closed;                     // its '\n' is here (else it runs off the piece)
    size_t begin, body, end;         // its first byte in the piece (its '>', or 0 when carried); the first behind the '>'; its '\n', or n
};

// The next header line of the piece src[0, n) at or behind `pos` (0 at first) -> `h`, and `pos` moves behind it.  `s` is the state
// in front of the piece; it follows the walk and is the state behind the piece when false comes back (no further header line).
inline bool next_header_line(LineState &s, const uint8_t *src, size_t n, size_t &pos, HeaderLine &h) {
    if (n == 0) return false;
    h.carried = pos == 0 && s.in_header;
    if (!h.carried) {
        if (s.in_header) return false;                           // (the line before ran off the piece)
        const uint8_t *p = nullptr;
        while (pos < n && (p = (const uint8_t *)memchr(src + pos, '>', n - pos)) != nullptr) {
            pos = (size_t)(p - src) + 1;
            if (p == src ? s.line_start != 0 : p[-1] == '\n') break;
            p = nullptr;
        }
        if (!p) { s.line_start = src[n - 1] == '\n'; pos = n; return false; }
    }
    h.body = pos;
    h.begin = h.carried ? 0 : pos - 1;
    const uint8_t *q = (const uint8_t *)memchr(src + pos, '\n', n - pos);
    h.closed = q != nullptr;
    h.end = q ? (size_t)(q - src) : n;
    s.in_header = !h.closed;
    s.line_start = h.closed;
    pos = h.closed ? h.end + 1 : n;
    return true;
}

}  // namespace coral_fasta
#endif /* CORAL_FASTA_HOST_H */
