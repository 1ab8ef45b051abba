// coral_sam_host.h - the host build of coral_sam_core.h (lanes as loops) and the header's part of `import`: what
// coral_sam_header / coral_sam_encode (coral_sam.cpp) and tests/native/sam_host.cpp are made of.  No HIP in here.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "coral_sam_core.h"

namespace coral_sam {

struct HostLanes {
    template <class F> uint64_t ballot(F f) {
        uint64_t m = 0;
        for (int l = 0; l < LANES; ++l) m |= (uint64_t)(f(l) ? 1 : 0) << l;
        return m;
    }
    template <class F> void each(F f) { for (int l = 0; l < LANES; ++l) f(l); }
    template <class F> uint64_t sum(F f) {
        uint64_t s = 0;
        for (int l = 0; l < LANES; ++l) s += f(l);
        return s;
    }
    bool leader() const { return true; }
    uint32_t uni(uint32_t x) const { return x; }
    void slow_float(const uint8_t *text, uint32_t n, uint8_t *dst) { store32(dst, strtof_bits(text, n)); }
    // strtof of exactly the n bytes at text (a copy: the text need not be terminated behind them)
    static uint32_t strtof_bits(const uint8_t *text, uint32_t n) {
        const std::string s((const char *)text, n);
        const float f = strtof(s.c_str(), nullptr);
        uint32_t b;
        memcpy(&b, &f, 4);
        return b;
    }
};

// What a SAM header's text says about the BAM file: the inflated header bytes (magic, l_text, the text verbatim, n_ref, per
// @SQ line l_name, the name with its NUL, l_ref) and the contig table of coral_sam_core.h.
struct Header {
    std::vector<uint8_t> bam, names;
    std::vector<int64_t> name_off{0};
    std::vector<uint32_t> slots;
    int64_t text_bytes = 0, n_lines = 0;             // the leading '@' lines: their bytes, their number
    Contigs contigs() const { return Contigs{names.data(), name_off.data(), slots.data(), (int32_t)(name_off.size() - 1), (uint32_t)slots.size()}; }
};

inline void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k)));
}

// The leading '@' lines of text[0, n) (a last one may lack its '\n').  false: an @SQ line without SN / LN, an LN that is no
// length, or a name given twice; err names the 1-based line.
inline bool parse_header(const uint8_t *text, int64_t n, Header &H, std::string &err) {
    std::vector<int64_t> lens;
    int64_t at = 0, line_no = 0;
    while (at < n && text[at] == '@') {
        const uint8_t *nl = (const uint8_t *)memchr(text + at, '\n', (size_t)(n - at));
        const int64_t end = nl ? nl - text : n;
        ++line_no;
        if (end - at >= 4 && memcmp(text + at, "@SQ\t", 4) == 0) {
            int64_t sn_b = -1, sn_e = -1, ln = -1;
            for (int64_t f = at + 4; f <= end;) {
                int64_t g = f;
                while (g < end && text[g] != '\t') ++g;
                if (g - f >= 3 && text[f + 2] == ':') {
                    if (text[f] == 'S' && text[f + 1] == 'N' && sn_b < 0) { sn_b = f + 3; sn_e = g; }
                    if (text[f] == 'L' && text[f + 1] == 'N' && ln < 0) {
                        int64_t x = 0;
                        bool good = g > f + 3;
                        for (int64_t k = f + 3; k < g && good; ++k) {
                            good = is_digit(text[k]) && x < (1ll << 40);
                            x = x * 10 + (text[k] - 48);
                        }
                        if (!good || x < 1 || x > 2147483647ll) { err = "line " + std::to_string(line_no) + ": @SQ with a bad LN"; return false; }
                        ln = x;
                    }
                }
                f = g + 1;
            }
            if (sn_b < 0 || sn_e == sn_b || ln < 0) { err = "line " + std::to_string(line_no) + ": @SQ without SN or LN"; return false; }
            H.names.insert(H.names.end(), text + sn_b, text + sn_e);
            H.name_off.push_back((int64_t)H.names.size());
            lens.push_back(ln);
        }
        at = nl ? end + 1 : end;
    }
    H.text_bytes = at;
    H.n_lines = line_no;
    const size_t n_ref = lens.size();
    size_t n_slots = 0;
    if (n_ref > 0) for (n_slots = 4; n_slots < 2 * n_ref; n_slots <<= 1) {}
    H.slots.assign(n_slots, 0u);
    if (H.names.empty()) H.names.push_back(0);        // (never a null pointer)
    for (size_t r = 0; r < n_ref; ++r) {
        const uint8_t *nm = H.names.data() + H.name_off[r];
        const uint32_t len = (uint32_t)(H.name_off[r + 1] - H.name_off[r]);
        if (find_contig(H.contigs(), nm, len) >= 0) { err = "@SQ: the name " + std::string((const char *)nm, len) + " is given twice"; return false; }
        uint32_t h = name_hash(nm, len) & (uint32_t)(n_slots - 1);
        while (H.slots[h]) h = (h + 1) & (uint32_t)(n_slots - 1);
        H.slots[h] = (uint32_t)r + 1;
    }
    H.bam.assign({'B', 'A', 'M', 1});
    put32(H.bam, (uint32_t)at);
    H.bam.insert(H.bam.end(), text, text + at);
    put32(H.bam, (uint32_t)n_ref);
    for (size_t r = 0; r < n_ref; ++r) {
        const uint32_t len = (uint32_t)(H.name_off[r + 1] - H.name_off[r]);
        put32(H.bam, len + 1);
        H.bam.insert(H.bam.end(), H.names.begin() + H.name_off[r], H.names.begin() + H.name_off[r + 1]);
        H.bam.push_back(0);
        put32(H.bam, (uint32_t)lens[r]);
    }
    return true;
}

struct EncodeCounts { int64_t lines = 0, written = 0, dropped = 0, out_bytes = 0, err_line = 0, err_field = 0; };

inline std::string refusal_text(int64_t line_no, uint32_t field) {
    return "SAM line " + std::to_string(line_no) + ": " + field_name(field) + (field >= F_QNAME ? " is malformed" : "");
}

// The whole lines of text[0, n) (the last one may lack its '\n'), the first being line `first_line` of the file, as records at
// out (out_cap bytes; out == nullptr: validated and counted only).  0: good, 1: refused (counts.err_line / err_field: the
// first bad line), 2: out is too short.
inline int encode_text(const uint8_t *text, int64_t n, int64_t first_line, const Contigs &C, const Keep &K, uint8_t *out, int64_t out_cap, EncodeCounts &X) {
    HostLanes w;
    for (int64_t at = 0; at < n;) {
        const uint8_t *nl = (const uint8_t *)memchr(text + at, '\n', (size_t)(n - at));
        const int64_t end = nl ? nl - text : n;
        uint32_t err;
        bool dropped;
        if (end - at > 0x7fffffffll) { X.err_line = first_line + X.lines; X.err_field = F_FIELDS; return 1; }
        const uint64_t bytes = line<HostLanes, false>(w, text + at, (uint32_t)(end - at), C, K, nullptr, err, dropped);
        if (err != F_NONE) { X.err_line = first_line + X.lines; X.err_field = err; return 1; }
        ++X.lines;
        if (dropped) ++X.dropped;
        else {
            if (out) {
                if (X.out_bytes + (int64_t)bytes > out_cap) return 2;
                line<HostLanes, true>(w, text + at, (uint32_t)(end - at), C, K, out + X.out_bytes, err, dropped);
            }
            ++X.written;
            X.out_bytes += (int64_t)bytes;
        }
        at = nl ? end + 1 : end;
    }
    return 0;
}

}  // namespace coral_sam
