// coral_sam_core.h - SAM text -> BAM records: the encoding rules of `import`, written once for the host and for a 64-lane wave.
//
// One line of SAM text becomes one BAM record by the rules of htslib's sam_parse1 + bam_write1 (what `samtools view -bS` does to a
// mapper's output, /root/reference/scripts/align_nanopore_reads.sh:34-38).  Two entry points per line, one function underneath
// (`line<W, EMIT>`): `size` finds the field boundaries, validates, takes the filter decision and returns the exact byte count of the
// record (0 for a dropped line); `encode` writes those bytes at a given address, which may have ANY alignment.
//
// The core is written against a small backend interface (`W`), as the inflate and the deflate core are: the host runs lanes as
// loops, the device runs one wave.
//   uint64_t ballot(f)    bit l = f(l) over the 64 lanes
//   void     each(f)      f(l) for every lane
//   uint64_t sum(f)       the sum of f(l) over the lanes
//   bool     leader()     true in the one lane that stores what all lanes computed alike (host: always)
//   uint32_t uni(x)       make a value all lanes hold alike wave-uniform (device: readfirstlane)
//   void     slow_float(text, n, dst)   a decimal outside the exact fast path: the host converts it with strtof, the device
//                                       notes (text offset, output offset) as a fix-up for the host
// What is serial in a line (the numeric fields, the tags' keys and integers) is computed by ALL lanes alike and stored by the
// leader; what is long (the tab search, CIGAR, SEQ, QUAL, Z / H values) is spread over the lanes.  Every output byte has one
// writer and no value depends on which lane's write lands last, so the bytes are a function of the text and the filter alone.
// No load reaches behind the line: the word loads stop 4 bytes short of a field's end and the tail goes byte by byte.
#pragma once
#include <stdint.h>

#include "coral_inflate_core.h"      // CORAL_HD

namespace coral_sam {

enum { LANES = 64, CG_LIMIT = 65535 };
// the field a refusal names (field_name)
enum Field : uint32_t { F_NONE = 0, F_FIELDS, F_EMPTY, F_HEADER_LINE, F_QNAME, F_FLAG, F_RNAME, F_POS, F_MAPQ, F_CIGAR, F_RNEXT, F_PNEXT, F_TLEN, F_SEQ, F_QUAL, F_TAG, F_N };

inline const char *field_name(uint32_t f) {
    static const char *const names[F_N] = {"none", "fewer than 11 fields", "an empty line", "an @ line behind the first record", "QNAME", "FLAG", "RNAME", "POS", "MAPQ",
                                           "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL", "a tag"};
    return f < F_N ? names[f] : "?";
}

// The contigs of the header's @SQ lines: the names back to back (no NUL), where each starts, and an open-addressing table
// (linear probing, a power of two of slots, at least twice n_ref; a slot holds 1 + the contig, 0: free) over name_hash.
struct Contigs {
    const uint8_t *names;
    const int64_t *name_off;
    const uint32_t *slots;
    int32_t n_ref;
    uint32_t n_slots;
};
struct Keep { uint32_t min_mapq, min_seq_length, require_flags, exclude_flags; };

CORAL_HD uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
CORAL_HD void store32(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
CORAL_HD void store16(uint8_t *p, uint32_t v) {
    const uint16_t h = (uint16_t)v;
    __builtin_memcpy(p, &h, 2);
}

CORAL_HD uint32_t name_hash(const uint8_t *p, uint32_t n) {          // FNV-1a
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}
// The contig named by the n bytes at p, or -2: the whole name is compared (chr1 is not chr10), along one probe sequence.
CORAL_HD int32_t find_contig(const Contigs &C, const uint8_t *p, uint32_t n) {
    if (C.n_slots == 0) return -2;
    for (uint32_t h = name_hash(p, n) & (C.n_slots - 1), probes = 0; probes < C.n_slots; h = (h + 1) & (C.n_slots - 1), ++probes) {
        const uint32_t v = C.slots[h];
        if (v == 0) return -2;
        const int64_t a = C.name_off[v - 1], len = C.name_off[v] - a;
        if (len != (int64_t)n) continue;
        uint32_t i = 0;
        while (i < n && C.names[a + i] == p[i]) ++i;
        if (i == n) return (int32_t)(v - 1);
    }
    return -2;
}

CORAL_HD uint32_t has_tab(uint32_t w) {                               // non-zero when one of the word's bytes is 9
    const uint32_t x = w ^ 0x09090909u;
    return (x - 0x01010101u) & ~x & 0x80808080u;
}
CORAL_HD bool is_digit(uint32_t c) { return c - 48u < 10u; }

// [+-]?[0-9]+ in [b, e) -> v; false for anything else, or beyond about 2^40 in magnitude
CORAL_HD bool parse_int(const uint8_t *p, uint32_t b, uint32_t e, int64_t &v) {
    bool neg = false;
    if (b < e && (p[b] == '-' || p[b] == '+')) neg = p[b++] == '-';
    if (b >= e) return false;
    uint64_t a = 0;
    for (; b < e; ++b) {
        if (!is_digit(p[b])) return false;
        if (a < (1ull << 40)) a = a * 10 + (p[b] - 48u);
    }
    if (a >= (1ull << 40)) return false;
    v = neg ? -(int64_t)a : (int64_t)a;
    return true;
}

// 4-bit code of a SEQ byte: "=ACMGRSVTWYHKDBN", either case; any other byte 15.  Two 16-nibble tables over the letter's low 5 bits.
CORAL_HD uint32_t seq_code(uint32_t c) {
    const uint32_t idx = c & 31u;
    const uint64_t t = idx < 16 ? 0xFF3FCFFB4FFD2E1Full : 0xFFFFFFAF97F865FFull;
    const uint32_t nib = (uint32_t)(t >> ((idx & 15u) * 4)) & 15u;
    return ((c & 0xdfu) - 65u < 26u) ? nib : (c == '=' ? 0u : 15u);
}
CORAL_HD uint32_t seq_pack8(uint32_t a, uint32_t b) {                 // 8 text bytes (two words) -> 4 packed bytes (one word)
    uint32_t o = 0;
    for (int k = 0; k < 2; ++k) {
        o |= ((seq_code((a >> (16 * k)) & 255u) << 4) | seq_code((a >> (16 * k + 8)) & 255u)) << (8 * k);
        o |= ((seq_code((b >> (16 * k)) & 255u) << 4) | seq_code((b >> (16 * k + 8)) & 255u)) << (8 * k + 16);
    }
    return o;
}
CORAL_HD uint32_t sub33(uint32_t a) {                                 // every byte of the word minus 33, modulo 256
    const uint32_t H = 0x80808080u, b = 0x21212121u;
    return ((a | H) - b) ^ ((a ^ ~b) & H);
}

CORAL_HD uint32_t reg2bin(int64_t beg, int64_t end) {                 // SAMv1 §5.3; the shifts are arithmetic, so beg = -1, end = 0 gives 4680
    --end;
    if ((beg >> 14) == (end >> 14)) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if ((beg >> 17) == (end >> 17)) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if ((beg >> 20) == (end >> 20)) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if ((beg >> 23) == (end >> 23)) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if ((beg >> 26) == (end >> 26)) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// A decimal number in [b, e) as binary32: 0 = not a number of the form [+-]digits[.digits][(e|E)[+-]digits] with at least one
// digit (inf, nan and hexadecimal floats are refused), 1 = `bits` is the correctly rounded value, 2 = outside the exact fast path.
// The fast path is Clinger's: a significand w <= 2^53 and a power of ten 10^|q|, |q| <= 22, are both doubles, so d = w * 10^q or
// w / 10^q is the correctly rounded double of the exact value x.  (float)d is then the correctly rounded float of x unless d
// lies exactly on the midpoint of two floats while x does not; the sign of x - d is the sign of the operation's residual, which
// an fma gives exactly, and it says on which side of the midpoint x lies.  d is between 1e-22 and 9.1e37: a normal float.
CORAL_HD int parse_float(const uint8_t *p, uint32_t b, uint32_t e, uint32_t &bits) {
    bool neg = false, any = false, big = false;
    if (b < e && (p[b] == '-' || p[b] == '+')) neg = p[b++] == '-';
    uint64_t w = 0;
    int64_t q = 0;
    for (; b < e && is_digit(p[b]); ++b) {
        any = true;
        if (w <= (0xffffffffffffffffull - 9) / 10) w = w * 10 + (p[b] - 48u);
        else { big = true; ++q; }
    }
    if (b < e && p[b] == '.')
        for (++b; b < e && is_digit(p[b]); ++b) {
            any = true;
            if (w <= (0xffffffffffffffffull - 9) / 10) { w = w * 10 + (p[b] - 48u); --q; }
            else big = true;
        }
    if (!any) return 0;
    if (b < e && (p[b] == 'e' || p[b] == 'E')) {
        bool eneg = false;
        if (++b < e && (p[b] == '-' || p[b] == '+')) eneg = p[b++] == '-';
        if (b >= e) return 0;
        int64_t x = 0;
        for (; b < e; ++b) {
            if (!is_digit(p[b])) return 0;
            if (x < 100000) x = x * 10 + (p[b] - 48u);
        }
        q += eneg ? -x : x;
    }
    if (b != e) return 0;
    if (w == 0 && !big) { bits = neg ? 0x80000000u : 0u; return 1; }
    if (big || w > (1ull << 53) || q < -22 || q > 22) return 2;
    const double P10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    const double m = (double)w, t = P10[q < 0 ? -q : q];
    const double d = q < 0 ? m / t : m * t;
    const double r = q < 0 ? __builtin_fma(-d, t, m) : __builtin_fma(m, t, -d);      // the sign of x - d, exactly
    float f = (float)d;
    uint32_t fb;
    __builtin_memcpy(&fb, &f, 4);
    if ((double)f != d && r != 0.0) {
        const uint32_t nb = (double)f < d ? fb + 1 : fb - 1;          // the float on the other side of d
        float g;
        __builtin_memcpy(&g, &nb, 4);
        if (((double)f + (double)g) * 0.5 == d) {                      // d is their midpoint and x is not: x's side decides
            const uint32_t lo = fb < nb ? fb : nb, hi = fb < nb ? nb : fb;
            fb = r > 0.0 ? hi : lo;
        }
    }
    bits = fb | (neg ? 0x80000000u : 0u);
    return 1;
}

// CIGAR text [b, e) -> number of ops, reference and query length; the ops as words at `out` when it is given (any alignment).
// 64 bytes per step: a lane whose byte is no digit holds an op, finds the end of the op in front of it in the step's ballot (or
// carried from the step before) and reads its own digits.  false: a byte that is no op, an op without a length, a length of
// 2^28 or more, or digits behind the last op.
template <class W>
CORAL_HD bool cigar(W &w, const uint8_t *p, uint32_t b, uint32_t e, uint32_t &n_ops, uint64_t &ref_len, uint64_t &query_len, uint8_t *out) {
    n_ops = 0;
    ref_len = query_len = 0;
    if (b >= e) return false;
    if (e - b == 1 && p[b] == '*') return true;
    uint32_t prev_end = b;                                            // behind the last op of the steps in front
    bool good = true;
    for (uint32_t base = b; base < e; base += LANES) {
        const uint64_t m = w.ballot([&](int l) { return base + l < e && !is_digit(p[base + l]); });
        auto op_of = [&](int l, uint32_t &len, uint32_t &op) {         // the op of lane l (bit l of m is set); false: a bad one
            const uint32_t c = p[base + l];
            op = c == 'M' ? 0u : c == 'I' ? 1u : c == 'D' ? 2u : c == 'N' ? 3u : c == 'S' ? 4u : c == 'H' ? 5u : c == 'P' ? 6u : c == '=' ? 7u : c == 'X' ? 8u : 9u;
            const uint64_t below = l > 0 ? m & (~0ull >> (64 - l)) : 0ull;
            const uint32_t from = below ? base + (63 - (uint32_t)__builtin_clzll(below)) + 1 : prev_end;
            uint64_t v = 0;
            for (uint32_t i = from; i < base + l; ++i)
                if (v < (1ull << 28)) v = v * 10 + (p[i] - 48u);
            len = (uint32_t)v;
            return op < 9 && from < base + l && v < (1ull << 28);
        };
        const uint64_t bad = w.ballot([&](int l) {
            uint32_t len, op;
            return ((m >> l) & 1) && !op_of(l, len, op);
        });
        if (bad) good = false;
        if (good) {
            ref_len += w.sum([&](int l) -> uint64_t {
                uint32_t len, op;
                if (!((m >> l) & 1)) return 0;
                op_of(l, len, op);
                return (0x18dull >> op) & 1 ? len : 0;               // M D N = X
            });
            query_len += w.sum([&](int l) -> uint64_t {
                uint32_t len, op;
                if (!((m >> l) & 1)) return 0;
                op_of(l, len, op);
                return (0x193ull >> op) & 1 ? len : 0;               // M I S = X
            });
            if (out)
                w.each([&](int l) {
                    uint32_t len, op;
                    if (!((m >> l) & 1)) return;
                    op_of(l, len, op);
                    const uint64_t below = l > 0 ? m & (~0ull >> (64 - l)) : 0ull;
                    store32(out + 4 * ((size_t)n_ops + (uint32_t)__builtin_popcountll(below)), (len << 4) | op);
                });
        }
        n_ops += (uint32_t)__builtin_popcountll(m);
        if (m) prev_end = base + (63 - (uint32_t)__builtin_clzll(m)) + 1;
    }
    return good && prev_end == e;
}

// One integer of a tag -> its smallest type: negative c >= -128, s >= -32768, else i; non-negative C <= 255, S <= 65535, else I
CORAL_HD uint32_t int_type(int64_t v, uint32_t &width) {
    if (v < 0) {
        if (v >= -128) { width = 1; return 'c'; }
        if (v >= -32768) { width = 2; return 's'; }
        width = 4;
        return 'i';
    }
    if (v <= 255) { width = 1; return 'C'; }
    if (v <= 65535) { width = 2; return 'S'; }
    width = 4;
    return 'I';
}
CORAL_HD void put_int(uint8_t *o, int64_t v, uint32_t width) {
    if (width == 1) *o = (uint8_t)v;
    else if (width == 2) store16(o, (uint32_t)v);
    else store32(o, (uint32_t)v);
}
// width and range of a B subtype; false: no subtype
CORAL_HD bool b_subtype(uint32_t c, uint32_t &width, int64_t &lo, int64_t &hi) {
    switch (c) {
        case 'c': width = 1; lo = -128; hi = 127; return true;
        case 'C': width = 1; lo = 0; hi = 255; return true;
        case 's': width = 2; lo = -32768; hi = 32767; return true;
        case 'S': width = 2; lo = 0; hi = 65535; return true;
        case 'i': width = 4; lo = -2147483648ll; hi = 2147483647ll; return true;
        case 'I': width = 4; lo = 0; hi = 4294967295ll; return true;
        case 'f': width = 4; lo = hi = 0; return true;
        default: return false;
    }
}

// The tags [t, n) of a line (t: behind the tab that ends QUAL) -> their bytes in the record; with EMIT written at out.
// false: a malformed tag.
template <class W, bool EMIT>
CORAL_HD bool tags(W &w, const uint8_t *p, uint32_t t, uint32_t n, uint8_t *out, uint64_t &bytes) {
    bytes = 0;
    const bool lead = w.leader();
    for (;;) {
        // the field's end: 256 bytes per step, one word per lane, so that a long Z value costs a search, not a walk
        uint32_t e = n;
        for (uint32_t base = t; base < n; base += 4 * LANES) {
            const uint64_t hit = w.ballot([&](int l) {
                const uint32_t i = base + 4 * l;
                if (i + 4 <= n) return has_tab(load32(p + i)) != 0;
                for (uint32_t k = i; k < n; ++k)
                    if (p[k] == '\t') return true;
                return false;
            });
            if (!hit) continue;
            uint32_t i = base + 4 * (uint32_t)__builtin_ctzll(hit);
            while (p[i] != '\t') ++i;
            e = i;
            break;
        }
        e = w.uni(e);
        if (e - t < 5 || p[t + 2] != ':' || p[t + 4] != ':') return false;
        const uint32_t k0 = p[t], k1 = p[t + 1], type = p[t + 3], v = t + 5;
        if (!((k0 & 0xdfu) - 65u < 26u) || !((k1 & 0xdfu) - 65u < 26u || is_digit(k1))) return false;
        uint8_t *o = EMIT ? out + bytes : nullptr;
        if (EMIT && lead) { o[0] = (uint8_t)k0; o[1] = (uint8_t)k1; }
        if (type == 'A') {
            if (e - v != 1 || p[v] < 33 || p[v] > 126) return false;
            if (EMIT && lead) { o[2] = 'A'; o[3] = p[v]; }
            bytes += 4;
        } else if (type == 'i') {
            int64_t x;
            if (!parse_int(p, v, e, x) || x < -2147483648ll || x > 4294967295ll) return false;
            uint32_t width;
            const uint32_t c = int_type(x, width);
            if (EMIT && lead) { o[2] = (uint8_t)c; put_int(o + 3, x, width); }
            bytes += 3 + width;
        } else if (type == 'f') {
            uint32_t fb = 0;
            const int how = parse_float(p, v, e, fb);
            if (how == 0) return false;
            if (EMIT) {
                if (lead) { o[2] = 'f'; store32(o + 3, fb); }
                if (how == 2) w.slow_float(p + v, e - v, o + 3);
            }
            bytes += 7;
        } else if (type == 'Z' || type == 'H') {
            const uint32_t len = e - v;
            if (type == 'H') {
                if (len & 1) return false;
                bool bad = false;
                for (uint32_t base = v; base < e; base += LANES)
                    if (w.ballot([&](int l) { const uint32_t c = base + l < e ? p[base + l] : 48u; return !(is_digit(c) || (c & 0xdfu) - 65u < 6u); })) bad = true;
                if (bad) return false;
            }
            if (EMIT) {
                if (lead) { o[2] = (uint8_t)type; o[3 + len] = 0; }
                w.each([&](int l) { for (uint32_t i = (uint32_t)l; i < len; i += LANES) o[3 + i] = p[v + i]; });
            }
            bytes += 3 + (uint64_t)len + 1;
        } else if (type == 'B') {
            uint32_t width;
            int64_t lo, hi;
            if (e == v || !b_subtype(p[v], width, lo, hi)) return false;
            const uint32_t sub = p[v];
            uint32_t count = 0;
            for (uint32_t i = v + 1; i < e;) {                       // ,value,value ...
                if (p[i] != ',') return false;
                uint32_t j = ++i;
                while (j < e && p[j] != ',') ++j;
                uint8_t *dst = EMIT ? o + 8 + (size_t)count * width : nullptr;
                if (sub == 'f') {
                    uint32_t fb = 0;
                    const int how = parse_float(p, i, j, fb);
                    if (how == 0) return false;
                    if (EMIT) {
                        if (lead) store32(dst, fb);
                        if (how == 2) w.slow_float(p + i, j - i, dst);
                    }
                } else {
                    int64_t x;
                    if (!parse_int(p, i, j, x) || x < lo || x > hi) return false;
                    if (EMIT && lead) put_int(dst, x, width);
                }
                ++count;
                i = j;
            }
            if (EMIT && lead) { o[2] = 'B'; o[3] = (uint8_t)sub; store32(o + 4, count); }
            bytes += 8 + (uint64_t)count * width;
        } else return false;
        if (e == n) return true;
        t = e + 1;
    }
}

// One line of n bytes at p (without its '\n') -> the record's byte count, block_size word included; 0 with err = F_NONE and
// dropped = true: the filter drops it; 0 with err set: refused.  With EMIT the bytes are written at out: the line has passed
// the size pass, which is where every check is reported.
template <class W, bool EMIT>
CORAL_HD uint64_t line(W &w, const uint8_t *p, uint32_t n, const Contigs &C, const Keep &K, uint8_t *out, uint32_t &err, bool &dropped) {
    err = F_NONE;
    dropped = false;
    auto refuse = [&](uint32_t f) { err = f; return (uint64_t)0; };
    if (n == 0) return refuse(F_EMPTY);
    if (p[0] == '@') return refuse(F_HEADER_LINE);
    // the eleven fields: 256 bytes per step, one word per lane; a step with a tab in it is taken again 64 bytes at a time, in order
    uint32_t fb[11] = {0}, fe[11] = {0}, nf = 0, beg = 0;
    for (uint32_t base = 0; base < n && nf < 11; base += 4 * LANES) {
        const uint64_t any = w.ballot([&](int l) {
            const uint32_t i = base + 4 * l;
            if (i + 4 <= n) return has_tab(load32(p + i)) != 0;
            for (uint32_t k = i; k < n; ++k)
                if (p[k] == '\t') return true;
            return false;
        });
        if (!any) continue;
        for (uint32_t sub = 0; sub < 4 && nf < 11; ++sub) {
            uint64_t m = w.ballot([&](int l) { const uint32_t i = base + LANES * sub + l; return i < n && p[i] == '\t'; });
            for (; m && nf < 11; m &= m - 1) {
                const uint32_t at = base + LANES * sub + (uint32_t)__builtin_ctzll(m);
                for (uint32_t k = 0; k < 11; ++k)                    // (constant indices: the two arrays stay in registers)
                    if (k == nf) { fb[k] = beg; fe[k] = at; }
                ++nf;
                beg = at + 1;
            }
        }
    }
    const bool has_tags = nf == 11;
    const uint32_t tags_at = beg;
    if (nf < 10) return refuse(F_FIELDS);
    if (nf == 10) { fb[10] = beg; fe[10] = n; }                       // (QUAL ends the line: no tags)
    for (int k = 0; k < 11; ++k) { fb[k] = w.uni(fb[k]); fe[k] = w.uni(fe[k]); }
    const uint32_t l_name = fe[0] - fb[0];
    if (l_name < 1 || l_name > 254) return refuse(F_QNAME);
    int64_t flag, pos, mapq, pnext, tlen;
    if (!parse_int(p, fb[1], fe[1], flag) || flag < 0 || flag > 65535) return refuse(F_FLAG);
    int32_t tid = -1, next_tid = -1;
    if (!(fe[2] - fb[2] == 1 && p[fb[2]] == '*') && (tid = find_contig(C, p + fb[2], fe[2] - fb[2])) < 0) return refuse(F_RNAME);
    if (!parse_int(p, fb[3], fe[3], pos) || pos < 0 || pos > 2147483647ll) return refuse(F_POS);
    if (!parse_int(p, fb[4], fe[4], mapq) || mapq < 0 || mapq > 255) return refuse(F_MAPQ);
    const bool seq_star = fe[9] - fb[9] == 1 && p[fb[9]] == '*', qual_star = fe[10] - fb[10] == 1 && p[fb[10]] == '*';
    const uint32_t l_seq = seq_star ? 0u : fe[9] - fb[9];
    uint32_t n_ops;
    uint64_t ref_len, query_len;
    // (the ops go straight into the record unless they are too many for it: then they follow the tags, as the CG tag's values)
    const uint64_t head = 36 + (uint64_t)l_name + 1;
    uint8_t *cig_out = nullptr;
    bool counted = false;
    if (EMIT) {
        if ((fe[5] - fb[5]) / 2 <= CG_LIMIT) cig_out = out + head;   // (an op is at least two bytes of text: they fit for certain)
        else {                                                        // a first, counting walk tells where the ops go
            if (!cigar(w, p, fb[5], fe[5], n_ops, ref_len, query_len, nullptr)) return refuse(F_CIGAR);
            if (n_ops <= CG_LIMIT) cig_out = out + head;
            else counted = true;
        }
    }
    if (!counted && !cigar(w, p, fb[5], fe[5], n_ops, ref_len, query_len, cig_out)) return refuse(F_CIGAR);
    const bool as_cg = n_ops > CG_LIMIT;
    if (as_cg && (l_seq >= (1u << 28) || ref_len >= (1ull << 28))) return refuse(F_CIGAR);
    if (fe[6] - fb[6] == 1 && p[fb[6]] == '=') next_tid = tid;
    else if (!(fe[6] - fb[6] == 1 && p[fb[6]] == '*') && (next_tid = find_contig(C, p + fb[6], fe[6] - fb[6])) < 0) return refuse(F_RNEXT);
    if (!parse_int(p, fb[7], fe[7], pnext) || pnext < 0 || pnext > 2147483647ll) return refuse(F_PNEXT);
    if (!parse_int(p, fb[8], fe[8], tlen) || tlen < -2147483648ll || tlen > 2147483647ll) return refuse(F_TLEN);
    if (fe[9] == fb[9] || (!seq_star && n_ops > 0 && query_len != l_seq)) return refuse(F_SEQ);
    if (fe[10] == fb[10] || (!qual_star && (seq_star || fe[10] - fb[10] != l_seq))) return refuse(F_QUAL);
    const uint32_t rec_ops = as_cg ? 2u : n_ops;
    const uint64_t fixed = head + 4ull * rec_ops + (l_seq + 1) / 2 + l_seq;
    uint64_t tag_bytes = 0;
    if (has_tags && !tags<W, EMIT>(w, p, tags_at, n, EMIT ? out + fixed : nullptr, tag_bytes)) return refuse(F_TAG);
    const uint64_t total = fixed + tag_bytes + (as_cg ? 8 + 4ull * n_ops : 0);
    if (total - 4 > 0x7fffffffull) return refuse(F_TAG);
    if (!(mapq >= (int64_t)K.min_mapq && l_seq >= K.min_seq_length && ((uint32_t)flag & K.require_flags) == K.require_flags && ((uint32_t)flag & K.exclude_flags) == 0)) {
        dropped = true;
        return 0;
    }
    if (!EMIT) return total;

    const int64_t pos0 = pos - 1, end = pos0 + ((flag & 4) == 0 && n_ops > 0 && ref_len > 0 ? (int64_t)ref_len : 1);
    if (w.leader()) {
        store32(out, (uint32_t)(total - 4));
        store32(out + 4, (uint32_t)tid);
        store32(out + 8, (uint32_t)pos0);
        store32(out + 12, (l_name + 1) | ((uint32_t)mapq << 8) | (reg2bin(pos0, end) << 16));
        store32(out + 16, rec_ops | ((uint32_t)flag << 16));
        store32(out + 20, l_seq);
        store32(out + 24, (uint32_t)next_tid);
        store32(out + 28, (uint32_t)(pnext - 1));
        store32(out + 32, (uint32_t)tlen);
        out[36 + l_name] = 0;
        if (as_cg) {
            store32(out + head, (l_seq << 4) | 4u);
            store32(out + head + 4, ((uint32_t)ref_len << 4) | 3u);
            uint8_t *cg = out + fixed + tag_bytes;
            cg[0] = 'C'; cg[1] = 'G'; cg[2] = 'B'; cg[3] = 'I';
            store32(cg + 4, n_ops);
        }
    }
    w.each([&](int l) { for (uint32_t i = (uint32_t)l; i < l_name; i += LANES) out[36 + i] = p[fb[0] + i]; });
    if (as_cg) {
        uint32_t n2;
        uint64_t r2, q2;
        cigar(w, p, fb[5], fe[5], n2, r2, q2, out + fixed + tag_bytes + 8);
    }
    // SEQ: 512 text bytes per step, 8 per lane -> one word; QUAL: 512 bytes per step, two words per lane
    uint8_t *seq_out = out + head + 4ull * rec_ops, *qual_out = seq_out + (l_seq + 1) / 2;
    const uint8_t *s = p + fb[9], *q = p + fb[10];
    for (uint32_t base = 0; base < l_seq; base += 8 * LANES)
        w.each([&](int l) {
            const uint32_t i = base + 8 * l;
            if (i + 8 <= l_seq) store32(seq_out + i / 2, seq_pack8(load32(s + i), load32(s + i + 4)));
            else
                for (uint32_t k = i; k < l_seq; k += 2) seq_out[k / 2] = (uint8_t)((seq_code(s[k]) << 4) | (k + 1 < l_seq ? seq_code(s[k + 1]) : 0u));
        });
    for (uint32_t base = 0; base < l_seq; base += 8 * LANES)
        w.each([&](int l) {
            const uint32_t i = base + 8 * l;
            if (qual_star) {
                for (uint32_t k = i; k < i + 8 && k < l_seq; ++k) qual_out[k] = 0xff;
            } else if (i + 8 <= l_seq) {
                store32(qual_out + i, sub33(load32(q + i)));
                store32(qual_out + i + 4, sub33(load32(q + i + 4)));
            } else
                for (uint32_t k = i; k < l_seq; ++k) qual_out[k] = (uint8_t)(q[k] - 33u);
        });
    return total;
}

// Record bytes against text bytes, per line of T text bytes (its '\n' included, if it has one):
//   the fixed part is 37 + l_name bytes against at least l_name + 17 (seven one-byte fields, ten tabs): at most 20 more;
//   a CIGAR op is 4 bytes against at least 2; the CG shape adds 16 (the placeholder, the tag's head);
//   SEQ + QUAL is 1.5 l_seq against at least l_seq + 1;
//   a tag is at most twice its text (B:f,1: four bytes per ",1"; an empty B: 8 bytes against a tab and 6).
// So a record is at most 2 T + 36 bytes.
CORAL_HD uint64_t record_bound(uint64_t text_bytes, uint64_t n_lines) { return 2 * text_bytes + 36 * n_lines; }

}  // namespace coral_sam
