// coral_deflate_core.h — RFC 1951 (DEFLATE) compressor core of the GPU BGZF writer (coral_bamgpu_deflate.h): the mirror image of
// coral_inflate_core.h.
//
// One 64-lane wave turns one input block of at most 0xff00 bytes into one complete BGZF member: the 18-byte header with BSIZE, one
// raw DEFLATE stream of ONE block — dynamic Huffman (BTYPE 2), or stored (BTYPE 0) when the dynamic stream would not be smaller
// than len + 5 bytes — and the CRC-32 / ISIZE trailer.  A member is therefore never larger than len + 5 + 26 bytes.
//
//   pass 1  match search, 64 positions per step: every lane hashes the 4 bytes at its own position into a table of 16-bit
//           positions (State::head), reads the candidate that EARLIER steps left there, measures the match at that candidate and at
//           distance 1 (positions of one step cannot find each other through the table, so byte runs are found directly), and
//           the wave picks tokens greedily left to right in a wave-uniform loop over the chosen matches (ballot, find-first).
//           The next step starts behind the last chosen match: bytes inside a match are neither searched nor hashed.
//           Tokens go to caller-provided memory (`tok`, one 32-bit word each, at most one per input byte), their symbols into
//           the two histograms.
//   codes   code lengths of both alphabets, limited to 15 bits (symbols ranked by frequency in parallel; the tree — Moffat and
//           Katajainen's in-place minimum-redundancy lengths — and the Kraft repair serially in one lane, over at most 286
//           symbols), canonical codes, the exact size of the dynamic stream from the histograms: the block type and BSIZE are
//           known before a bit is written.
//   pass 2  64 tokens per step: a wave prefix sum over their bit lengths, the bits OR-ed into a small staging buffer (OR
//           commutes), whole words stored to the member's slot.  The header, the stored bytes and the trailer take the same way.
//
// The bytes are a pure function of the input block: no value depends on which lane's write lands last (the hash table keeps
// the LARGEST position of a step, store_max16), on the launch, or on whether the host or the device backend runs the code.
// The core is written against a small backend interface (`W`), as the decoder's is; tests/test_deflate_core.py drives the host
// build (lanes as loops) against zlib.  The product only ever uses the device backend; nothing here is a CPU fallback.
//
// Replaces what the reference's workflow gets from `samtools view -b` / `samtools sort` when they write their output
// (/root/reference/scripts/align_nanopore_reads.sh:44, :49: htslib's bgzf_write + zlib deflate).
#pragma once
#include <stdint.h>

#include "coral_crc32.h"
#include "coral_inflate_core.h"      // CORAL_HD, CORAL_NOUNROLL, W_FOR_LANES

namespace coral_deflate {

using coral_inflate::WAVE_LANES;         // (W_FOR_LANES names it)
enum { LANES = 64, BLOCK_MAX = 0xff00, SLOT_BYTES = 65536, HASH_BITS = 13, MAX_MATCH = 258, MAX_DIST = 32768, N_LL = 286, N_D = 30,
       MAX_BITS = 15, HEADER_BYTES = 18, TRAILER_BYTES = 8, STAGE_WORDS = 128, MEMBER_MAX = BLOCK_MAX + 5 + HEADER_BYTES + TRAILER_BYTES };
// a token: a literal byte, or TOK_MATCH | (length - 3) << 16 | (distance - 1)
enum : uint32_t { TOK_MATCH = 1u << 31 };
static_assert(MEMBER_MAX + 3 < SLOT_BYTES, "a member, rounded up to whole words, fits its slot");

struct State {                           // per wave, in LDS on the device
    uint16_t head[1 << HASH_BITS];       // hash of 4 bytes -> 1 + the largest position seen with it (0: none)
    uint32_t ll_freq[288], d_freq[32];   // histograms of the literal / length and the distance symbols
    uint32_t work[288];                  // code construction: the used symbols' frequencies in ascending order, then their depths
    uint16_t order[288];                 //   ... and which symbol each is
    uint32_t num[16], next[16];          // codes per length; the next canonical code of each length
    uint16_t ll_code[288], d_code[32];   // canonical codes, bit-reversed (DEFLATE writes Huffman codes from their top bit)
    uint8_t ll_len[288], d_len[32];
    uint32_t stage[STAGE_WORDS];         // bits of the step being written, from the first word not yet in the slot
    uint32_t crc_table[256];
    uint32_t lane_word[LANES];           // per lane: the candidate of a step; the CRC pieces
    uint16_t mlen[LANES], mdist[LANES];  // per lane: the match of a step (length 0: none)
};
static_assert(sizeof(State) == 16384 + 1280 + 1152 + 576 + 128 + 640 + 320 + 512 + 1024 + 256 + 256, "State: 22 528 bytes of LDS per wave");

CORAL_HD uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
CORAL_HD uint32_t hash4(const uint8_t *p) { return (load32(p) * 2654435761u) >> (32 - HASH_BITS); }
CORAL_HD uint32_t rev16(uint32_t c, uint32_t len) {          // the low `len` bits of c in reverse order
    c = ((c & 0x5555u) << 1) | ((c >> 1) & 0x5555u);
    c = ((c & 0x3333u) << 2) | ((c >> 2) & 0x3333u);
    c = ((c & 0x0f0fu) << 4) | ((c >> 4) & 0x0f0fu);
    c = ((c & 0x00ffu) << 8) | ((c >> 8) & 0x00ffu);
    return c >> (16 - len);
}
// length - 3 (0..255) and distance - 1 (0..32767) -> symbol, number and value of the extra bits (RFC 1951 §3.2.5, computed: the
// inverse of coral_inflate::ll_entry / dist_entry)
CORAL_HD void len_code(uint32_t l, uint32_t &sym, uint32_t &xb, uint32_t &xv) {
    if (l < 8 || l == 255) {
        sym = l < 8 ? 257 + l : 285;
        xb = xv = 0;
        return;
    }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    sym = 257u + (((e + 1u) << 2) | ((l >> e) & 3u));
    xb = e;
    xv = l & ((1u << e) - 1u);
}
CORAL_HD void dist_code(uint32_t d0, uint32_t &sym, uint32_t &xb, uint32_t &xv) {
    if (d0 < 4) {
        sym = d0;
        xb = xv = 0;
        return;
    }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(d0)) - 1u;
    sym = ((e + 1u) << 1) | ((d0 >> e) & 1u);
    xb = e;
    xv = d0 & ((1u << e) - 1u);
}
CORAL_HD uint32_t ll_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261u) >> 2; }
CORAL_HD uint32_t d_extra(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1u; }

// Backend interface (`W`); per-lane execution is spelled W_FOR_LANES(w, lane), as in the decoder's core: the device runs the body
// once with the wave's own lane id, the host loops over 64 lanes IN LANE ORDER.  What one lane leaves for another goes through
// State, with a fence between the two W_FOR_LANES.
//   uint32_t uni(uint32_t)                  make a value read from State wave-uniform (device: readfirstlane)
//   void     fence()                        order the State / token writes of all lanes before later reads
//   void     add_count(uint32_t *c)         atomic / plain increment
//   void     or_bits(uint32_t *p, uint32_t v)     atomic / plain OR
//   void     store_max16(uint16_t *p, uint32_t v) *p = max(*p, v) over all lanes that name the same p; called by EVERY lane of a
//                                           W_FOR_LANES (v = 0: nothing to store)
//   void     vote(int lane, bool p); uint64_t vote_mask()     ballot: the lanes' predicates of the W_FOR_LANES just run
//   uint32_t scan_excl(uint32_t x); uint32_t scan_total()     exclusive prefix sum over the lanes, called by EVERY lane exactly
//                                           once per W_FOR_LANES; the sum of all lanes afterwards
template <class W>
struct Deflater {
    W &w;
    State *S;
    const uint8_t *in;        // the block
    uint32_t n;               // its bytes, <= BLOCK_MAX
    uint32_t *out;            // the member's slot (4-byte aligned, SLOT_BYTES)
    uint32_t *tok;            // room for n tokens
    uint32_t n_tok = 0;
    uint32_t bitpos = 0;      // bits of the member written so far (wave-uniform)
    uint32_t flushed = 0;     // whole words of it already in the slot

    CORAL_HD Deflater(W &w_, State *s, const uint8_t *in_, uint32_t n_, uint32_t *out_, uint32_t *tok_) : w(w_), S(s), in(in_), n(n_), out(out_), tok(tok_) {}

    // ---- the bit writer -------------------------------------------------------------------------------------------------
    // One step: every lane contributes `nb` <= 48 bits (f(lane, v, nb)); they are laid out in lane order behind bitpos.
    template <class F>
    CORAL_HD void emit_step(F f) {
        W_FOR_LANES(w, lane) {
            uint64_t v = 0;
            uint32_t nb = 0;
            f(lane, v, nb);
            const uint32_t rel = bitpos + w.scan_excl(nb) - 32u * flushed;
            if (nb) {
                const uint32_t wi = rel >> 5, sh = rel & 31u;
                const uint32_t lo = (uint32_t)(v << sh), mid = (uint32_t)((v << sh) >> 32), hi = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
                if (lo) w.or_bits(&S->stage[wi], lo);
                if (mid) w.or_bits(&S->stage[wi + 1], mid);
                if (hi) w.or_bits(&S->stage[wi + 2], hi);
            }
        }
        w.fence();
        bitpos += w.scan_total();
        const uint32_t full = (bitpos >> 5) - flushed;               // whole words: to the slot
        W_FOR_LANES(w, lane) { for (uint32_t i = (uint32_t)lane; i < full; i += LANES) out[flushed + i] = S->stage[i]; }
        w.fence();
        const uint32_t carry = w.uni(S->stage[full]);
        w.fence();
        W_FOR_LANES(w, lane) { for (uint32_t i = (uint32_t)lane; i <= full; i += LANES) S->stage[i] = i == 0 ? carry : 0u; }
        w.fence();
        flushed += full;
    }

    // ---- CRC-32 of the block: one contiguous chunk per lane, put together as k_bgzf_crc does --------------------------------
    CORAL_HD uint32_t crc32() {
        const uint32_t per = (n + LANES - 1) / LANES;
        W_FOR_LANES(w, lane) {
            const uint32_t a = (uint32_t)lane * per < n ? (uint32_t)lane * per : n, e = a + per < n ? a + per : n;
            uint32_t t = coral_crc::shift(coral_crc::raw(S->crc_table, in + a, e - a), n - e);
            if (lane == 0) t ^= coral_crc::shift(0xffffffffu, n);
            S->lane_word[lane] = t;
        }
        w.fence();
        uint32_t x = 0;
        CORAL_NOUNROLL
        for (int i = 0; i < LANES; ++i) x ^= w.uni(S->lane_word[i]);
        w.fence();
        return ~x;
    }

    // ---- pass 1 -----------------------------------------------------------------------------------------------------------
    // Equal bytes at in[a ..] and in[b ..], a < b, at most `maxlen` <= n - b of them: nothing behind the block's last byte is read.
    CORAL_HD uint32_t match_len(uint32_t a, uint32_t b, uint32_t maxlen) const {
        uint32_t k = 0;
        CORAL_NOUNROLL
        while (k + 4 <= maxlen) {
            const uint32_t x = load32(in + a + k) ^ load32(in + b + k);
            if (x) return k + ((uint32_t)__builtin_ctz(x) >> 3);
            k += 4;
        }
        while (k < maxlen && in[a + k] == in[b + k]) ++k;
        return k;
    }

    CORAL_HD void find_tokens() {
        uint32_t base = 0;
        CORAL_NOUNROLL
        while (base < n) {
            // what earlier steps left in the table: read by all lanes before any lane of this step inserts
            W_FOR_LANES(w, lane) {
                const uint32_t p = base + (uint32_t)lane;
                S->lane_word[lane] = p + 4 <= n ? S->head[hash4(in + p)] : 0u;
            }
            w.fence();
            W_FOR_LANES(w, lane) {
                const uint32_t p = base + (uint32_t)lane;
                const bool ins = p + 4 <= n;
                w.store_max16(&S->head[ins ? hash4(in + p) : 0u], ins ? p + 1u : 0u);
            }
            w.fence();
            W_FOR_LANES(w, lane) {
                const uint32_t p = base + (uint32_t)lane;
                uint32_t len = 0, dist = 0;
                if (p < n) {
                    const uint32_t maxlen = n - p < MAX_MATCH ? n - p : (uint32_t)MAX_MATCH;
                    const uint32_t c = S->lane_word[lane];
                    if (c != 0 && p - (c - 1u) <= MAX_DIST) {        // (a block is longer than the window: a hit may lie too far back)
                        const uint32_t l = match_len(c - 1u, p, maxlen);
                        if (l >= 4) {
                            len = l;
                            dist = p - (c - 1u);
                        }
                    }
                    if (p >= 1 && maxlen >= 3 && in[p] == in[p - 1]) {
                        const uint32_t l = match_len(p - 1u, p, maxlen);
                        if (l >= 3 && l >= len) {
                            len = l;
                            dist = 1;
                        }
                    }
                }
                S->mlen[lane] = (uint16_t)len;
                S->mdist[lane] = (uint16_t)(dist - 1u);
                w.vote(lane, len != 0);
            }
            w.fence();
            // greedy, left to right: the first match at or behind `cur` is taken, everything in front of it is literals
            const uint64_t m = w.vote_mask();
            uint64_t chosen = 0, covered = 0;
            uint32_t cur = 0;
            CORAL_NOUNROLL
            while (cur < LANES) {
                const uint64_t mm = (m >> cur) << cur;
                if (!mm) break;
                const uint32_t l = (uint32_t)__builtin_ctzll(mm);
                const uint32_t end = l + w.uni(S->mlen[l]);
                chosen |= 1ull << l;
                covered |= (end >= LANES ? ~0ull : (1ull << end) - 1ull) & ~((2ull << l) - 1ull);
                cur = end;
            }
            const uint64_t valid = n - base >= LANES ? ~0ull : (1ull << (n - base)) - 1ull;
            const uint64_t T = valid & ~covered;
            W_FOR_LANES(w, lane) {
                if ((T >> lane) & 1ull) {
                    const uint32_t at = n_tok + (uint32_t)__builtin_popcountll(T & ((1ull << lane) - 1ull));
                    uint32_t t;
                    if ((chosen >> lane) & 1ull) {
                        const uint32_t l = (uint32_t)S->mlen[lane] - 3u, d0 = S->mdist[lane];
                        uint32_t sym, xb, xv;
                        len_code(l, sym, xb, xv);
                        w.add_count(&S->ll_freq[sym]);
                        dist_code(d0, sym, xb, xv);
                        w.add_count(&S->d_freq[sym]);
                        t = TOK_MATCH | (l << 16) | d0;
                    } else {
                        t = in[base + (uint32_t)lane];
                        w.add_count(&S->ll_freq[t]);
                    }
                    tok[at] = t;
                }
            }
            w.fence();
            n_tok += (uint32_t)__builtin_popcountll(T);
            base += cur > LANES ? cur : (uint32_t)LANES;
        }
    }

    // ---- code construction -------------------------------------------------------------------------------------------------
    // Code lengths (<= MAX_BITS) and canonical codes of one alphabet from its histogram.  One used symbol gets one bit (RFC 1951
    // §3.2.7: "one distance code ... is encoded using one bit, not zero bits"), none leaves every length 0.
    CORAL_HD void build_code(const uint32_t *freq, int n_sym, uint8_t *lens, uint16_t *codes) {
        // the used symbols in ascending order of (frequency, symbol): every lane ranks its own
        W_FOR_LANES(w, lane) {
            uint32_t used = 0;
            for (int s = lane; s < n_sym; s += LANES) {
                const uint32_t f = freq[s];
                lens[s] = 0;
                codes[s] = 0;
                if (!f) continue;
                uint32_t r = 0;
                CORAL_NOUNROLL
                for (int t = 0; t < n_sym; ++t) {
                    const uint32_t ft = freq[t];
                    r += (ft != 0 && (ft < f || (ft == f && t < s))) ? 1u : 0u;
                }
                S->work[r] = f;
                S->order[r] = (uint16_t)s;
                ++used;
            }
            w.scan_excl(used);
        }
        w.fence();
        const int n_used = (int)w.scan_total();
        W_FOR_LANES(w, lane) {
            if (lane == 0 && n_used > 0) {
                uint32_t *A = S->work;
                for (int i = 0; i < 16; ++i) S->num[i] = 0;
                if (n_used == 1) {
                    S->num[1] = 1;
                } else {
                    // minimum-redundancy code lengths in place (Moffat & Katajainen 1995): A[] ascending frequencies -> depths
                    A[0] += A[1];
                    int root = 0, leaf = 2, next;
                    CORAL_NOUNROLL
                    for (next = 1; next < n_used - 1; ++next) {
                        if (leaf >= n_used || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
                        else A[next] = A[leaf++];
                        if (leaf >= n_used || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
                        else A[next] += A[leaf++];
                    }
                    A[n_used - 2] = 0;
                    CORAL_NOUNROLL
                    for (next = n_used - 3; next >= 0; --next) A[next] = A[A[next]] + 1u;
                    int avbl = 1, used = 0, dpth = 0;
                    root = n_used - 2;
                    next = n_used - 1;
                    CORAL_NOUNROLL
                    while (avbl > 0) {
                        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
                        while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
                        avbl = 2 * used;
                        ++dpth;
                        used = 0;
                    }
                    // codes per length, everything deeper than MAX_BITS counted there; then the Kraft sum is brought back to 1
                    CORAL_NOUNROLL
                    for (int i = 0; i < n_used; ++i) ++S->num[A[i] < MAX_BITS ? A[i] : (uint32_t)MAX_BITS];
                    uint32_t total = 0;
                    for (int i = MAX_BITS; i > 0; --i) total += S->num[i] << (MAX_BITS - i);
                    CORAL_NOUNROLL
                    while (total != (1u << MAX_BITS)) {
                        --S->num[MAX_BITS];
                        for (int i = MAX_BITS - 1; i > 0; --i)
                            if (S->num[i]) {
                                --S->num[i];
                                S->num[i + 1] += 2;
                                break;
                            }
                        --total;
                    }
                }
                // the shortest codes go to the most frequent symbols (the end of the ascending order)
                int j = n_used;
                for (int i = 1; i <= MAX_BITS; ++i)
                    for (uint32_t l = S->num[i]; l > 0; --l) lens[S->order[--j]] = (uint8_t)i;
                // canonical codes (RFC 1951 §3.2.2)
                uint32_t code = 0;
                S->next[0] = 0;
                for (int i = 1; i <= MAX_BITS; ++i) {
                    code = (code + S->num[i - 1]) << 1;
                    S->next[i] = code;
                }
                CORAL_NOUNROLL
                for (int s = 0; s < n_sym; ++s) {
                    const uint32_t l = lens[s];
                    if (l) codes[s] = (uint16_t)rev16(S->next[l]++, l);
                }
            }
        }
        w.fence();
    }

    // bits of the dynamic stream: header, every symbol with its extra bits, the end-of-block code
    CORAL_HD uint32_t dynamic_bits(int hlit, int hdist) {
        W_FOR_LANES(w, lane) {
            uint32_t bits = 0;
            for (int s = lane; s < N_LL; s += LANES) bits += S->ll_freq[s] * ((uint32_t)S->ll_len[s] + ll_extra((uint32_t)s));
            if (lane < N_D) bits += S->d_freq[lane] * ((uint32_t)S->d_len[lane] + d_extra((uint32_t)lane));
            w.scan_excl(bits);
        }
        return 3u + 5u + 5u + 4u + 19u * 3u + 4u * (uint32_t)(hlit + hdist) + w.scan_total();
    }

    // ---- pass 2 -----------------------------------------------------------------------------------------------------------
    CORAL_HD void emit_dynamic(int hlit, int hdist) {
        // BFINAL = 1, BTYPE = 2, HLIT, HDIST, HCLEN = 15: all 19 lengths of the code-length code, in the order of RFC 1951 §3.2.7
        // (16 17 18 0 8 7 ...): 0 for the three run-length symbols, 4 for the symbols 0..15 - a complete code, never tuned
        emit_step([&](int lane, uint64_t &v, uint32_t &nb) {
            if (lane == 0) {
                v = 1u | (2u << 1) | ((uint32_t)(hlit - 257) << 3) | ((uint32_t)(hdist - 1) << 8) | (15u << 13);
                nb = 17;
            } else if (lane <= 19) {
                v = lane <= 3 ? 0u : 4u;
                nb = 3;
            }
        });
        const int total = hlit + hdist;
        for (int s0 = 0; s0 < total; s0 += LANES)
            emit_step([&](int lane, uint64_t &v, uint32_t &nb) {
                const int s = s0 + lane;
                if (s < total) {
                    v = rev16(s < hlit ? S->ll_len[s] : S->d_len[s - hlit], 4);       // (the code of length l is l itself)
                    nb = 4;
                }
            });
        CORAL_NOUNROLL
        for (uint32_t t0 = 0; t0 < n_tok; t0 += LANES)
            emit_step([&](int lane, uint64_t &v, uint32_t &nb) {
                if (t0 + (uint32_t)lane >= n_tok) return;
                const uint32_t t = tok[t0 + (uint32_t)lane];
                if (!(t & TOK_MATCH)) {
                    v = S->ll_code[t];
                    nb = S->ll_len[t];
                    return;
                }
                uint32_t sym, xb, xv;
                len_code((t >> 16) & 0xffu, sym, xb, xv);
                v = S->ll_code[sym];
                nb = S->ll_len[sym];
                v |= (uint64_t)xv << nb;
                nb += xb;
                dist_code(t & 0x7fffu, sym, xb, xv);
                v |= (uint64_t)S->d_code[sym] << nb;
                nb += S->d_len[sym];
                v |= (uint64_t)xv << nb;
                nb += xb;
            });
        emit_step([&](int lane, uint64_t &v, uint32_t &nb) {
            if (lane == 0) {
                v = S->ll_code[256];
                nb = S->ll_len[256];
            }
        });
    }

    CORAL_HD void emit_stored() {
        emit_step([&](int lane, uint64_t &v, uint32_t &nb) {          // BFINAL = 1, BTYPE = 0, to the byte boundary; LEN, NLEN
            if (lane == 0) {
                v = 1u | ((uint64_t)n << 8) | ((uint64_t)(~n & 0xffffu) << 24);
                nb = 40;
            }
        });
        CORAL_NOUNROLL
        for (uint32_t s0 = 0; s0 < n; s0 += 4 * LANES)
            emit_step([&](int lane, uint64_t &v, uint32_t &nb) {
                const uint32_t p = s0 + 4u * (uint32_t)lane;
                if (p + 4 <= n) {
                    v = load32(in + p);
                    nb = 32;
                } else {
                    for (uint32_t k = 0; p + k < n; ++k) v |= (uint64_t)in[p + k] << (8 * k);
                    nb = p < n ? 8 * (n - p) : 0;
                }
            });
    }

    // The whole member; returns its length in bytes.
    CORAL_HD uint32_t run() {
        W_FOR_LANES(w, lane) {
            for (int i = lane; i < (1 << HASH_BITS); i += LANES) S->head[i] = 0;
            for (int i = lane; i < 288; i += LANES) S->ll_freq[i] = 0;
            for (int i = lane; i < 32; i += LANES) S->d_freq[i] = 0;
            for (int i = lane; i < STAGE_WORDS; i += LANES) S->stage[i] = 0;
            for (int i = lane; i < 256; i += LANES) S->crc_table[i] = coral_crc::table_entry((uint32_t)i);
        }
        w.fence();
        const uint32_t crc = crc32();
        int hlit = 257, hdist = 1;
        uint32_t payload = n + 5;
        bool dynamic = false;
        if (n > 0) {
            find_tokens();
            W_FOR_LANES(w, lane) { if (lane == 0) S->ll_freq[256] = 1; }
            w.fence();
            build_code(S->ll_freq, N_LL, S->ll_len, S->ll_code);
            build_code(S->d_freq, N_D, S->d_len, S->d_code);
            hlit = N_LL;                                             // trailing unused symbols are trimmed (256 is always used)
            while (hlit > 257 && w.uni(S->ll_len[hlit - 1]) == 0) --hlit;
            hdist = N_D;                                             // no distance code at all: HDIST = 1, one length of zero
            while (hdist > 1 && w.uni(S->d_len[hdist - 1]) == 0) --hdist;
            const uint32_t dyn_bytes = (dynamic_bits(hlit, hdist) + 7u) >> 3;
            dynamic = dyn_bytes < n + 5;
            if (dynamic) payload = dyn_bytes;
        }
        const uint32_t member = HEADER_BYTES + payload + TRAILER_BYTES;
        emit_step([&](int lane, uint64_t &v, uint32_t &nb) {          // 1f 8b 08 04, MTIME, XFL, OS, XLEN = 6, 'B' 'C' 2 0, BSIZE
            nb = lane < 4 ? 32 : lane == 4 ? 16 : 0;
            v = lane == 0 ? 0x04088b1fu : lane == 2 ? 0x0006ff00u : lane == 3 ? 0x00024342u : lane == 4 ? member - 1u : 0u;
        });
        if (dynamic) emit_dynamic(hlit, hdist);
        else emit_stored();
        bitpos = (bitpos + 7u) & ~7u;                                // (the padding bits are zero already)
        emit_step([&](int lane, uint64_t &v, uint32_t &nb) {
            nb = lane < 2 ? 32 : 0;
            v = lane == 0 ? crc : lane == 1 ? n : 0u;
        });
        if (bitpos & 31u) {                                           // the last, partial word: zero-padded, inside the slot
            W_FOR_LANES(w, lane) { if (lane == 0) out[flushed] = S->stage[0]; }
        }
        w.fence();
        return bitpos >> 3;                                           // == member
    }
};

}  // namespace coral_deflate
