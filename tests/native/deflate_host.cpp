// Host build of the DEFLATE compressor core of the GPU BGZF writer (coral_amd/csrc/coral_deflate_core.h) for
// tests/test_deflate_core.py: the match search, the code construction and the bit writer are the code the device runs; only the
// backend differs (lanes are loops in lane order, memory is plain arrays).  Test infrastructure, never part of libcoral_hip.so.
//
// As a shared library (coral_test_deflate), and with -DDEFLATE_HOST_MAIN as a stand-alone program for the sanitizer run
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DDEFLATE_HOST_MAIN tests/native/deflate_host.cpp -o deflate_host
//   ./deflate_host cases.bin members.bin
// cases.bin: per case a uint32 length and the bytes; members.bin: per case a uint32 length and the BGZF member.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../coral_amd/csrc/coral_deflate_core.h"

using namespace coral_deflate;

struct HostWave {
    uint64_t mask = 0;
    uint32_t acc = 0;
    uint32_t uni(uint32_t x) const { return x; }
    void fence() {}
    void add_count(uint32_t *c) { ++*c; }
    void or_bits(uint32_t *p, uint32_t v) { *p |= v; }
    void store_max16(uint16_t *p, uint32_t v) { if (*p < v) *p = (uint16_t)v; }
    void vote(int lane, bool p) {
        if (lane == 0) mask = 0;
        if (p) mask |= 1ull << lane;
    }
    uint64_t vote_mask() const { return mask; }
    uint32_t scan_excl(uint32_t x) {
        const uint32_t r = acc;
        acc += x;
        return r;
    }
    uint32_t scan_total() {
        const uint32_t t = acc;
        acc = 0;
        return t;
    }
};

// `in` n bytes -> the member in `out` (SLOT_BYTES, 4-byte aligned); tokens (n words, may be null) gets pass 1's tokens and
// *n_tokens their number (0 for an empty block).  Returns the member's length, or -1 for n > BLOCK_MAX.
// The input and the token array are copied into allocations of exactly their size, so that a sanitizer sees any access beyond them.
extern "C" int coral_test_deflate(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t *tokens, uint32_t *n_tokens) {
    if (n > BLOCK_MAX) return -1;
    std::vector<uint8_t> src(in, in + n);
    std::vector<uint32_t> tok(n);
    std::vector<uint32_t> slot(SLOT_BYTES / 4, 0u);
    State *S = new State;
    HostWave w;
    Deflater<HostWave> D(w, S, src.data(), n, slot.data(), tok.data());
    const uint32_t bytes = D.run();
    delete S;
    memcpy(out, slot.data(), SLOT_BYTES);
    if (tokens) memcpy(tokens, tok.data(), 4 * (size_t)D.n_tok);
    if (n_tokens) *n_tokens = D.n_tok;
    return (int)bytes;
}

// The code construction alone: the histogram of n_sym <= 286 symbols -> code lengths and (bit-reversed) canonical codes.
extern "C" int coral_test_code_lengths(const uint32_t *freq, int n_sym, uint8_t *lens, uint16_t *codes) {
    if (n_sym < 0 || n_sym > N_LL) return -1;
    State *S = new State;
    memset(S, 0, sizeof(State));
    for (int s = 0; s < n_sym; ++s) S->ll_freq[s] = freq[s];
    HostWave w;
    Deflater<HostWave> D(w, S, nullptr, 0, nullptr, nullptr);
    D.build_code(S->ll_freq, n_sym, S->ll_len, S->ll_code);
    memcpy(lens, S->ll_len, (size_t)n_sym);
    memcpy(codes, S->ll_code, 2 * (size_t)n_sym);
    delete S;
    return 0;
}

#ifdef DEFLATE_HOST_MAIN
static int code_length_checks() {        // the 15-bit limit on the Fibonacci histogram, under the sanitizers too
    uint32_t freq[N_LL] = {1, 1};
    for (int s = 2; s < 22; ++s) freq[s] = freq[s - 1] + freq[s - 2];
    uint8_t lens[N_LL];
    uint16_t codes[N_LL];
    if (coral_test_code_lengths(freq, N_LL, lens, codes) != 0) return 1;
    uint32_t kraft = 0, longest = 0;
    for (int s = 0; s < 22; ++s) {
        if (!lens[s] || lens[s] > MAX_BITS) return 1;
        kraft += 1u << (MAX_BITS - lens[s]);
        if (lens[s] > longest) longest = lens[s];
    }
    return kraft == (1u << MAX_BITS) && longest == MAX_BITS ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    if (code_length_checks() != 0) return 8;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 3;
    std::vector<uint8_t> out(SLOT_BYTES);
    uint32_t n, cases = 0;
    while (fread(&n, 4, 1, fi) == 1) {
        std::vector<uint8_t> data(n);
        if (n && fread(data.data(), 1, n, fi) != n) return 4;
        uint32_t n_tok = 0;
        const int bytes = coral_test_deflate(data.data(), n, out.data(), nullptr, &n_tok);
        if (bytes < 0 || n_tok > n) return 5;
        const uint32_t b = (uint32_t)bytes;
        if (fwrite(&b, 4, 1, fo) != 1 || fwrite(out.data(), 1, b, fo) != b) return 6;
        ++cases;
    }
    fclose(fi);
    if (fclose(fo) != 0) return 7;
    printf("deflate_host: %u cases\n", cases);
    return 0;
}
#endif
