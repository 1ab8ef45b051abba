// The k-mer counter's host backend (coral_amd/csrc/coral_kmer_host.h over coral_kmer_core.h) as a stand-alone program for a
// sanitizer run: kmer_host <cases> <results> reads the cases that tests/test_kmer_core.py packs (k, canonical, the FASTA bytes) and
// counts each of them whole and in awkward pieces, every piece in an allocation of exactly its size (a read one byte in front of
// or behind a piece is the bug to expect); all must agree.  It also holds mask_headers - the host's share of the device path -
// against the byte-by-byte rule on the same pieces.  It writes the statistics and the non-zero entries of each case.
// No HIP, no GPU: g++ alone builds it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../coral_amd/csrc/coral_kmer_host.h"

using namespace coral_kmer;

static const size_t PIECES[] = {0, 1, 7, 16, 17, 4096, 4097};      // 0: the whole text

struct Result {
    std::vector<uint32_t> table;
    Stats st;
};

static Result count_in_pieces(const std::vector<uint8_t> &text, int k, bool canonical, size_t piece) {
    Result r;
    r.table.assign((size_t)table_entries(k), 0);
    HostCounter hc(k, canonical, r.table.data(), 0);
    const size_t step = piece ? piece : (text.size() ? text.size() : 1);
    for (size_t at = 0; at < text.size(); at += step) {
        const size_t n = text.size() - at < step ? text.size() - at : step;
        uint8_t *p = (uint8_t *)malloc(n);
        memcpy(p, text.data() + at, n);
        if (!hc.feed(p, n)) { fprintf(stderr, "kmer_host: refused\n"); exit(2); }
        free(p);
    }
    r.st = hc.st;
    std::map<uint64_t, uint64_t> hist;
    table_histogram(r.table.data(), k, r.st, hist);
    return r;
}

// the kept symbols of the text: by next_symbol, and by mask_headers + classify on pieces
static bool masked_stream_agrees(const std::vector<uint8_t> &text, size_t piece) {
    std::vector<uint8_t> want, got;
    LineState a;
    uint64_t headers_a = 0, headers_b = 0;
    for (uint8_t c : text) {
        bool header;
        const uint8_t s = next_symbol(a, c, &header);
        headers_a += header;
        if (s != SYM_SKIP) want.push_back(s);
    }
    LineState b;
    const size_t step = piece ? piece : (text.size() ? text.size() : 1);
    for (size_t at = 0; at < text.size(); at += step) {
        const size_t n = text.size() - at < step ? text.size() - at : step;
        uint8_t *p = (uint8_t *)malloc(n);
        memcpy(p, text.data() + at, n);
        headers_b += mask_headers(b, p, n);
        for (size_t i = 0; i < n; ++i) if (classify(p[i]) != SYM_SKIP) got.push_back(classify(p[i]));
        free(p);
    }
    return want == got && headers_a == headers_b && a.in_header == b.in_header && (a.in_header || a.line_start == b.line_start);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: kmer_host <cases> <results>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "kmer_host: cannot open the files\n"); return 2; }
    int n_cases = 0;
    for (;;) {
        int32_t k, canonical;
        int64_t len;
        if (fread(&k, 4, 1, in) != 1) break;
        if (fread(&canonical, 4, 1, in) != 1 || fread(&len, 8, 1, in) != 1 || !k_ok(k) || len < 0) { fprintf(stderr, "kmer_host: bad cases\n"); return 2; }
        std::vector<uint8_t> text((size_t)len);
        if (len && fread(text.data(), 1, (size_t)len, in) != (size_t)len) { fprintf(stderr, "kmer_host: truncated cases\n"); return 2; }
        const Result whole = count_in_pieces(text, k, canonical != 0, 0);
        for (size_t piece : PIECES) {
            if (piece == 1 && text.size() > 100000) continue;
            const Result r = count_in_pieces(text, k, canonical != 0, piece);
            if (r.table != whole.table || r.st.n_sequences != whole.st.n_sequences || r.st.n_bases != whole.st.n_bases || r.st.total != whole.st.total ||
                r.st.distinct != whole.st.distinct) { fprintf(stderr, "kmer_host: case %d differs in pieces of %zu\n", n_cases, piece); return 1; }
            if (!masked_stream_agrees(text, piece)) { fprintf(stderr, "kmer_host: case %d: mask_headers differs in pieces of %zu\n", n_cases, piece); return 1; }
        }
        std::vector<uint64_t> kmers((size_t)whole.st.distinct);
        std::vector<uint32_t> counts((size_t)whole.st.distinct);
        const uint64_t m = table_select(whole.table.data(), k, 0, whole.st.distinct, kmers.data(), counts.data());
        if (m != whole.st.distinct) { fprintf(stderr, "kmer_host: case %d: select and distinct disagree\n", n_cases); return 1; }
        const int64_t head[5] = {(int64_t)whole.st.n_sequences, (int64_t)whole.st.n_bases, (int64_t)whole.st.total, (int64_t)whole.st.distinct, (int64_t)whole.st.max_count};
        fwrite(head, 8, 5, out);
        if (m) { fwrite(kmers.data(), 8, (size_t)m, out); fwrite(counts.data(), 4, (size_t)m, out); }
        ++n_cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("kmer_host: %d cases\n", n_cases);
    return 0;
}
