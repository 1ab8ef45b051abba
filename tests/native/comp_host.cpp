// The host backend of the reference's per-bin composition (coral_amd/csrc/coral_comp_host.h over coral_comp_core.h) as a
// stand-alone program for a sanitizer run: comp_host <cases> <results> reads the cases that tests/test_comp_core.py packs (bin_size,
// the FASTA bytes) and counts each of them whole and in awkward pieces, every piece in an allocation of exactly its size (a read
// one byte in front of or behind a piece is the bug to expect); all must agree.  It also holds scan_piece - the host's share of
// the device path - against the byte-by-byte rule: the pieces it cuts, blanked as the device session blanks them and counted
// stretch by stretch as the kernels do, must give the same contigs, names and tables.  It writes each case's contigs and tables.
// No HIP, no GPU: g++ alone builds it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../coral_amd/csrc/coral_comp_host.h"

using namespace coral_comp;

static const size_t PIECES[] = {0, 1, 7, 16, 17};      // 0: the whole text

struct Result {
    std::vector<uint32_t> gc, at, masked;
    std::vector<int64_t> lengths;
    std::string names;
    std::vector<int64_t> name_off;
    uint64_t bins = 0, positions = 0;
    bool operator==(const Result &o) const {
        return gc == o.gc && at == o.at && masked == o.masked && lengths == o.lengths && names == o.names && name_off == o.name_off && bins == o.bins && positions == o.positions;
    }
};

static uint8_t *exact_copy(const uint8_t *p, size_t n) {
    uint8_t *q = (uint8_t *)malloc(n ? n : 1);
    memcpy(q, p, n);
    return q;
}

static Result count_in_pieces(const std::vector<uint8_t> &text, int64_t bin_size, size_t capacity, size_t piece) {
    Result r;
    r.gc.assign(capacity, 0); r.at.assign(capacity, 0); r.masked.assign(capacity, 0);
    HostComposer hc(bin_size, r.gc.data(), r.at.data(), r.masked.data(), (int64_t)capacity);
    const size_t step = piece ? piece : (text.size() ? text.size() : 1);
    for (size_t at = 0; at < text.size(); at += step) {
        const size_t n = text.size() - at < step ? text.size() - at : step;
        uint8_t *p = exact_copy(text.data() + at, n);
        if (hc.feed(p, n) != COMP_OK) { fprintf(stderr, "comp_host: refused\n"); exit(2); }
        free(p);
    }
    if (hc.finish() != COMP_OK) { fprintf(stderr, "comp_host: refused at the end\n"); exit(2); }
    r.lengths = hc.lengths; r.names = hc.names.blob; r.name_off = hc.names.off; r.bins = hc.st.bins; r.positions = hc.st.positions;
    return r;
}

// the device session's path with the kernels' work done by a plain loop: pieces of at most `piece` bytes and `max_bounds` headers
static Result count_as_the_device_does(const std::vector<uint8_t> &text, int64_t bin_size, size_t capacity, size_t piece, size_t max_bounds) {
    Result r;
    r.gc.assign(capacity, 0); r.at.assign(capacity, 0); r.masked.assign(capacity, 0);
    LineState line;
    Names names;
    bool started = false;
    std::vector<uint32_t> bounds;
    std::vector<std::pair<uint32_t, uint32_t>> blanks;
    uint64_t cur_len = 0, bin_base = 0;
    const size_t step = piece ? piece : (text.size() ? text.size() : 1);
    for (size_t at = 0; at < text.size();) {
        const size_t n = text.size() - at < step ? text.size() - at : step;
        uint8_t *src = exact_copy(text.data() + at, n);
        const bool open_before = started;
        int e = COMP_OK;
        const size_t m = scan_piece(line, names, started, src, n, max_bounds, bounds, blanks, &e);
        if (e != COMP_OK || m == 0 || m > n || bounds.size() > max_bounds) { fprintf(stderr, "comp_host: scan_piece refused or took nothing\n"); exit(2); }
        uint8_t *buf = exact_copy(src, m);
        free(src);
        for (const auto &b : blanks) {
            if (b.first > b.second || b.second > m) { fprintf(stderr, "comp_host: a blank range outside the piece\n"); exit(2); }
            memset(buf + b.first, '\n', b.second - b.first);
        }
        size_t next = 0;
        for (size_t i = 0; i < m; ++i) {
            if (next < bounds.size() && bounds[next] == i) {
                if (next > 0 || open_before) { r.lengths.push_back((int64_t)cur_len); bin_base += bins_of(cur_len, (uint64_t)bin_size); }
                else if (cur_len) { fprintf(stderr, "comp_host: positions in front of the first header\n"); exit(2); }
                cur_len = 0;
                ++next;
            }
            if (!is_position(buf[i])) continue;
            const uint64_t bin = bin_base + cur_len / (uint64_t)bin_size;
            const uint32_t cls = classes(buf[i]);
            if (bin < capacity) { r.gc[bin] += cls & CLS_GC ? 1 : 0; r.at[bin] += cls & CLS_AT ? 1 : 0; r.masked[bin] += cls & CLS_MASKED ? 1 : 0; }
            ++cur_len; ++r.positions;
        }
        if (next != bounds.size()) { fprintf(stderr, "comp_host: a header offset outside the piece or out of order\n"); exit(2); }
        free(buf);
        at += m;
    }
    if (names.in_line && !names.close_line()) { fprintf(stderr, "comp_host: an empty name at the end\n"); exit(2); }
    if (started) { r.lengths.push_back((int64_t)cur_len); bin_base += bins_of(cur_len, (uint64_t)bin_size); }
    r.names = names.blob; r.name_off = names.off; r.bins = bin_base;
    return r;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: comp_host <cases> <results>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "comp_host: cannot open the files\n"); return 2; }
    int n_cases = 0;
    for (;;) {
        int64_t bin_size, len;
        if (fread(&bin_size, 8, 1, in) != 1) break;
        if (fread(&len, 8, 1, in) != 1 || !bin_size_ok(bin_size) || len < 0) { fprintf(stderr, "comp_host: bad cases\n"); return 2; }
        std::vector<uint8_t> text((size_t)len);
        if (len && fread(text.data(), 1, (size_t)len, in) != (size_t)len) { fprintf(stderr, "comp_host: truncated cases\n"); return 2; }
        const Result sized = count_in_pieces(text, bin_size, 1, 0);          // (a capacity of one bin: the rest is counted, not written)
        const size_t capacity = (size_t)sized.bins ? (size_t)sized.bins : 1;
        const Result whole = count_in_pieces(text, bin_size, capacity, 0);
        if (whole.bins != sized.bins || whole.lengths != sized.lengths || (sized.bins && whole.gc[0] != sized.gc[0])) { fprintf(stderr, "comp_host: case %d differs at a capacity of 1\n", n_cases); return 1; }
        for (size_t piece : PIECES) {
            if (piece == 1 && text.size() > 100000) continue;
            if (!(count_in_pieces(text, bin_size, capacity, piece) == whole)) { fprintf(stderr, "comp_host: case %d differs in pieces of %zu\n", n_cases, piece); return 1; }
            for (size_t max_bounds : {(size_t)1, (size_t)3, (size_t)1024})
                if (!(count_as_the_device_does(text, bin_size, capacity, piece, max_bounds) == whole)) {
                    fprintf(stderr, "comp_host: case %d: scan_piece differs in pieces of %zu with %zu headers a piece\n", n_cases, piece, max_bounds);
                    return 1;
                }
        }
        const int64_t head[2] = {(int64_t)whole.lengths.size(), (int64_t)whole.bins};
        fwrite(head, 8, 2, out);
        if (head[0]) fwrite(whole.lengths.data(), 8, (size_t)head[0], out);
        if (head[1]) { fwrite(whole.gc.data(), 4, (size_t)head[1], out); fwrite(whole.at.data(), 4, (size_t)head[1], out); fwrite(whole.masked.data(), 4, (size_t)head[1], out); }
        std::string names;
        for (size_t c = 0; c + 1 < whole.name_off.size(); ++c) names += whole.names.substr((size_t)whole.name_off[c], (size_t)(whole.name_off[c + 1] - whole.name_off[c])) + "\n";
        const int64_t nb = (int64_t)names.size();
        fwrite(&nb, 8, 1, out);
        if (nb) fwrite(names.data(), 1, (size_t)nb, out);
        ++n_cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("comp_host: %d cases\n", n_cases);
    return 0;
}
