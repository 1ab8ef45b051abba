// The SAM -> BAM encoding core (coral_amd/csrc/coral_sam_core.h) compiled for the HOST, lanes as loops: what
// tests/test_sam_core.py compares with its plain-Python restatement of the rules.  No HIP, no GPU: g++ alone builds it.
//
//   coral_test_sam        a whole SAM text -> the inflated BAM stream (header, records), or the refused line and its field
//   coral_test_sam_float  one decimal -> how the core converts it (1: the exact fast path, 2: left to strtof, 0: refused) and the bits
//
// With -DSAM_HOST_MAIN it is a stand-alone program for a sanitizer run: sam_host <cases> <results> reads texts (each in an
// allocation of exactly its size: the parser reads attacker-shaped text, and an over-read at a line's end is the bug to expect)
// and writes what coral_test_sam gives for each.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../coral_amd/csrc/coral_sam_host.h"

using namespace coral_sam;

// res[0..7] = rc (0 good, 1 a refused line, 2 out too short, 3 a refused header), header bytes, record bytes, lines, written,
// dropped, the refused line, its field.  out: header + records.
extern "C" int coral_test_sam(const uint8_t *text, int64_t n, const int32_t *keep, uint8_t *out, int64_t out_cap, int64_t *res) {
    for (int k = 0; k < 8; ++k) res[k] = 0;
    Header H;
    std::string err;
    if (!parse_header(text, n, H, err)) return (int)(res[0] = 3);
    res[1] = (int64_t)H.bam.size();
    if ((int64_t)H.bam.size() > out_cap) return (int)(res[0] = 2);
    memcpy(out, H.bam.data(), H.bam.size());
    const Keep K{(uint32_t)keep[0], (uint32_t)keep[1], (uint32_t)keep[2], (uint32_t)keep[3]};
    EncodeCounts X;
    const int rc = encode_text(text + H.text_bytes, n - H.text_bytes, H.n_lines + 1, H.contigs(), K, out + H.bam.size(), out_cap - (int64_t)H.bam.size(), X);
    res[0] = rc; res[2] = X.out_bytes; res[3] = X.lines; res[4] = X.written; res[5] = X.dropped; res[6] = X.err_line; res[7] = X.err_field;
    return rc;
}

extern "C" int coral_test_sam_float(const uint8_t *text, uint32_t n, uint32_t *bits) {
    uint32_t b = 0;
    const int how = parse_float(text, 0, n, b);
    *bits = how == 2 ? HostLanes::strtof_bits(text, n) : b;
    return how;
}

#ifdef SAM_HOST_MAIN
int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: sam_host <cases> <results>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "sam_host: cannot open the files\n"); return 2; }
    int n_cases = 0;
    for (;;) {
        uint32_t n;
        int32_t keep[4];
        if (fread(&n, 4, 1, in) != 1) break;
        uint8_t *text = (uint8_t *)malloc(n ? n : 1);                 // exactly the text: a read behind it is the sanitizer's to find
        if ((n && fread(text, 1, n, in) != n) || fread(keep, 4, 4, in) != 4) { fprintf(stderr, "sam_host: truncated cases\n"); return 2; }
        size_t lines = 1;
        for (uint32_t i = 0; i < n; ++i) lines += text[i] == '\n';
        const int64_t cap = (int64_t)(3 * (size_t)n + 36 * lines + 64);
        std::vector<uint8_t> buf((size_t)cap);
        int64_t res[8];
        coral_test_sam(text, n, keep, buf.data(), cap, res);
        const int64_t bytes = res[0] == 0 ? res[1] + res[2] : 0;
        fwrite(res, 8, 8, out);
        fwrite(buf.data(), 1, (size_t)bytes, out);
        free(text);
        ++n_cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("sam_host: %d cases\n", n_cases);
    return 0;
}
#endif
