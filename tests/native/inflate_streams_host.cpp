// The three host loops of the DEFLATE core (inflate_host.cpp) over a file of hand-built streams, stand-alone, for a sanitizer
// run on the CPU (never loaded into Python, never on a GPU):
//   python -m tests.deflate_streams streams.bin
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/inflate_streams_host.cpp -o inflate_streams_host
//   ./inflate_streams_host streams.bin
// File: per entry  u32 length, `length` stream bytes, u32 size, u8 valid, and `size` bytes of text when valid.  Stream and output
// live in heap blocks of exactly their size, so a read or write beyond either is an error here.  Exit 0: every valid stream gave
// (OK, its text) and every other one a status that is not OK, in all three loops.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "inflate_host.cpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    int n = 0, wrong = 0;
    for (;;) {
        uint32_t len, size;
        uint8_t valid;
        if (fread(&len, 4, 1, fp) != 1) break;
        std::vector<uint8_t> comp(len);
        if (len && fread(comp.data(), 1, len, fp) != len) return 2;
        if (fread(&size, 4, 1, fp) != 1 || fread(&valid, 1, 1, fp) != 1) return 2;
        std::vector<uint8_t> text(valid ? size : 0);
        if (valid && size && fread(text.data(), 1, size, fp) != size) return 2;
        for (int loop = 0; loop < 3; ++loop) {
            std::vector<uint8_t> out(size);
            int produced = -1;
            const int rc = coral_test_inflate(comp.data(), (long long)len, out.data(), (int)size, &produced, loop);
            const bool ok = valid ? (rc == OK && produced == (int)size && (size == 0 || memcmp(out.data(), text.data(), size) == 0))
                                  : (rc != OK && produced <= (int)size);
            if (!ok) {
                printf("entry %d loop %d: rc %d, %d of %u bytes (%s)\n", n, loop, rc, produced, size, valid ? "valid" : "to be refused");
                ++wrong;
            }
        }
        ++n;
    }
    fclose(fp);
    printf("%d streams, 3 loops each, %d wrong\n", n, wrong);
    return wrong ? 1 : 0;
}
