// The copy-number segmenter's host backend (coral_amd/csrc/coral_cn_host.h over coral_cn_core.h) as a stand-alone program for a
// sanitizer run: cnv_host <cases> <results> reads the tables that tests/cnv_cases.py packs (each array in an allocation of exactly
// its size: a read one entry past a contig's prefix sums, or past the last bin, is the bug to expect) and writes the counts and
// the rows of each.  No HIP, no GPU: g++ alone builds it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../coral_amd/csrc/coral_cn_host.h"

using namespace coral_cn;

template <class T>
static T *read_array(FILE *in, size_t n) {
    T *p = (T *)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "cnv_host: truncated cases\n"); exit(2); }
    return p;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: cnv_host <cases> <results>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cnv_host: cannot open the files\n"); return 2; }
    int n_cases = 0;
    for (;;) {
        int32_t n_contigs, levels, has_ref;
        int64_t bin_size;
        double q;
        if (fread(&n_contigs, 4, 1, in) != 1) break;
        if (fread(&bin_size, 8, 1, in) != 1 || fread(&levels, 4, 1, in) != 1 || fread(&has_ref, 4, 1, in) != 1 || fread(&q, 8, 1, in) != 1) { fprintf(stderr, "cnv_host: truncated cases\n"); return 2; }
        int64_t *bin_off = read_array<int64_t>(in, (size_t)n_contigs + 1), *lengths = read_array<int64_t>(in, (size_t)n_contigs);
        uint8_t *centre = read_array<uint8_t>(in, (size_t)n_contigs);
        const size_t n_bins = (size_t)bin_off[n_contigs];
        int64_t *bases = read_array<int64_t>(in, n_bins), *ref = has_ref ? read_array<int64_t>(in, n_bins) : nullptr;
        const Table T{n_contigs, bin_off, lengths, bin_size, bases, ref, centre};
        if (!table_ok(T, levels, q)) { fprintf(stderr, "cnv_host: case %d is not a table\n", n_cases); return 2; }
        Rows R;
        Counts X;
        segment_host(T, levels, q, R, X);
        const int64_t counts[5] = {X.rows, X.kept, X.centre, X.ref_centre, X.breakpoints};
        fwrite(counts, 8, 5, out);
        if (R.size()) {
            fwrite(R.contig.data(), 4, R.size(), out);
            for (const std::vector<int64_t> *v : {&R.start, &R.end, &R.probes, &R.sum_s, &R.sum_bases}) fwrite(v->data(), 8, R.size(), out);
        }
        free(bin_off); free(lengths); free(centre); free(bases); free(ref);
        ++n_cases;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("cnv_host: %d cases\n", n_cases);
    return 0;
}
