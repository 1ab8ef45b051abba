// Stand-alone host build of the host BAM pipeline (coral_amd/csrc/coral_bam.cpp with the shared rules of coral_bam_common.h) for a
// sanitizer run of the record filter: decodes a BAM file without a filter and with one and prints the record counts.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/record_filter_host.cpp -lz -lpthread
//   ./a.out FILE.bam MIN_MAPQ MIN_SEQ_LENGTH REQUIRE_FLAGS EXCLUDE_FLAGS [THREADS]
// Test infrastructure, never part of libcoral_hip.so.
#include "../../coral_amd/csrc/coral_bam.cpp"

static long long decode(const char *path, int threads, const coral_bam_request_t &q, long long *reads, long long depth_sum[2]) {
    void *h = nullptr;
    const int rc = coral_bam_decode_request(path, threads, &q, &h);
    if (rc != CORAL_OK) { fprintf(stderr, "decode failed (%d): %s\n", rc, coral_bam_last_error()); exit(2); }
    int64_t sz[8], qsz[2], dsz[2];
    if (coral_bam_decode_sizes(h, sz) != CORAL_OK || coral_bam_qc_sizes(h, qsz) != CORAL_OK || coral_bam_depth_sizes(h, dsz) != CORAL_OK) exit(3);
    std::vector<int64_t> off((size_t)dsz[0] + 1), bases((size_t)dsz[1]), n_reads((size_t)dsz[1]);
    if (coral_bam_depth_fill(h, off.data(), bases.data(), n_reads.data()) != CORAL_OK) exit(4);
    depth_sum[0] = depth_sum[1] = 0;
    for (int64_t v : bases) depth_sum[0] += v;
    for (int64_t v : n_reads) depth_sum[1] += v;
    *reads = qsz[1];
    coral_bam_decode_close(h);
    return sz[0];
}

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s FILE.bam MIN_MAPQ MIN_SEQ_LENGTH REQUIRE_FLAGS EXCLUDE_FLAGS [THREADS]\n", argv[0]); return 1; }
    const int threads = argc > 6 ? atoi(argv[6]) : 3;
    for (int world = 1; world <= 3; world += 2) {
        long long total[2] = {0, 0};
        for (int filtered = 0; filtered < 2; ++filtered)
            for (int rank = 0; rank < world; ++rank) {
                coral_bam_request_t q = range_request(rank, world);
                q.want_qc = 1;
                q.depth_bin = 1000;
                if (filtered) {
                    q.keep_min_mapq = (int32_t)strtol(argv[2], nullptr, 0);
                    q.keep_min_seq_length = (int32_t)strtol(argv[3], nullptr, 0);
                    q.keep_require_flags = (int32_t)strtol(argv[4], nullptr, 0);
                    q.keep_exclude_flags = (int32_t)strtol(argv[5], nullptr, 0);
                }
                long long reads = 0, depth[2];
                const long long n = decode(argv[1], threads, q, &reads, depth);
                total[filtered] += n;
                printf("world %d rank %d %s: %lld records, %lld reads, depth bases %lld, depth reads %lld\n", world, rank,
                       filtered ? "filtered" : "unfiltered", n, reads, depth[0], depth[1]);
            }
        printf("world %d: %lld records unfiltered, %lld kept\n", world, total[0], total[1]);
    }
    return 0;
}
