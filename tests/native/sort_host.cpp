// Stand-alone host build of the host BAM pipeline (coral_amd/csrc/coral_bam.cpp with the shared rules of coral_bam_common.h) for a
// sanitizer run of the coordinate order (reads_order = 1 of a coral_bam_request_t) and of coral_bam_records_merge:
// decodes a BAM file in coordinate order - whole, and as 3 byte ranges whose sorted results are merged (the bytes must be equal
// and in key order) -, merges with 1 and 4 threads (equal bytes), and runs the merge's edge shapes: no run, one run, an empty run
// between two others, a tie between runs, the refused arguments.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/sort_host.cpp -lz -lpthread
//   ./a.out FILE.bam
// Test infrastructure, never part of libcoral_hip.so; run on the CPU only.
#include "../../coral_amd/csrc/coral_bam.cpp"

struct Got { std::vector<uint8_t> data; std::vector<int64_t> off; };

static Got records(const char *path, coral_bam_request_t q, int order) {
    void *h = nullptr;
    q.want_reads = 2;
    q.reads_order = order;
    const int rc = coral_bam_decode_request(path, 3, &q, &h);
    if (rc != CORAL_OK) { fprintf(stderr, "decode of %s failed (%d): %s\n", path, rc, coral_bam_last_error()); exit(2); }
    int64_t sz[2];
    if (coral_bam_reads_sizes(h, sz) != CORAL_OK) exit(3);
    Got g;
    g.data.resize((size_t)sz[1]);
    g.off.resize((size_t)sz[0] + 1);
    if (coral_bam_reads_fill(h, g.data.data(), g.off.data()) != CORAL_OK) exit(4);
    coral_bam_decode_close(h);
    return g;
}

static int merged(const std::vector<const Got *> &runs, int n_threads, Got &out) {
    std::vector<const uint8_t *> data;
    std::vector<const int64_t *> off;
    std::vector<int64_t> n;
    size_t bytes = 0, total = 0;
    for (const Got *g : runs) {
        data.push_back(g->data.data());
        off.push_back(g->off.data());
        n.push_back((int64_t)g->off.size() - 1);
        bytes += g->data.size();
        total += g->off.size() - 1;
    }
    out.data.assign(bytes, 0xab);
    out.off.assign(total + 1, -1);
    return coral_bam_records_merge((int32_t)runs.size(), data.data(), off.data(), n.data(), out.data.data(), out.off.data(), n_threads);
}

static bool in_key_order(const Got &g) {
    for (size_t k = 2; k < g.off.size(); ++k)
        if (reads_sort_key_at(g.data.data() + g.off[k - 1]) < reads_sort_key_at(g.data.data() + g.off[k - 2])) return false;
    return true;
}

static Got one_record(int32_t tid, int32_t pos, uint16_t flag, const char *name) {
    std::vector<uint8_t> r;
    const uint32_t l_name = (uint32_t)strlen(name) + 1;
    put32(r, 32 + l_name); put32(r, (uint32_t)tid); put32(r, (uint32_t)pos);
    r.push_back((uint8_t)l_name); r.push_back(30); r.push_back(0x48); r.push_back(0x12);      // l_read_name, mapq, bin 4680
    r.push_back(0); r.push_back(0); r.push_back((uint8_t)(flag & 0xff)); r.push_back((uint8_t)(flag >> 8));
    put32(r, 0); put32(r, 0xffffffffu); put32(r, 0xffffffffu); put32(r, 0);
    r.insert(r.end(), name, name + l_name);
    Got g;
    g.data = r;
    g.off = {0, (int64_t)r.size()};
    return g;
}

static Got joined(const std::vector<Got> &recs) {
    Got g;
    g.off.push_back(0);
    for (const Got &r : recs) { g.data.insert(g.data.end(), r.data.begin(), r.data.end()); g.off.push_back((int64_t)g.data.size()); }
    return g;
}

static std::string name_at(const Got &g, size_t k) { return std::string((const char *)g.data.data() + g.off[k] + 36); }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s FILE.bam\n", argv[0]); return 1; }
    const Got file_order = records(argv[1], range_request(0, 1), 0), all = records(argv[1], range_request(0, 1), 1);
    if (all.data.size() != file_order.data.size() || all.off.size() != file_order.off.size() || !in_key_order(all)) { fprintf(stderr, "the ordered decode is not a sorted permutation\n"); return 5; }
    std::vector<Got> parts;
    for (int rank = 0; rank < 3; ++rank) parts.push_back(records(argv[1], range_request(rank, 3), 1));
    Got m1, m4;
    if (merged({&parts[0], &parts[1], &parts[2]}, 1, m1) != CORAL_OK || merged({&parts[0], &parts[1], &parts[2]}, 4, m4) != CORAL_OK) { fprintf(stderr, "merge: %s\n", coral_bam_last_error()); return 6; }
    if (m1.data != m4.data || m1.off != m4.off) { fprintf(stderr, "the merged bytes depend on the thread count\n"); return 7; }
    if (m1.data != all.data || m1.off != all.off) { fprintf(stderr, "3 sorted byte ranges do not merge to the sorted whole\n"); return 8; }
    printf("%zu records, %zu bytes in coordinate order; 3 sorted byte ranges merge to the same with 1 and 4 threads\n", all.off.size() - 1, all.data.size());
    // edge shapes
    Got none;
    if (merged({}, 2, none) != CORAL_OK || none.off != std::vector<int64_t>{0}) return 9;
    Got single;
    if (merged({&all}, 4, single) != CORAL_OK || single.data != all.data || single.off != all.off) return 10;
    const Got a = joined({one_record(0, 5, 0, "a0"), one_record(0, 9, 0, "tie_first"), one_record(-1, -1, 4, "un0")});
    const Got empty = joined({});
    const Got b = joined({one_record(0, 9, 0, "tie_second"), one_record(0, 9, 0x10, "rev"), one_record(1, 0, 0, "b1")});
    Got e1, e4;
    if (merged({&a, &empty, &b}, 1, e1) != CORAL_OK || merged({&a, &empty, &b}, 4, e4) != CORAL_OK || e1.data != e4.data || e1.off != e4.off) return 11;
    const char *want[] = {"a0", "tie_first", "tie_second", "rev", "b1", "un0"};
    for (size_t k = 0; k < 6; ++k)
        if (name_at(e1, k) != want[k]) { fprintf(stderr, "merged record %zu is %s, not %s\n", k, name_at(e1, k).c_str(), want[k]); return 12; }
    // refusals: a negative run count, no offsets for the result, reads_order outside 0..1, coordinate order of FASTQ text
    int64_t off0 = 0;
    if (coral_bam_records_merge(-1, nullptr, nullptr, nullptr, nullptr, &off0, 1) != CORAL_ERR_ARG || coral_bam_records_merge(0, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != CORAL_ERR_ARG) return 13;
    void *h = nullptr;
    coral_bam_request_t q = range_request(0, 1);
    q.want_reads = 2;
    q.reads_order = 2;
    if (coral_bam_decode_request(argv[1], 1, &q, &h) != CORAL_ERR_ARG || !strstr(coral_bam_last_error(), "reads_order")) return 14;
    q.want_reads = 1;
    q.reads_order = 1;
    if (coral_bam_decode_request(argv[1], 1, &q, &h) != CORAL_ERR_ARG || !strstr(coral_bam_last_error(), "reads_order")) return 15;
    printf("ok\n");
    return 0;
}
