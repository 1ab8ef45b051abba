// Stand-alone host build of the host BAM pipeline (coral_amd/csrc/coral_bam.cpp with the shared rules of coral_bam_common.h) for a
// sanitizer run of the records request (want_reads = 2: a memcpy per written record) and of coral_bgzf_write: decodes a BAM file
// with the request - whole, as 3 byte ranges, with a flag excluded and a name list -, writes header + records with coral_bgzf_write
// at levels 0, 1 and 9 with 1 and 4 threads (the files must be equal), and decodes what it wrote (the bytes must come back).
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/records_write_host.cpp -lz -lpthread
//   ./a.out FILE.bam OUT_PREFIX [EXCLUDE_FLAGS] [NAME ...]         (names sorted ascending by their bytes)
// Test infrastructure, never part of libcoral_hip.so; run on the CPU only.
#include "../../coral_amd/csrc/coral_bam.cpp"

struct Got { std::vector<uint8_t> data; std::vector<int64_t> off; };

static Got records(const char *path, coral_bam_request_t q) {
    void *h = nullptr;
    q.want_reads = 2;
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

static std::vector<uint8_t> file_bytes(const std::string &path) {
    std::vector<uint8_t> out;
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) exit(5);
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) out.insert(out.end(), buf, buf + n);
    fclose(fp);
    return out;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s FILE.bam OUT_PREFIX [EXCLUDE_FLAGS] [NAME ...]\n", argv[0]); return 1; }
    const Got all = records(argv[1], range_request(0, 1));
    Got joined;
    joined.off.push_back(0);
    for (int rank = 0; rank < 3; ++rank) {
        const Got part = records(argv[1], range_request(rank, 3));
        joined.data.insert(joined.data.end(), part.data.begin(), part.data.end());
        for (size_t k = 1; k < part.off.size(); ++k) joined.off.push_back(joined.off.back() + part.off[k] - part.off[k - 1]);
    }
    if (joined.data != all.data || joined.off != all.off) { fprintf(stderr, "the byte ranges do not concatenate to the whole\n"); return 6; }
    printf("%zu records, %zu bytes; 3 byte ranges concatenate to the same\n", all.off.size() - 1, all.data.size());
    // a header of its own with the file's contigs (coral_bgzf_write takes any bytes)
    MappedFile f;
    Decoded D;
    RefIds ids;
    size_t hdr = 0;
    if (!f.open(argv[1], D.error) || !read_bam_header(f, D, ids, &hdr)) { fprintf(stderr, "header: %s\n", D.error.c_str()); return 7; }
    std::vector<uint8_t> head;
    {
        std::vector<uint8_t> text = {'B', 'A', 'M', 1};
        std::string sam = "@HD\tVN:1.6\n";
        put32(text, (uint32_t)sam.size());
        text.insert(text.end(), sam.begin(), sam.end());
        put32(text, (uint32_t)D.ref_names.size());
        for (size_t r = 0; r < D.ref_names.size(); ++r) {
            put32(text, (uint32_t)D.ref_names[r].size() + 1);
            text.insert(text.end(), D.ref_names[r].c_str(), D.ref_names[r].c_str() + D.ref_names[r].size() + 1);
            put32(text, (uint32_t)D.ref_lens[r]);
        }
        head = text;
    }
    coral_bam_request_t sel = range_request(0, 1);
    std::vector<uint8_t> blob;
    std::vector<int64_t> name_off{0};
    if (argc > 3) sel.reads_exclude_flags = (int32_t)strtol(argv[3], nullptr, 0);
    for (int a = 4; a < argc; ++a) { blob.insert(blob.end(), argv[a], argv[a] + strlen(argv[a])); name_off.push_back((int64_t)blob.size()); }
    blob.push_back(0);
    if (argc > 4) { sel.reads_n_names = argc - 4; sel.reads_names = blob.data(); sel.reads_name_off = name_off.data(); }
    const Got some = records(argv[1], sel);
    printf("selection: %zu records, %zu bytes\n", some.off.size() - 1, some.data.size());
    for (const Got *g : {&all, &some}) {
        const uint8_t *parts[2] = {head.data(), g->data.data()};
        const int64_t sizes[2] = {(int64_t)head.size(), (int64_t)g->data.size()};
        for (int level : {0, 1, 9}) {
            const std::string one = std::string(argv[2]) + ".t1.bam", four = std::string(argv[2]) + ".t4.bam";
            if (coral_bgzf_write(one.c_str(), parts, sizes, 2, level, 1) != CORAL_OK || coral_bgzf_write(four.c_str(), parts, sizes, 2, level, 4) != CORAL_OK) {
                fprintf(stderr, "coral_bgzf_write: %s\n", coral_bam_last_error());
                return 8;
            }
            const std::vector<uint8_t> a = file_bytes(one), b = file_bytes(four);
            if (a != b) { fprintf(stderr, "level %d: the bytes depend on the thread count\n", level); return 9; }
            const Got back = records(one.c_str(), range_request(0, 1));
            if (back.data != g->data || back.off != g->off) { fprintf(stderr, "level %d: the written file decodes to other bytes\n", level); return 10; }
            printf("level %d: %zu file bytes, equal for 1 and 4 threads, decoded back to the same %zu records\n", level, a.size(), back.off.size() - 1);
        }
    }
    if (coral_bgzf_write(argv[2], nullptr, nullptr, -1, 1, 1) != CORAL_ERR_ARG || coral_bgzf_write(argv[2], nullptr, nullptr, 0, 10, 1) != CORAL_ERR_ARG) return 11;
    const std::string none = std::string(argv[2]) + ".none.bam";
    if (coral_bgzf_write(none.c_str(), nullptr, nullptr, 0, 1, 2) != CORAL_OK || file_bytes(none).size() != 28) return 12;
    printf("ok\n");
    return 0;
}
