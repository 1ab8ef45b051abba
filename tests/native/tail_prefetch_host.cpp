// Host check of the tail jobs of the interval search (coral_amd/csrc/coral_search.cpp: coral_smalldel_pass,
// coral_search_tail_prefetch / _collect), through the C API only: the jobs asked for ahead answer byte for byte like a handle
// without threads and like coral_smalldel_pass alone, collected in either order; a key that was not asked for is computed on
// demand; a handle is freed with tail jobs queued and in flight; a second handle finds the threads of the first; the threads
// are shut down with jobs queued and the collectors still answer.  A stand-alone program, never part of libcoral_hip.so; it
// is built from the library's own host sources.  Plain, and for the two sanitizer runs:
//   g++ -O1 -g -std=c++17 -pthread tests/native/tail_prefetch_host.cpp coral_amd/csrc/coral_search.cpp coral_amd/csrc/coral_bpcall.cpp coral_amd/csrc/coral_host.cpp -o tail_prefetch_host
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread tests/native/tail_prefetch_host.cpp coral_amd/csrc/coral_search.cpp coral_amd/csrc/coral_bpcall.cpp coral_amd/csrc/coral_host.cpp -o tail_prefetch_tsan
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/tail_prefetch_host.cpp coral_amd/csrc/coral_search.cpp coral_amd/csrc/coral_bpcall.cpp coral_amd/csrc/coral_host.cpp -o tail_prefetch_asan
//   ./tail_prefetch_host && ./tail_prefetch_tsan && ./tail_prefetch_asan
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

#include "../../include/coral_hip.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            ++g_failed;                                  \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                         \
            printf("\n");                                \
        }                                                \
    } while (0)

static int thread_count_now() {
    int n = 0;
    if (DIR *d = opendir("/proc/self/task")) {
        while (struct dirent *e = readdir(d)) n += e->d_name[0] != '.';
        closedir(d);
    }
    return n;
}

// (a joined thread leaves /proc/self/task a moment after join() returns: read 2 ms apart until two readings agree)
static int thread_count() {
    int n = thread_count_now();
    for (int k = 0; k < 50; ++k) {
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        const int m = thread_count_now();
        if (m == n) break;
        n = m;
    }
    return n;
}

// Three contigs of 300 CN segments of 10 kb.  Every read has two alignments on ONE contig, at the two sides of one of six
// junctions (a few bases of jitter) with a strand change, so `within` of an interval that holds both sides gives the read's
// pair, and the reads of a junction form one cluster and give one call.  The records of the small-deletion pass: one per
// read, spanning its junction, with one gap row (two for every fifth) whose ends jitter around the junction's.
struct Table {
    static const int64_t N_TID = 3, N_SEG = 300, SEG = 10000, N_JUNC = 6;
    int64_t n_reads = 0, n_rows = 0;
    std::vector<int64_t> off, row_read, row_tid, ra, rb, cni0, cni1, read_hash, read_name, e_key, e_row, seg_off, seg_start, seg_end;
    std::vector<int32_t> pairs;
    std::vector<int64_t> gaps;
    std::vector<int32_t> h_tid, h_pos, h_end, h_name, h_mapq;
    static int64_t junc_tid(int64_t j) { return j % N_TID; }
    static int64_t junc_pos(int64_t j, int side) { return side == 0 ? 50000 * (j + 1) + 5000 : 1500000 + 70000 * j + 3000; }
    explicit Table(int64_t n) : n_reads(n), n_rows(2 * n) {
        off.resize((size_t)n + 1);
        for (int64_t r = 0; r <= n; ++r) off[(size_t)r] = 2 * r;
        row_read.resize((size_t)n_rows); row_tid.resize((size_t)n_rows); ra.resize((size_t)n_rows); rb.resize((size_t)n_rows);
        cni0.resize((size_t)n_rows); cni1.resize((size_t)n_rows);
        read_hash.resize((size_t)n); read_name.resize((size_t)n);
        pairs.assign((size_t)(2 * n_rows) * 8, 0);
        for (int64_t r = 0; r < n; ++r) {
            const int64_t j = r % N_JUNC, jit = (r * 7) % 21;
            uint64_t h = (uint64_t)r * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
            read_hash[(size_t)r] = (int64_t)(h >> 1);
            read_name[(size_t)r] = 1000 + r;
            const int64_t k = 2 * r;
            row_read[(size_t)k] = row_read[(size_t)k + 1] = r;
            row_tid[(size_t)k] = row_tid[(size_t)k + 1] = junc_tid(j);
            ra[(size_t)k] = junc_pos(j, 0) - 1000 - jit; rb[(size_t)k] = junc_pos(j, 0) + jit;
            ra[(size_t)k + 1] = junc_pos(j, 1) + jit; rb[(size_t)k + 1] = junc_pos(j, 1) + 1000;
            for (int64_t q = k; q < k + 2; ++q) { cni0[(size_t)q] = ra[(size_t)q] / SEG; cni1[(size_t)q] = rb[(size_t)q] / SEG; }
            int32_t *p = pairs.data() + 8 * (2 * k);                       // slot of pair (k, k + 1)
            p[0] = (int32_t)row_tid[(size_t)k]; p[1] = (int32_t)rb[(size_t)k]; p[2] = (int32_t)row_tid[(size_t)k + 1]; p[3] = (int32_t)ra[(size_t)k + 1];
            p[4] = 0; p[5] = 2 | (1 << 3) | 32 | (60 << 8) | (60 << 16); p[6] = (int32_t)k; p[7] = (int32_t)k + 1;
            // the record of the read and its gap rows (record, op index, previous block end, next block start, first, last)
            h_tid.push_back((int32_t)junc_tid(j)); h_pos.push_back((int32_t)(junc_pos(j, 0) - 2000)); h_end.push_back((int32_t)(junc_pos(j, 1) + 2000));
            h_name.push_back((int32_t)(n - 1 - r / 2));                    // two records per name, ids descending: first appearance != id order
            h_mapq.push_back((int32_t)(r % 61));
            const int64_t g0[6] = {r, 3, junc_pos(j, 0) + jit, junc_pos(j, 1) - jit, h_pos.back(), h_end.back()};
            gaps.insert(gaps.end(), g0, g0 + 6);
            if (r % 5 == 0) {
                const int64_t g1[6] = {r, 8, junc_pos(j, 1) + 900, junc_pos(j, 1) + 100 + jit, h_pos.back(), h_end.back()};       // prv > nxt
                gaps.insert(gaps.end(), g1, g1 + 6);
            }
        }
        std::vector<std::pair<int64_t, int64_t>> ent;
        for (int64_t k = 0; k < n_rows; ++k) {
            ent.emplace_back((row_tid[(size_t)k] << 32) + cni0[(size_t)k], k);
            if (cni1[(size_t)k] != cni0[(size_t)k]) ent.emplace_back((row_tid[(size_t)k] << 32) + cni1[(size_t)k], k);
        }
        std::stable_sort(ent.begin(), ent.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (const auto &e : ent) { e_key.push_back(e.first); e_row.push_back(e.second); }
        seg_off.resize(N_TID + 1);
        for (int64_t t = 0; t <= N_TID; ++t) seg_off[(size_t)t] = t * N_SEG;
        for (int64_t t = 0; t < N_TID; ++t)
            for (int64_t k = 0; k < N_SEG; ++k) { seg_start.push_back(k * SEG); seg_end.push_back(k * SEG + SEG - 1); }
    }
    int64_t n_gap() const { return (int64_t)(gaps.size() / 6); }
    void *create() const {
        return coral_search_create(n_reads, n_rows, off.data(), row_read.data(), row_tid.data(), ra.data(), rb.data(), cni0.data(), cni1.data(),
                                   read_hash.data(), read_name.data(), (int64_t)e_key.size(), e_key.data(), e_row.data(), pairs.data(),
                                   (int32_t)N_TID, seg_off.data(), seg_start.data(), seg_end.data());
    }
    int prefetch(void *h, const std::vector<int64_t> &iv) const {
        return coral_search_tail_prefetch(h, (int32_t)(iv.size() / 3), iv.data(), n_gap(), gaps.data(), n_reads, h_tid.data(), h_pos.data(),
                                          h_end.data(), h_name.data(), h_mapq.data());
    }
    int collect(void *h, int32_t which, const std::vector<int64_t> &iv, const void **res) const {
        return coral_search_tail_collect(h, which, (int32_t)(iv.size() / 3), iv.data(), n_gap(), gaps.data(), n_reads, h_tid.data(),
                                         h_pos.data(), h_end.data(), h_name.data(), h_mapq.data(), res);
    }
};

static int params(void *h, int32_t n_threads) { return coral_search_params(h, 3.0, 2000000, 2000, 100, 3.0, n_threads); }

// every byte of a tail result
static std::vector<uint8_t> bytes_of(const void *res, bool want_calls) {
    std::vector<uint8_t> out;
    CHECK(res && coral_tail_result_rc(res) == CORAL_OK, "result: %s", coral_tail_result_error(res));
    int64_t n_calls = 0, n_cand = 0;
    for (int32_t which = 0; which < 12; ++which) {
        const void *p = nullptr;
        int64_t n = 0;
        CHECK(coral_tail_result_get(res, which, &p, &n) == CORAL_OK, "get %d", which);
        const int64_t width = (which == 1 || which == 6) ? 4 : 8;
        out.insert(out.end(), (const uint8_t *)&n, (const uint8_t *)&n + sizeof(n));
        if (n > 0) out.insert(out.end(), (const uint8_t *)p, (const uint8_t *)p + n * width);
        if (which == 0) n_cand = n / 13;
        if (which == 2) n_calls = n;
    }
    const void *p = nullptr;
    int64_t n = 0;
    CHECK(coral_tail_result_get(res, 12, &p, &n) == CORAL_ERR_ARG, "get 12");
    if (want_calls) CHECK(n_cand > 0 && n_calls > 0, "no candidate / call (%lld, %lld)", (long long)n_cand, (long long)n_calls);
    return out;
}

static std::vector<uint8_t> collected(const Table &T, void *h, int32_t which, const std::vector<int64_t> &iv, bool want_calls = true) {
    const void *res = nullptr;
    const int rc = T.collect(h, which, iv, &res);
    CHECK(rc == CORAL_OK, "collect %d rc %d: %s", which, rc, coral_search_error(h));
    return bytes_of(res, want_calls);
}

static void tail_stats(void *h, int64_t st[4]) { CHECK(coral_search_tail_stats(h, st) == CORAL_OK, "tail stats"); }

int main() {
    setenv("CORAL_SEARCH_PAR_MIN", "1", 1);                                // the pair filter is cut into helper-thread pieces
    setenv("CORAL_SEARCH_HELPERS", "3", 1);
    std::thread([] {}).join();                                             // (a sanitizer's own background thread starts with the first thread)
    const int threads0 = thread_count();
    const Table T(6000);
    // unsorted, overlapping, one empty, one that nothing touches; junctions 0, 3 (contig 0) and 1, 4 (contig 1) are inside
    const std::vector<int64_t> ivA = {1, 0, 2990000, 0, 100000, 2000000, 0, 0, 1800000, 2, 10, 5, 0, 2500000, 2600000};
    const std::vector<int64_t> ivB = {0, 0, 2990000, 2, 0, 2990000};
    const std::vector<int64_t> none;
    int64_t st[4];

    // ---- the expectation: a handle without threads, and the small-deletion pass alone
    void *ref = T.create();
    CHECK(ref && params(ref, 0) == CORAL_OK, "reference handle");
    CHECK(T.prefetch(ref, ivA) == CORAL_OK, "prefetch on a handle without threads");
    const std::vector<uint8_t> wantA[2] = {collected(T, ref, 0, ivA), collected(T, ref, 1, ivA)};
    const std::vector<uint8_t> wantB[2] = {collected(T, ref, 0, ivB), collected(T, ref, 1, ivB)};
    CHECK(wantA[0] != wantB[0] && wantA[1] != wantB[1], "the two interval lists give the same result");
    collected(T, ref, 0, none, false);
    collected(T, ref, 1, none, false);
    tail_stats(ref, st);
    CHECK(st[0] == 0 && st[1] == 0 && st[2] == 6 && st[3] == 0, "no threads: %lld queued, %lld served, %lld on demand", (long long)st[0],
          (long long)st[1], (long long)st[2]);
    {
        void *alone = coral_smalldel_pass(T.n_gap(), T.gaps.data(), T.n_reads, T.h_tid.data(), T.h_pos.data(), T.h_end.data(), T.h_name.data(),
                                          T.h_mapq.data(), (int32_t)(ivA.size() / 3), ivA.data(), 3.0, 2000, 100, 3.0);
        CHECK(alone && bytes_of(alone, true) == wantA[0], "coral_smalldel_pass differs from the handle's collector");
        coral_tail_result_free(alone);
        std::vector<int64_t> bad(T.gaps.begin(), T.gaps.begin() + 6);
        bad[0] = T.n_reads;                                                // a record that does not exist: refused, nothing is read
        void *r = coral_smalldel_pass(1, bad.data(), T.n_reads, T.h_tid.data(), T.h_pos.data(), T.h_end.data(), T.h_name.data(), T.h_mapq.data(),
                                      1, ivA.data(), 3.0, 2000, 100, 3.0);
        CHECK(r && coral_tail_result_rc(r) == CORAL_ERR_ARG, "a record ordinal out of range was accepted");
        coral_tail_result_free(r);
        coral_tail_result_free(nullptr);
    }
    CHECK(thread_count() == threads0, "a handle without threads started some");

    // ---- asked for ahead, collected in both orders; a result stays valid while the other kind is collected
    void *a = T.create();
    CHECK(a && params(a, 3) == CORAL_OK, "threaded handle");
    const int threads1 = thread_count();
    CHECK(threads1 == threads0 + 3 + 3, "%d threads before, %d with 3 workers + 3 helpers", threads0, threads1);
    for (int round = 0; round < 6; ++round) {
        const std::vector<int64_t> &iv = round % 2 ? ivB : ivA;
        const std::vector<uint8_t> *want = round % 2 ? wantB : wantA;
        CHECK(T.prefetch(a, iv) == CORAL_OK, "prefetch");
        const int first = round % 4 < 2 ? 0 : 1;
        const void *r0 = nullptr, *r1 = nullptr;
        CHECK(T.collect(a, first, iv, &r0) == CORAL_OK && T.collect(a, 1 - first, iv, &r1) == CORAL_OK, "collect");
        CHECK(bytes_of(r0, true) == want[first] && bytes_of(r1, true) == want[1 - first], "round %d: the prefetched jobs differ", round);
    }
    tail_stats(a, st);
    CHECK(st[0] == 12 && st[1] == 12 && st[2] == 0, "%lld queued, %lld served, %lld on demand", (long long)st[0], (long long)st[1], (long long)st[2]);
    // ---- a key that was not asked for; the same list with other arrays; a second collect of a key already served
    CHECK(T.prefetch(a, ivA) == CORAL_OK, "prefetch");
    CHECK(collected(T, a, 1, ivB) == wantB[1], "within of another list");
    CHECK(collected(T, a, 0, ivB) == wantB[0], "small deletions of another list");
    CHECK(collected(T, a, 0, ivA) == wantA[0], "the job was retired by the collect that missed it");
    {
        const Table U(6000);                                               // equal contents, other addresses
        CHECK(T.prefetch(a, ivA) == CORAL_OK, "prefetch");
        CHECK(collected(U, a, 0, ivA) == wantA[0], "the same list over other arrays");
        CHECK(collected(T, a, 1, ivA) == wantA[1], "within");
    }
    tail_stats(a, st);
    CHECK(st[0] == 16 && st[1] == 13 && st[2] == 4, "%lld queued, %lld served, %lld on demand", (long long)st[0], (long long)st[1], (long long)st[2]);
    // ---- a prefetch replaced by another before anybody collected
    CHECK(T.prefetch(a, ivA) == CORAL_OK && T.prefetch(a, ivB) == CORAL_OK, "two prefetches");
    CHECK(collected(T, a, 0, ivB) == wantB[0] && collected(T, a, 1, ivB) == wantB[1], "the second prefetch");

    // ---- a handle freed with tail jobs queued (120 steps in front of them) and in flight; the other handle goes on
    {
        void *b = T.create(), *c = T.create();
        CHECK(b && c && params(b, 3) == CORAL_OK && params(c, 3) == CORAL_OK, "two more handles");
        CHECK(thread_count() == threads1, "a later handle started threads: %d -> %d", threads1, thread_count());
        for (int64_t k = 0; k < 120; ++k) CHECK(coral_search_prefetch(b, k % 3, k * Table::SEG, k * Table::SEG + Table::SEG - 1, k, k) == CORAL_OK, "prefetch");
        CHECK(T.prefetch(b, ivA) == CORAL_OK, "tail prefetch behind the steps");
        CHECK(T.prefetch(c, ivB) == CORAL_OK, "tail prefetch");
        CHECK(coral_search_free(b) == CORAL_OK, "free with tail jobs queued");
        CHECK(collected(T, c, 1, ivB) == wantB[1] && collected(T, c, 0, ivB) == wantB[0], "the surviving handle");
        CHECK(T.prefetch(c, ivA) == CORAL_OK, "tail prefetch");
        CHECK(coral_search_free(c) == CORAL_OK, "free with tail jobs just handed to the threads");
        for (int cycle = 0; cycle < 40; ++cycle) {
            void *d = T.create();
            CHECK(d && params(d, 2 + cycle % 2) == CORAL_OK, "cycle %d", cycle);
            const int32_t which = cycle % 2;
            const std::vector<int64_t> &iv = which ? ivA : ivB;
            const std::vector<uint8_t> *want = which ? wantA : wantB;
            CHECK(T.prefetch(d, iv) == CORAL_OK, "prefetch");
            if (cycle % 3 == 0) CHECK(collected(T, d, which, iv) == want[which], "cycle %d", cycle);
            if (cycle % 4 == 1) std::this_thread::yield();
            CHECK(coral_search_free(d) == CORAL_OK, "free");
        }
        CHECK(thread_count() == threads1, "%d threads after the cycles, %d before", thread_count(), threads1);
    }
    // ---- shutdown with jobs queued: the collectors compute them; a later prefetch starts the threads again
    CHECK(T.prefetch(a, ivA) == CORAL_OK, "prefetch");
    CHECK(coral_search_shutdown() == CORAL_OK, "shutdown");
    CHECK(thread_count() == threads0, "%d threads after shutdown, %d at the start", thread_count(), threads0);
    CHECK(collected(T, a, 0, ivA) == wantA[0] && collected(T, a, 1, ivA) == wantA[1], "after shutdown");
    CHECK(T.prefetch(a, ivB) == CORAL_OK, "prefetch");
    CHECK(thread_count() == threads1, "a prefetch after shutdown starts the threads again");
    CHECK(collected(T, a, 1, ivB) == wantB[1] && collected(T, a, 0, ivB) == wantB[0], "after the restart");
    // ---- the handle's other calls are undisturbed by a tail job in flight
    CHECK(T.prefetch(a, ivA) == CORAL_OK, "prefetch");
    CHECK(coral_search_step(a, 0, 50000, 59999, 5, 5) == CORAL_OK, "step beside the tail jobs");
    CHECK(collected(T, a, 0, ivA) == wantA[0] && collected(T, a, 1, ivA) == wantA[1], "beside a step");
    CHECK(coral_search_free(a) == CORAL_OK && coral_search_free(ref) == CORAL_OK, "free");
    CHECK(coral_search_shutdown() == CORAL_OK, "shutdown");
    CHECK(thread_count() == threads0, "%d threads at the end, %d at the start", thread_count(), threads0);
    if (g_failed) { printf("%d check(s) FAILED\n", g_failed); return 1; }
    printf("tail_prefetch_host: ok\n");
    return 0;
}
