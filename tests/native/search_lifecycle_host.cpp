// Host check of the interval search's handle lifecycle (coral_amd/csrc/coral_search.cpp), through the C API only: a handle made
// in two parts (coral_search_create_early + coral_search_attach) answers byte for byte like one made by coral_search_create, on
// both sides of the table size at which the pack is filled on threads; the look-ahead and helper threads belong to the process
// (two handles share them, 200 create / free cycles leave their number unchanged, a handle may ask for more); a handle can be
// freed while its prefetched steps are queued or being computed, without ever being attached, or without a step ever asked;
// coral_search_shutdown may be called twice and a handle used afterwards.  A stand-alone program, never part of
// libcoral_hip.so; it is built from the library's own host sources.  Plain, and for the two sanitizer runs:
//   g++ -O1 -g -std=c++17 -pthread tests/native/search_lifecycle_host.cpp coral_amd/csrc/coral_search.cpp coral_amd/csrc/coral_bpcall.cpp coral_amd/csrc/coral_host.cpp -o search_lifecycle_host
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread tests/native/search_lifecycle_host.cpp coral_amd/csrc/coral_search.cpp coral_amd/csrc/coral_bpcall.cpp coral_amd/csrc/coral_host.cpp -o search_lifecycle_tsan
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/search_lifecycle_host.cpp coral_amd/csrc/coral_search.cpp coral_amd/csrc/coral_bpcall.cpp coral_amd/csrc/coral_host.cpp -o search_lifecycle_asan
//   ./search_lifecycle_host && ./search_lifecycle_tsan && ./search_lifecycle_asan
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>
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

// (join() returns when the thread's id is cleared, a moment before the kernel takes its entry out of /proc/self/task: a count
// that differs from the last one is read again, 2 ms apart, until two readings agree)
static int thread_count() {
    static int last = -1;
    int n = thread_count_now();
    for (int k = 0; k < 50 && n != last; ++k) {
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        const int m = thread_count_now();
        if (m == n) break;
        n = m;
    }
    return last = n;
}

// Three contigs of 300 CN segments of 10 kb; every read has two alignments, one at each side of one of six junctions (a few bases
// of jitter), so the reads of a junction form one cluster and give one call; the adjacent-pair slot of the first row is filled.
struct Table {
    static const int64_t N_TID = 3, N_SEG = 300, SEG = 10000, N_JUNC = 6;
    int64_t n_reads = 0, n_rows = 0;
    std::vector<int64_t> off, row_read, row_tid, ra, rb, cni0, cni1, read_hash, read_name, e_key, e_row, seg_off, seg_start, seg_end, seg_ix;
    std::vector<int32_t> pairs, chr_rank;
    std::vector<double> seg_cn;
    std::vector<uint8_t> has_rows;
    static int64_t junc_tid(int64_t j, int side) { return (j + side) % N_TID; }
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
            row_tid[(size_t)k] = junc_tid(j, 0); ra[(size_t)k] = junc_pos(j, 0) - 1000 - jit; rb[(size_t)k] = junc_pos(j, 0) + jit;
            row_tid[(size_t)k + 1] = junc_tid(j, 1); ra[(size_t)k + 1] = junc_pos(j, 1) + jit; rb[(size_t)k + 1] = junc_pos(j, 1) + 1000;
            for (int64_t q = k; q < k + 2; ++q) { cni0[(size_t)q] = ra[(size_t)q] / SEG; cni1[(size_t)q] = rb[(size_t)q] / SEG; }
            int32_t *p = pairs.data() + 8 * (2 * k);                       // slot of pair (k, k + 1)
            p[0] = (int32_t)row_tid[(size_t)k]; p[1] = (int32_t)rb[(size_t)k]; p[2] = (int32_t)row_tid[(size_t)k + 1]; p[3] = (int32_t)ra[(size_t)k + 1];
            p[4] = 0; p[5] = 2 | (1 << 3) | 32 | (60 << 8) | (60 << 16); p[6] = (int32_t)k; p[7] = (int32_t)k + 1;
        }
        std::vector<std::pair<int64_t, int64_t>> ent;                      // (key, row) in row order, then a stable sort by key
        for (int64_t k = 0; k < n_rows; ++k) {
            ent.emplace_back((row_tid[(size_t)k] << 32) + cni0[(size_t)k], k);
            if (cni1[(size_t)k] != cni0[(size_t)k]) ent.emplace_back((row_tid[(size_t)k] << 32) + cni1[(size_t)k], k);
        }
        std::stable_sort(ent.begin(), ent.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (const auto &e : ent) { e_key.push_back(e.first); e_row.push_back(e.second); }
        seg_off.resize(N_TID + 1);
        for (int64_t t = 0; t <= N_TID; ++t) seg_off[(size_t)t] = t * N_SEG;
        for (int64_t t = 0; t < N_TID; ++t)
            for (int64_t k = 0; k < N_SEG; ++k) {
                seg_start.push_back(k * SEG); seg_end.push_back(k * SEG + SEG - 1); seg_ix.push_back(k);
                seg_cn.push_back(k % 50 == 5 ? 8.0 : 2.0);
            }
        chr_rank = {0, 1, 2};
        has_rows.assign(N_TID, 1);
    }
    void *early() const {
        return coral_search_create_early(n_reads, n_rows, off.data(), row_read.data(), row_tid.data(), ra.data(), rb.data(), read_name.data(),
                                         pairs.data(), (int32_t)N_TID);
    }
    int attach(void *h, int64_t *first = nullptr) const {
        return coral_search_attach(h, cni0.data(), cni1.data(), read_hash.data(), (int64_t)e_key.size(), e_key.data(), e_row.data(),
                                   seg_off.data(), seg_start.data(), seg_end.data(), first);
    }
    void *create() const {
        return coral_search_create(n_reads, n_rows, off.data(), row_read.data(), row_tid.data(), ra.data(), rb.data(), cni0.data(), cni1.data(),
                                   read_hash.data(), read_name.data(), (int64_t)e_key.size(), e_key.data(), e_row.data(), pairs.data(),
                                   (int32_t)N_TID, seg_off.data(), seg_start.data(), seg_end.data());
    }
};

static int params(void *h, int32_t n_threads) { return coral_search_params(h, 3.0, 2000000, 2000, 100, 3.0, n_threads); }

template <class T>
static void put(std::vector<uint8_t> &out, const T *p, int64_t n) {
    const int64_t bytes = n * (int64_t)sizeof(T);
    out.insert(out.end(), (const uint8_t *)&n, (const uint8_t *)&n + sizeof(n));
    if (bytes > 0) out.insert(out.end(), (const uint8_t *)p, (const uint8_t *)p + bytes);
}

// every byte a caller can get out of a handle for junction j's interval: the step's result arrays, then the whole search from it
static std::vector<uint8_t> snapshot(void *h, const Table &T, int64_t j = 0, bool prefetch = true) {
    std::vector<uint8_t> out;
    const int64_t tid = Table::junc_tid(j, 0), seg = Table::junc_pos(j, 0) / Table::SEG, s = seg * Table::SEG, e = s + Table::SEG - 1;
    if (prefetch) CHECK(coral_search_prefetch(h, tid, s, e, seg, seg) == CORAL_OK, "prefetch");
    int rc = coral_search_step(h, tid, s, e, seg, seg);
    CHECK(rc == CORAL_OK, "step rc %d: %s", rc, coral_search_error(h));
    int64_t n_meta = 0, n_cand = 0, n_sup = 0;
    const int64_t *meta = nullptr, *cand = nullptr, *sup = nullptr, *order_off = nullptr;
    const double *stats = nullptr;
    const int32_t *order = nullptr;
    for (int twice = 0; twice < 2; ++twice) {                              // (the on-demand arrays are built once and stay)
        const size_t before = out.size();
        rc = coral_search_result(h, &n_meta, &meta, &n_cand, &cand, &n_sup, &sup, &stats, &order_off, &order);
        CHECK(rc == CORAL_OK && n_meta >= 1, "result");
        const int64_t ng = meta[0];
        int64_t n_calls = 0;
        put(out, meta, n_meta); put(out, cand, 13 * n_cand); put(out, sup, n_sup);
        for (int64_t g = 0, m = 1; g < ng; ++g) { n_calls += meta[m + 5]; m += 6 + meta[m + 4] + 6 * meta[m + 5]; }
        put(out, stats, 6 * n_calls); put(out, order_off, ng + 1); put(out, order, order_off[ng]);
        if (T.n_reads >= 1000) CHECK(ng >= 1 && n_cand > 0 && n_calls > 0, "the table gives no run / candidate / call (%lld %lld %lld)",
                                     (long long)ng, (long long)n_cand, (long long)n_calls);
        if (twice) {                                                       // (`out` was empty: the second answer follows the first)
            CHECK(out.size() == 2 * before && !memcmp(out.data(), out.data() + before, before), "coral_search_result twice");
            out.resize(before);
        }
    }
    const int64_t seed[4] = {tid, s, e, -1};
    rc = coral_search_bfs(h, 1, seed, T.seg_cn.data(), T.seg_ix.data(), T.chr_rank.data(), T.has_rows.data(), 5.0, 100000, 2);
    CHECK(rc == CORAL_OK, "bfs rc %d: %s", rc, coral_search_error(h));
    for (int32_t which = 0; which < 12; ++which) {
        const void *p = nullptr;
        int64_t n = 0;
        CHECK(coral_search_bfs_get(h, which, &p, &n) == CORAL_OK, "bfs_get %d", which);
        if (which == 3) put(out, (const double *)p, n); else put(out, (const int64_t *)p, n);
        if (which == 1 && T.n_reads >= 1000) CHECK(n > 0, "the search found no breakpoint");
    }
    return out;
}

static void stats_of(void *h, int64_t out[8]) { CHECK(coral_search_stats(h, out, 8) == CORAL_OK, "stats"); }

int main() {
    setenv("CORAL_SEARCH_PAR_MIN", "1", 1);                                // every step is cut into helper-thread pieces
    setenv("CORAL_SEARCH_HELPERS", "3", 1);
    std::thread([] {}).join();                                             // (a sanitizer's own background thread starts with the first thread)
    const int threads0 = thread_count();
    int64_t st[8];

    // ---- early + attach == create, both sides of the fill-thread threshold, threaded or not
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)39999, (int64_t)40000, (int64_t)40001}) {
        const Table T(n);
        void *a = T.create();
        CHECK(a != nullptr, "create(%lld)", (long long)n);
        CHECK(params(a, 0) == CORAL_OK, "params");
        const std::vector<uint8_t> want = snapshot(a, T);
        for (int32_t nt : {0, 3}) {
            void *b = T.early();
            CHECK(b != nullptr, "create_early(%lld)", (long long)n);
            // not attached: nothing can be asked of it
            const int32_t one = 0;
            const int64_t z = 0;
            CHECK(coral_search_step(b, 0, 0, 9, 0, 0) == CORAL_ERR_ARG, "step before attach");
            CHECK(coral_search_prefetch(b, 0, 0, 9, 0, 0) == CORAL_ERR_ARG, "prefetch before attach");
            CHECK(coral_search_within(b, 1, &z, &z, &z) == CORAL_ERR_ARG, "within before attach");
            CHECK(coral_search_between(b, 0, &one, 0, 0, 9, 1, 0, 9) == CORAL_ERR_ARG, "between before attach");
            CHECK(coral_search_bfs(b, 0, nullptr, T.seg_cn.data(), T.seg_ix.data(), T.chr_rank.data(), T.has_rows.data(), 5.0, 1, 0) == CORAL_ERR_ARG,
                  "bfs before attach");
            std::vector<int64_t> first((size_t)Table::N_TID, -7), slow((size_t)Table::N_TID, -1);
            CHECK(T.attach(b, first.data()) == CORAL_OK, "attach: %s", coral_search_error(b));
            CHECK(T.attach(b) == CORAL_ERR_ARG, "a second attach");
            for (int64_t k = T.n_rows - 1; k >= 0; --k) slow[(size_t)T.row_tid[(size_t)k]] = k;
            CHECK(first == slow, "first_row_of_tid (%lld reads)", (long long)n);
            CHECK(params(b, nt) == CORAL_OK, "params");
            const std::vector<uint8_t> got = snapshot(b, T);
            CHECK(got == want, "early + attach differs from create: %lld reads, %d threads (%zu / %zu bytes)", (long long)n, nt, got.size(), want.size());
            stats_of(b, st);
            CHECK(st[0] == 1 && (nt > 0 ? st[2] >= 1 : st[2] == 0), "stats: attached %lld, %lld steps queued with %d threads", (long long)st[0],
                  (long long)st[2], nt);
            if (nt > 0) CHECK(st[5] >= 3 && st[6] >= 3, "the process has %lld workers, %lld helpers", (long long)st[5], (long long)st[6]);
            CHECK(coral_search_free(b) == CORAL_OK, "free");
        }
        CHECK(coral_search_free(a) == CORAL_OK, "free");
    }
    const int threads1 = thread_count();
    CHECK(threads1 == threads0 + 3 + 3, "%d threads before, %d with 3 workers + 3 helpers", threads0, threads1);

    const Table T(40000), U(6000);
    void *ref = T.create();
    CHECK(ref && params(ref, 0) == CORAL_OK, "reference handle");
    std::vector<std::vector<uint8_t>> want;
    for (int64_t j = 0; j < Table::N_JUNC; ++j) want.push_back(snapshot(ref, T, j));
    void *uref = U.create();
    CHECK(uref && params(uref, 0) == CORAL_OK, "reference handle");
    const std::vector<uint8_t> uwant = snapshot(uref, U);

    // ---- two handles alive at once share the threads; one is freed with its steps queued and in flight, the other goes on
    {
        void *a = T.create(), *b = T.create();
        CHECK(a && b && params(a, 3) == CORAL_OK && params(b, 3) == CORAL_OK, "two handles");
        CHECK(thread_count() == threads1, "a second handle started threads: %d -> %d", threads1, thread_count());
        for (int64_t k = 0; k < 120; ++k) {                                // 120 steps for 3 workers: some run, most wait
            const int64_t s = k * Table::SEG;
            CHECK(coral_search_prefetch(a, k % 3, s, s + Table::SEG - 1, k, k) == CORAL_OK, "prefetch");
        }
        CHECK(coral_search_prefetch(b, 0, 50000, 59999, 5, 5) == CORAL_OK, "prefetch");
        CHECK(coral_search_free(a) == CORAL_OK, "free with queued steps");
        for (int64_t j = 0; j < Table::N_JUNC; ++j) CHECK(snapshot(b, T, j) == want[(size_t)j], "the surviving handle, junction %lld", (long long)j);
        // two callers of coral_search_result at once (the arrays are built on demand, once)
        CHECK(coral_search_step(b, 0, 50000, 59999, 5, 5) == CORAL_OK, "step");
        const int64_t *m[2] = {nullptr, nullptr};
        int64_t nm[2] = {0, 0};
        auto ask = [&](int q) {
            int64_t nc, ns;
            const int64_t *c, *s;
            const double *d;
            coral_search_result(b, &nm[q], &m[q], &nc, &c, &ns, &s, &d, nullptr, nullptr);
        };
        std::thread t1(ask, 0), t2(ask, 1);
        t1.join(); t2.join();
        CHECK(m[0] == m[1] && nm[0] == nm[1] && nm[0] > 1, "two callers of coral_search_result");
        CHECK(coral_search_free(b) == CORAL_OK, "free");
    }
    // ---- never attached; attached but never asked; params but never asked
    {
        void *a = T.early();
        CHECK(a && coral_search_free(a) == CORAL_OK, "free of a handle that was never attached");
        void *b = T.early();
        CHECK(b && T.attach(b) == CORAL_OK && coral_search_free(b) == CORAL_OK, "free of a handle without parameters");
        void *c = T.create();
        CHECK(c && params(c, 3) == CORAL_OK && coral_search_free(c) == CORAL_OK, "free of a handle no step was asked of");
    }
    // ---- 200 create / free cycles, with and without threads, handles of equal and of different n_reads in turn
    {
        int after_first = -1;
        int done = 0;
        for (int cycle = 0; cycle < 200; ++cycle) {
            const Table &W = (cycle % 12 == 8 || cycle % 12 == 3) ? T : U;  // (the big table now and then, made either way)
            void *h = cycle % 2 ? W.create() : W.early();
            CHECK(h != nullptr, "cycle %d", cycle);
            if (cycle % 2 == 0) CHECK(W.attach(h) == CORAL_OK, "attach");
            CHECK(params(h, cycle % 5 == 4 ? 0 : 2 + cycle % 2) == CORAL_OK, "params");
            if (cycle % 7 != 6) CHECK(snapshot(h, W, 0, cycle % 3 != 1) == (&W == &T ? want[0] : uwant), "cycle %d", cycle);
            else CHECK(coral_search_prefetch(h, 0, 50000, 59999, 5, 5) == CORAL_OK, "prefetch");
            CHECK(coral_search_free(h) == CORAL_OK, "free");
            ++done;
            if (after_first < 0) after_first = thread_count();
            else if (thread_count() != after_first) { CHECK(false, "cycle %d: %d threads, %d after the first cycle", cycle, thread_count(), after_first); break; }
        }
        CHECK(done == 200, "%d of 200 create / free cycles were completed", done);
        CHECK(after_first == threads1, "%d threads after a cycle, %d before", after_first, threads1);
    }
    // ---- a handle that asks for more threads makes the set grow; the results stay
    {
        void *a = T.create();
        CHECK(a && params(a, 5) == CORAL_OK, "params");
        stats_of(a, st);
        CHECK(st[5] == 5 && thread_count() == threads1 + 2, "5 workers asked for: %lld there, %d threads", (long long)st[5], thread_count());
        for (int64_t j = 0; j < Table::N_JUNC; ++j) CHECK(snapshot(a, T, j) == want[(size_t)j], "5 workers, junction %lld", (long long)j);
        // ---- shutdown, twice, with a handle alive and steps queued; the handle is used afterwards
        for (int64_t k = 0; k < 60; ++k) coral_search_prefetch(a, k % 3, k * Table::SEG, k * Table::SEG + Table::SEG - 1, k, k);
        CHECK(coral_search_shutdown() == CORAL_OK && coral_search_shutdown() == CORAL_OK, "shutdown");
        CHECK(thread_count() == threads0, "%d threads after shutdown, %d at the start", thread_count(), threads0);
        stats_of(a, st);
        CHECK(st[5] == 0 && st[6] == 0, "threads alive after shutdown");
        for (int64_t k = 0; k < 60; k += 7)                                // queued when the threads went: computed by the caller
            CHECK(coral_search_step(a, k % 3, k * Table::SEG, k * Table::SEG + Table::SEG - 1, k, k) == CORAL_OK, "step after shutdown");
        for (int64_t j = 0; j < Table::N_JUNC; ++j) CHECK(snapshot(a, T, j) == want[(size_t)j], "after shutdown, junction %lld", (long long)j);
        CHECK(coral_search_prefetch(a, 1, 200 * Table::SEG, 200 * Table::SEG + Table::SEG - 1, 200, 200) == CORAL_OK, "prefetch");       // a new step
        CHECK(coral_search_step(a, 1, 200 * Table::SEG, 200 * Table::SEG + Table::SEG - 1, 200, 200) == CORAL_OK, "step");
        stats_of(a, st);
        CHECK(st[5] == 5, "a prefetch after shutdown starts the threads again (%lld)", (long long)st[5]);
        CHECK(coral_search_free(a) == CORAL_OK, "free");
    }
    CHECK(coral_search_free(ref) == CORAL_OK && coral_search_free(uref) == CORAL_OK, "free");
    CHECK(coral_search_shutdown() == CORAL_OK, "shutdown");
    CHECK(thread_count() == threads0, "%d threads at the end, %d at the start", thread_count(), threads0);
    if (g_failed) { printf("%d check(s) FAILED\n", g_failed); return 1; }
    printf("search_lifecycle_host: ok\n");
    return 0;
}
