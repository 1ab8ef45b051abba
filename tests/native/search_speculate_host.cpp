// Host check of the interval search's exploring ahead (CORAL_SEARCH_SPECULATE, coral_amd/csrc/coral_search.cpp), through the C
// API only.  The table is 540 reads on two contigs, two alignments each, at three junctions:
//   J1  seed A (contig 0, 55 000)      <->  contig 1, 1 503 000          A's step yields interval C = contig 1 [1 403 000, 1 603 000]
//   J2  contig 1, 1 525 000 (inside C) <->  contig 0, 2 005 000          C's step yields interval D = contig 0 [1 905 000, 2 105 000]
//   J3  seed B (contig 0, 205 000)     <->  contig 1, 1 503 000          B's step yields C as well
// The whole search (coral_search_bfs) is run without threads, with threads and CORAL_SEARCH_SPECULATE=0, and with threads and
// speculation: all twelve coral_search_bfs_get arrays must be byte-identical, and so must the count of steps
// the caller queued.  The seeds are prefetched and waited for before the search, so the shadow pass at the start of the search
// guesses C from finished steps whatever the threads do later: at least one speculative entry is queued and at least one key
// the search asks for was speculated.  Then the lifecycle: a handle freed right after a search that left guesses queued and in
// flight, the threads shut down in the middle of a search, and the tail jobs asked for right after a search (they must be
// served, not wait behind guesses).  A stand-alone program, never part of libcoral_hip.so; plain, and for the sanitizer runs:
//   g++ -O1 -g -std=c++17 -pthread tests/native/search_speculate_host.cpp coral_amd/csrc/coral_search.cpp coral_amd/csrc/coral_bpcall.cpp coral_amd/csrc/coral_host.cpp -o search_speculate_host
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread ... -o search_speculate_tsan
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined ... -o search_speculate_asan
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
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

struct Table {
    static const int64_t N_TID = 2, N_SEG = 300, SEG = 10000, N_JUNC = 3, PER_JUNC = 180;
    int64_t n_reads = N_JUNC * PER_JUNC, n_rows = 2 * N_JUNC * PER_JUNC;
    std::vector<int64_t> off, row_read, row_tid, ra, rb, cni0, cni1, read_hash, read_name, e_key, e_row, seg_off, seg_start, seg_end, seg_ix;
    std::vector<int32_t> pairs, chr_rank;
    std::vector<double> seg_cn;
    std::vector<uint8_t> has_rows;
    static int64_t junc_tid(int64_t j, int side) { return j == 1 ? 1 - side : side; }
    static int64_t junc_pos(int64_t j, int side) {
        static const int64_t pos[3][2] = {{55000, 1503000}, {1525000, 2005000}, {205000, 1503000}};
        return pos[j][side];
    }
    Table() {
        const int64_t n = n_reads;
        off.resize((size_t)n + 1);
        for (int64_t r = 0; r <= n; ++r) off[(size_t)r] = 2 * r;
        row_read.resize((size_t)n_rows); row_tid.resize((size_t)n_rows); ra.resize((size_t)n_rows); rb.resize((size_t)n_rows);
        cni0.resize((size_t)n_rows); cni1.resize((size_t)n_rows);
        read_hash.resize((size_t)n); read_name.resize((size_t)n);
        pairs.assign((size_t)(2 * n_rows) * 8, 0);
        for (int64_t r = 0; r < n; ++r) {
            const int64_t j = r % N_JUNC;
            uint64_t h = (uint64_t)r * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
            read_hash[(size_t)r] = (int64_t)(h >> 1);
            read_name[(size_t)r] = 1000 + r;
            const int64_t k = 2 * r;
            row_read[(size_t)k] = row_read[(size_t)k + 1] = r;
            row_tid[(size_t)k] = junc_tid(j, 0); ra[(size_t)k] = junc_pos(j, 0) - 1000; rb[(size_t)k] = junc_pos(j, 0);
            row_tid[(size_t)k + 1] = junc_tid(j, 1); ra[(size_t)k + 1] = junc_pos(j, 1); rb[(size_t)k + 1] = junc_pos(j, 1) + 1000;
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
                seg_cn.push_back(2.0);
            }
        chr_rank = {0, 1};
        has_rows.assign(N_TID, 1);
    }
    void *create(int32_t n_threads) const {
        void *h = coral_search_create(n_reads, n_rows, off.data(), row_read.data(), row_tid.data(), ra.data(), rb.data(), cni0.data(), cni1.data(),
                                      read_hash.data(), read_name.data(), (int64_t)e_key.size(), e_key.data(), e_row.data(), pairs.data(),
                                      (int32_t)N_TID, seg_off.data(), seg_start.data(), seg_end.data());
        CHECK(h && coral_search_params(h, 3.0, 2000000, 2000, 100, 3.0, n_threads) == CORAL_OK, "create / params");
        return h;
    }
};

// the seeds: A and B, each one CN segment
static const int64_t SEEDS[8] = {0, 50000, 59999, -1, 0, 200000, 209999, -1};

template <class T>
static void put(std::vector<uint8_t> &out, const T *p, int64_t n) {
    const int64_t bytes = n * (int64_t)sizeof(T);
    out.insert(out.end(), (const uint8_t *)&n, (const uint8_t *)&n + sizeof(n));
    if (bytes > 0) out.insert(out.end(), (const uint8_t *)p, (const uint8_t *)p + bytes);
}

static void stats_of(void *h, int64_t out[12]) { CHECK(coral_search_stats(h, out, 12) == CORAL_OK, "stats"); }

// the seeds' steps queued as a build does at attach time and, when `wait`, finished before the search begins
static void seeds_ahead(void *h, bool wait) {
    for (int k = 0; k < 2; ++k) {
        const int64_t *s = SEEDS + 4 * k;
        CHECK(coral_search_prefetch(h, s[0], s[1], s[2], s[1] / Table::SEG, s[2] / Table::SEG) == CORAL_OK, "prefetch of a seed");
    }
    int64_t st[12];
    for (int spin = 0; wait && spin < 20000; ++spin) {                        // (at most 20 s; a step of this table takes microseconds)
        stats_of(h, st);
        if (st[11] >= 2) return;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    if (wait) CHECK(false, "the seeds' steps were not computed");
}

// all twelve arrays of the search from the two seeds
static std::vector<uint8_t> search(void *h, const Table &T, std::vector<int64_t> *intervals = nullptr) {
    std::vector<uint8_t> out;
    const int rc = coral_search_bfs(h, 2, SEEDS, T.seg_cn.data(), T.seg_ix.data(), T.chr_rank.data(), T.has_rows.data(), 5.0, 100000, 2);
    CHECK(rc == CORAL_OK, "bfs rc %d: %s", rc, coral_search_error(h));
    for (int32_t which = 0; which < 12; ++which) {
        const void *p = nullptr;
        int64_t n = 0;
        CHECK(coral_search_bfs_get(h, which, &p, &n) == CORAL_OK, "bfs_get %d", which);
        if (which == 3) put(out, (const double *)p, n); else put(out, (const int64_t *)p, n);
        if (which == 0 && intervals) intervals->assign((const int64_t *)p, (const int64_t *)p + n);
    }
    return out;
}

static bool has_interval(const std::vector<int64_t> &iv, int64_t t, int64_t s, int64_t e) {
    for (size_t k = 0; k + 5 <= iv.size(); k += 5)
        if (iv[k] == t && iv[k + 1] == s && iv[k + 2] == e) return true;
    return false;
}

// both tail jobs of an interval list, collected: the candidates of each
static std::vector<uint8_t> tails(void *h, const std::vector<int64_t> &iv5, bool ahead, int64_t served_want) {
    std::vector<int64_t> iv;
    for (size_t k = 0; k + 5 <= iv5.size(); k += 5) iv.insert(iv.end(), iv5.begin() + (long)k, iv5.begin() + (long)k + 3);
    const int32_t n_int = (int32_t)(iv.size() / 3);
    if (ahead) CHECK(coral_search_tail_prefetch(h, n_int, iv.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == CORAL_OK, "tail prefetch");
    std::vector<uint8_t> out;
    for (int32_t which = 0; which < 2; ++which) {
        const void *res = nullptr;
        const int rc = coral_search_tail_collect(h, which, n_int, iv.data(), 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &res);
        CHECK(rc == CORAL_OK && res, "tail collect %d: %d", which, rc);
        if (!res) continue;
        const void *p = nullptr;
        int64_t n = 0;
        CHECK(coral_tail_result_get(res, 0, &p, &n) == CORAL_OK, "tail result");
        put(out, (const int64_t *)p, n);
    }
    int64_t ts[4];
    CHECK(coral_search_tail_stats(h, ts) == CORAL_OK && ts[1] == served_want, "tail jobs served from the queue: %lld, expected %lld", (long long)ts[1],
          (long long)served_want);
    return out;
}

int main() {
    setenv("CORAL_SEARCH_PAR_MIN", "0", 1);                                // the pooled stages run on this size
    setenv("CORAL_SEARCH_HELPERS", "3", 1);
    const Table T;
    int64_t st[12];

    // ---- no threads: the reference arrays; the table does what the header says
    void *ref = T.create(0);
    std::vector<int64_t> iv_ref;
    const std::vector<uint8_t> want = search(ref, T, &iv_ref);
    CHECK(has_interval(iv_ref, 1, 1403000, 1603000), "the search did not find interval C");
    CHECK(has_interval(iv_ref, 0, 1905000, 2105000), "the search did not find interval D");
    const std::vector<uint8_t> tail_want = tails(ref, iv_ref, false, 0);     // (computed on demand: a handle without threads queues nothing)

    // ---- threads, speculation off: the A/B leg
    setenv("CORAL_SEARCH_SPECULATE", "0", 1);
    int64_t queued_off = -1;
    {
        void *h = T.create(3);
        seeds_ahead(h, true);
        CHECK(search(h, T) == want, "threads, CORAL_SEARCH_SPECULATE=0: the search differs");
        stats_of(h, st);
        queued_off = st[2];
        CHECK(st[2] >= 4 && st[7] == 0 && st[8] == 0 && st[9] == 0 && st[10] == 0, "off: queued %lld, speculation counters %lld %lld %lld %lld", (long long)st[2],
              (long long)st[7], (long long)st[8], (long long)st[9], (long long)st[10]);
        CHECK(coral_search_free(h) == CORAL_OK, "free");
    }

    // ---- threads, speculation on (set, and by default), several times each (the threads' timing differs from run to run)
    for (const char *mode : {"1", ""}) {
        if (mode[0]) setenv("CORAL_SEARCH_SPECULATE", mode, 1); else unsetenv("CORAL_SEARCH_SPECULATE");
        for (int rep = 0; rep < 10; ++rep) {
            void *h = T.create(3);
            seeds_ahead(h, true);
            std::vector<int64_t> iv;
            CHECK(search(h, T, &iv) == want, "CORAL_SEARCH_SPECULATE=%s, run %d: the search differs", mode, rep);
            stats_of(h, st);
            CHECK(st[2] == queued_off, "CORAL_SEARCH_SPECULATE=%s: the caller queued %lld steps, %lld without speculation", mode, (long long)st[2], (long long)queued_off);
            CHECK(st[7] >= 1 && st[8] >= 1, "CORAL_SEARCH_SPECULATE=%s: %lld speculative entries, %lld of them asked for", mode, (long long)st[7], (long long)st[8]);
            CHECK(st[8] <= st[7] && st[9] <= st[8] && st[10] == st[7] - st[8], "counters %lld %lld %lld %lld", (long long)st[7], (long long)st[8], (long long)st[9],
                  (long long)st[10]);
            // the tail jobs right after the search, with guesses possibly still being computed: served by the queue, and right
            if (rep % 2 == 0) {
                CHECK(tails(h, iv, true, 2) == tail_want, "the tail jobs after a search with guesses differ");
                int64_t later[12];                                         // no guess is queued once the search has returned
                stats_of(h, later);
                CHECK(later[7] == st[7], "%lld speculative entries when the search returned, %lld later", (long long)st[7], (long long)later[7]);
            }
            // (odd runs: freed at once, with guesses possibly queued and in flight)
            CHECK(coral_search_free(h) == CORAL_OK, "free");
        }
    }

    // ---- a cap of 0 entries: nothing is guessed, the same search
    {
        setenv("CORAL_SEARCH_SPECULATE_MAX", "0", 1);
        void *h = T.create(3);
        seeds_ahead(h, true);
        CHECK(search(h, T) == want, "CORAL_SEARCH_SPECULATE_MAX=0: the search differs");
        stats_of(h, st);
        CHECK(st[7] == 0 && st[2] == queued_off, "CORAL_SEARCH_SPECULATE_MAX=0: %lld speculative entries", (long long)st[7]);
        CHECK(coral_search_free(h) == CORAL_OK, "free");
        unsetenv("CORAL_SEARCH_SPECULATE_MAX");
    }

    // ---- a second search on the same handle (the guesses of the first are in its cache), and seeds not waited for
    {
        void *h = T.create(3);
        seeds_ahead(h, false);
        CHECK(search(h, T) == want, "seeds not waited for: the search differs");
        CHECK(search(h, T) == want, "the second search on a handle differs");
        CHECK(coral_search_free(h) == CORAL_OK, "free");
    }

    // ---- the threads shut down in the middle of a search, at different moments
    for (int rep = 0; rep < 12; ++rep) {
        void *h = T.create(3);
        seeds_ahead(h, rep % 2 == 0);
        std::atomic<bool> go{false};
        std::thread killer([&] {
            while (!go.load()) std::this_thread::yield();
            std::this_thread::sleep_for(std::chrono::microseconds(40 * rep));
            CHECK(coral_search_shutdown() == CORAL_OK, "shutdown");
        });
        go.store(true);
        CHECK(search(h, T) == want, "shutdown in the middle of a search, run %d: the search differs", rep);
        killer.join();
        CHECK(search(h, T) == want, "the search after a shutdown differs");
        CHECK(coral_search_free(h) == CORAL_OK, "free");
    }

    CHECK(coral_search_free(ref) == CORAL_OK, "free");
    CHECK(coral_search_shutdown() == CORAL_OK, "shutdown");
    if (g_failed) { printf("%d check(s) FAILED\n", g_failed); return 1; }
    printf("search_speculate_host: ok\n");
    return 0;
}
