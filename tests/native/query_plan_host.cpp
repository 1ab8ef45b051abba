// Host check of the batch planning behind coral_segment_coverage_host (coral_amd/csrc/coral_query_plan.h): every batch sorted by
// (tid, start) and pairwise disjoint, every segment in exactly one batch, and the batches the ones first fit in (tid, start)
// order gives (restated below the slow way).  A stand-alone program, never part of libcoral_hip.so; for the sanitizer run
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/query_plan_host.cpp -o query_plan_host
//   ./query_plan_host
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../coral_amd/csrc/coral_query_plan.h"

using coral_plan::BatchPlan;

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

// first fit the slow way: segments in (tid, start, input index) order by selection, each batch scanned from its first segment
static std::vector<std::vector<int32_t>> restated(const std::vector<int64_t> &s) {
    const int32_t n = (int32_t)(s.size() / 3);
    std::vector<char> done((size_t)n, 0);
    std::vector<std::vector<int32_t>> batches;
    for (int32_t step = 0; step < n; ++step) {
        int32_t best = -1;
        for (int32_t i = 0; i < n; ++i) {
            if (done[(size_t)i]) continue;
            if (best < 0 || s[3 * (size_t)i] < s[3 * (size_t)best] ||
                (s[3 * (size_t)i] == s[3 * (size_t)best] && s[3 * (size_t)i + 1] < s[3 * (size_t)best + 1]))
                best = i;
        }
        done[(size_t)best] = 1;
        size_t b = 0;
        for (; b < batches.size(); ++b) {
            const int32_t last = batches[b].back();
            if (s[3 * (size_t)last] != s[3 * (size_t)best] || s[3 * (size_t)last + 2] <= s[3 * (size_t)best + 1]) break;
        }
        if (b == batches.size()) batches.emplace_back();
        batches[b].push_back(best);
    }
    return batches;
}

static void check_plan(const char *what, const std::vector<int64_t> &s, int min_batches, bool compare) {
    const int32_t n = (int32_t)(s.size() / 3);
    const BatchPlan plan = coral_plan::plan_disjoint_batches(s.data(), n);
    CHECK(plan.batch_off.size() >= 1 && plan.batch_off.front() == 0 && plan.batch_off.back() == n, "%s: offsets", what);
    CHECK((int32_t)plan.order.size() == n, "%s: %zu entries for %d segments", what, plan.order.size(), n);
    CHECK(plan.n_batches() >= min_batches, "%s: %d batches, expected at least %d", what, plan.n_batches(), min_batches);
    std::vector<int> seen((size_t)n, 0);
    for (int b = 0; b < plan.n_batches(); ++b) {
        CHECK(plan.batch_off[(size_t)b] < plan.batch_off[(size_t)b + 1], "%s: batch %d is empty", what, b);
        for (int32_t k = plan.batch_off[(size_t)b]; k < plan.batch_off[(size_t)b + 1]; ++k) {
            const int32_t i = plan.order[(size_t)k];
            CHECK(i >= 0 && i < n, "%s: index %d", what, i);
            if (i < 0 || i >= n) continue;
            ++seen[(size_t)i];
            if (k > plan.batch_off[(size_t)b]) {
                const int32_t j = plan.order[(size_t)k - 1];
                const bool sorted = s[3 * (size_t)j] < s[3 * (size_t)i] || (s[3 * (size_t)j] == s[3 * (size_t)i] && s[3 * (size_t)j + 1] <= s[3 * (size_t)i + 1]);
                const bool disjoint = s[3 * (size_t)j] != s[3 * (size_t)i] || s[3 * (size_t)j + 2] <= s[3 * (size_t)i + 1];
                CHECK(sorted && disjoint, "%s: batch %d, segments %d and %d", what, b, j, i);
            }
        }
    }
    for (int32_t i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1, "%s: segment %d appears %d times", what, i, seen[(size_t)i]);
    if (compare) {
        const std::vector<std::vector<int32_t>> want = restated(s);
        CHECK((int)want.size() == plan.n_batches(), "%s: %d batches, first fit gives %zu", what, plan.n_batches(), want.size());
        for (size_t b = 0; b < want.size() && (int)b < plan.n_batches(); ++b) {
            const std::vector<int32_t> got(plan.order.begin() + plan.batch_off[b], plan.order.begin() + plan.batch_off[b + 1]);
            CHECK(got == want[b], "%s: batch %zu differs from first fit", what, b);
        }
    }
    const coral_plan::CoverageLayout lay = coral_plan::coverage_layout(n, plan.n_batches());
    CHECK(lay.sums >= 3 * sizeof(int32_t) * (size_t)n && lay.sums % 8 == 0 && lay.counts >= lay.sums + 2 * sizeof(uint64_t) * (size_t)n &&
              lay.bytes >= lay.counts + sizeof(uint32_t) * (size_t)plan.n_batches(),
          "%s: layout", what);
}

int main() {
    check_plan("empty", {}, 0, true);
    CHECK(coral_plan::plan_disjoint_batches(nullptr, 0).n_batches() == 0, "null table");
    check_plan("one", {3, 10, 20}, 1, true);
    check_plan("nested", {0, 100, 900, 0, 200, 800, 0, 300, 700, 0, 350, 360, 1, 0, 50, 0, 900, 950}, 4, true);
    check_plan("duplicates", {2, 5, 9, 2, 5, 9, 0, 1, 2, 2, 5, 9, 0, 1, 2}, 3, true);
    check_plan("touching", {0, 0, 10, 0, 10, 20, 0, 20, 30, 0, 5, 5, 0, 10, 10}, 1, true);
    check_plan("unsorted", {5, 70, 80, 1, 10, 30, 5, 10, 75, 1, 0, 12, -1, 4, 9, 1, 30, 31}, 2, true);
    uint64_t x = 88172645463325252ull;                         // xorshift: the same segments on every run
    auto next = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    std::vector<int64_t> big;
    for (int i = 0; i < 10000; ++i) {
        const int64_t t = (int64_t)(next() % 5), start = (int64_t)(next() % 1000000), len = (int64_t)(next() % 400);
        big.push_back(t);
        big.push_back(start);
        big.push_back(start + len);
    }
    check_plan("random 10^4", big, 2, false);
    big.resize(3 * 1500);
    check_plan("random 1500", big, 2, true);
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("query plan ok\n");
    return 0;
}
