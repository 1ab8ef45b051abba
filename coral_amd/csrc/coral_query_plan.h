// coral_query_plan.h — host-only planning of the short device queries of a graph build (no HIP in here: the file compiles
// and is checked on a machine without a device, tests/native/query_plan_host.cpp).
//
// coral_segment_coverage works on sorted, pairwise disjoint segments; the callers' segments come in any order and may
// overlap (sequence edges of several amplicons, nested plot windows).  plan_disjoint_batches splits them into batches
// the kernel accepts: first fit in (tid, start) order, ties in input order.
#ifndef CORAL_QUERY_PLAN_H
#define CORAL_QUERY_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace coral_plan {

struct BatchPlan {
    std::vector<int32_t> order;       // segment indices (positions in the caller's table), batch after batch
    std::vector<int32_t> batch_off;   // n_batches + 1 offsets into `order`
    int n_batches() const { return (int)batch_off.size() - 1; }
};

// segs: n_seg rows (tid, start, end), half-open.  Every batch lists its segments in (tid, start) order and no two of them
// overlap; a segment goes into the first batch whose last segment is on another contig or ends at or before its start.
inline BatchPlan plan_disjoint_batches(const int64_t *segs, int32_t n_seg) {
    BatchPlan plan;
    plan.batch_off.push_back(0);
    if (n_seg <= 0 || !segs) return plan;
    std::vector<int32_t> by_start((size_t)n_seg);
    for (int32_t i = 0; i < n_seg; ++i) by_start[(size_t)i] = i;
    std::stable_sort(by_start.begin(), by_start.end(), [segs](int32_t a, int32_t b) {
        const int64_t *x = segs + 3 * (size_t)a, *y = segs + 3 * (size_t)b;
        return x[0] != y[0] ? x[0] < y[0] : x[1] < y[1];
    });
    std::vector<int32_t> batch_of((size_t)n_seg), count;
    std::vector<int64_t> last_tid, last_end;
    for (int32_t i : by_start) {
        const int64_t t = segs[3 * (size_t)i], s = segs[3 * (size_t)i + 1], e = segs[3 * (size_t)i + 2];
        size_t b = 0;
        while (b < count.size() && last_tid[b] == t && last_end[b] > s) ++b;
        if (b == count.size()) {
            count.push_back(0);
            last_tid.push_back(t);
            last_end.push_back(e);
        }
        last_tid[b] = t;
        last_end[b] = e;
        ++count[b];
        batch_of[(size_t)i] = (int32_t)b;
    }
    for (size_t b = 0; b < count.size(); ++b) plan.batch_off.push_back(plan.batch_off.back() + count[b]);
    std::vector<int32_t> cursor(plan.batch_off.begin(), plan.batch_off.end() - 1);
    plan.order.resize((size_t)n_seg);
    for (int32_t i : by_start) plan.order[(size_t)cursor[(size_t)batch_of[(size_t)i]]++] = i;      // (tid, start) order inside a batch
    return plan;
}

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Byte layout of one coverage query, the same in the pinned block and in the device block (one copy each way):
//   tables  int32 [3][n_seg]   tid, start, end of the segments in plan order (a batch is a contiguous piece of each row)
//   sums    uint64 [2][n_seg]  n_reads, n_bases in plan order (uploaded as zeros, the kernels add)
//   counts  uint32 [n_batches] straddler counter of every batch (uploaded as zeros)
struct CoverageLayout {
    size_t tables = 0, sums = 0, counts = 0, bytes = 0;
};

inline CoverageLayout coverage_layout(int32_t n_seg, int n_batches) {
    CoverageLayout l;
    const size_t n = (size_t)(n_seg > 0 ? n_seg : 0), nb = (size_t)(n_batches > 0 ? n_batches : 0);
    l.tables = 0;
    l.sums = round_up(3 * n * sizeof(int32_t), 256);
    l.counts = l.sums + round_up(2 * n * sizeof(uint64_t), 256);
    l.bytes = l.counts + round_up(nb * sizeof(uint32_t), 256);
    return l;
}

}      // namespace coral_plan

#endif
