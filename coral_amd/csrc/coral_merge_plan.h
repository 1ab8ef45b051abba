// coral_merge_plan.h — host-only planning of the streamed coordinate sort's merge (coral_bamgpu_merge.h), and the reader of
// the spill file's runs (no HIP in here: the file compiles and is checked on a machine without a device,
// tests/native/merge_plan_host.cpp; the planner alone through coral_merge_plan, tests/test_merge_plan.py).
//
// Phase 1 of the sort left R sorted runs in a spill file, each a whole number of BGZF members of 0xff00 inflated bytes (a run's
// last one may be shorter).  The merge walks the N records in their final order - perm[j] = the run-major ordinal g of the
// record at sorted position j - in STEPS: a step [j0, j1) is the longest stretch of whole records whose sources fit
// `stage_bytes` of staging memory.  The merge keeps each run's order, so a step takes from every run a CONTIGUOUS range of its
// records; that range is rounded outwards to the run's blocks, which are staged one behind the other, run after run in run
// order (a run with nothing in the step contributes nothing):
//   part = {run, first block, block count, staging base};  bytes of a part = min(end block * 0xff00, run bytes) - first block * 0xff00
// A block that two consecutive steps share is staged by both.  A record whose own blocks do not fit: CORAL_ERR_CAPACITY.
#ifndef CORAL_MERGE_PLAN_H
#define CORAL_MERGE_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace coral_merge {

enum { PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_CAPACITY = -3, PLAN_ERR_FORMAT = -4 };      // (the values of CORAL_OK / CORAL_ERR_*)
constexpr int64_t BLOCK = 0xff00;              // inflated bytes of a spill member (coral_deflate::BLOCK_MAX)

struct Part {
    int64_t run, first_block, n_blocks, stage_base;
};

struct Plan {
    std::vector<int64_t> step_j;               // n_steps + 1 sorted positions: step s is [step_j[s], step_j[s + 1])
    std::vector<int64_t> step_part;            // n_steps + 1 offsets into `parts`
    std::vector<Part> parts;                   // per step its touched runs, in run order
    int64_t n_steps() const { return (int64_t)step_j.size() - 1; }
};

inline int64_t part_bytes(const Part &p, int64_t run_bytes) {
    const int64_t end = (p.first_block + p.n_blocks) * BLOCK;
    return (end < run_bytes ? end : run_bytes) - p.first_block * BLOCK;
}

// run_records[r]: records of run r; len[g]: bytes of record g (run-major); perm: N sorted positions.  perm must visit every
// run's records in their order (what a stable sort of run-major input gives): anything else is PLAN_ERR_ARG.
inline int plan_steps(int64_t n_runs, const int64_t *run_records, const uint32_t *len, const uint32_t *perm, int64_t stage_bytes, Plan &plan,
                      std::string &err) {
    plan = Plan();
    plan.step_j.push_back(0);
    plan.step_part.push_back(0);
    if (n_runs < 0 || stage_bytes < 0 || (n_runs > 0 && !run_records)) { err = "merge plan: bad arguments"; return PLAN_ERR_ARG; }
    std::vector<int64_t> first((size_t)n_runs + 1, 0);
    for (int64_t r = 0; r < n_runs; ++r) {
        if (run_records[r] < 0) { err = "merge plan: a run with a negative record count"; return PLAN_ERR_ARG; }
        first[(size_t)r + 1] = first[(size_t)r] + run_records[r];
    }
    const int64_t n = first[(size_t)n_runs];
    if (n >= ((int64_t)1 << 31)) { err = "merge plan: 2^31 records or more"; return PLAN_ERR_CAPACITY; }
    if (n > 0 && (!len || !perm)) { err = "merge plan: no lengths or no order"; return PLAN_ERR_ARG; }
    std::vector<int64_t> run_bytes((size_t)n_runs, 0);
    for (int64_t r = 0; r < n_runs; ++r)
        for (int64_t g = first[(size_t)r]; g < first[(size_t)r + 1]; ++g) run_bytes[(size_t)r] += len[g];
    // per run: the records taken by the steps so far, their bytes, and the range of the step being built
    std::vector<int64_t> taken((size_t)n_runs, 0), at((size_t)n_runs, 0), lo((size_t)n_runs, 0), hi((size_t)n_runs, 0), staged((size_t)n_runs, 0);
    std::vector<char> in_step((size_t)n_runs, 0);
    std::vector<int64_t> touched;
    int64_t total = 0, j0 = 0;
    auto close_step = [&](int64_t j1) {
        std::vector<char> mark((size_t)n_runs, 0);
        for (int64_t r : touched) mark[(size_t)r] = 1;
        int64_t base = 0;
        for (int64_t r = 0; r < n_runs; ++r) {
            if (!mark[(size_t)r]) continue;
            const int64_t b0 = lo[(size_t)r] / BLOCK, b1 = (hi[(size_t)r] + BLOCK - 1) / BLOCK;
            plan.parts.push_back(Part{r, b0, (b1 > b0 ? b1 : b0) - b0, base});
            base += staged[(size_t)r];
            in_step[(size_t)r] = 0;
            staged[(size_t)r] = 0;
        }
        touched.clear();
        total = 0;
        plan.step_j.push_back(j1);
        plan.step_part.push_back((int64_t)plan.parts.size());
        j0 = j1;
    };
    int64_t r_hint = 0;
    for (int64_t j = 0; j < n;) {
        const int64_t g = perm[j];
        if (g >= n) { err = "merge plan: the order names a record that does not exist"; return PLAN_ERR_ARG; }
        int64_t r = r_hint;
        if (!(first[(size_t)r] <= g && g < first[(size_t)r + 1])) {      // the run of g: the last r with first[r] <= g
            int64_t a = 0, b = n_runs;
            while (b - a > 1) {
                const int64_t m = (a + b) >> 1;
                if (first[(size_t)m] <= g) a = m; else b = m;
            }
            r = r_hint = a;
        }
        if (g != first[(size_t)r] + taken[(size_t)r]) { err = "merge plan: the order does not keep a run's records in their order"; return PLAN_ERR_ARG; }
        const int64_t new_lo = in_step[(size_t)r] ? lo[(size_t)r] : at[(size_t)r], new_hi = at[(size_t)r] + (int64_t)len[g];
        const int64_t b0 = new_lo / BLOCK, b1 = (new_hi + BLOCK - 1) / BLOCK;
        const int64_t end = b1 * BLOCK < run_bytes[(size_t)r] ? b1 * BLOCK : run_bytes[(size_t)r];
        const int64_t now = end > b0 * BLOCK ? end - b0 * BLOCK : 0;
        if (total - staged[(size_t)r] + now > stage_bytes) {
            if (j == j0) {
                char msg[160];
                snprintf(msg, sizeof msg, "merge plan: the blocks of one record (%lld bytes) do not fit stage_bytes = %lld", (long long)now, (long long)stage_bytes);
                err = msg;
                return PLAN_ERR_CAPACITY;
            }
            close_step(j);
            continue;                                              // (the same record opens the next step)
        }
        if (!in_step[(size_t)r]) { in_step[(size_t)r] = 1; lo[(size_t)r] = new_lo; touched.push_back(r); }
        hi[(size_t)r] = new_hi;
        total += now - staged[(size_t)r];
        staged[(size_t)r] = now;
        at[(size_t)r] = new_hi;
        ++taken[(size_t)r];
        ++j;
    }
    if (n > j0) close_step(n);
    return PLAN_OK;
}

// ---- the spill file's runs ------------------------------------------------------------------------------------------------------
// A run of the spill: `n_blocks` members from `file_off`, `bytes` inflated (all members but the last hold BLOCK bytes), the
// members of the next run - or the end of the file - at `file_end`.
struct RunExtent {
    int64_t file_off = 0, file_end = 0, bytes = 0;
    int64_t n_blocks() const { return (bytes + BLOCK - 1) / BLOCK; }
    int64_t block_bytes(int64_t b) const { return b + 1 < n_blocks() ? BLOCK : bytes - b * BLOCK; }
};

struct Member {                                // one member of a piece: its DEFLATE stream relative to the piece's first byte
    uint32_t src_off, src_len, isize, crc;
};

// The cursor of one run: walks the member headers (BSIZE at +16) forwards; the member in front of the cursor is remembered, so
// the block that two consecutive steps share can be read again.  Nothing but the run's extent is known beforehand.
struct RunCursor {
    int64_t block = 0, off = 0;                // the next member to read
    int64_t prev_off = -1;                     // where member block - 1 starts
};

// Reads whole members of run E, blocks [block, block + want), from `fp` into buf (cap bytes), as many as fit: *got members,
// their bytes in *used.  C is moved to `block` first (only block == C.block or C.block - 1 can be asked for) and ends behind
// the members read.  A short read, a bad magic, a member reaching behind its run, or an ISIZE other than the block's:
// PLAN_ERR_FORMAT.  A buffer too small for one member: PLAN_ERR_CAPACITY.
inline int read_members(FILE *fp, const RunExtent &E, RunCursor &C, int64_t block, int64_t want, uint8_t *buf, size_t cap, std::vector<Member> &members,
                        int64_t *got, size_t *used, std::string &err) {
    *got = 0;
    *used = 0;
    if (block == C.block - 1 && C.prev_off >= 0) { C.block = block; C.off = C.prev_off; C.prev_off = -1; }
    if (block != C.block || want < 0 || block + want > E.n_blocks()) { err = "spill reader: a block out of the cursor's reach"; return PLAN_ERR_ARG; }
    if (want == 0) return PLAN_OK;
    const int64_t left = E.file_end - C.off;
    const size_t n = (size_t)(left < (int64_t)cap ? (left > 0 ? left : 0) : (int64_t)cap);
    if (n > 0 && (fseeko(fp, (off_t)C.off, SEEK_SET) != 0 || fread(buf, 1, n, fp) != n)) { err = "spill reader: short read (the spill file is truncated)"; return PLAN_ERR_FORMAT; }
    size_t p = 0;
    while (*got < want) {
        if (p + 18 > n) break;
        const uint8_t *h = buf + p;
        if (!(h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && h[3] == 4 && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0)) {
            err = "spill reader: not a BGZF member (bad magic)";
            return PLAN_ERR_FORMAT;
        }
        const size_t size = (size_t)(h[16] | (h[17] << 8)) + 1;
        if (size < 26) { err = "spill reader: a member shorter than its own frame"; return PLAN_ERR_FORMAT; }
        if (C.off + (int64_t)size > E.file_end) { err = "spill reader: a member reaches behind its run"; return PLAN_ERR_FORMAT; }
        if (p + size > n) break;
        Member m;
        m.src_off = (uint32_t)(p + 18);
        m.src_len = (uint32_t)(size - 26);
        memcpy(&m.crc, h + size - 8, 4);
        memcpy(&m.isize, h + size - 4, 4);
        if ((int64_t)m.isize != E.block_bytes(C.block)) { err = "spill reader: a member's ISIZE is not its block's size"; return PLAN_ERR_FORMAT; }
        members.push_back(m);
        C.prev_off = C.off;
        C.off += (int64_t)size;
        ++C.block;
        ++*got;
        p += size;
    }
    *used = p;
    if (*got == 0) {
        if (C.off + 18 > E.file_end || n < cap) { err = "spill reader: the run ends inside a member (the spill file is truncated)"; return PLAN_ERR_FORMAT; }
        err = "spill reader: the buffer does not hold one member";
        return PLAN_ERR_CAPACITY;
    }
    return PLAN_OK;
}

}      // namespace coral_merge

#endif
