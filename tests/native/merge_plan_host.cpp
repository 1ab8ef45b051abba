// Host check of the streamed sort's merge planning and spill reader (coral_amd/csrc/coral_merge_plan.h) on a spill file the
// program writes itself with the host build of the compressor core (tests/native/deflate_host.cpp): random runs, a random merge
// order, and per stage size
//   - the plan against a slow restatement (longest stretch of whole records whose blocks fit; parts in run order, rounded
//     outwards to blocks), its steps tiling [0, N);
//   - every step read back through read_members with a small buffer (members split over several reads, the shared edge block read
//     twice), each member the bytes that were written, and the records gathered from the staged blocks with the merge's own
//     address arithmetic equal to the records in final order;
//   - a truncated spill, a bad magic, a member reaching behind its run and a wrong ISIZE: PLAN_ERR_FORMAT.
// A stand-alone program, never part of libcoral_hip.so; for the sanitizer run
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/merge_plan_host.cpp -o merge_plan_host
//   ./merge_plan_host <a directory to write in>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "deflate_host.cpp"      // coral_test_deflate: one block -> one BGZF member
#include "../../coral_amd/csrc/coral_merge_plan.h"

using namespace coral_merge;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_failed;                                   \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % n);
}

struct Spill {
    std::vector<std::vector<uint32_t>> lens;         // per run
    std::vector<std::vector<uint8_t>> data;          // per run, inflated
    std::vector<RunExtent> extent;
    std::vector<uint8_t> file;
    std::vector<int64_t> run_records;
    std::vector<uint32_t> flat, perm;
    std::vector<int64_t> first;
};

static Spill make_spill(int n_runs, int max_records, uint32_t max_len) {
    Spill S;
    std::vector<uint8_t> slot(SLOT_BYTES);
    for (int r = 0; r < n_runs; ++r) {
        std::vector<uint32_t> l((size_t)rnd((uint32_t)max_records + 1));
        std::vector<uint8_t> d;
        for (uint32_t &x : l) {
            const uint32_t pick = rnd(6);
            x = pick == 0 ? 40 : pick == 1 ? (uint32_t)BLOCK : pick == 2 ? (uint32_t)BLOCK + 1 : 40 + rnd(max_len - 39);
            const uint8_t tag = (uint8_t)(r * 31 + d.size());
            for (uint32_t k = 0; k < x; ++k) d.push_back((uint8_t)(tag + (k % 7 == 0 ? rnd(256) : k / 3)));
        }
        RunExtent E;
        E.file_off = (int64_t)S.file.size();
        E.bytes = (int64_t)d.size();
        for (int64_t b = 0; b < E.n_blocks(); ++b) {
            const int n = coral_test_deflate(d.data() + b * BLOCK, (uint32_t)E.block_bytes(b), slot.data(), nullptr, nullptr);
            CHECK(n >= 26, "deflate of a block failed");
            S.file.insert(S.file.end(), slot.begin(), slot.begin() + n);
        }
        E.file_end = (int64_t)S.file.size();
        S.lens.push_back(l);
        S.data.push_back(d);
        S.extent.push_back(E);
    }
    S.first.assign(1, 0);
    for (int r = 0; r < n_runs; ++r) {
        S.run_records.push_back((int64_t)S.lens[(size_t)r].size());
        S.first.push_back(S.first.back() + S.run_records.back());
        S.flat.insert(S.flat.end(), S.lens[(size_t)r].begin(), S.lens[(size_t)r].end());
    }
    std::vector<int64_t> taken((size_t)n_runs, 0);
    while ((int64_t)S.perm.size() < S.first.back()) {      // a random merge order: stretches of one run
        const int r = (int)rnd((uint32_t)n_runs);
        for (uint32_t k = rnd(5) + 1; k > 0 && taken[(size_t)r] < S.run_records[(size_t)r]; --k) S.perm.push_back((uint32_t)(S.first[(size_t)r] + taken[(size_t)r]++));
    }
    return S;
}

static int run_of(const Spill &S, int64_t g) {
    int r = 0;
    while (!(S.first[(size_t)r] <= g && g < S.first[(size_t)r + 1])) ++r;
    return r;
}

// the staged bytes of the records at the sorted positions [j0, j1), the slow way: per run the blocks that cover them
static int64_t cost(const Spill &S, const std::vector<int64_t> &pos, int64_t j0, int64_t j1, std::vector<Part> *parts) {
    int64_t base = 0;
    for (size_t r = 0; r + 1 < S.first.size(); ++r) {
        int64_t lo = -1, hi = -1;
        for (int64_t j = j0; j < j1; ++j) {
            const int64_t g = S.perm[(size_t)j];
            if (run_of(S, g) != (int)r) continue;
            if (lo < 0) lo = pos[(size_t)g];
            hi = pos[(size_t)g] + S.flat[(size_t)g];
        }
        if (lo < 0) continue;
        Part P{(int64_t)r, lo / BLOCK, (hi + BLOCK - 1) / BLOCK - lo / BLOCK, base};
        if (parts) parts->push_back(P);
        base += part_bytes(P, S.extent[r].bytes);
    }
    return base;
}

static void check_spill(const Spill &S, const std::string &path, int64_t stage, size_t buf_cap) {
    const int64_t n = S.first.back();
    const size_t n_runs = S.extent.size();
    std::vector<int64_t> pos((size_t)n, 0);                   // byte position of a record in its run
    for (size_t r = 0; r < n_runs; ++r)
        for (int64_t g = S.first[r], at = 0; g < S.first[r + 1]; at += S.flat[(size_t)g], ++g) pos[(size_t)g] = at;
    Plan plan;
    std::string err;
    const int rc = plan_steps((int64_t)n_runs, S.run_records.data(), S.flat.data(), S.perm.data(), stage, plan, err);
    int64_t need = 0;
    for (int64_t j = 0; j < n; ++j) need = std::max(need, cost(S, pos, j, j + 1, nullptr));
    if (need > stage) {
        CHECK(rc == PLAN_ERR_CAPACITY, "stage %lld below the largest record's %lld must be refused, got %d", (long long)stage, (long long)need, rc);
        return;
    }
    CHECK(rc == PLAN_OK, "plan failed: %s", err.c_str());
    if (rc != PLAN_OK) return;
    CHECK(plan.step_j.front() == 0 && plan.step_j.back() == n && plan.step_part.back() == (int64_t)plan.parts.size(), "the steps do not tile the records");
    FILE *fp = fopen(path.c_str(), "rb");
    CHECK(fp != nullptr, "cannot open %s", path.c_str());
    if (!fp) return;
    std::vector<RunCursor> cursor(n_runs);
    for (size_t r = 0; r < n_runs; ++r) cursor[r].off = S.extent[r].file_off;
    std::vector<uint8_t> buf(buf_cap), stage_buf((size_t)stage), out;
    std::vector<Member> members;
    for (int64_t s = 0; s < plan.n_steps(); ++s) {
        const int64_t j0 = plan.step_j[(size_t)s], j1 = plan.step_j[(size_t)s + 1];
        std::vector<Part> want;
        const int64_t bytes = cost(S, pos, j0, j1, &want);
        CHECK(j1 > j0 && bytes <= stage && (j1 == n || cost(S, pos, j0, j1 + 1, nullptr) > stage), "step %lld is not the longest stretch that fits", (long long)s);
        const size_t p0 = (size_t)plan.step_part[(size_t)s], p1 = (size_t)plan.step_part[(size_t)s + 1];
        CHECK(p1 - p0 == want.size(), "step %lld touches %zu runs, restated %zu", (long long)s, p1 - p0, want.size());
        std::vector<int64_t> delta(n_runs, 0);
        for (size_t p = p0; p < p1 && p - p0 < want.size(); ++p) {
            const Part &P = plan.parts[p], &Q = want[p - p0];
            CHECK(P.run == Q.run && P.first_block == Q.first_block && P.n_blocks == Q.n_blocks && P.stage_base == Q.stage_base, "part %zu of step %lld", p - p0, (long long)s);
            const RunExtent &E = S.extent[(size_t)P.run];
            delta[(size_t)P.run] = P.stage_base - P.first_block * BLOCK;
            for (int64_t b = P.first_block, end = P.first_block + P.n_blocks, member_at = -1; b < end;) {
                int64_t got = 0;
                size_t used = 0;
                members.clear();
                const int64_t off0 = b == cursor[(size_t)P.run].block ? cursor[(size_t)P.run].off : cursor[(size_t)P.run].prev_off;
                const int rrc = read_members(fp, E, cursor[(size_t)P.run], b, end - b, buf.data(), buf.size(), members, &got, &used, err);
                CHECK(rrc == PLAN_OK && got > 0, "read of run %lld block %lld: %s", (long long)P.run, (long long)b, err.c_str());
                if (rrc != PLAN_OK || got <= 0) { fclose(fp); return; }
                CHECK(used <= buf.size() && memcmp(buf.data(), S.file.data() + off0, used) == 0, "the members read are not the bytes written");
                member_at = 0;
                for (int64_t m = 0; m < got; ++m) {
                    const Member &M = members[(size_t)m];
                    CHECK((int64_t)M.isize == E.block_bytes(b + m) && M.src_off == (uint32_t)member_at + 18, "member fields of block %lld", (long long)(b + m));
                    // what the inflate would put there: the block's own bytes
                    memcpy(stage_buf.data() + P.stage_base + (b + m - P.first_block) * BLOCK, S.data[(size_t)P.run].data() + (b + m) * BLOCK, M.isize);
                    member_at += 18 + M.src_len + 8;
                }
                CHECK((size_t)member_at == used, "used bytes");
                b += got;
            }
        }
        for (int64_t j = j0; j < j1; ++j) {                    // the merge's gather: stage + position in the run + the run's word
            const int64_t g = S.perm[(size_t)j];
            const int r = run_of(S, g);
            const int64_t src = pos[(size_t)g] + delta[(size_t)r];
            CHECK(src >= 0 && src + S.flat[(size_t)g] <= stage, "a record's source lies outside the staged bytes");
            out.insert(out.end(), stage_buf.begin() + src, stage_buf.begin() + src + S.flat[(size_t)g]);
        }
    }
    fclose(fp);
    std::vector<uint8_t> expect;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t g = S.perm[(size_t)j];
        const int r = run_of(S, g);
        expect.insert(expect.end(), S.data[(size_t)r].begin() + pos[(size_t)g], S.data[(size_t)r].begin() + pos[(size_t)g] + S.flat[(size_t)g]);
    }
    CHECK(out == expect, "the gathered records are not the records in final order (stage %lld)", (long long)stage);
}

static bool write_file(const std::string &path, const std::vector<uint8_t> &bytes) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    const bool ok = bytes.empty() || fwrite(bytes.data(), 1, bytes.size(), fp) == bytes.size();
    return fclose(fp) == 0 && ok;
}

// reads every block of the last non-empty run; the answer must be `want`
static void expect_read(const Spill &S, const std::string &path, int want, const char *what) {
    size_t r = S.extent.size();
    while (r > 0 && S.extent[r - 1].bytes == 0) --r;
    if (r == 0) return;
    const RunExtent &E = S.extent[r - 1];
    FILE *fp = fopen(path.c_str(), "rb");
    CHECK(fp != nullptr, "cannot open %s", path.c_str());
    if (!fp) return;
    RunCursor C;
    C.off = E.file_off;
    std::vector<uint8_t> buf(200000);
    std::vector<Member> members;
    std::string err;
    int rc = PLAN_OK;
    for (int64_t b = 0; b < E.n_blocks() && rc == PLAN_OK;) {
        int64_t got = 0;
        size_t used = 0;
        rc = read_members(fp, E, C, b, E.n_blocks() - b, buf.data(), buf.size(), members, &got, &used, err);
        b += got;
    }
    fclose(fp);
    CHECK(rc == want, "%s: got %d (%s), want %d", what, rc, err.c_str(), want);
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::string path = dir + "/merge_plan_host.spill";
    // the planner alone: nothing to plan, and what is no merge order
    {
        Plan plan;
        std::string err;
        CHECK(plan_steps(0, nullptr, nullptr, nullptr, 0, plan, err) == PLAN_OK && plan.n_steps() == 0, "zero runs");
        const int64_t none[3] = {0, 0, 0};
        CHECK(plan_steps(3, none, nullptr, nullptr, 10, plan, err) == PLAN_OK && plan.n_steps() == 0, "zero records");
        const int64_t two[1] = {2};
        const uint32_t len[2] = {40, 50}, back[2] = {1, 0}, twice[2] = {0, 0};
        CHECK(plan_steps(1, two, len, back, 1 << 20, plan, err) == PLAN_ERR_ARG, "a run's records out of their order");
        CHECK(plan_steps(1, two, len, twice, 1 << 20, plan, err) == PLAN_ERR_ARG, "a record named twice");
        CHECK(plan_steps(-1, two, len, back, 1, plan, err) == PLAN_ERR_ARG && plan_steps(1, two, len, back, -1, plan, err) == PLAN_ERR_ARG, "bad arguments");
    }
    for (int trial = 0; trial < 6; ++trial) {
        const Spill S = make_spill(trial == 0 ? 1 : 2 + (int)rnd(4), trial == 1 ? 3 : 12, trial % 2 ? 3000u : 200000u);
        CHECK(write_file(path, S.file), "cannot write %s", path.c_str());
        int64_t need = 0, total = 0;
        for (const RunExtent &E : S.extent) total += E.bytes;
        for (size_t r = 0; r < S.extent.size(); ++r)
            for (int64_t g = S.first[r], at = 0; g < S.first[r + 1]; at += S.flat[(size_t)g], ++g) {
                const Part P{(int64_t)r, at / BLOCK, (at + S.flat[(size_t)g] + BLOCK - 1) / BLOCK - at / BLOCK, 0};
                need = std::max(need, part_bytes(P, S.extent[r].bytes));
            }
        for (int64_t stage : {need - 1, need, need + 1, need + BLOCK, 2 * need + 12345, total + 1})
            if (stage >= 0) check_spill(S, path, stage, 70000 + rnd(140000));
        if (total == 0) continue;
        expect_read(S, path, PLAN_OK, "the spill as written");
        // truncated: the last member loses its last byte; then most of itself
        for (size_t cut : {(size_t)1, (size_t)20}) {
            std::vector<uint8_t> t(S.file.begin(), S.file.end() - (std::ptrdiff_t)std::min(cut, S.file.size()));
            CHECK(write_file(path, t), "cannot write %s", path.c_str());
            expect_read(S, path, PLAN_ERR_FORMAT, "a truncated spill");
        }
        size_t r = S.extent.size();
        while (S.extent[r - 1].bytes == 0) --r;
        const size_t at = (size_t)S.extent[r - 1].file_off;
        const size_t size = (size_t)(S.file[at + 16] | (S.file[at + 17] << 8)) + 1;
        struct Flip { size_t where; uint8_t to; const char *what; };
        const size_t last_size_at = (size_t)S.extent[r - 1].file_end;      // (the run's last member: found by walking)
        size_t last = at;
        for (size_t p = at; p < last_size_at; p += (size_t)(S.file[p + 16] | (S.file[p + 17] << 8)) + 1) last = p;
        for (const Flip &F : {Flip{at + 1, 0x8c, "a bad magic"}, Flip{at + 12, 'X', "a bad extra field"}, Flip{last + 17, 0xff, "a member reaching behind its run"},
                              Flip{at + size - 4, (uint8_t)(S.file[at + size - 4] ^ 1), "a wrong ISIZE"}}) {
            std::vector<uint8_t> t = S.file;
            t[F.where] = F.to;
            CHECK(write_file(path, t), "cannot write %s", path.c_str());
            expect_read(S, path, PLAN_ERR_FORMAT, F.what);
        }
    }
    (void)unlink(path.c_str());
    if (g_failed) {
        printf("merge_plan_host: %d check(s) FAILED\n", g_failed);
        return 1;
    }
    printf("merge_plan_host: ok\n");
    return 0;
}
