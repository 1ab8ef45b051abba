// abi_layout_host.cpp — the layout of the structs that cross the C ABI by pointer, as the compiler lays them out: one line
// "<struct> sizeof <n>" and one "<struct> <field> <offset>" per field, for tests/test_cabi.py to compare with the ctypes mirrors in
// coral_amd/_lib.py.  A field added in the middle of a struct moves every offset behind it; counting arguments does not see that.
//   g++ -std=c++17 tests/native/abi_layout_host.cpp -o /tmp/abi_layout_host && /tmp/abi_layout_host
// Test infrastructure, never part of libcoral_hip.so; run on the CPU only.
#include <cstddef>
#include <cstdio>

#include "../../include/coral_hip.h"

#define SIZE(T) printf(#T " sizeof %zu\n", sizeof(T))
#define FIELD(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))

int main() {
    SIZE(coral_bam_request_t);
#define F(f) FIELD(coral_bam_request_t, f)
    F(rank); F(world); F(n_spans); F(span_beg); F(span_end); F(n_seg); F(seg_tid); F(seg_start); F(seg_end); F(quality_threshold); F(read_callback);
    F(want_index); F(want_qc); F(per_base); F(depth_bin); F(depth_min_mapq); F(depth_exclude_flags); F(depth_count_deletions); F(want_reads);
    F(reads_order); F(reads_exclude_flags); F(reads_n_seg); F(reads_seg_tid); F(reads_seg_start); F(reads_seg_end); F(reads_n_names); F(reads_names);
    F(reads_name_off); F(keep_min_mapq); F(keep_min_seq_length); F(keep_require_flags); F(keep_exclude_flags);
#undef F
    SIZE(coral_bam_sink_t);
#define F(f) FIELD(coral_bam_sink_t, f)
    F(kind); F(path); F(header); F(header_bytes); F(chunk_blocks);
#undef F
    return 0;
}
