// coral_bam_common.h — host-side pieces shared by the two BAM decoders of libcoral_hip.so: the CPU pipeline (coral_bam.cpp)
// and the GPU pipeline (coral_bamgpu.hip: BGZF inflate and record parsing on the device, these helpers for the file layout,
// the SA-tag tokeniser, the read-name table and the rare non-ACGT records).
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/coral_hip.h"
#include "coral_names.h"

namespace coral_bam {


// A BAI index request (want_index of a coral_bam_request_t): what one decode of a byte range contributes to the
// index of the file (SAMv1 §5.2), in a form that partial results of consecutive byte ranges merge into exactly.
//   heads     one entry per maximal run of file-consecutive records with the same (tid, bin), in file order: key =
//             tid * 65536 + reg2bin(beg, end) (-1 for a record without coordinates, which only ends the run in front of it) and
//             the virtual offset of the run's first record.  A run's chunk ends where the next head starts (the start of the
//             next record in the file), the file's last run at `end_voff`.
//   lin       per contig (len >> 14) + 1 windows of 16 384 bases: the smallest virtual offset of a record that overlaps the
//             window (~0: none).
//   counts    records per contig with / without flag 0x4 (the pseudo-bin 37450), and records without coordinates.
// A record is indexed as [beg, end) = [max(pos, 0), bam_endpos) (end = beg + 1 without a reference length, as htslib does).
// The linear index of a contig has the windows its header length gives; of a record that reaches further (which no aligner
// writes) the windows behind the last one are folded into the last one — the region query clamps its window the same way, so the
// record is still found (tests/test_bam_index.py::test_record_past_the_contig_end_is_still_found).
struct IndexPartial {
    bool on = false;
    std::vector<int64_t> head_key;
    std::vector<uint64_t> head_voff;
    std::vector<int64_t> lin_off;           // n_ref + 1
    std::vector<uint64_t> lin;
    std::vector<int64_t> n_mapped, n_unmapped;
    int64_t n_no_coor = 0, n_rec = 0;
    uint64_t end_voff = 0;                  // virtual offset just behind the range's last record (bgzf_tell's rule at the end of the file)
    uint64_t first_sort = 0, last_sort = 0; // (tid, pos) of the range's first and last record as one sortable word
    bool unsorted = false;

    void init(const std::vector<int32_t> &ref_lens) {
        on = true;
        lin_off.assign(1, 0);
        for (int32_t l : ref_lens) lin_off.push_back(lin_off.back() + ((int64_t)(l > 0 ? l : 0) >> 14) + 1);
        lin.assign((size_t)lin_off.back(), ~0ull);
        n_mapped.assign(ref_lens.size(), 0);
        n_unmapped.assign(ref_lens.size(), 0);
    }
    static uint64_t sort_word(int32_t tid, int32_t pos) {      // records without coordinates sort last
        return tid < 0 ? ~0ull : ((uint64_t)(uint32_t)tid << 32) | (uint32_t)(pos < 0 ? 0 : pos);
    }
    static int reg2bin(int64_t beg, int64_t end) {             // SAMv1 §5.3
        --end;
        if (beg >> 14 == end >> 14) return (int)(4681 + (beg >> 14));
        if (beg >> 17 == end >> 17) return (int)(585 + (beg >> 17));
        if (beg >> 20 == end >> 20) return (int)(73 + (beg >> 20));
        if (beg >> 23 == end >> 23) return (int)(9 + (beg >> 23));
        if (beg >> 26 == end >> 26) return (int)(1 + (beg >> 26));
        return 0;
    }
    void add_head(int64_t key, uint64_t voff) {                // heads of consecutive batches / chunks: a run that goes on is ONE run
        if (!head_key.empty() && head_key.back() == key) return;
        head_key.push_back(key);
        head_voff.push_back(voff);
    }
    void note_order(uint64_t first, uint64_t last) {           // a batch / record whose records are sorted among themselves
        if (n_rec == 0) first_sort = first;
        else if (first < last_sort) unsorted = true;
        last_sort = last;
    }
    void add(int32_t tid, int32_t pos, int32_t end, int32_t flag, uint64_t voff) {      // host pipeline: records in file order
        const uint64_t sw = sort_word(tid, pos);
        note_order(sw, sw);
        ++n_rec;
        if (tid < 0 || (size_t)tid >= n_mapped.size()) {
            ++n_no_coor;
            add_head(-1, voff);
            return;
        }
        const int64_t b = pos < 0 ? 0 : pos, e = end > b ? end : b + 1;
        add_head((int64_t)tid * 65536 + reg2bin(b, e), voff);
        ++((flag & 4) ? n_unmapped : n_mapped)[(size_t)tid];
        const int64_t nw = lin_off[(size_t)tid + 1] - lin_off[(size_t)tid];
        const int64_t w0 = std::min(b >> 14, nw - 1), w1 = std::min((e - 1) >> 14, nw - 1);
        uint64_t *l = lin.data() + lin_off[(size_t)tid];
        for (int64_t w = w0; w <= w1; ++w) l[w] = std::min(l[w], voff);
    }
};

// A read-QC request (want_qc of a coral_bam_request_t): per-read length and base-quality statistics, what the
// reference's scripts/report_nanopore_qc.py computes from the FASTQ the file was aligned from.  The rules both pipelines share:
//   a READ is a record with flag & 0x900 == 0 (neither secondary nor supplementary) and l_seq > 0, mapped or not;
//   its QUAL bytes start qc_qual_offset() bytes behind the record's first byte (its block_size field) - the record's OWN
//   n_cigar_op counts there, not the CG tag's -; a read whose first QUAL byte is 0xff has no quality.
// Per record: qual_sum = sum of the read's l_seq QUAL bytes, -1 when the record is not a read or has no quality (its length is
// the l_seq the decode keeps anyway).  hist counts every QUAL byte value of the reads that have quality.  Integers only: the
// result is the same on either pipeline, for any batch size and any split into byte ranges.
#ifdef __HIP__
#define CORAL_QC_HD __host__ __device__
#else
#define CORAL_QC_HD
#endif
CORAL_QC_HD inline bool qc_is_read(uint32_t flag, uint32_t l_seq) { return (flag & 0x900u) == 0 && l_seq > 0; }
CORAL_QC_HD inline unsigned long long qc_qual_offset(uint32_t l_read_name, uint32_t n_cigar_op, uint32_t l_seq) {
    return 36ull + l_read_name + 4ull * n_cigar_op + ((unsigned long long)l_seq + 1) / 2;
}
CORAL_QC_HD inline bool qc_has_quality(uint8_t first_qual_byte) { return first_qual_byte != 0xff; }

enum { QC_N_RECORDS = 0, QC_N_READS, QC_N_SECONDARY, QC_N_SUPPLEMENTARY, QC_N_UNMAPPED, QC_N_NO_SEQ, QC_N_NO_QUAL, QC_TOTAL_BASES, QC_N_COUNTERS };

struct QcPartial {
    bool on = false;
    std::vector<int64_t> qual_sum;          // per record, in file order
    int64_t hist[256];
    void init() {
        on = true;
        memset(hist, 0, sizeof(hist));
    }
    // the counters of the request from the per-record columns (flag; l_seq = has_seq ? qlen : 0; qual_sum)
    static void counters(const std::vector<int32_t> &flag, const std::vector<int32_t> &has_seq, const std::vector<int32_t> &qlen,
                         const std::vector<int64_t> &qual_sum, int64_t c[QC_N_COUNTERS]) {
        for (int k = 0; k < QC_N_COUNTERS; ++k) c[k] = 0;
        c[QC_N_RECORDS] = (int64_t)flag.size();
        for (size_t i = 0; i < flag.size(); ++i) {
            const uint32_t f = (uint32_t)flag[i], l_seq = has_seq[i] ? (uint32_t)qlen[i] : 0u;
            c[QC_N_SECONDARY] += (f & 0x100u) != 0;
            c[QC_N_SUPPLEMENTARY] += (f & 0x800u) != 0;
            c[QC_N_NO_SEQ] += (f & 0x900u) == 0 && l_seq == 0;
            if (!qc_is_read(f, l_seq)) continue;
            ++c[QC_N_READS];
            c[QC_N_UNMAPPED] += (f & 4u) != 0;
            c[QC_N_NO_QUAL] += qual_sum[i] < 0;
            c[QC_TOTAL_BASES] += l_seq;
        }
    }
};

// A binned-depth request (depth_bin > 0 of a coral_bam_request_t): read depth summed into fixed-size bins along every contig of
// the header, the one pass over the alignments behind the reference's scripts/call_cnvs.sh:12-17 (cnvkit.py batch --seq-method
// wgs: CNVkit's `coverage`).  Contig t of length LN[t] has ceil(LN[t] / bin) bins (none for a length of 0), bin_off is their
// exclusive prefix sum in tid order.  The rules both pipelines share:
//   a record TAKES PART when 0 <= tid < n_ref, pos >= 0, its real CIGAR (CG:B,I for the placeholder) has an op,
//   flag & exclude_flags == 0 and mapq >= min_mapq (depth_takes_part); SEQ and QUAL are not looked at, and flag 0x4 only
//   matters through exclude_flags;
//   bases[bin_off[tid] + x / bin] += 1 for every reference position x < LN[tid] covered by an M, = or X op, and by a D op with
//   count_deletions (depth_counts_op); N, I, S, H, P and zero-length ops add nothing; positions at or behind LN[tid] are dropped;
//   reads[bin_off[tid] + pos / bin] += 1 for every record that takes part and has pos < LN[tid].
// int64, exact: the tables do not depend on scheduling, batch size or rank count, and tables of byte ranges add up.
const int64_t DEPTH_MAX_BINS = 1ll << 28;

CORAL_QC_HD inline bool depth_takes_part(int32_t tid, int32_t pos, uint32_t n_ops, uint32_t flag, uint32_t mapq, int32_t n_ref,
                                         uint32_t exclude_flags, uint32_t min_mapq) {
    return tid >= 0 && tid < n_ref && pos >= 0 && n_ops > 0 && (flag & exclude_flags) == 0 && mapq >= min_mapq;
}
CORAL_QC_HD inline bool depth_counts_op(uint32_t op, bool count_deletions) {      // M = X, and D on request
    return ((0x181u >> op) & 1u) != 0 || (op == 2u && count_deletions);
}

struct DepthPartial {
    bool on = false;
    int32_t bin = 0, min_mapq = 0, exclude_flags = 0;
    bool count_deletions = false;
    std::vector<int32_t> len;               // LN per contig (a negative one counts as 0)
    std::vector<int64_t> bin_off;           // n_ref + 1
    std::vector<int64_t> bases, reads;      // n_bins each (filled by the decode)
    int64_t n_bins() const { return bin_off.empty() ? 0 : bin_off.back(); }
    // the bins of the header's contigs; false (nothing allocated): more than 2^28 of them
    bool init(int32_t bin_, int32_t min_mapq_, int32_t exclude_, bool count_del, const std::vector<int32_t> &ref_lens, std::string &err) {
        bin = bin_; min_mapq = min_mapq_; exclude_flags = exclude_; count_deletions = count_del;
        len.clear();
        bin_off.assign(1, 0);
        for (int32_t l : ref_lens) {
            len.push_back(l > 0 ? l : 0);
            bin_off.push_back(bin_off.back() + ((int64_t)len.back() + bin - 1) / bin);
        }
        if (n_bins() > DEPTH_MAX_BINS) { err = "binned-depth request: the contigs hold more than 2^28 bins of this size"; return false; }
        on = true;
        return true;
    }
    void zero_tables() {
        bases.assign((size_t)n_bins(), 0);
        reads.assign((size_t)n_bins(), 0);
    }
    // One record into the tables (host pipeline; ops = the real CIGAR, CG tag already resolved).  The tables are shared by the
    // threads that parse chunks, hence the relaxed atomic adds: one per op and bin it covers.
    void add(int32_t tid, int32_t pos, uint32_t flag, uint32_t mapq, const uint32_t *ops, uint32_t n_ops) {
        if (!depth_takes_part(tid, pos, n_ops, flag, mapq, (int32_t)len.size(), (uint32_t)exclude_flags, (uint32_t)min_mapq)) return;
        const int64_t ln = len[(size_t)tid];
        if (pos >= ln) return;
        int64_t *b = bases.data() + bin_off[(size_t)tid];
        __atomic_fetch_add(reads.data() + bin_off[(size_t)tid] + pos / bin, (int64_t)1, __ATOMIC_RELAXED);
        int64_t r = pos;
        for (uint32_t k = 0; k < n_ops && r < ln; ++k) {
            const uint32_t op = ops[k] & 15;
            const int64_t l = ops[k] >> 4;
            if (depth_counts_op(op, count_deletions)) {
                const int64_t e = std::min(r + l, ln);
                for (int64_t x = r; x < e;) {
                    const int64_t nx = std::min(e, (x / bin + 1) * bin);
                    __atomic_fetch_add(b + x / bin, nx - x, __ATOMIC_RELAXED);
                    x = nx;
                }
            }
            if ((0x18Du >> op) & 1u) r += l;      // M D N = X advance the reference
        }
    }
};

// A record filter (keep_* of a coral_bam_request_t): which records a decode keeps - samtools view -q / -f / -F and the length
// test of the reference's preparation step (scripts/align_nanopore_reads.sh:42-44), decided from the record's fixed fields
// alone.  A record is kept when all four tests hold; all-zero keeps everything (the filter is then not active: no work is added).
// The length is the fixed field l_seq: a record without SEQ has length 0, where awk sees `*` with length 1 - both fail any
// threshold of 2 or more.  Every result of a filtered decode is that of a file holding only the kept records; a dropped record
// is looked at no further than its fixed fields (its tags are not walked, so a malformed tag in it is not an error).
struct KeepRule {
    uint32_t min_mapq = 0, min_seq_length = 0, require_flags = 0, exclude_flags = 0;
    bool active() const { return (min_mapq | min_seq_length | require_flags | exclude_flags) != 0; }
};
CORAL_QC_HD inline bool keep_record(uint32_t mapq, uint32_t flag, uint32_t l_seq, uint32_t min_mapq, uint32_t min_seq_length,
                                    uint32_t require_flags, uint32_t exclude_flags) {
    return mapq >= min_mapq && l_seq >= min_seq_length && (flag & require_flags) == require_flags && (flag & exclude_flags) == 0;
}
// the same on a record's bytes (r points at block_size, which must be >= 32)
inline bool keep_record_at(const uint8_t *r, const KeepRule &K) {
    uint16_t flag; uint32_t l_seq;
    memcpy(&flag, r + 18, 2); memcpy(&l_seq, r + 20, 4);
    return keep_record(r[13], flag, l_seq, K.min_mapq, K.min_seq_length, K.require_flags, K.exclude_flags);
}

// A reads request (want_reads of a coral_bam_request_t): the selected records as FASTQ text, what the reference's workflow gets
// from `samtools view x.bam region... | samtools fastq` or `samtools view -N names.txt` in a second pass over the file (its own
// scripts start and end at FASTQ: scripts/align_nanopore_reads.sh, scripts/report_nanopore_qc.py).  The rules both pipelines share:
//   a record is WRITTEN when l_seq > 0, flag & exclude_flags == 0 (reads_takes_part), with segments: tid >= 0 and
//   [pos, bam_endpos) - [pos, pos + 1) with flag 0x4, which is what bam_endpos gives - meets a non-empty segment
//   (reads_meets_segment), with names: its read name without the NUL is in the sorted list (reads_name_listed: exact binary
//   search, bytes compared, nothing hashed).  Segments and names intersect; neither: every read.
//   Its text is `@` name `\n` SEQ `\n+\n` QUAL `\n`: 2 l_seq + l_read_name + 5 bytes (reads_text_bytes; l_read_name counts
//   the NUL).  SEQ characters are READS_SEQ_CHARS[code], QUAL characters min(q, 93) + 33; a record whose first QUAL byte is
//   0xff gets l_seq times '"' (quality 1).  With flag 0x10 the read is restored to the orientation it was sequenced in: SEQ
//   reversed and complemented - the complement of a 4-bit code is its bit reversal, so = and N stay - and QUAL reversed.
//   Nothing is appended to the name; records come in file order.  Bytes only: identical on either pipeline, for any batch size,
//   and texts of byte ranges concatenate.
// want_reads = 2 (READS_AS_RECORDS) selects by the same rule without the l_seq condition - a record without SEQ is still a record -
// and writes, instead of text, the record's own bytes: its block_size word and the block_size bytes behind it, as they stand in the
// inflated stream (reads_record_bytes; a CIGAR kept in a CG:B,I tag stays there).  The GPU pipeline copies them in work items of
// READS_COPY_SLICE bytes.
#define READS_SEQ_CHARS "=ACMGRSVTWYHKDBN"
const int64_t READS_SLICE = 16384;          // bases per work item of the GPU pipeline (as COV_SLICE and QC_SLICE)

const int READS_AS_FASTQ = 1, READS_AS_RECORDS = 2;      // the values of want_reads
const int64_t READS_COPY_SLICE = 32768;     // record bytes per work item of the GPU pipeline in mode 2 (what a FASTQ item writes)

CORAL_QC_HD inline bool reads_takes_part(uint32_t flag, uint32_t l_seq, uint32_t exclude_flags, int mode = READS_AS_FASTQ) {
    return (mode == READS_AS_RECORDS || l_seq > 0) && (flag & exclude_flags) == 0;
}
CORAL_QC_HD inline long long reads_record_bytes(uint32_t block_size) { return 4ll + block_size; }
// The order of a coordinate-ordered records request (reads_order = 1; want_reads = 2 only): ascending by this key, records with
// equal keys in their input order (stable).  tid = -1 becomes 0xffffffff - records without coordinates go last -, and at an equal
// position the forward strand comes before the reverse strand: the order `samtools sort` documents.  It refines
// IndexPartial::sort_word, so a file written in this order can always be indexed.
const int READS_ORDER_FILE = 0, READS_ORDER_COORDINATE = 1;      // the values of reads_order
CORAL_QC_HD inline unsigned long long reads_sort_key(int32_t tid, int32_t pos, uint32_t flag) {
    return ((unsigned long long)(uint32_t)tid << 32) | ((unsigned long long)((uint32_t)pos + 1u) << 1) | ((flag >> 4) & 1u);
}
CORAL_QC_HD inline uint32_t reads_complement(uint32_t code) {      // A <-> T, C <-> G, M <-> K, ...: the four bits reversed
    return ((code & 1u) << 3) | ((code & 2u) << 1) | ((code & 4u) >> 1) | ((code & 8u) >> 3);
}
CORAL_QC_HD inline uint8_t reads_seq_char(uint32_t code, bool reverse) { return (uint8_t)READS_SEQ_CHARS[reverse ? reads_complement(code & 15u) : (code & 15u)]; }
CORAL_QC_HD inline uint8_t reads_qual_char(uint32_t q) { return (uint8_t)((q < 93u ? q : 93u) + 33u); }
CORAL_QC_HD inline long long reads_text_bytes(uint32_t l_seq, uint32_t l_read_name) { return 2ll * l_seq + l_read_name + 5; }
// characters of the codes 8 * half .. 8 * half + 7 (complemented first with `reverse`) as one little-endian word
CORAL_QC_HD constexpr unsigned long long reads_char_table(int half, bool reverse) {
    unsigned long long w = 0;
    for (int k = 0; k < 8; ++k) {
        const unsigned c = (unsigned)(8 * half + k);
        const unsigned r = ((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3);
        w |= (unsigned long long)(unsigned char)READS_SEQ_CHARS[reverse ? r : c] << (8 * k);
    }
    return w;
}
// [pos, end) meets a non-empty one of the n sorted, disjoint segments (tid, lo, hi)
CORAL_QC_HD inline bool reads_meets_segment(const int32_t *tid, const int32_t *lo, const int32_t *hi, int n, int32_t t, long long pos, long long end) {
    if (t < 0) return false;
    int a = 0, b = n;
    while (a < b) {                            // first segment with tid > t, or tid == t and hi > pos
        const int m = (a + b) >> 1;
        if (tid[m] < t || (tid[m] == t && (long long)hi[m] <= pos)) a = m + 1; else b = m;
    }
    for (; a < n && tid[a] == t && (long long)lo[a] < end; ++a)
        if (hi[a] > lo[a]) return true;
    return false;
}
// `name` (len bytes, no NUL) is one of the n names blob[off[k] .. off[k + 1]), sorted ascending by their bytes, then by length
CORAL_QC_HD inline bool reads_name_listed(const uint8_t *blob, const int64_t *off, long long n, const uint8_t *name, uint32_t len) {
    long long a = 0, b = n;
    while (a < b) {
        const long long m = (a + b) >> 1;
        const uint8_t *s = blob + off[m];
        const uint32_t sl = (uint32_t)(off[m + 1] - off[m]), common = sl < len ? sl : len;
        int c = 0;
        for (uint32_t k = 0; k < common && c == 0; ++k) c = (int)s[k] - (int)name[k];
        if (c == 0) c = sl < len ? -1 : sl > len ? 1 : 0;
        if (c == 0) return true;
        if (c < 0) a = m + 1; else b = m;
    }
    return false;
}

struct ReadsRule {                          // the request, checked and copied (parse_request)
    bool on = false;
    int mode = READS_AS_FASTQ;              // READS_AS_FASTQ: the text; READS_AS_RECORDS: the records' own bytes
    int order = READS_ORDER_FILE;           // READS_ORDER_COORDINATE (mode READS_AS_RECORDS only): sorted by reads_sort_key, stable
    uint32_t exclude_flags = 0;
    std::vector<int32_t> tid, lo, hi;       // no segment: no region limit
    std::vector<uint8_t> names;             // no name: no name limit
    std::vector<int64_t> name_off;          // n + 1
    long long n_names() const { return name_off.empty() ? 0 : (long long)name_off.size() - 1; }
    // the whole rule on a record's bytes (r points at block_size; end = bam_endpos of the record)
    bool written(const uint8_t *r, int32_t end) const {
        uint16_t flag; uint32_t l_seq; int32_t t, pos;
        memcpy(&t, r + 4, 4); memcpy(&pos, r + 8, 4); memcpy(&flag, r + 18, 2); memcpy(&l_seq, r + 20, 4);
        if (!reads_takes_part(flag, l_seq, exclude_flags, mode)) return false;
        if (!tid.empty() && !reads_meets_segment(tid.data(), lo.data(), hi.data(), (int)tid.size(), t, pos, end)) return false;
        return n_names() == 0 || reads_name_listed(names.data(), name_off.data(), n_names(), r + 36, (uint32_t)r[12] - 1u);
    }
};

// reads_sort_key of a record's bytes (r points at block_size): tid at +4, pos at +8, flag at +18
inline unsigned long long reads_sort_key_at(const uint8_t *r) {
    int32_t tid, pos; uint16_t flag;
    memcpy(&tid, r + 4, 4); memcpy(&pos, r + 8, 4); memcpy(&flag, r + 18, 2);
    return reads_sort_key(tid, pos, flag);
}

// the text of one record (r points at block_size; its fields have been checked to lie inside it), appended to `out`
inline void reads_append_text(const uint8_t *r, std::vector<uint8_t> &out) {
    uint16_t flag, n_cigar_op; uint32_t l_seq;
    memcpy(&n_cigar_op, r + 16, 2); memcpy(&flag, r + 18, 2); memcpy(&l_seq, r + 20, 4);
    const uint32_t l_read_name = r[12];
    const bool reverse = (flag & 0x10u) != 0;
    const uint8_t *seq = r + 36 + l_read_name + 4ull * n_cigar_op, *qual = seq + ((size_t)l_seq + 1) / 2;
    const size_t at = out.size();
    out.resize(at + (size_t)reads_text_bytes(l_seq, l_read_name));
    uint8_t *w = out.data() + at;
    *w++ = '@';
    memcpy(w, r + 36, l_read_name - 1); w += l_read_name - 1;
    *w++ = '\n';
    for (uint32_t j = 0; j < l_seq; ++j) {
        const uint32_t s = reverse ? l_seq - 1 - j : j;
        *w++ = reads_seq_char((s & 1) ? (seq[s >> 1] & 15u) : (uint32_t)(seq[s >> 1] >> 4), reverse);
    }
    *w++ = '\n'; *w++ = '+'; *w++ = '\n';
    const bool has_qual = qual[0] != 0xff;
    for (uint32_t j = 0; j < l_seq; ++j) *w++ = has_qual ? reads_qual_char(qual[reverse ? l_seq - 1 - j : j]) : (uint8_t)'"';
    *w++ = '\n';
}

// the bytes of one record as they stand (r points at block_size), appended to `out`: what want_reads = 2 writes
inline void reads_append_record(const uint8_t *r, std::vector<uint8_t> &out) {
    uint32_t block_size;
    memcpy(&block_size, r, 4);
    const size_t at = out.size(), n = (size_t)reads_record_bytes(block_size);
    out.resize(at + n);
    memcpy(out.data() + at, r, n);
}

// A span of virtual offsets [beg, end) (span_beg / span_end of a coral_bam_request_t): the records that START in it.
struct Span {
    uint64_t beg = 0, end = 0;
};

struct Decoded {
    IndexPartial idx;                       // BAI index request (empty without one)
    QcPartial qc;                           // read-QC request (empty without one)
    DepthPartial depth;                     // binned-depth request (empty without one)
    std::vector<int32_t> tid, pos, end, flag, mapq, qlen, has_seq, nm, name_id, n_cigar;
    std::vector<int64_t> cigar_off{0}, sa_off{0};
    std::vector<uint32_t> cigar;
    std::vector<int32_t> sa;      // 8 per row: tid, pos1, strand, c5, m, x, c3, mapq   (c5 = -2: unparseable shape)
    std::vector<int32_t> sa_nm;
    std::vector<int64_t> na_rec;
    std::vector<int32_t> na_pos;
    coral_names::NameIndex names;           // read names: blob + offsets, ids in first-seen order (coral_names.h)
    std::vector<std::string> ref_names;
    std::vector<int32_t> ref_lens;
    std::string error;
    bool bad_request = false;               // `error` is about the request, not the file (a rule that needs the header)
    // statistics of the decode (coral_bam_decode_stats)
    int64_t compressed_bytes = 0, uncompressed_bytes = 0, n_blocks = 0;
    double seconds = 0.0;
    std::vector<int64_t> cov;               // window-coverage counts per segment (coral_bam_coverage_result)
    bool has_pileup = false;                // a pileup request (per_base of a coral_bam_request_t; it may hold no position)
    std::vector<uint32_t> pileup;           // its table [positions in segment order][A, C, G, T] (coral_bam_pileup_result)
    bool has_reads = false;                 // a reads request (it may have written no record)
    std::vector<uint8_t> reads_text;        // its FASTQ text (want_reads = 2: the records' bytes), the written records in file order (coral_bam_reads_fill)
    std::vector<int64_t> reads_off{0};      // where every written record starts in it, n + 1 entries
    std::vector<int64_t> reads_runs;        // coordinate order, GPU pipeline: the written record each batch's sorted run begins at
    bool reads_in_file = false;             // GPU pipeline with a file sink (coral_bam_sink_t): the records went to a file; nothing of them
    int64_t reads_file_records = 0, reads_file_bytes = 0;      //   is kept here but their number and their inflated bytes
};

struct Partial {   // what stage 3 produces for one chunk
    std::vector<int32_t> tid, pos, end, flag, mapq, qlen, has_seq, nm, n_cigar;
    std::vector<uint32_t> cigar;            // padded per record
    std::vector<int64_t> cigar_len;         // padded op count per record
    std::vector<int32_t> sa, sa_nm, sa_cnt;
    std::vector<int64_t> na_rec_local;
    std::vector<int32_t> na_pos;
    std::vector<char> names;                // NUL-separated
    std::vector<int64_t> cov;               // window-coverage counts of the chunk's records (per segment; empty without a request)
    std::vector<int64_t> qc_sum, qc_hist;   // read-QC request: qual_sum per record, the chunk's 256-bin histogram (empty without a request)
    std::vector<uint8_t> reads_text;        // reads request: the text (or bytes) of the chunk's written records and its length per written record
    std::vector<int64_t> reads_len;
    std::string error;
};

inline uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint16_t rd16(const uint8_t *p) { uint16_t v; memcpy(&v, p, 2); return v; }

static const int REF_ADV[16] = {1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const int IS_ALN[16] = {1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const int QRY_ADV[16] = {1, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0};

typedef std::unordered_map<std::string, int> RefIds;

// A window-coverage request (the segments of a coral_bam_request_t): pysam count_coverage summed over the four
// bases, for n sorted, pairwise disjoint half-open segments (tid, lo, hi) — the caller cuts its (possibly overlapping) windows
// at every start and stop and sums the segments back.  A base counts when the record is on the segment's contig (with
// filter_all: none of the flags 0x4 | 0x100 | 0x200 | 0x400), has SEQ, the base is an aligned (M / = / X) base inside the
// segment, its SEQ code is A, C, G or T, and either threshold is 0 or the record has QUAL (first byte not 0xff) and
// QUAL >= threshold there.
// A pileup request (per_base of the request) is the same rule split by position and base: a counted base adds 1 to
// table[(seg_off[segment] + position - lo[segment]) * 4 + b], b = 0..3 for the SEQ codes 1, 2, 4, 8 (A, C, G, T); the
// per-segment counts of such a request are the sums of the table (pileup_segment_sums), not counted on their own.
const int64_t PILEUP_MAX_POSITIONS = 1ll << 28;     // 4 x 2^28 counters: int32-indexable, a table of at most 4 GiB

CORAL_QC_HD inline bool pileup_base(uint32_t code, uint32_t *b) {      // SEQ code -> column of the table; false: not A, C, G or T
    *b = (code >> 1) - (code >> 3);                           // 1, 2, 4, 8 -> 0, 1, 2, 3
    return code != 0 && (code & (code - 1)) == 0;
}

struct CovTable {
    std::vector<int32_t> tid, lo, hi;
    int32_t threshold = 0;
    bool filter_all = false;
    bool per_base = false;
    std::vector<int64_t> seg_off;           // per_base: positions in front of every segment, n + 1 entries
    size_t size() const { return tid.size(); }
    int64_t n_pos() const { return seg_off.empty() ? 0 : seg_off.back(); }
    // first segment at or after (t, pos) in (tid, hi) order: tid > t, or tid == t and hi > pos
    size_t first(int32_t t, int64_t pos, size_t from = 0) const {
        size_t a = from, b = tid.size();
        while (a < b) {
            const size_t m = (a + b) / 2;
            if (tid[m] < t || (tid[m] == t && hi[m] <= pos)) a = m + 1; else b = m;
        }
        return a;
    }
};

// Validate a request (sorted by (tid, lo), disjoint, lo <= hi, threshold 0..255) and copy it; false: `err` says why.
inline bool make_cov_table(int32_t n_seg, const int32_t *tid, const int32_t *lo, const int32_t *hi, int32_t threshold,
                           int32_t read_callback, CovTable &T, std::string &err) {
    if (n_seg < 0 || (n_seg > 0 && (!tid || !lo || !hi))) { err = "coverage request: bad segment arrays"; return false; }
    if (threshold < 0 || threshold > 255) { err = "coverage request: the quality threshold must be 0..255"; return false; }
    if (read_callback != 0 && read_callback != 1) { err = "coverage request: read_callback must be 0 (nofilter) or 1 (all)"; return false; }
    for (int32_t k = 0; k < n_seg; ++k) {
        if (tid[k] < 0 || lo[k] < 0 || hi[k] < lo[k]) { err = "coverage request: bad segment"; return false; }
        if (k > 0 && (tid[k] < tid[k - 1] || (tid[k] == tid[k - 1] && lo[k] < hi[k - 1]))) {
            err = "coverage request: segments must be sorted by (tid, start) and disjoint";
            return false;
        }
    }
    T.tid.assign(tid, tid + n_seg);
    T.lo.assign(lo, lo + n_seg);
    T.hi.assign(hi, hi + n_seg);
    T.threshold = threshold;
    T.filter_all = read_callback == 1;
    return true;
}

// What one decode is asked for: a coral_bam_request_t, checked and copied (parse_request).  Both pipelines take it.
struct Request {
    int32_t rank = 0, world = 1;            // the byte range (0, 1 on a span decode: spans are not sharded)
    bool span_mode = false;                 // only the records that start inside `spans`
    std::vector<Span> spans;
    bool has_cov = false;                   // a window-coverage request (it may have no segment)
    CovTable cov;
    bool want_index = false, want_qc = false;
    int32_t depth_bin = 0, depth_min_mapq = 0, depth_exclude_flags = 0;      // a binned-depth request (depth_bin > 0; the bins need the header: DepthPartial::init)
    bool depth_count_deletions = false;
    ReadsRule reads;                        // a reads request (reads.on)
    KeepRule keep;                          // the record filter (not active: every record is kept)
    const CovTable *cov_table() const { return has_cov ? &cov : nullptr; }
};

// Every argument rule of a request but one (the spans lie inside the file: spans_inside_file); false: `err` says why.
inline bool parse_request(const coral_bam_request_t *q, Request &R, std::string &err) {
    if (!q) { err = "request: null pointer"; return false; }
    R.want_index = q->want_index != 0;
    R.want_qc = q->want_qc != 0;
    if (q->depth_bin < 0) { err = "binned-depth request: depth_bin must be >= 1 (0: no request)"; return false; }
    if (q->depth_bin > 0) {
        if (q->depth_min_mapq < 0 || q->depth_min_mapq > 255) { err = "binned-depth request: min_mapq must be 0..255"; return false; }
        if (q->depth_exclude_flags < 0 || q->depth_exclude_flags > 0xffff) { err = "binned-depth request: exclude_flags must be 0..0xffff"; return false; }
        if (q->depth_count_deletions != 0 && q->depth_count_deletions != 1) { err = "binned-depth request: count_deletions must be 0 or 1"; return false; }
        if (q->n_spans >= 0) { err = "request: a binned-depth request does not go with a span decode"; return false; }
        R.depth_bin = q->depth_bin;
        R.depth_min_mapq = q->depth_min_mapq;
        R.depth_exclude_flags = q->depth_exclude_flags;
        R.depth_count_deletions = q->depth_count_deletions != 0;
    }
    if (q->want_reads != 0) {
        ReadsRule &W = R.reads;
        if (q->want_reads != READS_AS_FASTQ && q->want_reads != READS_AS_RECORDS) { err = "reads request: want_reads must be 0, 1 or 2"; return false; }
        if (R.want_index) { err = "request: want_reads does not go with want_index (an index request decodes every record of the file, a reads request a selection)"; return false; }
        if (q->reads_exclude_flags < 0 || q->reads_exclude_flags > 0xffff) { err = "reads request: reads_exclude_flags must be 0..0xffff"; return false; }
        if (q->reads_n_seg < 0 || (q->reads_n_seg > 0 && (!q->reads_seg_tid || !q->reads_seg_start || !q->reads_seg_end))) { err = "reads request: bad reads_seg arrays"; return false; }
        for (int32_t k = 0; k < q->reads_n_seg; ++k) {
            const int32_t *t = q->reads_seg_tid, *lo = q->reads_seg_start, *hi = q->reads_seg_end;
            if (t[k] < 0 || lo[k] < 0 || hi[k] < lo[k]) { err = "reads request: bad segment in reads_seg"; return false; }
            if (k > 0 && (t[k] < t[k - 1] || (t[k] == t[k - 1] && lo[k] < hi[k - 1]))) { err = "reads request: the reads_seg segments must be sorted by (tid, start) and disjoint"; return false; }
        }
        if (q->reads_n_names < 0 || (q->reads_n_names > 0 && (!q->reads_names || !q->reads_name_off))) { err = "reads request: bad reads_names arrays"; return false; }
        for (int32_t k = 0; k < q->reads_n_names; ++k) {
            const int64_t *o = q->reads_name_off;
            const int64_t len = o[k + 1] - o[k];
            if (o[k] < 0 || len < 1 || len > 254) { err = "reads request: every name of reads_names must have 1..254 bytes"; return false; }
            if (k > 0) {                       // strictly ascending: by bytes, a prefix in front of what it is a prefix of
                const int64_t pl = o[k] - o[k - 1];
                const int c = memcmp(q->reads_names + o[k - 1], q->reads_names + o[k], (size_t)std::min(pl, len));
                if (c > 0 || (c == 0 && pl >= len)) { err = "reads request: reads_names must be sorted ascending (bytes, then length) without duplicates"; return false; }
            }
        }
        W.on = true;
        W.mode = q->want_reads;
        W.exclude_flags = (uint32_t)q->reads_exclude_flags;
        if (q->reads_n_seg > 0) {
            W.tid.assign(q->reads_seg_tid, q->reads_seg_tid + q->reads_n_seg);
            W.lo.assign(q->reads_seg_start, q->reads_seg_start + q->reads_n_seg);
            W.hi.assign(q->reads_seg_end, q->reads_seg_end + q->reads_n_seg);
        }
        if (q->reads_n_names > 0) {
            W.name_off.assign(q->reads_name_off, q->reads_name_off + q->reads_n_names + 1);
            W.names.assign(q->reads_names + W.name_off.front(), q->reads_names + W.name_off.back());
            const int64_t first = W.name_off.front();
            for (int64_t &o : W.name_off) o -= first;
        }
    }
    if (q->n_spans >= 0) {
        if (q->n_spans > 0 && (!q->span_beg || !q->span_end)) { err = "request: bad span arrays"; return false; }
        if (R.want_index || R.want_qc) { err = "request: an index or read-QC request does not go with a span decode"; return false; }
        for (int32_t k = 0; k < q->n_spans; ++k) {
            if (q->span_end[k] <= q->span_beg[k] || (k > 0 && q->span_beg[k] < q->span_end[k - 1])) {
                err = "request: the spans must be sorted, disjoint and non-empty";
                return false;
            }
            R.spans.push_back(Span{q->span_beg[k], q->span_end[k]});
        }
        R.span_mode = true;                   // (not sharded: rank 0 of 1 whatever the request says)
    } else {
        if (q->world < 1 || q->rank < 0 || q->rank >= q->world) { err = "request: needs world >= 1 and 0 <= rank < world"; return false; }
        R.rank = q->rank;
        R.world = q->world;
    }
    if (q->keep_min_mapq < 0 || q->keep_min_mapq > 255) { err = "record filter: keep_min_mapq must be 0..255"; return false; }
    if (q->keep_min_seq_length < 0 || q->keep_min_seq_length > (1 << 29)) { err = "record filter: keep_min_seq_length must be 0..2^29"; return false; }
    if (q->keep_require_flags < 0 || q->keep_require_flags > 0xffff) { err = "record filter: keep_require_flags must be 0..0xffff"; return false; }
    if (q->keep_exclude_flags < 0 || q->keep_exclude_flags > 0xffff) { err = "record filter: keep_exclude_flags must be 0..0xffff"; return false; }
    R.keep.min_mapq = (uint32_t)q->keep_min_mapq; R.keep.min_seq_length = (uint32_t)q->keep_min_seq_length;
    R.keep.require_flags = (uint32_t)q->keep_require_flags; R.keep.exclude_flags = (uint32_t)q->keep_exclude_flags;
    if (R.keep.active() && R.want_index) {
        err = "request: a record filter does not go with an index request (the virtual offsets of a file that holds only the kept records do not exist)";
        return false;
    }
    R.has_cov = q->n_seg >= 0;
    if (q->per_base != 0 && !R.has_cov) { err = "pileup request: per_base needs segments (n_seg >= 0)"; return false; }
    if (R.has_cov && !make_cov_table(q->n_seg, q->seg_tid, q->seg_start, q->seg_end, q->quality_threshold, q->read_callback, R.cov, err)) return false;
    if (q->per_base != 0) {
        CovTable &T = R.cov;
        T.per_base = true;
        T.seg_off.assign(1, 0);
        for (size_t k = 0; k < T.size(); ++k) T.seg_off.push_back(T.seg_off.back() + ((int64_t)T.hi[k] - T.lo[k]));
        if (T.n_pos() > PILEUP_MAX_POSITIONS) { err = "pileup request: the segments hold more than 2^28 positions"; return false; }
    }
    if (q->reads_order != READS_ORDER_FILE && q->reads_order != READS_ORDER_COORDINATE) { err = "reads request: reads_order must be 0 (file order) or 1 (coordinate order)"; return false; }
    if (q->reads_order == READS_ORDER_COORDINATE && !(R.reads.on && R.reads.mode == READS_AS_RECORDS)) {
        err = "reads request: reads_order = 1 sorts records: it needs want_reads = 2";
        return false;
    }
    R.reads.order = q->reads_order;
    return true;
}

// The per-segment counts of a pileup request: the sums of the table over every segment's positions and the four bases.
inline void pileup_segment_sums(const CovTable &T, const uint32_t *table, std::vector<int64_t> &counts) {
    counts.assign(T.size(), 0);
    for (size_t t = 0; t < T.size(); ++t) {
        int64_t c = 0;
        for (int64_t k = 4 * T.seg_off[t]; k < 4 * T.seg_off[t + 1]; ++k) c += table[k];
        counts[t] = c;
    }
}

// The rule that needs the file: every span begins at a block inside the file and ends at one or at the file's end.
inline bool spans_inside_file(const Request &R, uint64_t file_size, std::string &err) {
    for (const Span &s : R.spans)
        if ((s.beg >> 16) >= file_size || (s.end >> 16) > file_size) { err = "request: a span of virtual offsets lies outside the file"; return false; }
    return true;
}

// The plain request of the rank-th of `world` byte ranges.
inline coral_bam_request_t range_request(int32_t rank, int32_t world) {
    coral_bam_request_t q;
    memset(&q, 0, sizeof(q));
    q.rank = rank;
    q.world = world;
    q.n_spans = q.n_seg = -1;
    return q;
}

// Add one record's counted bases to counts[segment] or, for a pileup request (T.per_base), to `table` - shared by the
// threads that parse chunks, hence the atomic add (host pipeline; ops = the real CIGAR, CG tag already resolved).
inline void count_record_coverage(const CovTable &T, int32_t refID, int64_t pos, uint32_t flag, uint32_t l_seq, const uint32_t *ops,
                                  uint32_t n_ops, const uint8_t *seq, const uint8_t *qual, int64_t *counts, uint32_t *table = nullptr) {
    if (refID < 0 || l_seq == 0 || n_ops == 0 || T.size() == 0) return;
    if (T.filter_all && (flag & 0x704u)) return;
    const uint32_t thr = (uint32_t)T.threshold;
    if (thr > 0 && qual[0] == 0xff) return;                // no QUAL: pysam's query_qualities is None
    size_t s = T.first(refID, pos);
    int64_t q = 0, r = pos;
    for (uint32_t k = 0; k < n_ops; ++k) {
        if (s >= T.size() || T.tid[s] != refID) return;     // no segment left on this contig
        const uint32_t op = ops[k] & 15, len = ops[k] >> 4;
        if (IS_ALN[op] && len) {
            const int64_t r1 = r + len;
            s = T.first(refID, r, s);
            for (size_t t = s; t < T.size() && T.tid[t] == refID && T.lo[t] < r1; ++t) {
                const int64_t a = std::max<int64_t>(r, T.lo[t]), b = std::min<int64_t>(r1, T.hi[t]);
                int64_t c = 0;
                for (int64_t x = a; x < b; ++x) {
                    const uint64_t qi = (uint64_t)(q + (x - r));
                    if (qi >= l_seq) break;
                    const uint8_t code = (qi & 1) ? (seq[qi >> 1] & 15) : (seq[qi >> 1] >> 4);
                    uint32_t b;
                    const bool counted = pileup_base(code, &b) && qual[qi] >= thr;
                    c += counted;
                    if (counted && T.per_base) __atomic_fetch_add(table + 4 * (T.seg_off[t] + (x - T.lo[t])) + b, 1u, __ATOMIC_RELAXED);
                }
                if (!T.per_base) counts[t] += c;
            }
        }
        if (QRY_ADV[op]) q += len;
        if (REF_ADV[op]) r += len;
    }
}

// Tokenise one SA entry "rname,pos,strand,CIGAR,mapQ,NM" into 8 ints + nm.  The CIGAR must be
// [c5 S] m M [x I | x D] [c3 S]; anything else containing S and M is marked c5 = -2 (the reference raises
// KeyError for it, cigar_parsing.py:255); a CIGAR without S or without M gets c5 = c3 = 0 / m = 0 as parsed.
inline bool parse_sa_entry(const char *s, const char *e, const RefIds &ref_id, int32_t out[8], int32_t *nm) {
    const char *f[6];
    const char *fe[6];
    int nf = 0;
    const char *p = s;
    f[0] = s;
    for (; p < e && nf < 6; ++p)
        if (*p == ',') {
            fe[nf++] = p;
            if (nf < 6) f[nf] = p + 1;
        }
    if (nf == 5) fe[nf++] = e;
    if (nf != 6) return false;
    auto it = ref_id.find(std::string(f[0], fe[0]));
    out[0] = (it == ref_id.end()) ? -1 : it->second;
    auto to_int = [](const char *a, const char *b) {
        bool neg = a < b && *a == '-';
        if (neg || (a < b && *a == '+')) ++a;
        int64_t v = 0;
        for (; a < b && *a >= '0' && *a <= '9'; ++a) v = v * 10 + (*a - '0');
        return (int32_t)(neg ? -v : v);
    };
    out[1] = to_int(f[1], fe[1]);
    out[2] = (*f[2] == '-') ? 1 : 0;
    out[7] = to_int(f[4], fe[4]);
    *nm = to_int(f[5], fe[5]);
    // CIGAR
    int64_t nums[8];
    char ops[8];
    int n = 0;
    int64_t cur = 0;
    bool overflow = false;
    for (const char *c = f[3]; c < fe[3]; ++c) {
        if (*c >= '0' && *c <= '9') cur = cur * 10 + (*c - '0');
        else {
            if (n < 8) { nums[n] = cur; ops[n] = *c; ++n; } else overflow = true;
            cur = 0;
        }
    }
    bool hasS = false, hasM = false;
    for (int i = 0; i < n; ++i) { hasS |= ops[i] == 'S'; hasM |= ops[i] == 'M'; }
    out[3] = out[4] = out[5] = out[6] = 0;
    if (!hasS || !hasM) {      // reference: the whole read becomes ([], [], []) (cigar_parsing.py:248-253)
        out[4] = 0;
        return true;
    }
    int i = 0;
    bool ok = !overflow;
    if (ok && i < n && ops[i] == 'S') out[3] = (int32_t)nums[i++];
    if (ok && i < n && ops[i] == 'M') out[4] = (int32_t)nums[i++]; else ok = false;
    if (ok && i < n && (ops[i] == 'I' || ops[i] == 'D')) { out[5] = (ops[i] == 'I') ? (int32_t)nums[i] : -(int32_t)nums[i]; ++i; }
    if (ok && i < n && ops[i] == 'S') out[6] = (int32_t)nums[i++];
    if (!ok || i != n || (out[3] == 0 && out[6] == 0)) { out[3] = -2; }
    return true;
}

// true when every 4-bit base code of the packed sequence is A, C, G or T (1, 2, 4, 8); 8 bytes at a time: a nibble x is a
// power of two iff x != 0 and (x & (x - 1)) == 0
inline bool all_acgt(const uint8_t *seq, uint32_t l_seq) {
    const uint32_t full = l_seq / 2;
    uint32_t k = 0;
    const uint64_t LO = 0x0f0f0f0f0f0f0f0full, ONE = 0x0101010101010101ull;
    for (; k + 8 <= full; k += 8) {
        uint64_t w;
        memcpy(&w, seq + k, 8);
        const uint64_t a = w & LO, b = (w >> 4) & LO;
        // per byte (values 0..15): bad if zero or not a power of two
        const uint64_t a1 = (a - ONE) & LO & a, b1 = (b - ONE) & LO & b;          // x & (x - 1) per byte (no borrow across bytes for x >= 1;
        const uint64_t az = ((a | 0x1010101010101010ull) - ONE) & 0x1010101010101010ull;      // for x == 0 the borrow is caught by the zero test)
        const uint64_t bz = ((b | 0x1010101010101010ull) - ONE) & 0x1010101010101010ull;
        // az / bz have bit 4 set in every byte where x >= 1; a zero byte clears it
        if (a1 | b1 | (az ^ 0x1010101010101010ull) | (bz ^ 0x1010101010101010ull)) {
            // the fast test is conservative around borrows: confirm byte by byte
            for (uint32_t j = k; j < k + 8; ++j) {
                const uint8_t hi = seq[j] >> 4, lo = seq[j] & 15;
                if (!((hi == 1 || hi == 2 || hi == 4 || hi == 8) && (lo == 1 || lo == 2 || lo == 4 || lo == 8))) return false;
            }
        }
    }
    for (; k < full; ++k) {
        const uint8_t hi = seq[k] >> 4, lo = seq[k] & 15;
        if (!((hi == 1 || hi == 2 || hi == 4 || hi == 8) && (lo == 1 || lo == 2 || lo == 4 || lo == 8))) return false;
    }
    if (l_seq & 1) {
        const uint8_t hi = seq[full] >> 4;
        if (!(hi == 1 || hi == 2 || hi == 4 || hi == 8)) return false;
    }
    return true;
}

// Decode one BAM record (p points at refID, i.e. after block_size) into the partial.
// With `cov`, the record's bases also go into o.cov (sized by the caller) or, for a pileup request, into `pileup` (the decode's table).
// With `qc`, the record's qual_sum goes to o.qc_sum and its QUAL bytes into o.qc_hist (256 bins, sized by the caller).
// With `depth`, the record goes into the tables of the binned-depth request (the decode's, shared by the parse tasks).
inline bool decode_record(const uint8_t *p, uint32_t block_size, const RefIds &ref_id, Partial &o, std::string &err,
                          const CovTable *cov = nullptr, bool qc = false, uint32_t *pileup = nullptr, DepthPartial *depth = nullptr) {
    if (block_size < 32) { err = "record shorter than its fixed fields"; return false; }
    const int32_t refID = (int32_t)rd32(p), pos = (int32_t)rd32(p + 4);
    const uint32_t l_read_name = p[8], mapq = p[9];
    uint32_t n_cigar_op = rd16(p + 12);
    const uint32_t flag = rd16(p + 14), l_seq = rd32(p + 16);
    const uint8_t *name = p + 32;
    const uint8_t *cig = name + l_read_name;
    const uint8_t *seq = cig + 4ull * n_cigar_op;
    const uint8_t *qual = seq + ((uint64_t)l_seq + 1) / 2;
    const uint8_t *tags = qual + l_seq;
    const uint8_t *endp = p + block_size;
    if (tags > endp || l_read_name == 0) { err = "record fields overrun the record"; return false; }
    if (qc) {
        int64_t sum = -1;
        const uint8_t *q = p - 4 + qc_qual_offset(l_read_name, n_cigar_op, l_seq);
        if (qc_is_read(flag, l_seq) && qc_has_quality(q[0])) {
            sum = 0;
            int64_t *h = o.qc_hist.data();
            for (uint32_t k = 0; k < l_seq; ++k) { sum += q[k]; ++h[q[k]]; }
        }
        o.qc_sum.push_back(sum);
    }
    // tags: NM, SA, CG
    int32_t nm = 0;
    const char *sa = nullptr;
    const uint8_t *cg = nullptr;
    uint32_t cg_n = 0;
    for (const uint8_t *t = tags; t + 3 <= endp;) {
        const char a = (char)t[0], b = (char)t[1], ty = (char)t[2];
        const uint8_t *v = t + 3;
        size_t sz = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': { const uint8_t *z = (const uint8_t *)memchr(v, 0, (size_t)(endp - v)); sz = z ? (size_t)(z - v) + 1 : (size_t)(endp - v) + 1; break; }
            case 'B': {
                if (v + 5 > endp) { err = "truncated B tag"; return false; }
                const char sub = (char)v[0];
                const uint32_t cnt = rd32(v + 1);
                const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                if (a == 'C' && b == 'G' && sub == 'I') { cg = v + 5; cg_n = cnt; }
                sz = 5 + es * (size_t)cnt;
                break;
            }
            default: err = "unknown tag type"; return false;
        }
        if (v + sz > endp) { err = "tag overruns the record"; return false; }
        if (a == 'N' && b == 'M') {
            switch (ty) {
                case 'c': nm = (int8_t)v[0]; break;
                case 'C': nm = v[0]; break;
                case 's': nm = (int16_t)rd16(v); break;
                case 'S': nm = rd16(v); break;
                case 'i': case 'I': nm = (int32_t)rd32(v); break;
                default: break;
            }
        } else if (a == 'S' && b == 'A' && ty == 'Z') {
            sa = (const char *)v;
        }
        t = v + sz;
    }
    // long CIGARs live in the CG tag (SAM spec §4.2.2): placeholder is <l_seq>S<rlen>N
    const uint8_t *cig_src = cig;
    if (cg && n_cigar_op == 2 && (rd32(cig) & 15u) == 4 && (rd32(cig) >> 4) == l_seq && (rd32(cig + 4) & 15u) == 3) {
        cig_src = cg;
        n_cigar_op = cg_n;
    }
    int64_t rlen = 0, qinf = 0;
    const size_t c0 = o.cigar.size();
    const size_t padded = ((size_t)n_cigar_op + 3) & ~(size_t)3;
    o.cigar.resize(c0 + padded);
    uint32_t *dst = o.cigar.data() + c0;
    if (n_cigar_op) memcpy(dst, cig_src, 4ull * n_cigar_op);
    for (size_t k = n_cigar_op; k < padded; ++k) dst[k] = 15u;
    for (uint32_t k = 0; k < n_cigar_op; ++k) {
        const uint32_t v = dst[k];
        rlen += REF_ADV[v & 15] ? (v >> 4) : 0;
        qinf += QRY_ADV[v & 15] ? (v >> 4) : 0;
    }
    o.cigar_len.push_back((int64_t)padded);
    if (cov) count_record_coverage(*cov, refID, pos, flag, l_seq, dst, n_cigar_op, seq, qual, o.cov.data(), pileup);
    if (depth) depth->add(refID, pos, flag, mapq, dst, n_cigar_op);
    if ((flag & 4) || n_cigar_op == 0) rlen = 0;                 // htslib bam_endpos
    o.tid.push_back(refID);
    o.pos.push_back(pos);
    o.end.push_back(pos + (int32_t)(rlen > 0 ? rlen : 1));
    o.flag.push_back((int32_t)flag);
    o.mapq.push_back((int32_t)mapq);
    o.has_seq.push_back(l_seq > 0 ? 1 : 0);
    o.qlen.push_back(l_seq > 0 ? (int32_t)l_seq : (int32_t)qinf);
    o.nm.push_back(nm);
    o.n_cigar.push_back((int32_t)n_cigar_op);
    o.names.insert(o.names.end(), (const char *)name, (const char *)name + l_read_name - 1);
    o.names.push_back('\0');
    // SA rows
    int32_t cnt = 0;
    if (sa) {
        const char *s = sa;
        while (*s) {
            const char *e = s;
            while (*e && *e != ';') ++e;
            if (e > s) {
                int32_t row[8], snm = 0;
                if (!parse_sa_entry(s, e, ref_id, row, &snm)) { err = "malformed SA entry"; return false; }
                o.sa.insert(o.sa.end(), row, row + 8);
                o.sa_nm.push_back(snm);
                ++cnt;
            }
            s = (*e == ';') ? e + 1 : e;
        }
    }
    o.sa_cnt.push_back(cnt);
    // aligned non-ACGT bases
    if (l_seq > 0 && !(flag & 4) && n_cigar_op > 0 && !all_acgt(seq, l_seq)) {
        int64_t q = 0, r = pos;
        const int64_t local = (int64_t)o.tid.size() - 1;
        for (uint32_t k = 0; k < n_cigar_op; ++k) {
            const uint32_t v = dst[k], op = v & 15, len = v >> 4;
            if (IS_ALN[op]) {
                for (uint32_t j = 0; j < len && q + j < l_seq; ++j) {
                    const uint64_t qi = (uint64_t)(q + j);
                    const uint8_t code = (qi & 1) ? (seq[qi >> 1] & 15) : (seq[qi >> 1] >> 4);
                    if (!(code == 1 || code == 2 || code == 4 || code == 8)) {
                        o.na_rec_local.push_back(local);
                        o.na_pos.push_back((int32_t)(r + j));
                    }
                }
            }
            if (QRY_ADV[op]) q += len;
            if (REF_ADV[op]) r += len;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// a small pool: tasks run on n - 1 threads and, while waiting, on the thread that waits
// ---------------------------------------------------------------------------------------------
class Pool {
public:
    explicit Pool(int n) {
        for (int i = 1; i < n; ++i) threads_.emplace_back([this] { loop(); });
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : threads_) t.join();
    }
    void submit(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> lk(m_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }
    bool help_one() {                          // run one queued task on the calling thread, if any
        std::function<void()> f;
        {
            std::lock_guard<std::mutex> lk(m_);
            if (q_.empty()) return false;
            f = std::move(q_.front());
            q_.pop_front();
        }
        f();
        return true;
    }

private:
    void loop() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (stop_ && q_.empty()) return;
                f = std::move(q_.front());
                q_.pop_front();
            }
            f();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    bool stop_ = false;
};

struct Flag {                                  // one-shot completion flag
    std::atomic<int> v{0};
    void set() { v.store(1, std::memory_order_release); }
    bool get() const { return v.load(std::memory_order_acquire) != 0; }
};

// ---------------------------------------------------------------------------------------------
// BGZF
// ---------------------------------------------------------------------------------------------
struct Block {
    uint64_t off;        // file offset of the block
    uint32_t hdr;        // header bytes (12 + xlen)
    uint32_t csize;      // whole block (BSIZE + 1)
    uint32_t isize;      // uncompressed bytes
};

// Parse a BGZF block header at `p` (n bytes available).  Returns false when it is not one.
inline bool bgzf_header(const uint8_t *p, uint64_t n, Block &b) {
    if (n < 18 || p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return false;
    const uint32_t xlen = rd16(p + 10);
    if (n < 12ull + xlen) return false;
    int bsize = -1;
    for (uint32_t i = 0; i + 4 <= xlen;) {
        const uint32_t slen = rd16(p + 12 + i + 2);
        if (p[12 + i] == 'B' && p[12 + i + 1] == 'C' && slen == 2 && i + 6 <= xlen) bsize = rd16(p + 12 + i + 4);
        i += 4 + slen;
    }
    if (bsize < 0) return false;
    const uint64_t csize = (uint64_t)bsize + 1;
    if (csize < 12ull + xlen + 8 || csize > n) return false;
    b.hdr = 12 + xlen;
    b.csize = (uint32_t)csize;
    b.isize = rd32(p + csize - 4);
    return b.isize <= 65536;
}

struct MappedFile {
    const uint8_t *data = nullptr;
    uint64_t size = 0;
    int fd = -1;
    bool open(const char *path, std::string &err) {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) { err = std::string("cannot open ") + path; return false; }
        struct stat st;
        if (fstat(fd, &st) != 0) { err = "cannot stat the file"; return false; }
        size = (uint64_t)st.st_size;
        if (size == 0) { err = "empty file"; return false; }
        void *p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) { err = "cannot map the file"; return false; }
        data = (const uint8_t *)p;
        (void)madvise(p, size, MADV_SEQUENTIAL);
        return true;
    }
    ~MappedFile() {
        if (data) munmap((void *)data, size);
        if (fd >= 0) ::close(fd);
    }
};

// First BGZF block starting at or after `from`: magic + BC subfield, and the two blocks that follow must parse as well.
inline bool find_block(const MappedFile &f, uint64_t from, uint64_t *at) {
    for (uint64_t p = from; p + 18 <= f.size; ++p) {
        if (f.data[p] != 31 || f.data[p + 1] != 139) continue;
        uint64_t q = p;
        bool ok = true;
        for (int k = 0; k < 3 && ok && q < f.size; ++k) {
            Block b;
            ok = bgzf_header(f.data + q, f.size - q, b);
            if (ok) q += b.csize;
        }
        if (ok) { *at = p; return true; }
    }
    return false;
}

inline bool inflate_block(z_stream &zs, const MappedFile &f, const Block &b, uint8_t *out) {
    if (b.isize == 0) return true;
    if (inflateReset(&zs) != Z_OK) return false;
    zs.next_in = (Bytef *)(f.data + b.off + b.hdr);
    zs.avail_in = (uInt)(b.csize - b.hdr - 8);
    zs.next_out = out;
    zs.avail_out = b.isize;
    const int rc = inflate(&zs, Z_FINISH);
    if (rc != Z_STREAM_END || zs.avail_out != 0) return false;
    // the trailer's CRC-32 of the inflated bytes (what htslib's bgzf_read_block checks; the GPU pipeline does the same)
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), out, b.isize) == rd32(f.data + b.off + b.csize - 8);
}

struct ZStream {
    z_stream zs;
    bool ok;
    ZStream() { memset(&zs, 0, sizeof(zs)); ok = inflateInit2(&zs, -15) == Z_OK; }
    ~ZStream() { if (ok) inflateEnd(&zs); }
};

// ---------------------------------------------------------------------------------------------
// plausibility of a BAM record at `p` (n bytes available): used to find the first record of a byte range
// ---------------------------------------------------------------------------------------------
inline bool plausible_record(const uint8_t *p, uint64_t n, int32_t n_ref, uint64_t *len) {
    if (n < 36) return false;
    const uint32_t bs = rd32(p);
    if (bs < 34 || bs > (1u << 29)) return false;
    const int32_t refID = (int32_t)rd32(p + 4), pos = (int32_t)rd32(p + 8);
    const uint32_t l_name = p[12], n_cig = rd16(p + 16), l_seq = rd32(p + 20);
    const int32_t mate = (int32_t)rd32(p + 24), mpos = (int32_t)rd32(p + 28);
    if (refID < -1 || refID >= n_ref || mate < -1 || mate >= n_ref || pos < -1 || mpos < -1) return false;
    if (l_name < 2 || l_seq > (1u << 29)) return false;
    const uint64_t fixed = 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + l_seq;
    if (fixed > bs) return false;
    if (n >= 36ull + l_name) {                                   // read name: printable, NUL-terminated
        const uint8_t *nm = p + 36;
        if (nm[l_name - 1] != 0) return false;
        for (uint32_t k = 0; k + 1 < l_name; ++k)
            if (nm[k] < 33 || nm[k] > 126) return false;
    }
    *len = 4ull + bs;
    return true;
}

// BAM header: magic, text, reference list (inflated from block 0 on, as many blocks as it takes).  Fills D.ref_names /
// D.ref_lens / ref_id and the header's length in the uncompressed stream.
inline bool read_bam_header(const MappedFile &f, Decoded &D, RefIds &ref_id, size_t *hdr_bytes) {
    std::vector<uint8_t> head;
    ZStream z;
    if (!z.ok) { D.error = "zlib init failed"; return false; }
    uint64_t at = 0;
    auto more = [&]() -> bool {
        Block b;
        if (at >= f.size || !bgzf_header(f.data + at, f.size - at, b)) return false;
        b.off = at;
        const size_t o = head.size();
        head.resize(o + b.isize);
        if (!inflate_block(z.zs, f, b, head.data() + o)) return false;
        at += b.csize;
        return true;
    };
    auto need = [&](size_t n) { while (head.size() < n) if (!more()) return false; return true; };
    if (!need(12) || memcmp(head.data(), "BAM\1", 4) != 0) { D.error = "not a BAM file"; return false; }
    const uint32_t l_text = rd32(head.data() + 4);
    if (!need(12 + (size_t)l_text)) { D.error = "truncated BAM header"; return false; }
    size_t cur = 8 + l_text;
    const uint32_t n_ref = rd32(head.data() + cur);
    cur += 4;
    for (uint32_t i = 0; i < n_ref; ++i) {
        if (!need(cur + 4)) { D.error = "truncated reference list"; return false; }
        const uint32_t l_name = rd32(head.data() + cur);
        if (!need(cur + 8 + (size_t)l_name)) { D.error = "truncated reference list"; return false; }
        std::string nm((const char *)head.data() + cur + 4, l_name ? l_name - 1 : 0);
        D.ref_lens.push_back((int32_t)rd32(head.data() + cur + 4 + l_name));
        ref_id[nm] = (int)i;
        D.ref_names.push_back(nm);
        cur += 8 + l_name;
    }
    *hdr_bytes = cur;
    return true;
}

void set_error(const std::string &msg);         // coral_bam_last_error() of the calling thread (defined in coral_bam.cpp)

}  // namespace coral_bam
