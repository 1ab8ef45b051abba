// coral_fastq_host.h - the host side of the FASTQ session: the host backend, one thread and a byte-wise state machine over
// coral_fastq_core.h that carries its state across feeds (what the kernels of coral_fastq.hip are compared against, and
// `device="cpu"` of coral_amd/fastq.py), and what both backends share: the rows of the listed reads (Rows), the positions of the
// '\n' bytes that close records in a piece (record_ends: the host's share of the device path) and the writer of the kept
// records' bytes (RecordWriter).  It stands in for the reference's scripts/report_nanopore_qc.py:35-48.  No HIP: g++ alone builds it.
#ifndef CORAL_FASTQ_HOST_H
#define CORAL_FASTQ_HOST_H

#include <errno.h>
#include <string.h>
#include <unistd.h>

#include <chrono>
#include <string>
#include <vector>

#include "coral_fastq_core.h"

namespace coral_fastq {

struct Stats {
    uint64_t records = 0, reads = 0, no_seq = 0, bases = 0, kept = 0, kept_bases = 0;
    uint64_t bad_offset = NO_OFFSET;
};

// The listed reads (records with a sequence), 13 bytes each, and the counters of every closed record.
struct Rows {
    Thresholds thr;
    std::vector<int32_t> length;
    std::vector<int64_t> qual_sum;
    std::vector<uint8_t> kept;
    Stats st;
    // a closed record; -> whether the filter keeps it
    bool close(uint64_t len, uint64_t qsum) {
        const bool k = keeps(thr, len, qsum);
        ++st.records;
        if (k) { ++st.kept; st.kept_bases += len; }
        if (len == 0) { ++st.no_seq; return k; }
        ++st.reads; st.bases += len;
        length.push_back((int32_t)len); qual_sum.push_back((int64_t)qsum); kept.push_back(k ? 1 : 0);
        return k;
    }
};

// The kept records' bytes, exactly as they were read.  Per piece: its bytes, the offsets behind the '\n' bytes that close its
// records and whether each is kept; the head of the record still open at the piece's end is saved until its tail arrives.
// Consecutive kept records go out in one write.
struct RecordWriter {
    int fd = -1;
    std::string head, error;
    double seconds = 0;

    bool put(const void *p, size_t n) {
        const char *c = (const char *)p;
        while (n > 0) {
            const ssize_t w = ::write(fd, c, n);
            if (w < 0) {
                if (errno == EINTR) continue;
                error = std::string("write to the output: ") + strerror(errno);
                return false;
            }
            c += w; n -= (size_t)w;
        }
        return true;
    }

    bool piece(const uint8_t *text, size_t n, const uint32_t *ends, const uint8_t *kept, size_t k) {
        if (fd < 0) return true;
        const auto t0 = std::chrono::steady_clock::now();
        bool good = true;
        size_t run_from = 0, run_to = 0, at = 0;            // the run of kept bytes that is not yet written
        for (size_t j = 0; j < k && good; ++j) {
            if (kept[j]) {
                if (j == 0 && !head.empty()) good = put(head.data(), head.size());
                if (run_to != at) { if (run_to > run_from) good = good && put(text + run_from, run_to - run_from); run_from = at; }
                run_to = ends[j];
            }
            at = ends[j];
        }
        if (good && run_to > run_from) good = put(text + run_from, run_to - run_from);
        if (k) head.clear();
        head.append((const char *)text + at, n - at);
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return good;
    }

    // the end of the stream: the record it closes, when one is open
    bool finish(bool closes, bool kept) {
        if (fd < 0) return true;
        const auto t0 = std::chrono::steady_clock::now();
        const bool good = !(closes && kept && !head.empty()) || put(head.data(), head.size());
        head.clear();
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return good;
    }
};

// The '\n' bytes of the next piece, found before it is copied: `ends` gets the offset behind every '\n' that closes a record,
// at most max_records of them: the piece ends behind the last one it may hold.  `lines` ('\n' bytes so far) and `first` (the
// last byte was one, or none was read) are the state in front of the piece and become the state behind what was taken.
// Returns the bytes taken.
inline size_t record_ends(uint64_t &lines, bool &first, const uint8_t *src, size_t n, size_t max_records, std::vector<uint32_t> &ends) {
    ends.clear();
    size_t at = 0;
    while (at < n) {
        const uint8_t *nl = (const uint8_t *)memchr(src + at, '\n', n - at);
        if (!nl) break;
        at = (size_t)(nl - src) + 1;
        if (phase_of(lines++) == 3) {
            ends.push_back((uint32_t)at);
            if (ends.size() == max_records) { first = true; return at; }
        }
    }
    if (n > 0) first = src[n - 1] == '\n';
    return n;
}

enum { FASTQ_OK = 0, FASTQ_FORMAT = 1, FASTQ_WRITE = 2 };

// One pass, one thread.  `hist` holds 256 zeroed counters, the caller's.
struct HostFastq {
    Rows rows;
    RecordWriter out;
    uint64_t *hist;
    uint64_t lines = 0, offset = 0, len = 0, qcnt = 0, qsum = 0;
    bool first = true, finished = false;
    int error = FASTQ_OK;
    std::string error_text;
    std::vector<uint32_t> ends;
    std::vector<uint8_t> kept;

    HostFastq(const Thresholds &t, int fd, uint64_t *hist_) : hist(hist_) { rows.thr = t; out.fd = fd; }

    int refuse(uint64_t at, const char *what) {
        rows.st.bad_offset = at;
        error_text = std::string(what) + " at byte " + std::to_string(at) + " (line " + std::to_string(lines + 1) + ")";
        return error = FASTQ_FORMAT;
    }

    bool close_record(uint64_t at) {
        if (!record_ok(len, qcnt)) { refuse(at, len > MAX_LENGTH ? "a read of more than 2^31 - 1 bases" : "a quality line that is not as long as its sequence, closed"); return false; }
        kept.push_back(rows.close(len, qsum) ? 1 : 0);
        len = qcnt = qsum = 0;
        return true;
    }

    int feed(const uint8_t *bytes, size_t n) {
        if (error != FASTQ_OK) return error;
        for (size_t done = 0; done < n && error == FASTQ_OK;) {          // in steps whose record ends fit uint32
            const size_t m = n - done < ((size_t)1 << 30) ? n - done : (size_t)1 << 30;
            const uint8_t *p = bytes + done;
            ends.clear(); kept.clear();
            for (size_t i = 0; i < m; ++i) {
                const uint8_t c = p[i];
                const Byte b = classify(phase_of(lines), first, c);
                first = false;
                if (b == BYTE_BAD) { refuse(offset + i, phase_of(lines) == 3 ? "a quality character outside 33 .. 126" : "a record line that does not start with '@', or a separator line that does not start with '+',"); break; }
                if (b == BYTE_BASE) ++len;
                else if (b == BYTE_QUAL) { ++qcnt; qsum += c - QUAL_BASE; ++hist[c - QUAL_BASE]; }
                else if (b == BYTE_END_LINE) { ++lines; first = true; }
                else if (b == BYTE_CLOSE) {
                    if (!close_record(offset + i)) break;
                    ends.push_back((uint32_t)(i + 1));
                    ++lines; first = true;
                }
            }
            if (error != FASTQ_OK) break;
            if (!out.piece(p, m, ends.data(), kept.data(), ends.size())) { error_text = out.error; return error = FASTQ_WRITE; }
            offset += m; done += m;
        }
        return error;
    }

    // the end of the stream
    int finish() {
        if (error != FASTQ_OK) return error;
        finished = true;
        const End e = end_of_stream(lines, first);
        if (e == END_BAD) return refuse(offset, "the stream ends inside the first three lines of a record,");
        bool k = false;
        if (e == END_CLOSES) {
            kept.clear();
            if (!close_record(offset)) return error;
            k = kept.back() != 0;
        }
        if (!out.finish(e == END_CLOSES, k)) { error_text = out.error; return error = FASTQ_WRITE; }
        return FASTQ_OK;
    }
};

}  // namespace coral_fastq
#endif /* CORAL_FASTQ_HOST_H */
