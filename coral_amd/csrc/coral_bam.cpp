// coral_bam.cpp — host-side BAM (BGZF) codec of libcoral_hip.so: file -> structure-of-arrays records (and back, for tests
// and benchmarks).
//
// Replaces what the reference gets from pysam.AlignmentFile(path, 'rb') + the whole-file fetch()
// (/root/reference/src/infer_breakpoint_graph.py:65, :140-158): every record is decoded ONCE into the SoA layout of
// include/coral_hip.h (CIGAR padded to 16 bytes with op 15), the SA tag is tokenised into numeric rows, NM is extracted,
// and aligned non-ACGT bases are listed (pysam count_coverage counts only A/C/G/T).
//
// Decoder pipeline (one pass, bounded memory — SEQ / QUAL bytes are dropped as soon as their chunk is parsed):
//   file (mmap) -> BGZF block table of the byte range -> chunks of consecutive blocks
//     stage 1 (worker pool)   inflate a chunk (zlib raw inflate, one z_stream per thread, inflateReset per block)
//     stage 2 (caller, cheap) hop along the record lengths: record starts of the chunk, hand-over of the record that
//                             straddles into the next chunk
//     stage 3 (worker pool)   parse the chunk's records into a per-chunk partial (CIGAR copy + padding, SA tokens, NM,
//                             non-ACGT scan; with a window-coverage request the chunk's
//                             partial counts per segment, added up in stage 4; with a reads request the
//                             FASTQ text - or, with want_reads = 2, the own bytes - of the chunk's written records,
//                             concatenated in stage 4)
//     stage 4 (caller)        append the partials in file order; read names -> ids
// A byte range [rank, world) of the file can be decoded on its own (one process per GPU): the range
// starts at the first BGZF block at or after its first byte (blocks are found by their magic + BC subfield and a chained
// check), its first record is the first offset at or after that block's first uncompressed byte from which a chain of
// plausible records starts, and it ends with the record that straddles into the next range — the same rule seen from
// both sides, so consecutive ranges neither drop nor repeat a record.
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
#include <queue>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/coral_hip.h"

#include "coral_bam_common.h"
#include "coral_merge_plan.h"

using namespace coral_bam;

namespace {

// ---------------------------------------------------------------------------------------------
// the decoder
// ---------------------------------------------------------------------------------------------
const size_t CHUNK_BLOCKS = 48;               // ~3 MiB of inflated bytes per chunk
const size_t HEADROOM = 1 << 20;              // room in front of a chunk's bytes for the head of a straddling record
const size_t OVERHANG_BLOCKS = 1024;          // blocks after the byte range that its last record may straddle into (64 MiB)

struct Chunk {
    size_t b0 = 0, b1 = 0;                    // blocks [b0, b1)
    std::vector<uint8_t> buf;                 // [HEADROOM | inflated blocks]
    size_t own = 0;                           // inflated bytes
    size_t begin = HEADROOM;                  // first byte that matters (HEADROOM - carried bytes)
    std::vector<size_t> starts;               // record starts (offsets into buf)
    std::vector<uint64_t> ustarts;            // the same starts as offsets in the range's uncompressed stream (index request only)
    Partial part;
    Flag inflated, parsed;
    std::atomic<int> bad{0};
    bool submitted_parse = false;
};

// With `span` the range is not the rank-th byte range but the records that start inside [span->beg, span->end) (virtual
// offsets, e.g. from a BAI index): the first record is at a known place, nothing is searched, and the decode stops in front of
// the record that starts at or behind span->end.  Spans may be decoded one after the other into the same `D`.
bool decode_file(const char *path, int n_threads, const Request &R, const Span *span, Decoded &D) {
    const int rank = R.rank, world = R.world;
    const CovTable *cov = R.cov_table();
    const bool want_index = R.want_index, want_qc = R.want_qc, filtered = R.keep.active();
    const auto t_start = std::chrono::steady_clock::now();
    MappedFile f;
    if (!f.open(path, D.error)) return false;
    n_threads = n_threads < 1 ? 1 : (n_threads > 256 ? 256 : n_threads);
    // ---- header (every rank): inflate from block 0 until the reference list is complete
    size_t hdr_bytes = 0;                      // header length in the uncompressed stream
    RefIds ref_id;
    {
        Decoded H;
        if (!read_bam_header(f, H, ref_id, &hdr_bytes)) { D.error = H.error; return false; }
        if (D.ref_names.empty()) { D.ref_names = H.ref_names; D.ref_lens = H.ref_lens; }
    }
    const int32_t n_ref = (int32_t)D.ref_names.size();
    if (want_index) D.idx.init(D.ref_lens);
    if (want_qc) D.qc.init();
    if (R.depth_bin > 0) {                     // (never on a span decode: this is the decode's one call)
        if (!D.depth.init(R.depth_bin, R.depth_min_mapq, R.depth_exclude_flags, R.depth_count_deletions, D.ref_lens, D.error)) { D.bad_request = true; return false; }
        D.depth.zero_tables();
    }
    DepthPartial *depth = D.depth.on ? &D.depth : nullptr;
    const ReadsRule *reads = R.reads.on ? &R.reads : nullptr;
    if (reads) D.has_reads = true;
    // ---- block table: the blocks that START inside this rank's byte range, plus an overhang for the last record
    const uint64_t byte_lo = rank == 0 ? 0 : f.size / (uint64_t)world * (uint64_t)rank;
    const uint64_t byte_hi = rank == world - 1 ? f.size : f.size / (uint64_t)world * (uint64_t)(rank + 1);
    uint64_t first = 0;
    if (rank > 0 && !find_block(f, byte_lo, &first)) first = f.size;
    const uint64_t span_end_block = span ? span->end >> 16 : 0;
    const uint32_t span_end_off = span ? (uint32_t)(span->end & 0xffff) : 0;
    if (span) first = span->beg >> 16;
    std::vector<Block> blocks;
    std::vector<uint64_t> ublk;                // offset of every block's first byte in the range's uncompressed stream
    size_t n_own = 0;
    uint64_t own_bytes = 0;                    // uncompressed offset (from this rank's first block) of the next rank's first block
    uint64_t limit = ~0ull, total_bytes = 0;   // a record that starts at or behind `limit` (uncompressed offset) is not this range's
    uint64_t table_end = first;                // file offset behind the last block of the table
    for (uint64_t at = first; at < f.size && blocks.size() < n_own + OVERHANG_BLOCKS;) {
        Block b;
        if (!bgzf_header(f.data + at, f.size - at, b)) { D.error = "not a BGZF block"; return false; }
        b.off = at;
        if (span) {
            if (at == span_end_block) limit = total_bytes + span_end_off;
            if (at < span_end_block || (at == span_end_block && span_end_off > 0)) { ++n_own; own_bytes += b.isize; }
        } else if (at < byte_hi) { ++n_own; own_bytes += b.isize; }
        ublk.push_back(total_bytes);
        total_bytes += b.isize;
        blocks.push_back(b);
        at += b.csize;
        table_end = at;
    }
    if (span && limit == ~0ull && span_end_block < f.size) { D.error = "the end of a span is not the start of a BGZF block"; return false; }
    // virtual offset of the record that starts at uncompressed offset u; behind the last byte: the block that follows (bgzf_tell)
    auto voffset = [&](uint64_t u) -> uint64_t {
        if (u < total_bytes) {
            const size_t b = (size_t)(std::upper_bound(ublk.begin(), ublk.end(), u) - ublk.begin()) - 1;
            return (blocks[b].off << 16) | (u - ublk[b]);
        }
        const size_t b = (size_t)(std::lower_bound(ublk.begin(), ublk.end(), u) - ublk.begin());
        return (b < blocks.size() ? blocks[b].off : table_end) << 16;
    };
    std::vector<std::unique_ptr<Chunk>> chunks;
    for (size_t b = 0; b < blocks.size();) {     // (a span's own blocks end with a chunk: what lies behind is inflated only if needed)
        size_t e = std::min(blocks.size(), b + CHUNK_BLOCKS);
        if (span && b < n_own && e > n_own) e = n_own;
        chunks.emplace_back(new Chunk());
        chunks.back()->b0 = b;
        chunks.back()->b1 = e;
        b = e;
    }
    const size_t n_chunks = chunks.size();
    const size_t own_chunks = (n_own + CHUNK_BLOCKS - 1) / CHUNK_BLOCKS;      // chunks holding at least one owned block
    const bool last_rank = rank == world - 1 && !span;
    if (!span && !last_rank) limit = own_bytes;

    Pool pool(n_threads);
    const size_t window = (size_t)std::max(4, 3 * n_threads);
    auto submit_inflate = [&](size_t k) {
        Chunk *c = chunks[k].get();
        pool.submit([&, c]() {
            thread_local ZStream z;
            size_t total = 0;
            for (size_t b = c->b0; b < c->b1; ++b) total += blocks[b].isize;
            c->buf.resize(HEADROOM + total);
            c->own = total;
            size_t o = HEADROOM;
            for (size_t b = c->b0; b < c->b1; ++b) {
                if (!z.ok || !inflate_block(z.zs, f, blocks[b], c->buf.data() + o)) { c->bad = 1; break; }
                o += blocks[b].isize;
            }
            c->inflated.set();
        });
    };
    auto submit_parse = [&](size_t k) {
        Chunk *c = chunks[k].get();
        c->submitted_parse = true;
        pool.submit([&, c]() {
            Partial &pt = c->part;
            pt.cigar.reserve(c->own / 6 + 64);
            if (cov && !cov->per_base) pt.cov.assign(cov->size(), 0);    // the chunk's partial counts, added up in merge()
            if (want_qc) pt.qc_hist.assign(256, 0);              // the chunk's partial histogram, likewise
            for (size_t s : c->starts) {
                const uint8_t *q = c->buf.data() + s;
                if (filtered && !keep_record_at(q, R.keep)) continue;      // dropped: no field, no tag, no counter sees it
                if (!decode_record(q + 4, rd32(q), ref_id, pt, pt.error, cov, want_qc, D.pileup.data(), depth)) break;
                if (reads && reads->written(q, pt.end.back())) {      // the reads request: the chunk's text, concatenated in merge()
                    const size_t at = pt.reads_text.size();
                    if (reads->mode == READS_AS_RECORDS) reads_append_record(q, pt.reads_text);
                    else reads_append_text(q, pt.reads_text);
                    pt.reads_len.push_back((int64_t)(pt.reads_text.size() - at));
                }
            }
            std::vector<uint8_t>().swap(c->buf);            // SEQ / QUAL bytes are gone from here on
            c->parsed.set();
        });
    };
    auto wait = [&](Flag &fl) { while (!fl.get()) if (!pool.help_one()) std::this_thread::yield(); };

    if (D.tid.empty()) D.names.grow(1 << 21);
    if (cov && D.cov.size() != cov->size()) D.cov.assign(cov->size(), 0);
    if (cov && cov->per_base && !D.has_pileup) {                 // one table for the decode (a span decode comes here once per span)
        D.pileup.assign((size_t)(4 * cov->n_pos()), 0);
        D.has_pileup = true;
    }
    auto merge = [&](Chunk &c) -> bool {
        Partial &pt = c.part;
        if (!pt.error.empty()) { D.error = pt.error; return false; }
        const int64_t base = (int64_t)D.tid.size();
        if (D.idx.on)                          // the index request: records in file order, each with its virtual offset
            for (size_t j = 0; j < pt.tid.size(); ++j) D.idx.add(pt.tid[j], pt.pos[j], pt.end[j], pt.flag[j], voffset(c.ustarts[j]));
        auto app = [](std::vector<int32_t> &d, const std::vector<int32_t> &s) { d.insert(d.end(), s.begin(), s.end()); };
        app(D.tid, pt.tid); app(D.pos, pt.pos); app(D.end, pt.end); app(D.flag, pt.flag); app(D.mapq, pt.mapq);
        app(D.qlen, pt.qlen); app(D.has_seq, pt.has_seq); app(D.nm, pt.nm); app(D.n_cigar, pt.n_cigar);
        D.cigar.insert(D.cigar.end(), pt.cigar.begin(), pt.cigar.end());
        for (int64_t l : pt.cigar_len) D.cigar_off.push_back(D.cigar_off.back() + l);
        app(D.sa, pt.sa); app(D.sa_nm, pt.sa_nm);
        for (int32_t cnt : pt.sa_cnt) D.sa_off.push_back(D.sa_off.back() + cnt);
        for (int64_t l : pt.na_rec_local) D.na_rec.push_back(base + l);
        app(D.na_pos, pt.na_pos);
        for (size_t t = 0; t < pt.cov.size(); ++t) D.cov[t] += pt.cov[t];
        D.qc.qual_sum.insert(D.qc.qual_sum.end(), pt.qc_sum.begin(), pt.qc_sum.end());
        for (size_t t = 0; t < pt.qc_hist.size(); ++t) D.qc.hist[t] += pt.qc_hist[t];
        D.reads_text.insert(D.reads_text.end(), pt.reads_text.begin(), pt.reads_text.end());
        for (int64_t l : pt.reads_len) D.reads_off.push_back(D.reads_off.back() + l);
        for (const char *s = pt.names.data(), *e = s + pt.names.size(); s < e;) {
            const size_t len = strlen(s);
            D.name_id.push_back(D.names.intern(s, len));
            s += len + 1;
        }
        c.part = Partial();
        return true;
    };

    // ---- the ordered walk: stage 2 for chunk k, stage 4 for the chunks whose parse is done (in order)
    size_t next_inflate = 0, merged = 0;
    auto top_up = [&](size_t k) {               // beyond the owned chunks only one chunk ahead (the overhang is rarely needed)
        const size_t upto = std::min(n_chunks, std::max(k + 1, std::min(k + window, own_chunks + (span ? 0 : 1))));
        while (next_inflate < upto) submit_inflate(next_inflate++);
    };
    bool searching = rank > 0 && !span;        // still looking for the first record of the range
    uint64_t pos = span ? (span->beg & 0xffff) : rank == 0 ? hdr_bytes : 0;  // offset (in this rank's uncompressed stream) of the next record start
    std::vector<uint8_t> carry;                // bytes [pos, end of the previous chunk): head of a straddling record
    uint64_t ubase = 0;                        // stream offset of the current chunk's first inflated byte
    bool done = false;
    for (size_t k = 0; k < n_chunks && !done; ++k) {
        top_up(k);
        Chunk &c = *chunks[k];
        wait(c.inflated);
        if (c.bad) { D.error = "zlib inflate failed or CRC32 mismatch (corrupt BGZF block)"; return false; }
        if (carry.size() > HEADROOM) {         // (a record of more than 1 MiB straddles) make room
            c.buf.insert(c.buf.begin(), carry.size() - HEADROOM, 0);
            c.begin = 0;
            memcpy(c.buf.data(), carry.data(), carry.size());
        } else {
            c.begin = HEADROOM - carry.size();
            if (!carry.empty()) memcpy(c.buf.data() + c.begin, carry.data(), carry.size());
        }
        const size_t carried = carry.size();
        carry.clear();
        const uint8_t *base = c.buf.data() + c.begin;
        const size_t nbytes = c.buf.size() - c.begin;
        const uint64_t u0 = ubase - carried;     // stream offset of base[0]
        size_t p;
        if (searching) {
            p = nbytes;
            for (size_t cand = 0; cand + 36 <= nbytes; ++cand) {
                size_t q = cand;
                int chain = 0;
                bool ok = true;
                while (chain < 8 && q + 36 <= nbytes) {
                    uint64_t len;
                    if (!plausible_record(base + q, nbytes - q, n_ref, &len)) { ok = false; break; }
                    q += len;
                    ++chain;
                }
                if (ok && chain >= 3) { p = cand; break; }
            }
            if (p == nbytes) {                   // nothing yet (e.g. inside one enormous record): search on with these bytes kept
                if (k + 1 == n_chunks) break;    // no record starts in this range at all
                carry.assign(base, base + nbytes);
                ubase += c.own;
                continue;
            }
            searching = false;
        } else {
            if (pos - u0 >= nbytes) {            // the BAM header is longer than this chunk (rank 0 only)
                ubase += c.own;
                continue;
            }
            p = (size_t)(pos - u0);
        }
        while (p < nbytes) {
            if (u0 + p >= limit) { done = true; break; }                       // starts in the next rank's range (behind the span): not ours
            if (nbytes - p < 4) break;
            const uint64_t len = 4ull + rd32(base + p);
            if (len < 36) { D.error = "record shorter than its fixed fields"; return false; }
            if (p + len > nbytes) break;                                       // straddles into the next chunk
            c.starts.push_back(c.begin + p);
            if (want_index) c.ustarts.push_back(u0 + p);
            p += (size_t)len;
        }
        if (!done) {
            if (u0 + p >= limit) done = true;
            else if (p < nbytes) carry.assign(base + p, base + nbytes);
        }
        pos = u0 + p;
        ubase += c.own;
        submit_parse(k);
        while (merged <= k && (chunks[merged]->parsed.get() || !chunks[merged]->submitted_parse || k + 1 - merged > window)) {
            Chunk &m = *chunks[merged];
            if (m.submitted_parse) {
                wait(m.parsed);
                if (!merge(m)) return false;
            }
            ++merged;
        }
    }
    if (searching && rank > 0 && n_own > 0) { /* the whole range lies inside one record of the previous range */ }
    if (!carry.empty() && !done && !searching) { D.error = last_rank ? "truncated record at the end of the file" : "a record straddles further than the supported overhang"; return false; }
    for (; merged < n_chunks; ++merged) {
        Chunk &m = *chunks[merged];
        if (!m.submitted_parse) continue;
        wait(m.parsed);
        if (!merge(m)) return false;
    }
    // inflate tasks that were submitted ahead but never used must finish before the pool (and the chunks) go away
    for (size_t k = 0; k < next_inflate; ++k) wait(chunks[k]->inflated);
    // statistics: the range's own blocks; of a span every block that was inflated (its overhang included)
    const size_t n_read = span ? (next_inflate ? chunks[next_inflate - 1]->b1 : 0) : n_own;
    for (size_t b = 0; b < n_read; ++b) { D.compressed_bytes += blocks[b].csize; D.uncompressed_bytes += blocks[b].isize; }
    D.n_blocks += (int64_t)n_read;
    if (D.idx.on) {
        if (D.idx.unsorted) { D.error = "the records are not in coordinate order: no index can be built"; return false; }
        D.idx.end_voff = voffset(pos);
    }
    D.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return true;
}

// ---------------------------------------------------------------------------------------------
// writer (tests, benchmarks): SoA records -> coordinate-sorted BAM with deterministic SEQ
// ---------------------------------------------------------------------------------------------
inline void put32(std::vector<uint8_t> &o, uint32_t v) { const size_t n = o.size(); o.resize(n + 4); memcpy(o.data() + n, &v, 4); }
inline void put16(std::vector<uint8_t> &o, uint16_t v) { const size_t n = o.size(); o.resize(n + 2); memcpy(o.data() + n, &v, 2); }

inline uint32_t mix32(uint32_t x) {            // the finaliser of MurmurHash3
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

struct WriteJob {
    int64_t n_rec;
    const int32_t *tid, *pos, *flag, *mapq, *qlen, *has_seq, *nm, *name_id, *n_cigar;
    const int64_t *cigar_off;
    const uint32_t *cigar;
    const int64_t *sa_off;
    const int32_t *sa, *sa_nm;
    int64_t n_na;
    const int64_t *na_rec;
    const int32_t *na_pos;
    const char *const *names;
    int32_t n_ref;
    const char *const *ref_names;
    uint32_t seed;
};

void sa_text(const WriteJob &J, int64_t row, std::string &out) {
    const int32_t *r = J.sa + 8 * row;
    char buf[160];
    std::string cg;
    if (r[3] > 0) { snprintf(buf, sizeof(buf), "%dS", r[3]); cg += buf; }
    snprintf(buf, sizeof(buf), "%dM", r[4]); cg += buf;
    if (r[5] > 0) { snprintf(buf, sizeof(buf), "%dI", r[5]); cg += buf; }
    if (r[5] < 0) { snprintf(buf, sizeof(buf), "%dD", -r[5]); cg += buf; }
    if (r[6] > 0) { snprintf(buf, sizeof(buf), "%dS", r[6]); cg += buf; }
    snprintf(buf, sizeof(buf), "%s,%d,%c,%s,%d,%d;", (r[0] >= 0 && r[0] < J.n_ref) ? J.ref_names[r[0]] : "*", r[1], r[2] ? '-' : '+',
             cg.c_str(), r[7], J.sa_nm[row]);
    out += buf;
}

void write_record(const WriteJob &J, int64_t i, std::vector<uint8_t> &o, std::vector<uint8_t> &seq) {
    const uint32_t *ops = J.cigar + J.cigar_off[i];
    const uint32_t n_ops = (uint32_t)J.n_cigar[i];
    const uint32_t l_seq = J.has_seq[i] ? (uint32_t)J.qlen[i] : 0;
    int64_t rlen = 0;
    for (uint32_t k = 0; k < n_ops; ++k) rlen += REF_ADV[ops[k] & 15] ? (ops[k] >> 4) : 0;
    if (J.flag[i] & 4) rlen = 0;
    // SEQ: hash-made ACGT, N at the listed aligned positions of this record
    seq.assign(((size_t)l_seq + 1) / 2, 0);
    if (l_seq) {
        static const uint8_t CODE[4] = {1, 2, 4, 8};
        uint32_t state = mix32(J.seed ^ (uint32_t)(i * 2654435761u));
        for (uint32_t q = 0; q < l_seq; q += 16) {
            state = mix32(state + 0x9e3779b9u);
            uint32_t bits = state;
            for (uint32_t j = q; j < q + 16 && j < l_seq; ++j, bits >>= 2)
                seq[j >> 1] |= (uint8_t)(CODE[bits & 3] << ((j & 1) ? 0 : 4));
        }
        const int64_t *lo = std::lower_bound(J.na_rec, J.na_rec + J.n_na, i), *hi = std::upper_bound(J.na_rec, J.na_rec + J.n_na, i);
        for (const int64_t *it = lo; it < hi; ++it) {
            const int64_t want = J.na_pos[it - J.na_rec];
            int64_t q = 0, r = J.pos[i];
            for (uint32_t k = 0; k < n_ops; ++k) {
                const uint32_t op = ops[k] & 15, len = ops[k] >> 4;
                if (IS_ALN[op] && want >= r && want < r + (int64_t)len) {
                    const uint64_t qi = (uint64_t)(q + (want - r));
                    if (qi < l_seq) {
                        seq[qi >> 1] &= (uint8_t)((qi & 1) ? 0xf0 : 0x0f);
                        seq[qi >> 1] |= (uint8_t)(15 << ((qi & 1) ? 0 : 4));
                    }
                    break;
                }
                if (QRY_ADV[op]) q += len;
                if (REF_ADV[op]) r += len;
            }
        }
    }
    // tags
    std::vector<uint8_t> tags;
    tags.push_back('N'); tags.push_back('M'); tags.push_back('i'); put32(tags, (uint32_t)J.nm[i]);
    if (J.sa_off[i + 1] > J.sa_off[i]) {
        std::string s;
        for (int64_t r = J.sa_off[i]; r < J.sa_off[i + 1]; ++r) sa_text(J, r, s);
        tags.push_back('S'); tags.push_back('A'); tags.push_back('Z');
        tags.insert(tags.end(), s.begin(), s.end());
        tags.push_back(0);
    }
    uint32_t cig_field_n = n_ops;
    uint32_t placeholder[2];
    const uint32_t *cig_field = ops;
    if (n_ops > 65535) {                       // long CIGAR -> CG:B,I tag + the <l_seq>S<rlen>N placeholder (SAM spec §4.2.2)
        tags.push_back('C'); tags.push_back('G'); tags.push_back('B'); tags.push_back('I'); put32(tags, n_ops);
        const size_t n = tags.size();
        tags.resize(n + 4ull * n_ops);
        memcpy(tags.data() + n, ops, 4ull * n_ops);
        placeholder[0] = (l_seq << 4) | 4;
        placeholder[1] = ((uint32_t)rlen << 4) | 3;
        cig_field = placeholder;
        cig_field_n = 2;
    }
    const char *name = J.names[J.name_id[i]];
    const uint32_t l_name = (uint32_t)strlen(name) + 1;
    const uint32_t block_size = 32 + l_name + 4 * cig_field_n + (uint32_t)seq.size() + l_seq + (uint32_t)tags.size();
    put32(o, block_size);
    put32(o, (uint32_t)J.tid[i]);
    put32(o, (uint32_t)J.pos[i]);
    o.push_back((uint8_t)l_name);
    o.push_back((uint8_t)J.mapq[i]);
    put16(o, (uint16_t)reg2bin(J.pos[i], J.pos[i] + (rlen > 0 ? rlen : 1)));
    put16(o, (uint16_t)cig_field_n);
    put16(o, (uint16_t)J.flag[i]);
    put32(o, l_seq);
    put32(o, (uint32_t)-1);
    put32(o, (uint32_t)-1);
    put32(o, 0);
    o.insert(o.end(), (const uint8_t *)name, (const uint8_t *)name + l_name);
    { const size_t n = o.size(); o.resize(n + 4ull * cig_field_n); if (cig_field_n) memcpy(o.data() + n, cig_field, 4ull * cig_field_n); }
    o.insert(o.end(), seq.begin(), seq.end());
    o.insert(o.end(), (size_t)l_seq, (uint8_t)0xff);
    o.insert(o.end(), tags.begin(), tags.end());
}

// deflate `n` bytes into BGZF blocks of at most 0xff00 input bytes, appended to `out`
bool bgzf_compress(const uint8_t *in, size_t n, int level, std::vector<uint8_t> &out) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    std::vector<uint8_t> comp(70000);
    for (size_t at = 0; at < n; at += 0xff00) {
        const size_t len = std::min<size_t>(0xff00, n - at);
        deflateReset(&zs);
        zs.next_in = (Bytef *)(in + at);
        zs.avail_in = (uInt)len;
        zs.next_out = comp.data();
        zs.avail_out = (uInt)comp.size();
        if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { deflateEnd(&zs); return false; }
        const size_t clen = comp.size() - zs.avail_out;
        static const uint8_t HDR[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
        out.insert(out.end(), HDR, HDR + 16);
        put16(out, (uint16_t)(clen + 25));
        out.insert(out.end(), comp.begin(), comp.begin() + (long)clen);
        put32(out, (uint32_t)crc32(crc32(0L, Z_NULL, 0), in + at, (uInt)len));
        put32(out, (uint32_t)len);
    }
    deflateEnd(&zs);
    return true;
}

thread_local std::string g_bam_err;

}  // namespace

void coral_bam::set_error(const std::string &msg) { g_bam_err = msg; }

extern "C" const char *coral_bam_last_error(void) { return g_bam_err.c_str(); }

// The written records of a records request in coordinate order (host pipeline: the parity partner of the GPU path, not a fast
// path): a stable sort of the records by reads_sort_key, then the bytes gathered in that order.
static void sort_written_records(Decoded &D) {
    const size_t n = D.reads_off.size() - 1;
    std::vector<unsigned long long> key(n);
    std::vector<size_t> order(n);
    for (size_t k = 0; k < n; ++k) { key[k] = reads_sort_key_at(D.reads_text.data() + D.reads_off[k]); order[k] = k; }
    if (std::is_sorted(key.begin(), key.end())) return;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key[a] < key[b]; });
    std::vector<uint8_t> text(D.reads_text.size());
    std::vector<int64_t> off(1, 0);
    off.reserve(n + 1);
    for (size_t k = 0; k < n; ++k) {
        const int64_t a = D.reads_off[order[k]], len = D.reads_off[order[k] + 1] - a;
        memcpy(text.data() + off.back(), D.reads_text.data() + a, (size_t)len);
        off.push_back(off.back() + len);
    }
    D.reads_text.swap(text);
    D.reads_off.swap(off);
}

extern "C" int coral_bam_decode_request(const char *path, int32_t n_threads, const coral_bam_request_t *req, void **handle) {
    if (!path || !handle) return CORAL_ERR_ARG;
    Request R;
    if (!parse_request(req, R, g_bam_err)) return CORAL_ERR_ARG;
    std::unique_ptr<Decoded> D(new Decoded());
    bool ok = false;
    try {
        if (!R.span_mode) {
            ok = decode_file(path, n_threads, R, nullptr, *D);
        } else {                                 // spans in the given order, into one result (no span: the header only)
            MappedFile f;
            RefIds ids;
            size_t hdr = 0;
            ok = f.open(path, D->error) && read_bam_header(f, *D, ids, &hdr);
            if (ok && !spans_inside_file(R, f.size, g_bam_err)) return CORAL_ERR_ARG;
            if (ok && R.has_cov) D->cov.assign(R.cov.size(), 0);
            if (ok && R.cov.per_base) { D->pileup.assign((size_t)(4 * R.cov.n_pos()), 0); D->has_pileup = true; }
            if (ok && R.reads.on) D->has_reads = true;
            for (size_t k = 0; k < R.spans.size() && ok; ++k) ok = decode_file(path, n_threads, R, &R.spans[k], *D);
        }
    } catch (const std::exception &e) {          // e.g. bad_alloc on a corrupt size field: never across the C boundary
        D->error = std::string("decoder failed: ") + e.what();
    }
    if (!ok) {
        g_bam_err = D->error;
        return D->bad_request ? CORAL_ERR_ARG : CORAL_ERR_FORMAT;
    }
    if (D->has_pileup) pileup_segment_sums(R.cov, D->pileup.data(), D->cov);
    if (R.reads.order == READS_ORDER_COORDINATE) sort_written_records(*D);
    *handle = D.release();
    return CORAL_OK;
}

extern "C" int coral_bam_decode_range(const char *path, int32_t n_threads, int32_t rank, int32_t world, void **handle) {
    const coral_bam_request_t q = range_request(rank, world);
    return coral_bam_decode_request(path, n_threads, &q, handle);
}

extern "C" int coral_bam_index_sizes(void *handle, int64_t sizes[4]) {
    if (!handle || !sizes) return CORAL_ERR_ARG;
    const IndexPartial &X = ((Decoded *)handle)->idx;
    if (!X.on) { g_bam_err = "coral_bam_index_sizes: the handle holds no index request"; return CORAL_ERR_ARG; }
    sizes[0] = (int64_t)X.head_key.size();
    sizes[1] = (int64_t)X.lin.size();
    sizes[2] = (int64_t)X.n_mapped.size();
    sizes[3] = X.n_rec;
    return CORAL_OK;
}

extern "C" int coral_bam_index_fill(void *handle, int64_t *head_key, uint64_t *head_voff, uint64_t *lin, int64_t *n_mapped,
                                    int64_t *n_unmapped, uint64_t scalars[4]) {
    if (!handle || !scalars) return CORAL_ERR_ARG;
    const IndexPartial &X = ((Decoded *)handle)->idx;
    if (!X.on) { g_bam_err = "coral_bam_index_fill: the handle holds no index request"; return CORAL_ERR_ARG; }
    auto cp = [](auto *dst, const auto &v) { if (!v.empty() && dst) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    cp(head_key, X.head_key); cp(head_voff, X.head_voff); cp(lin, X.lin); cp(n_mapped, X.n_mapped); cp(n_unmapped, X.n_unmapped);
    scalars[0] = (uint64_t)X.n_no_coor; scalars[1] = X.end_voff; scalars[2] = X.first_sort; scalars[3] = X.last_sort;
    return CORAL_OK;
}

// The read-QC request of a handle (either pipeline): sizes = records, reads; fill = the reads' rows in file order (length,
// qual_sum with -1 for no quality, mapq, flag), the 256-bin histogram and the counters (QC_N_RECORDS ...).
extern "C" int coral_bam_qc_sizes(void *handle, int64_t sizes[2]) {
    if (!handle || !sizes) return CORAL_ERR_ARG;
    const Decoded *D = (const Decoded *)handle;
    if (!D->qc.on || D->qc.qual_sum.size() != D->flag.size()) { g_bam_err = "coral_bam_qc_sizes: the handle holds no read-QC request"; return CORAL_ERR_ARG; }
    int64_t c[QC_N_COUNTERS];
    QcPartial::counters(D->flag, D->has_seq, D->qlen, D->qc.qual_sum, c);
    sizes[0] = c[QC_N_RECORDS];
    sizes[1] = c[QC_N_READS];
    return CORAL_OK;
}

extern "C" int coral_bam_qc_fill(void *handle, int32_t *length, int64_t *qual_sum, int32_t *mapq, int32_t *flag, int64_t hist[256],
                                 int64_t counters[8]) {
    if (!handle || !hist || !counters) return CORAL_ERR_ARG;
    const Decoded *D = (const Decoded *)handle;
    if (!D->qc.on || D->qc.qual_sum.size() != D->flag.size()) { g_bam_err = "coral_bam_qc_fill: the handle holds no read-QC request"; return CORAL_ERR_ARG; }
    static_assert(QC_N_COUNTERS == 8, "the counters of the C ABI");
    QcPartial::counters(D->flag, D->has_seq, D->qlen, D->qc.qual_sum, counters);
    if (counters[QC_N_READS] > 0 && (!length || !qual_sum || !mapq || !flag)) return CORAL_ERR_ARG;
    size_t r = 0;
    for (size_t i = 0; i < D->flag.size(); ++i) {
        const uint32_t l_seq = D->has_seq[i] ? (uint32_t)D->qlen[i] : 0u;
        if (!qc_is_read((uint32_t)D->flag[i], l_seq)) continue;
        length[r] = (int32_t)l_seq; qual_sum[r] = D->qc.qual_sum[i]; mapq[r] = D->mapq[i]; flag[r] = D->flag[i];
        ++r;
    }
    memcpy(hist, D->qc.hist, sizeof(D->qc.hist));
    return CORAL_OK;
}

// The binned-depth request of a handle (either pipeline): sizes = contigs, bins; fill = bin_off (n_ref + 1) and the two tables.
extern "C" int coral_bam_depth_sizes(void *handle, int64_t sizes[2]) {
    if (!handle || !sizes) return CORAL_ERR_ARG;
    const DepthPartial &P = ((Decoded *)handle)->depth;
    if (!P.on) { g_bam_err = "coral_bam_depth_sizes: the handle holds no binned-depth request"; return CORAL_ERR_ARG; }
    sizes[0] = (int64_t)P.len.size();
    sizes[1] = P.n_bins();
    return CORAL_OK;
}

extern "C" int coral_bam_depth_fill(void *handle, int64_t *bin_off, int64_t *bases, int64_t *reads) {
    if (!handle || !bin_off) return CORAL_ERR_ARG;
    const DepthPartial &P = ((Decoded *)handle)->depth;
    if (!P.on || (int64_t)P.bases.size() != P.n_bins()) { g_bam_err = "coral_bam_depth_fill: the handle holds no binned-depth request"; return CORAL_ERR_ARG; }
    if (P.n_bins() > 0 && (!bases || !reads)) return CORAL_ERR_ARG;
    memcpy(bin_off, P.bin_off.data(), P.bin_off.size() * 8);
    if (P.n_bins() > 0) {
        memcpy(bases, P.bases.data(), P.bases.size() * 8);
        memcpy(reads, P.reads.data(), P.reads.size() * 8);
    }
    return CORAL_OK;
}

// The reads request of a handle (either pipeline): sizes = records written, text bytes; fill = the text and the n + 1 offsets
// (want_reads = 2: the records' own bytes in place of the text).
// Stable k-way merge of sorted runs of raw records (include/coral_hip.h): first the order - a heap of the runs' heads by (key,
// run), so a tie goes to the earlier run - and the output offsets, then the bytes, copied by n_threads workers that each take a
// stretch of consecutive output records.
extern "C" int coral_bam_records_merge(int32_t n_runs, const uint8_t *const *data, const int64_t *const *off, const int64_t *n,
                                       uint8_t *out_data, int64_t *out_off, int32_t n_threads) {
    if (n_runs < 0 || !out_off || (n_runs > 0 && (!data || !off || !n))) { g_bam_err = "coral_bam_records_merge: bad arguments"; return CORAL_ERR_ARG; }
    int64_t total = 0;
    for (int32_t r = 0; r < n_runs; ++r) {
        if (n[r] < 0 || !off[r] || (n[r] > 0 && !data[r])) { g_bam_err = "coral_bam_records_merge: bad run"; return CORAL_ERR_ARG; }
        for (int64_t k = 0; k < n[r]; ++k)
            if (off[r][k] < 0 || off[r][k + 1] - off[r][k] < 20) { g_bam_err = "coral_bam_records_merge: a record is shorter than its key fields (bad offsets)"; return CORAL_ERR_ARG; }
        total += n[r];
    }
    struct Head { unsigned long long key; int32_t run; };
    auto later = [](const Head &a, const Head &b) { return a.key != b.key ? a.key > b.key : a.run > b.run; };
    std::priority_queue<Head, std::vector<Head>, decltype(later)> heads(later);
    std::vector<int64_t> at((size_t)n_runs, 0);
    for (int32_t r = 0; r < n_runs; ++r)
        if (n[r] > 0) heads.push(Head{reads_sort_key_at(data[r] + off[r][0]), r});
    std::vector<const uint8_t *> src((size_t)total);
    out_off[0] = 0;
    for (int64_t j = 0; j < total; ++j) {
        const int32_t r = heads.top().run;
        heads.pop();
        const int64_t k = at[(size_t)r]++;
        src[(size_t)j] = data[r] + off[r][k];
        out_off[j + 1] = out_off[j] + (off[r][k + 1] - off[r][k]);
        if (k + 1 < n[r]) heads.push(Head{reads_sort_key_at(data[r] + off[r][k + 1]), r});
    }
    if (total > 0 && !out_data) { g_bam_err = "coral_bam_records_merge: no output buffer"; return CORAL_ERR_ARG; }
    const int64_t nt = std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_threads, (int64_t)64, total}));
    auto copy = [&](int64_t t) {
        for (int64_t j = total * t / nt, e = total * (t + 1) / nt; j < e; ++j)
            memcpy(out_data + out_off[j], src[(size_t)j], (size_t)(out_off[j + 1] - out_off[j]));
    };
    std::vector<std::thread> workers;
    for (int64_t t = 1; t < nt; ++t) workers.emplace_back(copy, t);
    copy(0);
    for (auto &w : workers) w.join();
    return CORAL_OK;
}

// The step plan of the streamed sort's merge (coral_merge_plan.h) on its own: counts = {steps, parts}; with step_j (steps + 1),
// step_part (steps + 1) and parts (rows of run, first block, block count, staging base) given, of the capacities max_steps /
// max_parts, the plan itself.
extern "C" int coral_merge_plan(int32_t n_runs, const int64_t *run_records, const uint32_t *len, const uint32_t *perm, int64_t stage_bytes,
                                int64_t max_steps, int64_t max_parts, int64_t *step_j, int64_t *step_part, int64_t *parts, int64_t counts[2]) {
    if (!counts) { g_bam_err = "coral_merge_plan: no counts"; return CORAL_ERR_ARG; }
    counts[0] = counts[1] = 0;
    coral_merge::Plan plan;
    if (const int rc = coral_merge::plan_steps(n_runs, run_records, len, perm, stage_bytes, plan, g_bam_err)) return rc;
    counts[0] = plan.n_steps();
    counts[1] = (int64_t)plan.parts.size();
    if (!step_j && !step_part && !parts) return CORAL_OK;
    if (!step_j || !step_part || (counts[1] > 0 && !parts)) { g_bam_err = "coral_merge_plan: a missing output array"; return CORAL_ERR_ARG; }
    if (max_steps < counts[0] || max_parts < counts[1]) { g_bam_err = "coral_merge_plan: the output arrays are too short (counts holds the sizes)"; return CORAL_ERR_CAPACITY; }
    memcpy(step_j, plan.step_j.data(), plan.step_j.size() * 8);
    memcpy(step_part, plan.step_part.data(), plan.step_part.size() * 8);
    static_assert(sizeof(coral_merge::Part) == 32, "a part is four int64");
    if (counts[1] > 0) memcpy(parts, plan.parts.data(), plan.parts.size() * sizeof(coral_merge::Part));
    return CORAL_OK;
}

extern "C" int coral_bam_reads_sizes(void *handle, int64_t sizes[2]) {
    if (!handle || !sizes) return CORAL_ERR_ARG;
    const Decoded *D = (const Decoded *)handle;
    if (!D->has_reads) { g_bam_err = "coral_bam_reads_sizes: the handle holds no reads request"; return CORAL_ERR_ARG; }
    sizes[0] = D->reads_in_file ? D->reads_file_records : (int64_t)D->reads_off.size() - 1;
    sizes[1] = D->reads_in_file ? D->reads_file_bytes : (int64_t)D->reads_text.size();
    return CORAL_OK;
}

extern "C" int coral_bam_reads_fill(void *handle, uint8_t *text, int64_t *rec_off) {
    if (!handle || !rec_off) return CORAL_ERR_ARG;
    const Decoded *D = (const Decoded *)handle;
    if (D->reads_in_file) { g_bam_err = "coral_bam_reads_fill: the records were written to a file, none is kept (a file sink of coral_bamgpu_open_request)"; return CORAL_ERR_ARG; }
    if (!D->has_reads || D->reads_off.back() != (int64_t)D->reads_text.size()) { g_bam_err = "coral_bam_reads_fill: the handle holds no reads request"; return CORAL_ERR_ARG; }
    if (!D->reads_text.empty() && !text) return CORAL_ERR_ARG;
    if (!D->reads_text.empty()) memcpy(text, D->reads_text.data(), D->reads_text.size());
    memcpy(rec_off, D->reads_off.data(), D->reads_off.size() * 8);
    return CORAL_OK;
}

extern "C" int coral_bam_coverage_result(void *handle, int32_t n_seg, int64_t *counts) {
    if (!handle || n_seg < 0 || (n_seg > 0 && !counts)) return CORAL_ERR_ARG;
    Decoded *D = (Decoded *)handle;
    if ((size_t)n_seg != D->cov.size()) { g_bam_err = "coral_bam_coverage_result: the handle holds no request of this size"; return CORAL_ERR_ARG; }
    if (n_seg) memcpy(counts, D->cov.data(), (size_t)n_seg * 8);
    return CORAL_OK;
}

extern "C" int coral_bam_pileup_result(void *handle, int64_t n_pos, uint32_t *counts) {
    if (!handle || n_pos < 0 || (n_pos > 0 && !counts)) return CORAL_ERR_ARG;
    Decoded *D = (Decoded *)handle;
    if (!D->has_pileup || (uint64_t)n_pos * 4 != D->pileup.size()) { g_bam_err = "coral_bam_pileup_result: the handle holds no pileup request of this size"; return CORAL_ERR_ARG; }
    if (n_pos) memcpy(counts, D->pileup.data(), (size_t)n_pos * 16);
    return CORAL_OK;
}

extern "C" int coral_bam_decode_open(const char *path, int32_t n_threads, void **handle) {
    return coral_bam_decode_range(path, n_threads, 0, 1, handle);
}

extern "C" int coral_bam_decode_sizes(void *handle, int64_t sizes[8]) {
    if (!handle || !sizes) return CORAL_ERR_ARG;
    Decoded *D = (Decoded *)handle;
    int64_t nb = (int64_t)D->names.blob.size(), rb = 0;
    for (auto &s : D->ref_names) rb += (int64_t)s.size() + 1;
    sizes[0] = (int64_t)D->tid.size();
    sizes[1] = (int64_t)D->cigar.size();
    sizes[2] = (int64_t)D->sa_nm.size();
    sizes[3] = (int64_t)D->na_pos.size();
    sizes[4] = (int64_t)D->names.size();
    sizes[5] = nb;
    sizes[6] = (int64_t)D->ref_names.size();
    sizes[7] = rb;
    return CORAL_OK;
}

extern "C" int coral_bam_decode_stats(void *handle, int64_t stats[3], double *seconds) {
    if (!handle || !stats || !seconds) return CORAL_ERR_ARG;
    Decoded *D = (Decoded *)handle;
    stats[0] = D->compressed_bytes;
    stats[1] = D->uncompressed_bytes;
    stats[2] = D->n_blocks;
    *seconds = D->seconds;
    return CORAL_OK;
}

extern "C" int coral_bam_decode_fill(void *handle, int32_t *tid, int32_t *pos, int32_t *end, int32_t *flag, int32_t *mapq,
                                     int32_t *qlen, int32_t *has_seq, int32_t *nm, int32_t *name_id, int32_t *n_cigar,
                                     int64_t *cigar_off, uint32_t *cigar, int64_t *sa_off, int32_t *sa, int32_t *sa_nm,
                                     int64_t *na_rec, int32_t *na_pos, char *names, int64_t *name_off, char *ref_names,
                                     int32_t *ref_lens) {
    if (!handle) return CORAL_ERR_ARG;
    Decoded *D = (Decoded *)handle;
    auto cp = [](auto *dst, const auto &v) { if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    cp(tid, D->tid); cp(pos, D->pos); cp(end, D->end); cp(flag, D->flag); cp(mapq, D->mapq); cp(qlen, D->qlen);
    cp(has_seq, D->has_seq); cp(nm, D->nm); cp(name_id, D->name_id); cp(n_cigar, D->n_cigar);
    cp(cigar_off, D->cigar_off); cp(cigar, D->cigar); cp(sa_off, D->sa_off); cp(sa, D->sa); cp(sa_nm, D->sa_nm);
    cp(na_rec, D->na_rec); cp(na_pos, D->na_pos); cp(ref_lens, D->ref_lens);
    cp(names, D->names.blob); cp(name_off, D->names.off);
    char *w = ref_names;
    for (auto &s : D->ref_names) { memcpy(w, s.c_str(), s.size() + 1); w += s.size() + 1; }
    return CORAL_OK;
}

extern "C" int coral_bam_decode_close(void *handle) {
    delete (Decoded *)handle;
    return CORAL_OK;
}

// SoA records -> BAM file (tests / benchmarks; the product only reads BAM).  SEQ is deterministic ACGT (hash of seed and
// record ordinal) with N at the listed aligned non-ACGT positions, QUAL absent, tags NM:i, SA:Z and CG:B,I for long CIGARs.
extern "C" int coral_bam_write(const char *path, int64_t n_rec, const int32_t *tid, const int32_t *pos, const int32_t *flag,
                               const int32_t *mapq, const int32_t *qlen, const int32_t *has_seq, const int32_t *nm,
                               const int32_t *name_id, const int32_t *n_cigar, const int64_t *cigar_off, const uint32_t *cigar,
                               const int64_t *sa_off, const int32_t *sa, const int32_t *sa_nm, int64_t n_na, const int64_t *na_rec,
                               const int32_t *na_pos, const char *const *names, int32_t n_ref, const char *const *ref_names,
                               const int32_t *ref_lens, uint32_t seed, int32_t level, int32_t n_threads) {
    if (!path || n_rec < 0 || n_ref < 0 || (n_ref > 0 && (!ref_names || !ref_lens))) return CORAL_ERR_ARG;
    if (n_rec > 0 && (!tid || !pos || !flag || !mapq || !qlen || !has_seq || !nm || !name_id || !n_cigar || !cigar_off || !sa_off || !names))
        return CORAL_ERR_ARG;
    FILE *fp = fopen(path, "wb");
    if (!fp) { g_bam_err = std::string("cannot create ") + path; return CORAL_ERR_ARG; }
    WriteJob J{n_rec, tid, pos, flag, mapq, qlen, has_seq, nm, name_id, n_cigar, cigar_off, cigar, sa_off, sa, sa_nm, n_na, na_rec, na_pos,
               names, n_ref, ref_names, seed};
    bool ok = true;
    {   // header
        std::vector<uint8_t> h;
        std::string text = "@HD\tVN:1.6\tSO:coordinate\n";
        for (int32_t r = 0; r < n_ref; ++r) text += std::string("@SQ\tSN:") + ref_names[r] + "\tLN:" + std::to_string(ref_lens[r]) + "\n";
        h.insert(h.end(), {'B', 'A', 'M', 1});
        put32(h, (uint32_t)text.size());
        h.insert(h.end(), text.begin(), text.end());
        put32(h, (uint32_t)n_ref);
        for (int32_t r = 0; r < n_ref; ++r) {
            const size_t ln = strlen(ref_names[r]) + 1;
            put32(h, (uint32_t)ln);
            h.insert(h.end(), (const uint8_t *)ref_names[r], (const uint8_t *)ref_names[r] + ln);
            put32(h, (uint32_t)ref_lens[r]);
        }
        std::vector<uint8_t> out;
        ok = bgzf_compress(h.data(), h.size(), level, out) && fwrite(out.data(), 1, out.size(), fp) == out.size();
    }
    // records: tasks of consecutive records, compressed independently (their last block is short), written in order
    const int nt = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads);
    const int64_t per_task = 256;
    const int64_t n_tasks = (n_rec + per_task - 1) / per_task;
    for (int64_t wave = 0; wave < n_tasks && ok; wave += 4 * nt) {
        const int64_t w1 = std::min<int64_t>(n_tasks, wave + 4 * nt);
        std::vector<std::vector<uint8_t>> outs((size_t)(w1 - wave));
        std::atomic<int64_t> next{wave};
        std::atomic<bool> bad{false};
        auto work = [&]() {
            std::vector<uint8_t> raw, seq;
            for (;;) {
                const int64_t t = next.fetch_add(1);
                if (t >= w1) return;
                raw.clear();
                for (int64_t i = t * per_task; i < std::min(n_rec, (t + 1) * per_task); ++i) write_record(J, i, raw, seq);
                if (!bgzf_compress(raw.data(), raw.size(), level, outs[(size_t)(t - wave)])) bad = true;
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        ok = !bad;
        for (auto &o : outs) ok = ok && fwrite(o.data(), 1, o.size(), fp) == o.size();
    }
    static const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    ok = ok && fwrite(EOF_BLOCK, 1, 28, fp) == 28;
    ok = (fclose(fp) == 0) && ok;
    if (!ok) { g_bam_err = "writing the BAM file failed"; return CORAL_ERR_FORMAT; }
    return CORAL_OK;
}

// `n_parts` byte strings -> one BGZF file (the writer behind bam.RecordBytes.write: part 0 the BAM header, part 1 the records).
// Every part is cut into blocks of at most 0xff00 input bytes and starts a block of its own, so the header ends a block as
// htslib's does and the first record's virtual offset has a zero low half; an empty part makes no block.  The blocks are shared
// out over n_threads as tasks of BGZF_TASK_BLOCKS consecutive blocks of one part, deflated independently of each other (the
// bytes do not depend on n_threads) and written in order; the 28-byte EOF block goes last.
extern "C" int coral_bgzf_write(const char *path, const uint8_t *const *parts, const int64_t *part_bytes, int32_t n_parts, int32_t level,
                                int32_t n_threads) {
    if (!path) { g_bam_err = "coral_bgzf_write: no path"; return CORAL_ERR_ARG; }
    if (level < 0 || level > 9) { g_bam_err = "coral_bgzf_write: level must be 0..9"; return CORAL_ERR_ARG; }
    if (n_parts < 0 || (n_parts > 0 && (!parts || !part_bytes))) { g_bam_err = "coral_bgzf_write: n_parts must be >= 0, with the parts and their sizes"; return CORAL_ERR_ARG; }
    struct Task { const uint8_t *in; size_t n; };
    const size_t BGZF_TASK_BLOCKS = 16, task_bytes = BGZF_TASK_BLOCKS * 0xff00;
    std::vector<Task> tasks;
    for (int32_t k = 0; k < n_parts; ++k) {
        if (part_bytes[k] < 0 || (part_bytes[k] > 0 && !parts[k])) { g_bam_err = "coral_bgzf_write: bad part"; return CORAL_ERR_ARG; }
        for (size_t at = 0, n = (size_t)part_bytes[k]; at < n; at += task_bytes) tasks.push_back(Task{parts[k] + at, std::min(task_bytes, n - at)});
    }
    FILE *fp = fopen(path, "wb");
    if (!fp) { g_bam_err = std::string("cannot create ") + path; return CORAL_ERR_ARG; }
    const int nt = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads);
    const size_t n_tasks = tasks.size();
    bool ok = true;
    for (size_t wave = 0; wave < n_tasks && ok; wave += 4 * (size_t)nt) {
        const size_t w1 = std::min(n_tasks, wave + 4 * (size_t)nt);
        std::vector<std::vector<uint8_t>> outs(w1 - wave);
        std::atomic<size_t> next{wave};
        std::atomic<bool> bad{false};
        auto work = [&]() {
            for (;;) {
                const size_t t = next.fetch_add(1);
                if (t >= w1) return;
                if (!bgzf_compress(tasks[t].in, tasks[t].n, level, outs[t - wave])) bad = true;
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nt && (size_t)t < w1 - wave; ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        ok = !bad;
        for (auto &o : outs) ok = ok && fwrite(o.data(), 1, o.size(), fp) == o.size();
    }
    static const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    ok = ok && fwrite(EOF_BLOCK, 1, 28, fp) == 28;
    ok = (fclose(fp) == 0) && ok;
    if (!ok) { g_bam_err = std::string("writing ") + path + " failed"; return CORAL_ERR_FORMAT; }
    return CORAL_OK;
}
