// coral_bamgpu.hip — BAM (BGZF) decode ON THE GPU: compressed file bytes go over PCIe, everything else happens in HBM.
//
// Replaces, like coral_bam.cpp, what the reference gets from pysam.AlignmentFile(path, 'rb') + the whole-file fetch()
// (/root/reference/src/infer_breakpoint_graph.py:65, :140-158), and produces the same SoA records as the CPU pipeline
// (tests/test_bam_gpu.py compares the two field by field).  The CPU pipeline tops out at the host's inflate rate (zlib,
// ~0.3 GB/s per core); here the host only moves compressed bytes:
//
//   feeder thread   pread(file) -> ring of small pinned buffers -> BGZF block table of the batch -> H2D          (copy stream)
//   k_bgzf_inflate  one wave per BGZF block: DEFLATE decode (coral_inflate_core.h) into the batch's buffer (inflate stream)
//   k_bgzf_crc      one wave per block: CRC-32 of the inflated bytes against the block's trailer (coral_crc32.h)
//   k_bam_find      one wave per 128 KiB segment: first plausible record start (chained check) + hop along block_size
//   k_bam_verify    one workgroup: follows the chain of segment landings from the batch's KNOWN first record; a segment
//                   whose guess is not on the chain is re-walked exactly, so record boundaries never rest on a heuristic
//   k_bam_starts    record start offsets, in file order
//   k_bam_keep + scan + k_bam_keep_compact   only with a record filter (keep_* of the request): the starts of the kept records,
//                   in order, in a second array - everything below sees only those
//   k_bam_meta      one wave per record: fixed fields, tag walk (NM, SA, CG), sizes of what the record contributes
//   (hipcub scans)  offsets of CIGAR ops (padded to 4), read-name bytes and SA text
//   k_bam_emit      one wave per record: CIGAR -> padded SoA op array (+ reference / query lengths), SEQ scan for non-ACGT
//                   codes, read name and SA text -> compact blobs for the host
//   worker thread   per batch, a few hundred bytes per record: read names -> ids, SA text -> numeric rows; the rare
//                   records with non-ACGT bases are gathered whole (k_bam_gather) and handled by the CPU pipeline's own routine.
// Requests that ride along a decode (coral_bam_request_t), each queued per batch before the slot is reused:
//   k_bam_cov_plan + k_bam_cov_count   window coverage: pysam count_coverage with a base-quality threshold over the segments
//   k_bam_cov_plan + k_bam_pileup      the same split by position and base (per_base): one 32-bit atomic per counted base
//                   (both kernels are cov_walk, the one CIGAR walk that applies the coverage rule, with a sink each)
//   k_bam_qc_plan + k_bam_qc           read QC: per read the sum of its QUAL bytes, and the 256-bin histogram of all of them
//   k_bam_index + k_bam_index_compact  index: per record the virtual offset, the UCSC bin and the linear-index windows of a
//                   BAI index, per batch the heads of the runs of equal (tid, bin)
//   k_bam_depth     binned depth: per record one walk of its CIGAR, one 64-bit atomic per run of lanes in the same bin
//   k_bam_reads_plan + k_bam_reads_emit   reads: the selected records as FASTQ text (nibbles -> ASCII, reverse strand mirrored
//                   and complemented), scattered to scanned offsets of a per-batch buffer the host collects one batch later
//   k_bam_reads_copy   reads, want_reads = 2: the selected records' own bytes, gathered to the same scanned offsets
// Host: one struct per request (carve / start / batch / finish); what it may borrow of the parse's scratch: struct Borrowed.
// Batches (64 MiB first, doubling up to 2.52 GiB inflated, coral_bamgpu_open) are double-buffered: while batch k is parsed, batch k + 1 is inflated
// and k + 2 is read.
// A record that straddles two batches is carried in front of the next batch's buffer.
//
// Multi-GPU: rank r of `world` decodes the BGZF blocks that start in its byte range of the file, with the
// same first-record / last-record rule as coral_bam_decode_range, so consecutive ranges neither drop nor repeat a record.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../../include/coral_hip.h"
#include "coral_bam_common.h"
#include "coral_crc32.h"
#include "coral_inflate_core.h"

using namespace coral_bam;

namespace {

#define WAVE 64
#define SEG_BYTES (128ll << 10)          // granularity of the speculative record-start search
#define CARRY_CAP (64ll << 20)           // room in front of a batch for the head of a straddling record
#define COMP_SLACK 4096                  // readable bytes behind the compressed batch (the input window reads ahead)
#define OVERHANG_BLOCKS 1024             // blocks behind a byte range its last record may straddle into (as coral_bam.cpp)
#define N_STAGE 4                        // pinned staging buffers of the feeder (file -> pinned -> device, round robin)
#define STAGE_BYTES (32ull << 20)
#define FIRST_BATCH (64ull << 20)        // inflated bytes of the first batch; the following ones double up to the cap

struct BlockDesc {
    uint32_t src_off;     // first DEFLATE byte, relative to the compressed batch
    uint32_t src_len;     // DEFLATE bytes
    uint32_t dst_off;     // first output byte, relative to the batch's first inflated byte
    uint32_t isize;
};

// ---------------------------------------------------------------------------------------------
// K_inflate
// ---------------------------------------------------------------------------------------------
#ifndef RING_LOG
#define RING_LOG 11                      // 2 KiB: with the tables 5.75 KiB of LDS per wave -> 27 waves per CU (4 KiB: 19 waves, +14 % time:
#endif                                   // the kernel is bound by the latency of its LDS round trips, profiles/r03_pmc_inflate.md)
#define RING_BYTES (1 << RING_LOG)       // recent output per wave, in LDS: LZ77 matches read it instead of global memory
#define RING_MASK (RING_BYTES - 1)

// Backend of coral_inflate::Inflater for one wave (the symbol loop is Inflater::codes_vector).
// Output positions are counted in "aligned coordinates" A = (out & 255) + o, so that A = 0 is a 256-byte line of global memory:
// ring index = A & RING_MASK, global address = gbase + A.  Every byte goes to the ring first (a literal: one ds_write_b8 of all
// lanes to the same address; a match: ring -> ring, or global -> ring when the source has left the ring); each time the
// position crosses a 256-byte line, the completed lines go to global memory as one dword store per lane.
// Input: two registers of 64 dwords each, used alternately (the bit buffer is refilled with v_readlane, never from memory).
// ABLATE (timing experiments of tools/bench_inflate.py with a -DCORAL_EXPERIMENTS build only; the product instantiates 0): 1 = no stores to global memory, 2 = matches whose
// source left the ring read the ring anyway, 4 = no match copy, 8 = no literal write.
template <int ABLATE>
struct DevWaveT {
    static constexpr bool vector_loop = true;
    int lane;
    float lane_half;            // lane + 0.5
    const char *in_base;        // dword-aligned start of the stream's input window (global memory)
    int stream_off;             // first byte of the DEFLATE stream, relative to in_base (0..3)
    int stream_len;
    int base_dw;                // dword index (from in_base) the Inflater's `dwords` counts from
    int win;                    // dword index of lane 0 of r0
    int last_dw;                // dword index of the stream's last byte
    uint32_t r0, r1;            // lane i: dwords win + i (being consumed) and win + 64 + i (loaded ahead) of the input
    int idx;                    // next dword of r0 (0..63)
    uint8_t *gbase;             // out - (out & 255)
    uint8_t *ring;              // LDS, RING_BYTES
    int a0, aend;               // aligned coordinates of the block's first byte and of the byte behind its last
    int a;                      // next output byte
    int gdone;                  // first byte not yet in global memory
    int attend;                 // the symbol loop calls attention() once `a` has reached this: a 256-byte line is complete (or,
                                // set to a - 1 by the rare paths, `over` was raised)
    uint32_t badv;              // (vector) a distance reached in front of the output
    bool over;                  // more output than the block may have, more input than the stream holds, or fail(): stop
    int err;                    // the first fail() code

    __device__ __forceinline__ uint32_t uni(uint32_t x) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    __device__ __forceinline__ uint32_t vec(uint32_t x) const {      // keeps what is computed from x on the vector pipe
        asm("" : "+v"(x));
        return x;
    }
    __device__ __forceinline__ uint32_t bfe(uint32_t x, uint32_t off, uint32_t width) const { return __builtin_amdgcn_ubfe(x, off, width); }
    __device__ __forceinline__ bool bad() const { return uni(badv) != 0u; }
    __device__ __forceinline__ void fail(int code) {                 // stop the symbol loop at its next round
        if (!err) err = code;
        over = true;
        attend = a - 1;
    }
    __device__ __forceinline__ bool failed() const { return over || err != 0 || bad(); }
    __device__ __forceinline__ int error_code() const { return err ? err : bad() ? (int)coral_inflate::ERR_DISTANCE : (int)coral_inflate::ERR_OVERFLOW; }
    __device__ __forceinline__ bool needs_attention() const { return a >= attend; }
    // Input window loads never start behind the stream's last dword: a corrupt stream that keeps asking for input re-reads the
    // end (and is stopped by the pull limit) instead of walking out of the compressed buffer (readable COMP_SLACK bytes beyond
    // its last stream, more than one 256-byte window).
    __device__ __forceinline__ uint32_t input_load(int dw) const {
        const int d = dw < last_dw ? dw : last_dw;
        return *reinterpret_cast<const uint32_t *>(in_base + (uint32_t)(d * 4 + lane * 4));
    }
    __device__ __forceinline__ void load_window() {
        r0 = input_load(win);
        r1 = input_load(win + WAVE);
        idx = 0;
    }
    // The next 32 input bits: one v_readlane; every 64th call moves on to the register loaded 64 dwords ago and starts the
    // load of its successor.
    __device__ __forceinline__ uint32_t next_dword() {
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)r0, idx);
        if (__builtin_expect(++idx == WAVE, 0)) {
            win += WAVE;
            r0 = r1;
            r1 = input_load(win + WAVE);
            idx = 0;
            if (win > last_dw + WAVE) fail(coral_inflate::ERR_INPUT);    // a whole window behind the stream's end: corrupt
        }
        return v;
    }
    __device__ __forceinline__ bool input_exhausted() const { return win + idx > last_dw + 4; }
    __device__ __forceinline__ bool input_overrun(long long dwords, int bc) const {
        return 32 * (base_dw + (int)dwords) - bc > 8 * (stream_off + stream_len);
    }
    __device__ __forceinline__ uint8_t *ring_at(uint32_t av) const { return ring + (av & RING_MASK); }
    // completed 256-byte lines ring -> global memory (the block's first line may start inside a line: byte stores there);
    // never beyond the block's last byte
    // Called by the symbol loop once per round when a >= attend; false = stop decoding.
    __device__ __forceinline__ bool attention() {
        drain();
        return !over;
    }
    __device__ __forceinline__ void drain() {
        if (a > aend) over = true;
        const int upto = (a < aend ? a : aend) & ~255;
        int g = gdone;
        if ((g & 255) && g < upto) {
            const int head = (g | 255) + 1;
_Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
            for (int p = g + lane; p < head; p += WAVE) gbase[p] = *ring_at((uint32_t)p);
            g = head;
        }
_Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
        for (; g < upto; g += 256) {
            const int p = g + 4 * lane;
            if (!(ABLATE & 1)) *reinterpret_cast<uint32_t *>(gbase + p) = *reinterpret_cast<const uint32_t *>(ring_at((uint32_t)p));
        }
        gdone = (int)uni((uint32_t)g);
        attend = over ? a - 1 : (gdone | 255) + 1;
    }
    __device__ __forceinline__ void finish() {                        // what is left goes out byte by byte
        drain();
        const int end = a < aend ? a : aend;
_Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
        for (int p = gdone + lane; p < end; p += WAVE) gbase[p] = *ring_at((uint32_t)p);
        gdone = end;
    }
    __device__ __forceinline__ void lit(uint32_t bytev) {
        if (!(ABLATE & 8)) *ring_at(vec((uint32_t)a)) = (uint8_t)bytev;
        ++a;
    }
    __device__ __forceinline__ void put_literal(uint32_t b) { lit(b); }
    // lenv, distv: the same value in every lane (vector registers)
    __device__ __forceinline__ void match(uint32_t lenv, uint32_t distv) {
        const uint32_t av = vec((uint32_t)a);
        // one byte more than the block may still take: a match that does not fit leaves `a` behind aend, which drain() turns into
        // `over` (cut to what fits, it would end the block at exactly its size and pass for a good one); the byte goes to the ring
        // only.  (a <= aend + 255; behind aend the room is 0 or, as unsigned, huge, and `over` is raised all the same)
        const uint32_t room = vec((uint32_t)(aend - a) + 1u);
        const uint32_t far_back = distv > av - (uint32_t)a0 ? 1u : 0u;    // reaches in front of the block's output: corrupt
        badv |= far_back;
        lenv = far_back ? 0u : (lenv < room ? lenv : room);
        const int len = (int)uni(lenv);
        const uint32_t dist = uni(distv);
        if (ABLATE & 4) {
            a += len;
            return;
        }
        if (__builtin_expect(dist <= RING_BYTES - 64 || (ABLATE & 2), 1)) {
            // byte k of the match = byte (k mod dist) of the dist bytes in front of it (k mod dist = k when dist >= 64 > lane)
            const float rd = __builtin_amdgcn_rcpf((float)distv);
            auto copy = [&](uint32_t k, float kh) {
                const uint32_t q = (uint32_t)(kh * rd);               // floor((k + 0.5) / dist): exact, (k + 0.5) / dist is >= 0.5 / dist off an integer
                const uint32_t km = distv < 64u ? k - q * distv : k;
                if (k < lenv) *ring_at(av + k) = *ring_at(av - distv + km);
            };
            copy((uint32_t)lane, lane_half);
            if (__builtin_expect(len > WAVE, 0)) {                    // chunks in order: LDS operations of a wave execute in order
_Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
                for (int k = lane + WAVE; k < len; k += WAVE) copy((uint32_t)k, (float)k + 0.5f);
            }
        } else {
            // the source left the ring: it is in global memory (drained up to the last line boundary; a - dist + len lies below it)
            const uint8_t *src = gbase + (a - (int)dist);
_Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
            for (int k = lane; k < len; k += WAVE) *ring_at(av + (uint32_t)k) = src[k];
        }
        a += len;
    }
    // The hot path of the symbol loop, by hand (gfx950 ISA).  The compiler turns Inflater::codes_vector into a state machine of
    // boolean SGPR pairs and register copies at every join (≈42 scalar + 13 branch + 35 vector instructions per symbol); this loop
    // needs ≈20 + 7 + 24 (rocprofv3 counters): a literal is 9 scalar + 8 vector instructions behind its table
    // look-up, a short match ≈20 + 25.  It takes
    // what is common — literal / length / distance codes found in the LDS tables, refills from the current input register,
    // every match whose distance is known to lie inside the block (from the ring, or from global memory once the source has left
    // the ring) — and RETURNS, with nothing half-done, where it cannot go on:
    //   0  at a symbol boundary: the block's last 260 bytes begin, its first (partial) line is complete or fail() asked for a stop
    //      (completed whole lines are written to global memory inside the loop), the refill would switch the input register, or
    //      the code is not in the table (long code, end of block)
    //   1  a length has been read (lenv) and the input register must be switched, or the distance code is not in the table
    //   2  length and distance have been read (lenv, distv), but the distance reaches further back than this call's first byte
    //      was from the block's start (`span` is taken at entry: a distance the general path accepts may come back here, never
    //      the other way round)
    // and Inflater::codes_vector does that one step.  Everything is wave-uniform; the lanes only differ in the copy.  The bit
    // buffer lives in s[70:71] inside (its low half is needed on its own), s[72:73] hold a refill.
    // Hazards of gfx940-class hardware that the assembler does not pad inside inline assembly: a VALU result read by
    // v_readfirstlane needs one wait state, a transcendental result (v_rcp_f32) read by another VALU instruction one.
    static constexpr bool has_fast = (ABLATE == 0);
    __device__ __forceinline__ int fast(uint64_t &bb, int &bc, long long &dwords, const coral_inflate::Tables *T, uint32_t &lenv, uint32_t &distv) {
        int lim = attend < aend - 260 ? attend : aend - 260;
        const uint32_t span = (uint32_t)(a - a0);
        const uint32_t dlim = span < (uint32_t)(RING_BYTES - 64) ? span : (uint32_t)(RING_BYTES - 64);
        const uint32_t ring_lds = (uint32_t)(uintptr_t)ring, ll_lds = (uint32_t)(uintptr_t)T->ll, dt_lds = (uint32_t)(uintptr_t)T->dt;
        int state;
        const int idx_in = idx;
        uint32_t se, sn, sx, slen;
        uint32_t vb, ve, vt, vn, vxb, vx, vq, vs, out_len, out_dist;
        // (ring addresses: the ring is aligned to its size, so (x & RING_MASK) | ring is one v_and_or_b32 with the mask in a VGPR)
#define CORAL_INFL_REFILL                                           \
            "v_readlane_b32 s72, %[r0], %[idx]\n"                   \
            "s_mov_b32 s73, 0\n"                                    \
            "s_lshl_b64 s[72:73], s[72:73], %[bc]\n"                \
            "s_or_b64 s[70:71], s[70:71], s[72:73]\n"               \
            "s_add_i32 %[bc], %[bc], 32\n"                          \
            "s_add_i32 %[idx], %[idx], 1\n"
#define CORAL_INFL_LOOKUP                                           \
            "v_mov_b32 %[vb], s70\n"                                \
            "v_and_b32 %[vt], 0x3ff, %[vb]\n"                       \
            "v_lshl_add_u32 %[vt], %[vt], 1, %[llb]\n"              \
            "ds_read_u16 %[ve], %[vt]\n"                            \
            "s_waitcnt lgkmcnt(0)\n"                                \
            "v_readfirstlane_b32 %[se], %[ve]\n"                    \
            "s_bitcmp1_b32 %[se], 4\n"
#define CORAL_INFL_LITERAL                                          \
            "s_and_b32 %[sn], %[se], 15\n"                          \
            "v_mov_b32 %[vt], %[a]\n"                               \
            "s_lshr_b64 s[70:71], s[70:71], %[sn]\n"                \
            "v_lshrrev_b32 %[vx], 8, %[ve]\n"                       \
            "s_sub_i32 %[bc], %[bc], %[sn]\n"                       \
            "v_and_or_b32 %[vt], %[vt], %[vmask], %[ring]\n"        \
            "s_mov_b64 exec, 1\n"                                   \
            "ds_write_b8 %[vt], %[vx]\n"                            \
            "s_mov_b64 exec, -1\n"                                  \
            "s_add_i32 %[a], %[a], 1\n"
        asm volatile(
            "s_mov_b64 s[70:71], %[bb]\n"
            "v_mov_b32 %[olen], 0\n"
            "v_mov_b32 %[odist], 0\n"
            "Ltop_%=:\n"
            "s_cmp_ge_i32 %[a], %[lim]\n"
            "s_cbranch_scc1 Lattn_%=\n"
            "Lbits_%=:\n"
            "s_cmp_gt_i32 %[bc], 32\n"
            "s_cbranch_scc1 Lsym_%=\n"
            "s_cmp_eq_u32 %[idx], 63\n"
            "s_cbranch_scc1 Lexit0_%=\n"
            CORAL_INFL_REFILL
            "Lsym_%=:\n"                                       // more than 32 bits: first table look-up of the round
            CORAL_INFL_LOOKUP
            "s_cbranch_scc1 Lnotlit_%=\n"
            CORAL_INFL_LITERAL                                 // (one lane stores: 64 lanes storing to one address are 64 LDS accesses)
            CORAL_INFL_LOOKUP                                  // at least 23 bits left: second look-up without a refill check
            "s_cbranch_scc1 Lnotlit_%=\n"
            CORAL_INFL_LITERAL
            "s_branch Ltop_%=\n"
            "Lnotlit_%=:\n"                                    // ve / se = table entry, vb = the bits it was looked up with (>= 23)
            "s_and_b32 %[sn], %[se], 15\n"
            "v_and_b32 %[vn], 15, %[ve]\n"
            "v_bfe_u32 %[vxb], %[ve], 5, 3\n"                  // extra bits of the length code
            "s_cmp_eq_u32 %[sn], 0\n"
            "v_bfe_u32 %[vt], %[vb], %[vn], %[vxb]\n"
            "v_lshrrev_b32 %[vx], 8, %[ve]\n"                  // length base - 3
            "s_cbranch_scc1 Lexit0_%=\n"                       // not in the table (nothing consumed)
            "v_add_u32 %[vn], %[vn], %[vxb]\n"
            "v_add3_u32 %[olen], %[vx], %[vt], 3\n"
            "v_readfirstlane_b32 %[sn], %[vn]\n"               // (one instruction between the VALU write and this read)
            "s_lshr_b64 s[70:71], s[70:71], %[sn]\n"
            "s_sub_i32 %[bc], %[bc], %[sn]\n"
            "v_readfirstlane_b32 %[slen], %[olen]\n"
            "s_cmp_gt_i32 %[bc], 32\n"                         // the distance code needs up to 8 + 13 bits
            "s_cbranch_scc1 Ldist_%=\n"
            "s_cmp_eq_u32 %[idx], 63\n"
            "s_cbranch_scc1 Lexit1_%=\n"
            CORAL_INFL_REFILL
            "Ldist_%=:\n"
            "v_mov_b32 %[vb], s70\n"
            "v_and_b32 %[vt], 0xff, %[vb]\n"
            "v_lshl_add_u32 %[vt], %[vt], 2, %[dtb]\n"
            "ds_read_b32 %[ve], %[vt]\n"
            "s_waitcnt lgkmcnt(0)\n"
            "v_and_b32 %[vn], 15, %[ve]\n"
            "v_bfe_u32 %[vxb], %[ve], 8, 4\n"
            "v_lshrrev_b32 %[vx], 16, %[ve]\n"
            "v_bfe_u32 %[vt], %[vb], %[vn], %[vxb]\n"
            "v_add_u32 %[vn], %[vn], %[vxb]\n"
            "v_add_u32 %[odist], %[vx], %[vt]\n"               // a code that is not in the table has entry 0: distance 0, no bits
            "v_readfirstlane_b32 %[sn], %[vn]\n"
            "v_add_u32 %[vt], -1, %[odist]\n"
            "s_lshr_b64 s[70:71], s[70:71], %[sn]\n"
            "s_sub_i32 %[bc], %[bc], %[sn]\n"
            "v_cmp_le_u32 vcc, %[dlim], %[vt]\n"               // dist - 1 >= dlim: not in the table (0), behind the ring, or maybe
            "s_cbranch_vccnz Lfarq_%=\n"                       // in front of the block's first byte
            "v_min_u32 %[vt], 64, %[odist]\n"                  // longer than 64 bytes, or overlapping its own source (dist < len):
            "v_cmp_lt_u32 vcc, %[vt], %[olen]\n"               // the general copy below; otherwise byte k comes from a - dist + k
            "s_cbranch_vccnz Llong_%=\n"
            "v_sub_u32 %[vs], %[a], %[odist]\n"
            "v_add_u32 %[vt], %[a], %[lane]\n"
            "v_add_u32 %[vs], %[vs], %[lane]\n"
            "v_and_or_b32 %[vt], %[vt], %[vmask], %[ring]\n"
            "v_and_or_b32 %[vs], %[vs], %[vmask], %[ring]\n"
            "v_cmp_gt_u32 vcc, %[slen], %[lane]\n"
            "s_mov_b64 exec, vcc\n"
            "ds_read_u8 %[vx], %[vs]\n"
            "s_waitcnt lgkmcnt(0)\n"
            "ds_write_b8 %[vt], %[vx]\n"
            "s_mov_b64 exec, -1\n"
            "s_add_i32 %[a], %[a], %[slen]\n"
            "s_branch Ltop_%=\n"
            "Llong_%=:\n"                                      // source in the ring, any length: byte k of the match = byte (k mod dist) of the
            "v_cvt_f32_u32 %[vq], %[odist]\n"                  // dist bytes in front; chunks of 64 in order (a chunk may read what the chunk
                                                               // before it wrote: LDS operations of a wave execute in order)
            "v_rcp_f32 %[vn], %[vq]\n"
            "v_mov_b32 %[vxb], %[lane]\n"                      // k
            "v_mov_b32 %[ve], %[laneh]\n"                      // k + 0.5
            "s_mov_b32 %[sx], 0\n"
            "Lchunk_%=:\n"
            "v_mul_f32 %[vq], %[ve], %[vn]\n"
            "v_cvt_u32_f32 %[vq], %[vq]\n"
            "v_mul_lo_u32 %[vq], %[vq], %[odist]\n"
            "v_sub_u32 %[vq], %[vxb], %[vq]\n"                 // k mod dist (when dist < 64): floor((k + 0.5) / dist) is exact (DevWaveT::match)
            "v_cmp_gt_u32 vcc, 64, %[odist]\n"
            "v_cndmask_b32 %[vq], %[vxb], %[vq], vcc\n"        // dist >= 64: k itself
            "v_sub_u32 %[vs], %[a], %[odist]\n"
            "v_add_u32 %[vs], %[vs], %[vq]\n"
            "v_and_or_b32 %[vs], %[vs], %[vmask], %[ring]\n"
            "v_add_u32 %[vt], %[a], %[vxb]\n"
            "v_and_or_b32 %[vt], %[vt], %[vmask], %[ring]\n"
            "v_cmp_gt_u32 vcc, %[slen], %[vxb]\n"
            "s_mov_b64 exec, vcc\n"
            "ds_read_u8 %[vx], %[vs]\n"
            "s_waitcnt lgkmcnt(0)\n"
            "ds_write_b8 %[vt], %[vx]\n"
            "s_mov_b64 exec, -1\n"
            "v_add_u32 %[vxb], 64, %[vxb]\n"
            "v_add_f32 %[ve], 0x42800000, %[ve]\n"             // + 64.0
            "s_add_i32 %[sx], %[sx], 64\n"
            "s_cmp_lt_u32 %[sx], %[slen]\n"
            "s_cbranch_scc1 Lchunk_%=\n"
            "s_add_i32 %[a], %[a], %[slen]\n"
            "s_branch Ltop_%=\n"
            "Lfarq_%=:\n"
            "v_cmp_eq_u32 vcc, 0, %[odist]\n"                  // distance code not in the table (nothing of it consumed)
            "s_cbranch_vccnz Lexit1_%=\n"
            "v_cmp_lt_u32 vcc, %[dspan], %[odist]\n"           // further back than this call's first output byte was from the
            "s_cbranch_vccnz Lexit2_%=\n"                      // block's start: the general path tells a bad distance from a good one
            // the source has left the ring (dist > RING_BYTES - 64): it is in global memory, drained up to the last 256-byte line
            // boundary, and a - dist + len lies below that (DevWaveT::match)
            "v_sub_u32 %[vs], %[a], %[odist]\n"
            "v_add_u32 %[vs], %[vs], %[lane]\n"
            "v_add_u32 %[vt], %[a], %[lane]\n"
            "v_mov_b32 %[vxb], %[lane]\n"
            "s_mov_b32 %[sx], 0\n"
            "Lfchunk_%=:\n"
            "v_and_or_b32 %[vq], %[vt], %[vmask], %[ring]\n"
            "v_cmp_gt_u32 vcc, %[slen], %[vxb]\n"
            "s_mov_b64 exec, vcc\n"
            "global_load_ubyte %[vx], %[vs], %[gb]\n"
            "s_waitcnt vmcnt(0)\n"
            "ds_write_b8 %[vq], %[vx]\n"
            "s_mov_b64 exec, -1\n"
            "v_add_u32 %[vs], 64, %[vs]\n"
            "v_add_u32 %[vt], 64, %[vt]\n"
            "v_add_u32 %[vxb], 64, %[vxb]\n"
            "s_add_i32 %[sx], %[sx], 64\n"
            "s_cmp_lt_u32 %[sx], %[slen]\n"
            "s_cbranch_scc1 Lfchunk_%=\n"
            "s_add_i32 %[a], %[a], %[slen]\n"
            "s_branch Ltop_%=\n"
            "Lattn_%=:\n"                                      // a >= lim.  Completed 256-byte lines go ring -> global memory right here
            "s_cmp_lt_i32 %[a], %[attend]\n"                  // (one dword per lane, DevWaveT::drain) unless the block's last bytes
            "s_cbranch_scc1 Lexit0_%=\n"                       // begin, the block's first line is a partial one, or fail() moved `attend`
            "s_cmp_gt_i32 %[a], %[aendz]\n"
            "s_cbranch_scc1 Lexit0_%=\n"
            "s_and_b32 %[sn], %[gdone], 255\n"
            "s_cmp_lg_u32 %[sn], 0\n"
            "s_cbranch_scc1 Lexit0_%=\n"
            "s_add_i32 %[sx], %[gdone], 256\n"
            "s_cmp_lg_u32 %[sx], %[attend]\n"
            "s_cbranch_scc1 Lexit0_%=\n"
            "Ldrain_%=:\n"
            "v_lshl_add_u32 %[vt], %[lane], 2, %[gdone]\n"
            "v_and_or_b32 %[vs], %[vt], %[vmask], %[ring]\n"
            "ds_read_b32 %[vx], %[vs]\n"
            "s_mov_b32 %[gdone], %[sx]\n"
            "s_add_i32 %[sx], %[sx], 256\n"
            "s_waitcnt lgkmcnt(0)\n"
            "global_store_dword %[vt], %[vx], %[gb]\n"
            "s_cmp_le_i32 %[sx], %[a]\n"
            "s_cbranch_scc1 Ldrain_%=\n"
            "s_mov_b32 %[attend], %[sx]\n"                     // = (gdone | 255) + 1
            "s_min_i32 %[lim], %[sx], %[aendz]\n"
            "s_cmp_ge_i32 %[a], %[lim]\n"                      // (only when the block's last 260 bytes have begun)
            "s_cbranch_scc1 Lexit0_%=\n"
            "s_branch Lbits_%=\n"
            "Lexit2_%=:\n"
            "s_mov_b32 %[state], 2\n"
            "s_branch Lout_%=\n"
            "Lexit1_%=:\n"
            "s_mov_b32 %[state], 1\n"
            "s_branch Lout_%=\n"
            "Lexit0_%=:\n"
            "s_mov_b32 %[state], 0\n"
            "Lout_%=:\n"
            "s_mov_b64 %[bb], s[70:71]\n"
            : [bb] "+s"(bb), [bc] "+s"(bc), [idx] "+s"(idx), [a] "+s"(a), [gdone] "+s"(gdone), [attend] "+s"(attend), [lim] "+s"(lim), [state] "=&s"(state), [se] "=&s"(se), [sn] "=&s"(sn),
              [sx] "=&s"(sx), [slen] "=&s"(slen), [vb] "=&v"(vb), [ve] "=&v"(ve), [vt] "=&v"(vt), [vn] "=&v"(vn), [vxb] "=&v"(vxb),
              [vx] "=&v"(vx), [vq] "=&v"(vq), [vs] "=&v"(vs), [olen] "=&v"(out_len), [odist] "=&v"(out_dist)
            : [aendz] "s"(aend - 260), [dlim] "s"(dlim), [dspan] "s"(span), [gb] "s"(gbase), [ring] "s"(ring_lds), [llb] "s"(ll_lds), [dtb] "s"(dt_lds),
              [r0] "v"(r0), [lane] "v"(lane), [laneh] "v"(lane_half), [vmask] "v"((uint32_t)RING_MASK)
            : "s70", "s71", "s72", "s73", "vcc", "scc", "memory");
#undef CORAL_INFL_REFILL
#undef CORAL_INFL_LOOKUP
#undef CORAL_INFL_LITERAL
        dwords += idx - idx_in;                             // (the input register is only switched by the general path)
        lenv = out_len;
        distv = out_dist;
        return state;
    }
    __device__ __forceinline__ bool copy_match(int len, int dist) {   // (the plain loop's interface; unused on the device)
        match((uint32_t)len, (uint32_t)dist);
        return true;
    }
    __device__ __forceinline__ bool copy_stored(int dwords, uint32_t n) {
        const int from = 4 * (base_dw + dwords) - stream_off;          // relative to the stream
        if (from < 0 || from + (int)n > stream_len) return false;
        const uint8_t *src = reinterpret_cast<const uint8_t *>(in_base) + stream_off + from;
_Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
        for (uint32_t done = 0; done < n;) {                      // through the ring, 256 bytes at a time (it is drained in step)
            const uint32_t step = n - done < 256u ? n - done : 256u;
_Pragma("clang loop unroll(disable) vectorize(disable) interleave(disable)")
            for (uint32_t k = (uint32_t)lane; k < step; k += WAVE) *ring_at((uint32_t)a + k) = src[done + k];
            a += (int)step;
            drain();
            done += step;
        }
        return true;
    }
    __device__ __forceinline__ uint32_t reset_input_after_stored(int dwords, uint32_t n) {
        const int byte = 4 * (base_dw + dwords) + (int)n;
        base_dw = byte >> 2;
        win = base_dw;
        load_window();
        return (uint32_t)(byte & 3) * 8u;
    }
    __device__ __forceinline__ int produced() const { return a - a0; }
    __device__ __forceinline__ int capacity() const { return aend - a0; }
    __device__ __forceinline__ void add_count(uint32_t *c) { atomicAdd(c, 1u); }
    __device__ __forceinline__ void fence() {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

typedef DevWaveT<0> DevWave;

#ifndef INFL_WAVES
#define INFL_WAVES 1                     // one wave per workgroup: LDS (tables + ring, 5.75 KiB) is allocated per wave
#endif
#ifdef INFL_WAVES_PER_EU                  // (occupancy experiments: caps the kernel's VGPRs so that this many waves fit a SIMD)
#define INFL_OCCUPANCY __attribute__((amdgpu_waves_per_eu(INFL_WAVES_PER_EU, INFL_WAVES_PER_EU)))
#else
#define INFL_OCCUPANCY
#endif
template <int ABLATE>
__global__ __launch_bounds__(INFL_WAVES *WAVE) INFL_OCCUPANCY void k_bgzf_inflate(const uint8_t *__restrict__ comp, const BlockDesc *__restrict__ desc,
                                                                     int n_blocks, uint8_t *out, int32_t *__restrict__ status) {
    __shared__ coral_inflate::Tables tables[INFL_WAVES];
    __shared__ __attribute__((aligned(RING_BYTES))) uint8_t rings[INFL_WAVES][RING_BYTES];      // (DevWaveT::fast relies on the alignment)
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * INFL_WAVES + wib;
    if (b >= n_blocks) return;
    const BlockDesc d = desc[b];
    if (d.isize == 0) {
        if (lane == 0) status[b] = 0;
        return;
    }
    // (comp is a 4-byte aligned allocation of the caller; pointers keep their kernel-argument provenance so that the loads and
    // stores are global_*, not flat_*)
    const uint32_t mis = (uint32_t)(((uintptr_t)comp + d.src_off) & 3u);
    DevWaveT<ABLATE> w;
    w.lane = lane;
    w.lane_half = (float)lane + 0.5f;
    w.in_base = reinterpret_cast<const char *>(comp) + (d.src_off - mis);
    w.stream_off = (int)mis;
    w.stream_len = (int)d.src_len;
    w.base_dw = 0;
    w.win = 0;
    w.last_dw = (int)((mis + d.src_len) >> 2);
    w.a0 = (int)(((uintptr_t)out + d.dst_off) & 255u);
    w.aend = w.a0 + (int)d.isize;
    w.gbase = out + ((long long)d.dst_off - w.a0);
    w.ring = rings[wib];
    w.a = w.gdone = w.a0;
    w.attend = (w.a0 | 255) + 1;
    w.badv = 0;
    w.over = false;
    w.err = 0;
    w.load_window();
    coral_inflate::Inflater<DevWaveT<ABLATE>> inf(w, &tables[wib]);
    int rc = inf.run((int)mis * 8);
    w.finish();
    if (rc == coral_inflate::OK && w.failed()) rc = w.error_code();
    if (lane == 0) status[b] = rc;
}

// ---------------------------------------------------------------------------------------------
// K_crc: the CRC-32 of every inflated block against the one in its BGZF trailer (what htslib checks in bgzf_read_block)
// ---------------------------------------------------------------------------------------------
#define ERR_CRC 100
// One wave per block: every lane takes a contiguous chunk, computes its remainder, shifts it by the number of bytes behind its
// chunk (multiplication by x^(8 n) mod P, coral_crc32.h) and the wave XORs the 64 results.  A block that inflated cleanly but has
// another checksum gets status ERR_CRC.
// Round 3 (the decode timeline showed this kernel at 3.8 ms per 1 GiB batch, serialised behind the inflate): (i) chunks start on
// 64-byte lines of global memory (lane 0 also takes the block's unaligned head) and are read 64 bytes at a time as four aligned
// 16-byte loads, so a cache line is fetched once by the one lane that owns it — with 4-byte loads at a 1 KB lane stride every
// line was touched sixteen times; (ii) four 256-entry tables in LDS (slicing by 4): the four look-ups of a dword are independent
// instead of a chain of four; (iii) the kernel runs on a stream of its own, next to the following batch's inflate.
// One-wave workgroups (as every kernel that runs beside the next batch's inflate launch): that launch keeps 27 waves per CU
// resident — 7 + 7 + 7 + 6 on the four SIMDs, 504 of 512 VGPRs on the full ones — so a four-wave workgroup, which needs room on
// all four SIMDs at once, only started when the inflate launch was nearly over (rocprofv3 timeline: 25 ms instead of 1 ms);
// its 4 KiB of tables fit the LDS the inflate waves leave (27 x 5 888 B of 160 KiB).
__global__ __launch_bounds__(WAVE) void k_bgzf_crc(const uint8_t *__restrict__ out, const BlockDesc *__restrict__ desc, const uint32_t *__restrict__ want,
                                                    int n_blocks, int32_t *__restrict__ status) {
    __shared__ uint32_t T[4][256];
    for (uint32_t i = threadIdx.x; i < 256u; i += WAVE) T[0][i] = coral_crc::table_entry(i);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 256u; i += WAVE) {
        uint32_t c = T[0][i];
        for (int k = 1; k < 4; ++k) {                     // T[k][i] = T[0][i] followed by k zero bytes
            c = (c >> 8) ^ T[0][c & 0xffu];
            T[k][i] = c;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int b = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (b >= n_blocks) return;
    const uint32_t n = desc[b].isize;
    if (n == 0 || status[b] != 0) return;
    const uint8_t *p = out + desc[b].dst_off;
    const uint32_t head = (uint32_t)((64u - (uint32_t)((uintptr_t)p & 63u)) & 63u);      // bytes in front of the first 64-byte line
    const uint32_t body = n > head ? n - head : 0u;
    const uint32_t per = ((((body + 63u) >> 6) + 63u) >> 6) << 6;                        // bytes per lane: whole lines
    const uint32_t a = lane == 0 ? 0u : min(n, head + (uint32_t)lane * per);
    const uint32_t e = min(n, head + (uint32_t)(lane + 1) * per);
    auto byte_step = [&](uint32_t r, uint32_t v) { return T[0][(r ^ v) & 0xffu] ^ (r >> 8); };
    auto dword_step = [&](uint32_t r, uint32_t w) {
        r ^= w;
        return T[3][r & 0xffu] ^ T[2][(r >> 8) & 0xffu] ^ T[1][(r >> 16) & 0xffu] ^ T[0][r >> 24];
    };
    uint32_t r = 0, k = a;
    for (; k < e && (((uintptr_t)(p + k)) & 15u); ++k) r = byte_step(r, p[k]);           // (lane 0 only: the unaligned head)
    for (; k + 64 <= e; k += 64) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p + k);
        const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
        r = dword_step(r, v0.x); r = dword_step(r, v0.y); r = dword_step(r, v0.z); r = dword_step(r, v0.w);
        r = dword_step(r, v1.x); r = dword_step(r, v1.y); r = dword_step(r, v1.z); r = dword_step(r, v1.w);
        r = dword_step(r, v2.x); r = dword_step(r, v2.y); r = dword_step(r, v2.z); r = dword_step(r, v2.w);
        r = dword_step(r, v3.x); r = dword_step(r, v3.y); r = dword_step(r, v3.z); r = dword_step(r, v3.w);
    }
    for (; k + 4 <= e; k += 4) r = dword_step(r, *reinterpret_cast<const uint32_t *>(p + k));      // (4-byte aligned: k is, from the loop above)
    for (; k < e; ++k) r = byte_step(r, p[k]);
    uint32_t t = coral_crc::shift(r, n - e);
    if (lane == 0) t ^= coral_crc::shift(0xffffffffu, n);
    for (int d = 32; d > 0; d >>= 1) t ^= (uint32_t)__shfl_xor((int)t, d);
    if (lane == 0 && ~t != want[b]) status[b] = ERR_CRC;
}

// ---------------------------------------------------------------------------------------------
// record boundaries
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

// the plausibility test of coral_bam.cpp (plausible_record), on device memory
__device__ __forceinline__ bool plausible(const uint8_t *buf, long long q, long long data_end, int n_ref, long long *len) {
    const long long n = data_end - q;
    if (n < 36) return false;
    const uint8_t *p = buf + q;
    const uint32_t bs = ld32(p);
    if (bs < 34 || bs > (1u << 29)) return false;
    const int32_t refID = (int32_t)ld32(p + 4), pos = (int32_t)ld32(p + 8);
    const uint32_t l_name = p[12], n_cig = ld16(p + 16), l_seq = ld32(p + 20);
    const int32_t mate = (int32_t)ld32(p + 24), mpos = (int32_t)ld32(p + 28);
    if (refID < -1 || refID >= n_ref || mate < -1 || mate >= n_ref || pos < -1 || mpos < -1) return false;
    if (l_name < 2 || l_seq > (1u << 29)) return false;
    const unsigned long long fixed = 32ull + l_name + 4ull * n_cig + ((unsigned long long)l_seq + 1) / 2 + l_seq;
    if (fixed > bs) return false;
    if (n >= 36ll + l_name) {
        const uint8_t *nm = p + 36;
        if (nm[l_name - 1] != 0) return false;
        for (uint32_t k = 0; k + 1 < l_name; ++k)
            if (nm[k] < 33 || nm[k] > 126) return false;
    }
    *len = 4ll + bs;
    return true;
}

// Hop along block_size from x while the record starts inside [.., seg_end) and in front of `limit` and is complete in the
// batch.  Returns the landing position (first start not counted) and the count; *err is set for a record shorter than its
// fixed fields.  The SAME function serves the speculative pass and the exact re-walk.
__device__ __forceinline__ long long hop(const uint8_t *buf, long long x, long long seg_end, long long limit, long long data_end, int *count,
                                         int *err) {
    int c = 0;
    while (x < seg_end && x < limit) {
        if (x + 4 > data_end) break;
        const long long len = 4ll + ld32(buf + x);
        if (len < 36) { *err = 1; break; }
        if (x + len > data_end) break;
        ++c;
        x += len;
    }
    *count = c;
    return x;
}

// per segment s (buffer offsets [s * SEG, (s + 1) * SEG) clipped to [begin, data_end)): first plausible start, landing, count
__global__ __launch_bounds__(256) void k_bam_find(const uint8_t *__restrict__ buf, long long begin, long long data_end, long long limit,
                                                   int n_ref, int seg0, int n_seg, long long *__restrict__ seg_first,
                                                   long long *__restrict__ seg_land, int32_t *__restrict__ seg_count,
                                                   int32_t *__restrict__ seg_valid) {
    const int lane = threadIdx.x & 63;
    const int s = seg0 + (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (s >= seg0 + n_seg) return;
    const long long a = max((long long)s * SEG_BYTES, begin), b = min((long long)(s + 1) * SEG_BYTES, data_end);
    long long first = -1;
    // 256 positions per round: the first eight bytes of all four positions of a lane (block_size, refID) are loaded together —
    // ONE memory round trip per round, and that filter alone rejects nearly every position that is not a record start (round 3:
    // with one position per lane and round the kernel was a chain of ~280 dependent round trips per segment)
    for (long long x0 = a; x0 < b && first < 0; x0 += 4 * WAVE) {
        bool pre[4];
        unsigned long long head[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long x = x0 + j * WAVE + lane;
            pre[j] = x < b && x + 36 <= data_end;
            head[j] = 0;
            if (pre[j]) __builtin_memcpy(&head[j], buf + x, 8);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t bs = (uint32_t)head[j];
            const int32_t refID = (int32_t)(head[j] >> 32);
            pre[j] = pre[j] && bs >= 34 && bs <= (1u << 29) && refID >= -1 && refID < n_ref;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (first >= 0) break;
            bool ok = false;
            if (pre[j]) {
                long long q = x0 + j * WAVE + lane;
                int chain = 0;
                ok = true;
                while (chain < 8 && q + 36 <= data_end) {
                    long long len;
                    if (!plausible(buf, q, data_end, n_ref, &len)) { ok = false; break; }
                    q += len;
                    ++chain;
                }
                ok = ok && chain >= 3;
            }
            const unsigned long long m = __ballot(ok);
            if (m != 0ull) first = x0 + j * WAVE + (long long)__builtin_ctzll(m);
        }
    }
    int count = 0, err = 0;
    long long land = first;
    if (first >= 0) land = hop(buf, first, b, limit, data_end, &count, &err);
    if (lane == 0) {
        seg_first[s] = err ? -1 : first;           // (a guess that runs into a malformed record is no guess)
        seg_land[s] = land;
        seg_count[s] = count;
        seg_valid[s] = 0;
    }
}

// result: [0] records, [1] carry position (first start not counted; may lie behind data_end), [2] done (limit reached),
//         [3] error (1 = malformed record, 2 = no record start found while searching), [4] segments re-walked, [5] first start
__global__ __launch_bounds__(WAVE) void k_bam_verify(const uint8_t *__restrict__ buf, long long known_start, long long begin, long long data_end,
                                                      long long limit, int seg0, int n_seg, long long *__restrict__ seg_first,
                                                      long long *__restrict__ seg_land, int32_t *__restrict__ seg_count,
                                                      int32_t *__restrict__ seg_valid, long long *__restrict__ seg_base,
                                                      long long *__restrict__ result) {
    const int lane = threadIdx.x;
    long long cur = known_start;
    if (cur < 0) {                                   // first batch of a byte range: the lowest confirmed candidate
        for (int s0 = seg0; s0 < seg0 + n_seg && cur < 0; s0 += WAVE) {
            const int s = s0 + lane;
            const long long f = s < seg0 + n_seg ? seg_first[s] : -1;
            const unsigned long long m = __ballot(f >= 0);
            if (m != 0ull) cur = __shfl(f, (int)__builtin_ctzll(m));
        }
        if (cur < 0) {
            if (lane == 0) { result[0] = 0; result[1] = data_end; result[2] = 0; result[3] = 2; result[4] = 0; result[5] = -1; }
            return;
        }
    }
    const long long first_start = cur;
    long long total = 0, fixups = 0;
    int error = 0, done = 0;
    const int s_end = seg0 + n_seg;
    // The walk is serial (the next segment is where this one's records land), but its memory round trips need not be: lane k
    // loads the guess of segment sb + k, and the chain is followed through those 64 segments in registers with v_readlane.
    // Positions inside a batch fit 32 bits (coral_bamgpu_open keeps CARRY_CAP + the batch below 4 GiB), which halves the
    // arithmetic of the loop — one wave, one instruction at a time: the instruction count IS the time (round 3: one dependent
    // round trip and ~140 instructions per segment were 6 ms per 2.4 GiB batch, on the parse stream's critical path).
    const uint32_t lim32 = limit > 0xffffffffll ? 0xffffffffu : (uint32_t)limit, end32 = (uint32_t)data_end;
    uint32_t c32 = (uint32_t)cur;
    for (bool stop = false; !stop;) {
        if (c32 >= lim32) { done = 1; break; }
        if ((unsigned long long)c32 + 4 > (unsigned long long)data_end) break;
        const int sb = (int)(c32 / (uint32_t)SEG_BYTES), sl = sb + lane;
        const bool have = sl < s_end;
        const long long f64 = have ? seg_first[sl] : -1, land64 = have ? seg_land[sl] : -1;
        const int f_l = f64 < 0 ? -1 : (int)(uint32_t)f64;             // (a position is never 0xffffffff: it would lie beyond data_end)
        const int land_l = (int)(uint32_t)land64, cnt_l = have ? seg_count[sl] : 0;
        long long base_l = 0;
        bool visited_l = false;
        for (;;) {
            const int k = __builtin_amdgcn_readfirstlane((int)(c32 / (uint32_t)SEG_BYTES) - sb);
            if (k >= WAVE) break;                        // the next 64 segments
            const uint32_t seg_end = min((uint32_t)(sb + k + 1) * (uint32_t)SEG_BYTES - 1u, end32 - 1u) + 1u;    // (no overflow at 4 GiB)
            uint32_t land = (uint32_t)__builtin_amdgcn_readlane(land_l, k);
            int cnt = __builtin_amdgcn_readlane(cnt_l, k);
            if ((uint32_t)__builtin_amdgcn_readlane(f_l, k) != c32) {           // the guess is not on the chain (or there was none): exact walk
                int err = 0;
                const int s = sb + k;
                const long long l64 = hop(buf, (long long)c32, (long long)seg_end, limit, data_end, &cnt, &err);
                if (err) { error = 1; stop = true; break; }
                land = (uint32_t)l64;
                ++fixups;
                if (lane == 0) { seg_first[s] = (long long)c32; seg_land[s] = l64; seg_count[s] = cnt; }
            }
            if (lane == k) { base_l = total; visited_l = true; }
            total += cnt;
            c32 = land;
            if (c32 >= lim32) { done = 1; stop = true; break; }
            if (c32 < seg_end || (unsigned long long)c32 + 4 > (unsigned long long)data_end) { stop = true; break; }   // stopped inside its segment: an incomplete record starts here
        }
        if (visited_l) { seg_base[sl] = base_l; seg_valid[sl] = 1; }
    }
    cur = (long long)c32;
    if (lane == 0) {
        result[0] = total; result[1] = cur; result[2] = done; result[3] = error; result[4] = fixups; result[5] = first_start;
    }
}

__global__ void k_bam_starts(const uint8_t *__restrict__ buf, int seg0, int n_seg, const long long *__restrict__ seg_first,
                             const int32_t *__restrict__ seg_count, const int32_t *__restrict__ seg_valid,
                             const long long *__restrict__ seg_base, long long *__restrict__ rec_start) {
    const int s = seg0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= seg0 + n_seg || !seg_valid[s]) return;
    long long x = seg_first[s];
    const long long base = seg_base[s];
    const int n = seg_count[s];
    for (int i = 0; i < n; ++i) {
        rec_start[base + i] = x;
        x += 4ll + ld32(buf + x);
    }
}

enum { REC_ERR_SHORT = 1, REC_ERR_FIELDS = 2, REC_ERR_TAG_B = 3, REC_ERR_TAG_TYPE = 4, REC_ERR_TAG_OVERRUN = 5 };

// ---------------------------------------------------------------------------------------------
// K_keep: the record filter (keep_* of the request; KeepRule / keep_record in coral_bam_common.h), between the boundary walk
// and k_bam_meta.  One thread per record in one-wave workgroups (they run beside the inflate launch): the
// three fixed fields decide, keep[i] = 0 / 1 (slot n_rec: the scan's extra 0).  After one exclusive scan, k_bam_keep_compact
// writes the kept starts in order into a second array - not in place: record i's slot may be another thread's source.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_bam_keep(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                   KeepRule K, long long *__restrict__ keep, int32_t *__restrict__ error) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    long long k = 0;
    if (i < n_rec) {
        const uint8_t *r = buf + rec_start[i];
        if (ld32(r) < 32) atomicMax(error, (int)REC_ERR_SHORT);          // (the boundary walk has refused it already)
        else k = keep_record(r[13], ld16(r + 18), ld32(r + 20), K.min_mapq, K.min_seq_length, K.require_flags, K.exclude_flags) ? 1 : 0;
    }
    keep[i] = k;
}

__global__ __launch_bounds__(WAVE) void k_bam_keep_compact(const long long *__restrict__ rec_start, long long n_rec, const long long *__restrict__ keep,
                                                           const long long *__restrict__ keep_off, long long *__restrict__ kept_start) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && keep[i]) kept_start[keep_off[i]] = rec_start[i];
}

// ---------------------------------------------------------------------------------------------
// K_meta: one wave per record
// ---------------------------------------------------------------------------------------------
struct MetaArrays {
    int32_t *tid, *pos, *flag, *mapq, *l_seq, *nm, *n_cigar;       // what the host mirrors need (+ end, qlen from k_bam_emit)
    long long *cig_src, *seq_src, *sa_src;                         // buffer offsets
    long long *pad_ops, *name_len, *sa_len;                        // scan inputs (n + 1 entries, the last one 0)
};

__global__ __launch_bounds__(256) void k_bam_meta(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                   MetaArrays M, int32_t *__restrict__ error) {
    const int lane = threadIdx.x & 63;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (i > n_rec) return;
    if (i == n_rec) {                                               // the extra scan slot
        if (lane == 0) { M.pad_ops[i] = 0; M.name_len[i] = 0; M.sa_len[i] = 0; }
        return;
    }
    const long long x = rec_start[i];
    const uint8_t *r = buf + x;
    const uint32_t block_size = ld32(r);
    const uint8_t *p = r + 4;
    int err = 0;
    int32_t refID = -1, pos = -1, nm = 0;
    uint32_t l_read_name = 0, mapq = 0, n_cigar_op = 0, flag = 0, l_seq = 0;
    long long cig_src = 0, seq_src = 0, sa_src = 0, sa_len = 0;
    if (block_size < 32) {
        err = REC_ERR_SHORT;
    } else {
        refID = (int32_t)ld32(p);
        pos = (int32_t)ld32(p + 4);
        l_read_name = p[8];
        mapq = p[9];
        n_cigar_op = ld16(p + 12);
        flag = ld16(p + 14);
        l_seq = ld32(p + 16);
        const uint8_t *name = p + 32;
        const uint8_t *cig = name + l_read_name;
        const uint8_t *seq = cig + 4ull * n_cigar_op;
        const uint8_t *qual = seq + ((unsigned long long)l_seq + 1) / 2;
        const uint8_t *tags = qual + l_seq;
        const uint8_t *endp = p + block_size;
        if (tags > endp || l_read_name == 0) {
            err = REC_ERR_FIELDS;
        } else {
            const uint8_t *cg = nullptr;
            uint32_t cg_n = 0;
            const uint8_t *t = tags;
            while (t + 3 <= endp) {                                  // wave-uniform walk; Z / H strings are searched 64 bytes per step
                const uint8_t ta = t[0], tb = t[1], ty = t[2];
                const uint8_t *v = t + 3;
                unsigned long long sz = 0;
                if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
                else if (ty == 's' || ty == 'S') sz = 2;
                else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
                else if (ty == 'Z' || ty == 'H') {
                    long long found = -1;
                    for (const uint8_t *q = v; q < endp; q += WAVE) {
                        const uint8_t c = (q + lane < endp) ? q[lane] : (uint8_t)1;
                        const unsigned long long m = __ballot(c == 0);
                        if (m != 0ull) { found = (q - v) + (long long)__builtin_ctzll(m); break; }
                    }
                    sz = found >= 0 ? (unsigned long long)found + 1 : (unsigned long long)(endp - v) + 1;
                } else if (ty == 'B') {
                    if (v + 5 > endp) { err = REC_ERR_TAG_B; break; }
                    const uint8_t sub = v[0];
                    const uint32_t cnt = ld32(v + 1);
                    const unsigned long long es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                    if (ta == 'C' && tb == 'G' && sub == 'I') { cg = v + 5; cg_n = cnt; }
                    sz = 5 + es * cnt;
                } else { err = REC_ERR_TAG_TYPE; break; }
                if (v + sz > endp) { err = REC_ERR_TAG_OVERRUN; break; }
                if (ta == 'N' && tb == 'M') {
                    if (ty == 'c') nm = (int8_t)v[0];
                    else if (ty == 'C') nm = v[0];
                    else if (ty == 's') nm = (int16_t)ld16(v);
                    else if (ty == 'S') nm = (int32_t)ld16(v);
                    else if (ty == 'i' || ty == 'I') nm = (int32_t)ld32(v);
                } else if (ta == 'S' && tb == 'A' && ty == 'Z') {
                    sa_src = v - buf;
                    sa_len = (long long)sz;                          // with the terminating NUL
                }
                t = v + sz;
            }
            const uint8_t *cig_from = cig;
            if (!err && cg && n_cigar_op == 2 && (ld32(cig) & 15u) == 4 && (ld32(cig) >> 4) == l_seq && (ld32(cig + 4) & 15u) == 3) {
                cig_from = cg;                                       // long CIGAR in the CG tag (SAM spec §4.2.2)
                n_cigar_op = cg_n;
            }
            cig_src = cig_from - buf;
            seq_src = seq - buf;
        }
    }
    if (lane == 0) {
        if (err) atomicMax(error, err);
        M.tid[i] = refID; M.pos[i] = pos; M.flag[i] = (int32_t)flag; M.mapq[i] = (int32_t)mapq; M.l_seq[i] = (int32_t)l_seq;
        M.nm[i] = nm; M.n_cigar[i] = err ? 0 : (int32_t)n_cigar_op;
        M.cig_src[i] = cig_src; M.seq_src[i] = seq_src; M.sa_src[i] = sa_src;
        M.pad_ops[i] = err ? 0 : (long long)(((unsigned long long)n_cigar_op + 3ull) & ~3ull);
        M.name_len[i] = err ? 0 : (long long)l_read_name;
        M.sa_len[i] = err ? 0 : sa_len;
    }
}

// ---------------------------------------------------------------------------------------------
// K_emit: one wave per record
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bam_emit(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                   MetaArrays M, const long long *__restrict__ cig_off, const long long *__restrict__ name_off,
                                                   const long long *__restrict__ sa_off, uint32_t *__restrict__ cigar_dst,
                                                   int32_t *__restrict__ end_out, int32_t *__restrict__ qlen_out, uint8_t *__restrict__ names,
                                                   uint8_t *__restrict__ sa_text, int32_t *__restrict__ na_list, int32_t *__restrict__ na_count) {
    const int lane = threadIdx.x & 63;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (i >= n_rec) return;
    const int n = M.n_cigar[i];
    const long long padded = M.pad_ops[i];
    const uint8_t *cig = buf + M.cig_src[i];
    uint32_t *dst = cigar_dst + cig_off[i];
    long long rlen = 0, qinf = 0;
    for (long long k = lane; k < padded; k += WAVE) {
        const uint32_t w = k < n ? ld32(cig + 4 * k) : 15u;
        dst[k] = w;
        const uint32_t op = w & 15u, len = w >> 4;
        rlen += ((0x18Du >> op) & 1u) ? len : 0;                      // M D N = X
        qinf += ((0x1B3u >> op) & 1u) ? len : 0;                      // M I S H = X
    }
    for (int d = 32; d > 0; d >>= 1) {
        rlen += __shfl_xor(rlen, d);
        qinf += __shfl_xor(qinf, d);
    }
    const int32_t flag = M.flag[i], l_seq = M.l_seq[i], pos = M.pos[i];
    if ((flag & 4) || n == 0) rlen = 0;                               // htslib bam_endpos
    if (lane == 0) {
        end_out[i] = pos + (int32_t)(rlen > 0 ? rlen : 1);
        qlen_out[i] = l_seq > 0 ? l_seq : (int32_t)qinf;
    }
    // read name (with its NUL) and SA text (with its NUL)
    {
        const uint8_t *src = buf + rec_start[i] + 36;
        const long long nl = M.name_len[i];
        uint8_t *d = names + name_off[i];
        for (long long k = lane; k < nl; k += WAVE) d[k] = src[k];
        const long long sl = M.sa_len[i];
        if (sl) {
            const uint8_t *s = buf + M.sa_src[i];
            uint8_t *e = sa_text + sa_off[i];
            for (long long k = lane; k < sl; k += WAVE) e[k] = s[k];
        }
    }
    // aligned non-ACGT bases are rare: only FIND the records that have any non-ACGT code (pysam count_coverage counts A/C/G/T)
    if (l_seq > 0 && !(flag & 4) && n > 0) {
        const uint8_t *seq = buf + M.seq_src[i];
        const long long full = l_seq / 2;
        uint32_t bad = 0;
        const long long words = full / 4;
        for (long long k = lane; k < words; k += WAVE) {
            const uint32_t x = ld32(seq + 4 * k);
            const uint32_t lo = x & 0x0f0f0f0fu, hi = (x >> 4) & 0x0f0f0f0fu;
            const uint32_t tl = (lo | 0x10101010u) - 0x01010101u, th = (hi | 0x10101010u) - 0x01010101u;
            bad |= (tl & lo & 0x0f0f0f0fu) | (~tl & 0x10101010u) | (th & hi & 0x0f0f0f0fu) | (~th & 0x10101010u);
        }
        for (long long k = words * 4 + lane; k < full; k += WAVE) {
            const uint32_t h = seq[k] >> 4, l = seq[k] & 15u;
            bad |= (h == 0 || (h & (h - 1))) | (l == 0 || (l & (l - 1)));
        }
        if ((l_seq & 1) && lane == 0) {
            const uint32_t h = seq[full] >> 4;
            bad |= (h == 0 || (h & (h - 1)));
        }
        if (__ballot(bad != 0) != 0ull && lane == 0) na_list[atomicAdd(na_count, 1)] = (int32_t)i;
    }
}

// whole records (the rare ones with non-ACGT bases) -> one contiguous buffer for the host: one wave per record
__global__ __launch_bounds__(256) void k_bam_gather(const uint8_t *__restrict__ buf, const long long *__restrict__ src, const long long *__restrict__ dst,
                                                     const long long *__restrict__ len, int n, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int j = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (j >= n) return;
    const uint8_t *s = buf + src[j];
    uint8_t *d = out + dst[j];
    const long long m = len[j];
    for (long long k = lane; k < m; k += WAVE) d[k] = s[k];
}

// ---------------------------------------------------------------------------------------------
// K_cov: window coverage with a base-quality threshold (the segments of the request), counted while SEQ and QUAL are in HBM
// ---------------------------------------------------------------------------------------------
#define COV_SLICE 16384ll                // query bases per work item: a 1 Mb read is 62 waves' work, not one wave's

struct CovSegs {                         // the request's sorted, disjoint segments (device arrays in the workspace)
    const int32_t *tid, *lo, *hi;
    int n;
};

// first segment at or after (t, pos) in (tid, hi) order, searching [from, n); wave-uniform when its arguments are
__device__ __forceinline__ int cov_first(const CovSegs &S, int32_t t, long long pos, int from) {
    int a = from, b = S.n;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (S.tid[m] < t || (S.tid[m] == t && (long long)S.hi[m] <= pos)) a = m + 1; else b = m;
    }
    return a;
}

// one thread per record: how many work items (COV_SLICE query bases each) the record needs; 0 when it is filtered out, has no
// SEQ, has no QUAL at a threshold above 0, or overlaps no segment.  Slot n_rec gets 0 (the scan's extra entry).
__global__ __launch_bounds__(256) void k_bam_cov_plan(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M,
                                                       const int32_t *__restrict__ end_in, CovSegs S, int threshold, int filter_all,
                                                       long long *__restrict__ n_items) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    long long cnt = 0;
    if (i < n_rec) {
        const int32_t tid = M.tid[i], l_seq = M.l_seq[i], flag = M.flag[i];
        if (tid >= 0 && l_seq > 0 && M.n_cigar[i] > 0 && !(filter_all && (flag & 0x704))) {
            const uint8_t *qual = buf + M.seq_src[i] + ((long long)l_seq + 1) / 2;
            if (threshold == 0 || qual[0] != 0xff) {
                const int32_t pos = M.pos[i];
                // end_in is htslib's bam_endpos: pos + 1 for an unmapped record, whose CIGAR is walked all the same
                const long long end = (flag & 4) ? (1ll << 40) : (long long)end_in[i];
                const int s = cov_first(S, tid, pos, 0);
                if (s < S.n && S.tid[s] == tid && (long long)S.lo[s] < end) cnt = ((long long)l_seq + COV_SLICE - 1) / COV_SLICE;
            }
        }
    }
    n_items[i] = cnt;
}

// the record of work item w: the last i with item_off[i] <= w (item_off: the exclusive sums of n_rec + 1 item counts)
__device__ __forceinline__ long long item_record(const long long *__restrict__ item_off, long long n_rec, long long w) {
    long long a = 0, b = n_rec;
    while (b - a > 1) {
        const long long m = (a + b) >> 1;
        if (item_off[m] <= w) a = m; else b = m;
    }
    return a;
}

// The CIGAR walk of one work item, the query bases [q_lo, q_hi) of record i, for both coverage kernels: the coverage rule
// (CovTable in coral_bam_common.h) is applied here and nowhere else on the device.  The wave walks the CIGAR 64 ops at a time
// (prefix sums of the query / reference advance), and for every aligned op that meets the query range the lanes stride over the
// op's bases inside each segment, testing the SEQ code and QUAL.  What becomes of a counted base is the sink's business:
//   segment(t, lo)   wave-uniform, in front of the bases of an op inside segment t (lo = S.lo[t]); segments are met in
//                    increasing order, the same one again for every further op inside it
//   base(x, col)     per lane: the base at reference position x counts, col = 0..3 for A, C, G, T
template <class Segment, class Base>
__device__ __forceinline__ void cov_walk(const uint8_t *__restrict__ buf, const MetaArrays &M, const CovSegs &S, uint32_t thr, long long i,
                                         long long q_lo, long long q_hi, int lane, Segment segment, Base base) {
    const int32_t tid = M.tid[i], l_seq = M.l_seq[i], pos = M.pos[i];
    const int n_ops = M.n_cigar[i];
    const uint8_t *ops = buf + M.cig_src[i];
    const uint8_t *seq = buf + M.seq_src[i];
    const uint8_t *qual = seq + ((long long)l_seq + 1) / 2;
    int s = cov_first(S, tid, pos, 0);
    long long q_base = 0, r_base = pos;
    for (int c = 0; c < n_ops && q_base < q_hi; c += WAVE) {
        if (s >= S.n || S.tid[s] != tid) break;                   // no segment left on this contig
        const int kk = c + lane;
        const uint32_t wd = kk < n_ops ? ld32(ops + 4ll * kk) : 15u;
        const uint32_t op = wd & 15u;
        const long long len = (long long)(wd >> 4);
        const long long qa = ((0x193u >> op) & 1u) ? len : 0;     // M I S = X advance the query
        const long long ra = ((0x18Du >> op) & 1u) ? len : 0;     // M D N = X advance the reference
        long long qs = qa, rs = ra;
        for (int d = 1; d < WAVE; d <<= 1) {
            const long long tq = __shfl_up(qs, d), tr = __shfl_up(rs, d);
            if (lane >= d) { qs += tq; rs += tr; }
        }
        const long long q_op = q_base + qs - qa, r_op = r_base + rs - ra;
        const bool cand = ((0x181u >> op) & 1u) && len > 0 && q_op < q_hi && q_op + len > q_lo;     // M = X meeting the item
        unsigned long long m = __ballot(cand);
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const long long oq = __shfl(q_op, j), orf = __shfl(r_op, j), ol = __shfl(len, j);
            const long long aq = max(oq, q_lo), bq = min(oq + ol, q_hi);
            const long long r0 = orf + (aq - oq), r1 = orf + (bq - oq);
            // r0 only grows: the cursor is usually still right (this op ends inside its segment) or one further
            if (s < S.n && S.tid[s] == tid && (long long)S.hi[s] <= r0)
                s = (s + 1 < S.n && S.tid[s + 1] == tid && (long long)S.hi[s + 1] > r0) ? s + 1 : cov_first(S, tid, r0, s + 1);
            for (int t = s; t < S.n && S.tid[t] == tid && (long long)S.lo[t] < r1; ++t) {
                const long long lo = S.lo[t], xa = max(r0, lo), xb = min(r1, (long long)S.hi[t]);
                segment(t, lo);
                for (long long x = xa + lane; x < xb; x += WAVE) {
                    const long long qi = aq + (x - r0);                    // < bq <= q_hi <= l_seq
                    const uint8_t byte = seq[qi >> 1];
                    const uint32_t code = (qi & 1) ? (byte & 15u) : (uint32_t)(byte >> 4);
                    uint32_t col;
                    if (pileup_base(code, &col) && qual[qi] >= thr) base(x, col);
                }
            }
        }
        q_base += __shfl(qs, WAVE - 1);
        r_base += __shfl(rs, WAVE - 1);
    }
}

// one wave per work item (grid-stride): the query bases [k * COV_SLICE, (k + 1) * COV_SLICE) of record i.  The counting sink:
// per-lane counts, reduced in the wave and added with ONE 64-bit atomic per (work item, segment).
__global__ __launch_bounds__(256) void k_bam_cov_count(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M, CovSegs S,
                                                        int threshold, const long long *__restrict__ item_off,
                                                        unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long total = item_off[n_rec];
    for (long long w = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < total; w += n_waves) {
        const long long i = item_record(item_off, n_rec, w);
        const long long q_lo = (w - item_off[i]) * COV_SLICE, q_hi = min((long long)M.l_seq[i], q_lo + COV_SLICE);
        int cur = -1;                                                  // the segment the lanes' counts belong to
        uint32_t acc = 0;
        auto flush = [&]() {
            long long sum = (long long)acc;
            for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
            if (cur >= 0 && lane == 0 && sum) atomicAdd(counts + cur, (unsigned long long)sum);
            acc = 0;
        };
        cov_walk(buf, M, S, (uint32_t)threshold, i, q_lo, q_hi, lane, [&](int t, long long) { if (t != cur) { flush(); cur = t; } },
                 [&](long long, uint32_t) { ++acc; });
        flush();
    }
}

// K_pileup (per_base of the request): k_bam_cov_count's work items and walk with the table sink: every counted base is one
// no-return 32-bit atomic at table[(seg_off[t] + x - lo[t]) * 4 + col].  There is nothing to reduce: the 64 lanes of a stride are
// 64 different positions, so a wave never collides with itself - only different records at the same position do.  One wave per
// workgroup (grid-stride), no LDS: it fits beside resident inflate waves.
__global__ __launch_bounds__(WAVE) void k_bam_pileup(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M, CovSegs S,
                                                     const long long *__restrict__ seg_off, int threshold,
                                                     const long long *__restrict__ item_off, uint32_t *__restrict__ table) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const long long q_lo = (w - item_off[i]) * COV_SLICE, q_hi = min((long long)M.l_seq[i], q_lo + COV_SLICE);
        long long row0 = 0;                                            // lo <= x < hi: 4 * x + row0 lies in the segment's rows
        cov_walk(buf, M, S, (uint32_t)threshold, i, q_lo, q_hi, lane, [&](int t, long long lo) { row0 = 4 * (seg_off[t] - lo); },
                 [&](long long x, uint32_t col) { atomicAdd(table + (row0 + 4 * x + col), 1u); });
    }
}

// ---------------------------------------------------------------------------------------------
// K_qc: per-read base-quality sums and the base-quality histogram (want_qc; the rules: QcPartial in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
#define QC_SLICE 16384ll                 // QUAL bytes per work item (as COV_SLICE: a 1 Mb read is 62 waves' work)
#ifndef QC_COPIES
#define QC_COPIES 4                      // copies of the 256-bin table per wave, interleaved: 4 KiB of LDS (a -DQC_COPIES=1 build is
#endif                                   // the single table to measure it against)

// One thread per record (one-wave workgroups): qual_sum[i] = 0 for a read with quality (k_bam_qc adds to it), -1 otherwise, and
// the number of work items its QUAL is cut into.  Slot n_rec gets 0 items (the scan's extra entry).
__global__ __launch_bounds__(WAVE) void k_bam_qc_plan(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                      MetaArrays M, long long *__restrict__ qual_sum, long long *__restrict__ n_items) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    long long cnt = 0;
    if (i < n_rec) {
        const uint32_t l_seq = (uint32_t)M.l_seq[i];
        bool counted = false;
        if (qc_is_read((uint32_t)M.flag[i], l_seq)) {
            const uint8_t *r = buf + rec_start[i];
            counted = qc_has_quality(r[qc_qual_offset(r[12], ld16(r + 16), l_seq)]);
        }
        if (counted) cnt = ((long long)l_seq + QC_SLICE - 1) / QC_SLICE;
        qual_sum[i] = counted ? 0 : -1;
    }
    n_items[i] = cnt;
}

// One wave per work item (one-wave workgroups, grid-stride): QUAL bytes [k * QC_SLICE, (k + 1) * QC_SLICE) of record i.
// QUAL begins at any byte address: the wave reads the 16-byte aligned chunks that cover its bytes, lane l the chunks l, l + 64,
// ... - one load instruction of the wave is 1 KiB of consecutive memory, every cache line is fetched once - and the bytes of the
// first and the last chunk that are not the item's are masked out.  Sum: v_sad_u8 per dword, reduced in the wave, ONE 64-bit
// atomic per item.  Histogram: COPIES copies of the 256 bins in LDS, interleaved (bin v of copy c at word v * COPIES + c, lane l
// uses copy l % COPIES): real QUAL sits on a few values, and lanes that add to the same word are serialised - with the copies
// side by side, lanes with the same value spread over COPIES words in COPIES different banks.  The workgroup adds its table to the
// device histogram once, at its end, with 64-bit atomics.  4 KiB of LDS (COPIES = 4): fits beside the inflate launch's 27 x 5.75 KiB
// of a CU's 160 KiB, as k_bgzf_crc's tables do.
__global__ __launch_bounds__(WAVE) void k_bam_qc(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                 MetaArrays M, const long long *__restrict__ item_off,
                                                 unsigned long long *__restrict__ qual_sum, unsigned long long *__restrict__ hist) {
    constexpr int COPIES = QC_COPIES;
    // (a 32-bit bin cannot overflow: the grid-stride loop gives a workgroup at most ceil(items / 2 048) work items of 16 KiB, and
    // CARRY_CAP + a batch stay below 4 GiB - under 2^21 bytes per workgroup and launch)
    __shared__ uint32_t H[256 * COPIES];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256 * COPIES; k += WAVE) H[k] = 0;
    __syncthreads();
    uint32_t *mine = H + (lane % COPIES);
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const uint32_t l_seq = (uint32_t)M.l_seq[i];
        const uint8_t *r = buf + rec_start[i];
        const long long q_lo = (w - item_off[i]) * QC_SLICE, q_hi = min((long long)l_seq, q_lo + QC_SLICE);
        const uint8_t *p = r + qc_qual_offset(r[12], ld16(r + 16), l_seq) + q_lo;
        const int n = (int)(q_hi - q_lo);                             // 1 .. QC_SLICE
        const int head = (int)((uintptr_t)p & 15u);
        const uint4 *chunks = reinterpret_cast<const uint4 *>(p - head);       // (inside the batch buffer: a record starts >= 36 bytes in front of its QUAL)
        const int n_chunks = (head + n + 15) >> 4;
        uint32_t acc = 0;
        for (int c = lane; c < n_chunks; c += WAVE) {
            const uint4 v = chunks[c];
            const uint32_t word[4] = {v.x, v.y, v.z, v.w};
            const int first = c * 16 - head;                          // item-relative index of the chunk's byte 0
            if (first >= 0 && first + 16 <= n) {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const uint32_t x = word[d];
                    acc = __builtin_amdgcn_sad_u8(x, 0u, acc);
                    atomicAdd(mine + (x & 0xffu) * COPIES, 1u);
                    atomicAdd(mine + ((x >> 8) & 0xffu) * COPIES, 1u);
                    atomicAdd(mine + ((x >> 16) & 0xffu) * COPIES, 1u);
                    atomicAdd(mine + (x >> 24) * COPIES, 1u);
                }
            } else {                                                  // the item's first or last chunk: byte by byte
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t q = (word[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    if (first + j >= 0 && first + j < n) {
                        acc += q;
                        atomicAdd(mine + q * COPIES, 1u);
                    }
                }
            }
        }
        unsigned long long sum = acc;
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) atomicAdd(qual_sum + i, sum);
    }
    __syncthreads();
    for (int v = lane; v < 256; v += WAVE) {
        unsigned long long t = 0;
#pragma unroll
        for (int c = 0; c < COPIES; ++c) t += H[v * COPIES + c];
        if (t) atomicAdd(hist + v, t);
    }
}

// ---------------------------------------------------------------------------------------------
// K_reads: the selected records as FASTQ text (want_reads; the rules: ReadsRule and reads_* in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
struct ReadsDev {                        // the request's device arrays, carved from the caller's workspace
    const int32_t *tid, *lo, *hi;        // the segments (n_seg = 0: no region limit)
    const uint8_t *names;                // the sorted names as one blob and n_names + 1 offsets (n_names = 0: no name limit)
    const int64_t *name_off;
    int n_seg;
    long long n_names;
    uint32_t exclude_flags;
    int mode;                            // READS_AS_FASTQ or READS_AS_RECORDS
};

// One thread per record (one-wave workgroups: they run beside the inflate launch): the rule, from the fixed
// fields k_bam_meta left, the end position k_bam_emit left and the name behind the record's fixed fields.  out_len[i] = bytes of
// the record's text, n_items[i] = its work items of READS_SLICE bases; both 0 when the record is not written, and in slot n_rec
// (the scans' extra entry).  In mode READS_AS_RECORDS a record without SEQ takes part too, out_len[i] is the record's own size,
// 4 + block_size, and its work items are slices of READS_COPY_SLICE of those bytes.
__global__ __launch_bounds__(WAVE) void k_bam_reads_plan(const uint8_t *__restrict__ buf, const long long *__restrict__ rec_start, long long n_rec,
                                                         MetaArrays M, const int32_t *__restrict__ end_in, ReadsDev X,
                                                         long long *__restrict__ out_len, long long *__restrict__ n_items) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rec) return;
    long long bytes = 0, items = 0;
    if (i < n_rec) {
        const uint32_t l_seq = (uint32_t)M.l_seq[i];
        const uint8_t *r = buf + rec_start[i];
        const uint32_t l_read_name = r[12];
        bool w = l_read_name > 0 && reads_takes_part((uint32_t)M.flag[i], l_seq, X.exclude_flags, X.mode);
        if (w && X.n_seg > 0) w = reads_meets_segment(X.tid, X.lo, X.hi, X.n_seg, M.tid[i], M.pos[i], end_in[i]);
        if (w && X.n_names > 0) w = reads_name_listed(X.names, X.name_off, X.n_names, r + 36, l_read_name - 1u);
        if (w && X.mode == READS_AS_RECORDS) {
            bytes = reads_record_bytes(ld32(r));
            items = (bytes + READS_COPY_SLICE - 1) / READS_COPY_SLICE;
        } else if (w) {
            bytes = reads_text_bytes(l_seq, l_read_name);
            items = ((long long)l_seq + READS_SLICE - 1) / READS_SLICE;
        }
    }
    out_len[i] = bytes;
    n_items[i] = items;
}

// The 16 bytes buf[p .. p + 16) for any p, from the two aligned 16-byte chunks that cover them (the second one is the first one
// of the lane that makes the next 16 characters: the same or the next cache line, served by the L1).  A chunk that does not lie
// inside [0, buf_bytes) reads as zeros: only the windows of an item's edge chunks reach outside the record, with bytes that are
// not used.
__device__ __forceinline__ uint4 reads_window(const uint8_t *__restrict__ buf, long long p, long long buf_bytes) {
    const long long base = p & ~15ll;
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
    if (base >= 0 && base + 16 <= buf_bytes) lo = *reinterpret_cast<const uint4 *>(buf + base);
    if (base + 16 >= 0 && base + 32 <= buf_bytes) hi = *reinterpret_cast<const uint4 *>(buf + base + 16);
    const uint32_t sh = (uint32_t)(p & 15);
    uint32_t d0 = lo.x, d1 = lo.y, d2 = lo.z, d3 = lo.w, d4 = hi.x, d5 = hi.y, d6 = hi.z, d7 = hi.w;
    if (sh & 8u) { d0 = d2; d1 = d3; d2 = d4; d3 = d5; d4 = d6; d5 = d7; }
    if (sh & 4u) { d0 = d1; d1 = d2; d2 = d3; d3 = d4; d4 = d5; }
    const uint32_t bs = (sh & 3u) * 8u;
    return make_uint4(__builtin_amdgcn_alignbit(d1, d0, bs), __builtin_amdgcn_alignbit(d2, d1, bs), __builtin_amdgcn_alignbit(d3, d2, bs),
                      __builtin_amdgcn_alignbit(d4, d3, bs));
}

__device__ __forceinline__ uint4 reads_mirror(uint4 v) {      // the 16 bytes in reverse order
    return make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
}

// 16 characters of SEQ.  Forward: of the bases s0 .. s0 + 15, in that order; reverse: of the same bases from s0 + 15 down to s0,
// complemented.  The nine bytes that hold the bases are read as one big-endian number N whose nibble k (from the top) is base
// s0 + k - shifted by one nibble when s0 is odd -, so that character t is the table entry of nibble t (forward) or 15 - t
// (reverse): mirroring the indices is all a reverse-strand record costs.  s0 may be negative or reach behind l_seq in an item's
// edge chunks; those characters are not stored.
template <bool REV>
__device__ __forceinline__ uint4 reads_seq_chunk(const uint8_t *__restrict__ buf, long long seq_at, long long s0, long long buf_bytes) {
    constexpr unsigned long long T_LO = reads_char_table(0, REV), T_HI = reads_char_table(1, REV);
    const uint4 v = reads_window(buf, seq_at + (s0 >> 1), buf_bytes);
    unsigned long long N = ((unsigned long long)__builtin_bswap32(v.x) << 32) | __builtin_bswap32(v.y);
    if (s0 & 1) N = (N << 4) | ((v.z & 0xffu) >> 4);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t code = (uint32_t)(N >> (REV ? 4 * t : 60 - 4 * t)) & 15u;
        const uint32_t c = (uint32_t)(((code & 8u) ? T_HI : T_LO) >> ((code & 7u) * 8u)) & 0xffu;
        w[t >> 2] |= c << (8 * (t & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t reads_qual_word(uint32_t x) {      // min(q, 93) + 33 on each of the four bytes
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= (uint32_t)reads_qual_char((x >> (8 * k)) & 0xffu) << (8 * k);
    return r;
}

// One run of an item's output: the characters [a, b) of a field (SEQ or QUAL) whose character 0 lies at out[origin].  Lane l takes
// the 16-byte aligned chunks l, l + 64, ... of the output that the run touches: one store instruction of the wave is 1 KiB of
// consecutive memory.  A chunk that lies inside the run is ONE aligned 16-byte store; the run's first and last chunk, which it may
// share with a neighbouring item or field, are stored byte by byte, only the run's own bytes.  make(j0) gives the characters
// j0 .. j0 + 15 of the field.
template <class Make>
__device__ __forceinline__ void reads_run(uint8_t *__restrict__ out, long long origin, long long a, long long b, int lane, Make make) {
    const long long c0 = (origin + a) >> 4, c1 = (origin + b - 1) >> 4;
    for (long long c = c0 + lane; c <= c1; c += WAVE) {
        const long long j0 = 16 * c - origin;
        const uint4 v = make(j0);
        if (j0 >= a && j0 + 16 <= b) {
            *reinterpret_cast<uint4 *>(out + 16 * c) = v;
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (j0 + t >= a && j0 + t < b) out[16 * c + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
        }
    }
}

// One wave per work item (one-wave workgroups, grid-stride, no LDS): the bases [k * READS_SLICE, (k + 1) * READS_SLICE) of a
// written record - their SEQ characters and their QUAL characters, two runs of the record's text at out_off[i].  Item 0 also
// writes what is not a base: `@`, the name, and the three line ends.  With flag 0x10 character j of either field comes from base
// l_seq - 1 - j: the source window of a chunk is the mirrored one, read once - no second pass.  Every output byte has exactly
// one writer (the items of a record split [0, l_seq), the records split the text): no atomics.
__global__ __launch_bounds__(WAVE) void k_bam_reads_emit(const uint8_t *__restrict__ buf, long long buf_bytes, const long long *__restrict__ rec_start,
                                                         long long n_rec, MetaArrays M, const long long *__restrict__ item_off,
                                                         const long long *__restrict__ out_off, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const long long l_seq = (long long)(uint32_t)M.l_seq[i];
        const long long rs = rec_start[i];
        const uint8_t *r = buf + rs;
        const long long l_read_name = r[12];
        const bool rev = (ld16(r + 18) & 0x10u) != 0;
        const long long seq_at = M.seq_src[i], qual_at = seq_at + (l_seq + 1) / 2;
        const bool has_qual = buf[qual_at] != 0xff;
        const long long at = out_off[i];
        const long long seq_origin = at + l_read_name + 1, qual_origin = seq_origin + l_seq + 3;
        const long long k = w - item_off[i], a = k * READS_SLICE, b = min(l_seq, a + READS_SLICE);
        if (k == 0) {
            uint8_t *o = out + at;
            for (long long j = lane; j < l_read_name - 1; j += WAVE) o[1 + j] = r[36 + j];
            if (lane == 0) {
                o[0] = '@';
                o[l_read_name] = '\n';
                out[seq_origin + l_seq] = '\n'; out[seq_origin + l_seq + 1] = '+'; out[seq_origin + l_seq + 2] = '\n';
                out[qual_origin + l_seq] = '\n';
            }
        }
        if (rev) reads_run(out, seq_origin, a, b, lane, [&](long long j0) { return reads_seq_chunk<true>(buf, seq_at, l_seq - 16 - j0, buf_bytes); });
        else reads_run(out, seq_origin, a, b, lane, [&](long long j0) { return reads_seq_chunk<false>(buf, seq_at, j0, buf_bytes); });
        reads_run(out, qual_origin, a, b, lane, [&](long long j0) {
            if (!has_qual) return make_uint4(0x22222222u, 0x22222222u, 0x22222222u, 0x22222222u);
            uint4 v = reads_window(buf, qual_at + (rev ? l_seq - 16 - j0 : j0), buf_bytes);
            if (rev) v = reads_mirror(v);
            return make_uint4(reads_qual_word(v.x), reads_qual_word(v.y), reads_qual_word(v.z), reads_qual_word(v.w));
        });
    }
}

// One wave per work item (one-wave workgroups, grid-stride, no LDS), mode READS_AS_RECORDS: the bytes [k * READS_COPY_SLICE,
// (k + 1) * READS_COPY_SLICE) of a written record - block_size word first - go from buf + rec_start[i] to out + out_off[i] as
// they stand.  Source and destination have byte alignments of their own: a lane takes an aligned 16-byte chunk of the OUTPUT,
// filled from the two aligned source chunks that cover it (reads_window) and stored as one uint4; the item's first and last
// chunk, which it may share with the neighbouring item or record, are stored byte by byte, only the item's own bytes
// (reads_run).  Every output byte has exactly one writer (the items split the record, the records split the output): no atomics.
__global__ __launch_bounds__(WAVE) void k_bam_reads_copy(const uint8_t *__restrict__ buf, long long buf_bytes, const long long *__restrict__ rec_start,
                                                         long long n_rec, const long long *__restrict__ item_off,
                                                         const long long *__restrict__ out_off, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long i = item_record(item_off, n_rec, w);
        const long long rs = rec_start[i], at = out_off[i], bytes = out_off[i + 1] - at;
        const long long a = (w - item_off[i]) * READS_COPY_SLICE, b = min(bytes, a + READS_COPY_SLICE);
        reads_run(out, at, a, b, lane, [&](long long j0) { return reads_window(buf, rs + j0, buf_bytes); });
    }
}

// Coordinate order (reads_order = 1 of a records request): between the plan and the scans the batch's records are sorted by
// reads_sort_key - hipcub's radix sort of (key, ordinal), stable, so records with equal keys keep their file order - and
// everything behind works on sorted positions: position j holds record ord[j].  All three kernels are one-wave workgroups
// (DESIGN.md §10 (vi)).
// One thread per record: its key from the fixed fields k_bam_meta left, and its ordinal.
__global__ __launch_bounds__(WAVE) void k_bam_sort_keys(long long n_rec, MetaArrays M, unsigned long long *__restrict__ key, uint32_t *__restrict__ ord) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    key[i] = reads_sort_key(M.tid[i], M.pos[i], (uint32_t)M.flag[i]);
    ord[i] = (uint32_t)i;
}

// One thread per sorted position: the plan's out_len / n_items of the record that sorts there (0 for a record that is not
// written, wherever it sorts); slot n_rec, the scans' extra entry, is 0.
__global__ __launch_bounds__(WAVE) void k_bam_sort_permute(long long n_rec, const uint32_t *__restrict__ ord, const long long *__restrict__ out_len,
                                                           const long long *__restrict__ n_items, long long *__restrict__ sorted_len,
                                                           long long *__restrict__ sorted_items) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_rec) return;
    const long long i = j < n_rec ? (long long)ord[j] : n_rec;
    sorted_len[j] = j < n_rec ? out_len[i] : 0;
    sorted_items[j] = j < n_rec ? n_items[i] : 0;
}

// k_bam_reads_copy for sorted positions (same launch shape, same work items of READS_COPY_SLICE bytes): item_off / out_off are
// the scans over the PERMUTED arrays, so work item w belongs to sorted position j, whose bytes come from record ord[j].  Every
// output byte still has exactly one writer (the items split the record, the sorted positions split the output): no atomics.
__global__ __launch_bounds__(WAVE) void k_bam_reads_copy_sorted(const uint8_t *__restrict__ buf, long long buf_bytes, const long long *__restrict__ rec_start,
                                                                long long n_rec, const uint32_t *__restrict__ ord,
                                                                const long long *__restrict__ item_off, const long long *__restrict__ out_off,
                                                                uint8_t *__restrict__ out) {
    const int lane = threadIdx.x;
    const long long total = item_off[n_rec];
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long j = item_record(item_off, n_rec, w);
        const long long rs = rec_start[ord[j]], at = out_off[j], bytes = out_off[j + 1] - at;
        const long long a = (w - item_off[j]) * READS_COPY_SLICE, b = min(bytes, a + READS_COPY_SLICE);
        reads_run(out, at, a, b, lane, [&](long long j0) { return reads_window(buf, rs + j0, buf_bytes); });
    }
}

// ---------------------------------------------------------------------------------------------
// K_index: what a batch contributes to the BAI index of the file (want_index; IndexPartial in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
struct IndexDev {                        // device arrays of the request, carved from the caller's workspace
    unsigned long long *lin;             // linear index: smallest virtual offset per (contig, 16 384-base window), ~0 = none
    long long *lin_off;                  // n_ref + 1: first window of every contig
    unsigned long long *n_mapped, *n_unmapped, *n_no_coor;      // n_ref, n_ref, 1 counters
    unsigned long long *state;           // [2]: virtual offset of the position a batch ends at (read by the next batch: the
                                         // start of the record it carries in), alternating
    int32_t *unsorted;                   // set when a record sorts in front of its predecessor
    int n_ref;
};

// virtual offset of byte `rel` of the batch's inflated bytes: the block that holds it (the last one that starts at or in front
// of it: an empty block starts where its successor does); behind the batch's last byte the block that follows it (bgzf_tell)
__device__ __forceinline__ unsigned long long batch_voffset(const BlockDesc *__restrict__ desc, const uint32_t *__restrict__ boff, int n_blocks,
                                                            unsigned long long file_off, unsigned long long comp_bytes, long long rel,
                                                            long long infl_bytes) {
    if (rel < infl_bytes) {
        int a = 0, b = n_blocks;                                   // the last block with dst_off <= rel
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if ((long long)desc[m].dst_off <= rel) a = m; else b = m;
        }
        return ((file_off + boff[a]) << 16) | (unsigned long long)(rel - (long long)desc[a].dst_off);
    }
    int a = 0, b = n_blocks;                                       // the first block with dst_off >= rel
    while (a < b) {
        const int m = (a + b) >> 1;
        if ((long long)desc[m].dst_off < rel) a = m + 1; else b = m;
    }
    return (a < n_blocks ? file_off + boff[a] : file_off + comp_bytes) << 16;
}

__device__ __forceinline__ long long index_key(int32_t tid, int32_t pos, int32_t end, int n_ref, long long *beg_out, long long *end_out) {
    if (tid < 0 || tid >= n_ref) return -1;
    const long long b = pos < 0 ? 0 : pos, e = (long long)end > b ? (long long)end : b + 1, l = e - 1;
    *beg_out = b;
    *end_out = e;
    int bin = 0;
    if (b >> 14 == l >> 14) bin = (int)(4681 + (b >> 14));
    else if (b >> 17 == l >> 17) bin = (int)(585 + (b >> 17));
    else if (b >> 20 == l >> 20) bin = (int)(73 + (b >> 20));
    else if (b >> 23 == l >> 23) bin = (int)(9 + (b >> 23));
    else if (b >> 26 == l >> 26) bin = (int)(1 + (b >> 26));
    return (long long)tid * 65536 + bin;
}

__device__ __forceinline__ unsigned long long index_sort_word(int32_t tid, int32_t pos) {
    return tid < 0 ? ~0ull : ((unsigned long long)(uint32_t)tid << 32) | (uint32_t)(pos < 0 ? 0 : pos);
}

// One thread per record (one-wave workgroups: the kernel runs beside the next batch's inflate), thread n_rec for the batch's end.
// Record i: virtual offset of its first byte (a record carried in from the previous batch: where it STARTED, state[parity]),
// key = tid * 65536 + bin, head[i] = 1 when the key differs from its predecessor's (record 0 always: the host joins a run that
// goes on across batches), 64-bit atomicMin into every linear-index window it overlaps, the per-contig counters (one atomic per
// wave when the wave's records are on one contig), and the order check against its predecessor.
__global__ __launch_bounds__(WAVE) void k_bam_index(const long long *__restrict__ rec_start, long long n_rec, MetaArrays M,
                                                    const int32_t *__restrict__ end_in, const BlockDesc *__restrict__ desc,
                                                    const uint32_t *__restrict__ boff, int n_blocks, unsigned long long file_off,
                                                    unsigned long long comp_bytes, long long infl_bytes, long long carry_pos, int parity,
                                                    IndexDev X, unsigned long long *__restrict__ voff_out, long long *__restrict__ key_out,
                                                    long long *__restrict__ head_out) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == n_rec) {
        head_out[i] = 0;                                               // the scan's extra slot
        // where the batch ends: the start of the record that is carried into the next batch (or still the one carried into this
        // one: a record may span several batches), or the place just behind the batch's last record
        X.state[parity ^ 1] = carry_pos < CARRY_CAP ? X.state[parity]
                                                    : batch_voffset(desc, boff, n_blocks, file_off, comp_bytes, carry_pos - CARRY_CAP, infl_bytes);
    }
    const bool valid = i < n_rec;
    int32_t tid = -1, flag = 0;
    if (valid) {
        const long long x = rec_start[i];
        const unsigned long long voff = x < CARRY_CAP ? X.state[parity]
                                                      : batch_voffset(desc, boff, n_blocks, file_off, comp_bytes, x - CARRY_CAP, infl_bytes);
        tid = M.tid[i];
        flag = M.flag[i];
        const int32_t pos = M.pos[i];
        long long b = 0, e = 0;
        const long long key = index_key(tid, pos, end_in[i], X.n_ref, &b, &e);
        bool head = true;
        if (i > 0) {
            long long pb, pe;
            const int32_t ptid = M.tid[i - 1], ppos = M.pos[i - 1];
            head = index_key(ptid, ppos, end_in[i - 1], X.n_ref, &pb, &pe) != key;
            if (index_sort_word(tid, pos) < index_sort_word(ptid, ppos)) *X.unsorted = 1;
        }
        voff_out[i] = voff;
        key_out[i] = key;
        head_out[i] = head ? 1 : 0;
        if (key >= 0) {
            const long long w_first = X.lin_off[tid], nw = X.lin_off[tid + 1] - w_first;
            const long long w0 = min(b >> 14, nw - 1), w1 = min((e - 1) >> 14, nw - 1);
            for (long long w = w0; w <= w1; ++w) atomicMin(X.lin + w_first + w, voff);
        } else {
            tid = -1;
        }
    }
    // counters
    const unsigned long long act = __ballot(valid);
    if (act == 0ull) return;
    const int32_t t0 = __shfl(tid, (int)__builtin_ctzll(act));
    if (__ballot(valid && tid != t0) == 0ull) {
        const unsigned long long unm = __ballot(valid && (flag & 4));
        if (lane == (int)__builtin_ctzll(act)) {
            if (t0 < 0) atomicAdd(X.n_no_coor, (unsigned long long)__popcll(act));
            else {
                if (act & ~unm) atomicAdd(X.n_mapped + t0, (unsigned long long)__popcll(act & ~unm));
                if (unm) atomicAdd(X.n_unmapped + t0, (unsigned long long)__popcll(unm));
            }
        }
    } else if (valid) {
        atomicAdd(tid < 0 ? X.n_no_coor : (flag & 4) ? X.n_unmapped + tid : X.n_mapped + tid, 1ull);
    }
}

// the heads, compacted in file order: head_off = exclusive prefix sum of head
__global__ __launch_bounds__(WAVE) void k_bam_index_compact(long long n_rec, const long long *__restrict__ head, const long long *__restrict__ head_off,
                                                            const unsigned long long *__restrict__ voff, const long long *__restrict__ key,
                                                            unsigned long long *__restrict__ voff_out, long long *__restrict__ key_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec || !head[i]) return;
    voff_out[head_off[i]] = voff[i];
    key_out[head_off[i]] = key[i];
}

// ---------------------------------------------------------------------------------------------
// K_depth: whole-genome binned read depth (depth_bin of the request; the rules: DepthPartial in coral_bam_common.h)
// ---------------------------------------------------------------------------------------------
struct DepthDev {                        // device arrays of the request, carved from the caller's workspace
    long long *bin_off;                  // n_ref + 1: first bin of every contig
    int32_t *len;                        // n_ref: LN (>= 0)
    unsigned long long *bases, *reads;   // n_bins each
    int n_ref;
    uint32_t bin, min_mapq, exclude_flags;
    int count_deletions;
};

// `key` does not decrease from lane to lane: the sum of `v` over every run of equal keys, in the run's first lane (a segmented
// suffix sum by doubling; the other lanes of a run hold partial sums).
__device__ __forceinline__ uint32_t depth_run_sum(uint32_t key, uint32_t v, int lane) {
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t tv = __shfl_down(v, d), tk = __shfl_down(key, d);
        if (lane + d < WAVE && tk == key) v += tv;
    }
    return v;
}

// One wave per record (grid-stride), one-wave workgroups without LDS: it fits beside resident inflate waves.
// Only the fixed fields and the real CIGAR (M.cig_src / M.n_cigar: the CG tag is resolved) are read.  The wave takes 64 ops at a
// time; the wave prefix sum of the reference advance gives every lane its op's interval [a, e), clipped to the contig - so no bin
// at or behind ceil(LN / bin) is ever addressed.  Ops come in increasing reference order, hence the lanes' bins do not decrease:
//   first bin   every lane adds the part of its op inside the op's first bin b0; lanes with the same b0 are summed in the wave
//               (an op that is not counted joins the run with 0) and the run's first lane issues ONE no-return 64-bit atomic;
//   last bin    the same for the part inside the op's last bin b1, for the ops that cross a bin edge (rare unless bin is small);
//   in between  the whole bins b0 + 1 .. b1 - 1 of such an op get `bin` each, 64 bins per step of the wave.
// A run's sum fits 32 bits: the positions one record covers are disjoint, so a bin gets at most `bin` from it.
// Atomics per record: the bins it touches (at most twice each) plus its 64-op chunks - not its ops.
__global__ __launch_bounds__(WAVE) void k_bam_depth(const uint8_t *__restrict__ buf, long long n_rec, MetaArrays M, DepthDev X) {
    const int lane = threadIdx.x;
    const uint32_t bin = X.bin;
    for (long long i = blockIdx.x; i < n_rec; i += gridDim.x) {
        const int32_t tid = M.tid[i], pos = M.pos[i];
        const int n_ops = M.n_cigar[i];
        if (!depth_takes_part(tid, pos, (uint32_t)n_ops, (uint32_t)M.flag[i], (uint32_t)M.mapq[i], X.n_ref, X.exclude_flags, X.min_mapq)) continue;
        const long long ln = X.len[tid];
        if (pos >= ln) continue;                                       // (so ln >= 1 below)
        const long long bo = X.bin_off[tid];
        unsigned long long *bases = X.bases + bo;
        if (lane == 0) atomicAdd(X.reads + bo + (uint32_t)pos / bin, 1ull);
        const uint8_t *ops = buf + M.cig_src[i];
        long long r_base = pos;
        for (int c = 0; c < n_ops && r_base < ln; c += WAVE) {
            const int kk = c + lane;
            const uint32_t wd = kk < n_ops ? ld32(ops + 4ll * kk) : 15u;
            const uint32_t op = wd & 15u;
            const long long len = (long long)(wd >> 4);
            const long long ra = ((0x18Du >> op) & 1u) ? len : 0;     // M D N = X advance the reference
            long long rs = ra;
            for (int d = 1; d < WAVE; d <<= 1) {
                const long long t = __shfl_up(rs, d);
                if (lane >= d) rs += t;
            }
            const uint32_t a = (uint32_t)min(r_base + rs - ra, ln), e = (uint32_t)min(r_base + rs, ln);      // 0 <= a <= e <= LN
            const bool counted = depth_counts_op(op, X.count_deletions != 0) && e > a;
            const uint32_t b0 = min(a, (uint32_t)ln - 1u) / bin, b1 = (max(e, 1u) - 1u) / bin;               // counted: b0 <= b1 < the contig's bins
            const unsigned long long edge = ((unsigned long long)b0 + 1ull) * bin;
            const uint32_t first = counted ? (uint32_t)(min((unsigned long long)e, edge) - a) : 0u;
            const uint32_t last = counted && b1 > b0 ? (uint32_t)(e - (unsigned long long)b1 * bin) : 0u;
            {
                const uint32_t sum = depth_run_sum(b0, first, lane), prev = __shfl_up(b0, 1);
                if ((lane == 0 || prev != b0) && sum) atomicAdd(bases + b0, (unsigned long long)sum);
            }
            if (__ballot(last != 0u) != 0ull) {
                const uint32_t sum = depth_run_sum(b1, last, lane), prev = __shfl_up(b1, 1);
                if ((lane == 0 || prev != b1) && sum) atomicAdd(bases + b1, (unsigned long long)sum);
                unsigned long long m = __ballot(counted && b1 > b0 + 1u);
                while (m) {
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t k0 = __shfl(b0, j) + 1u, k1 = __shfl(b1, j);
                    for (uint32_t k = k0 + (uint32_t)lane; k < k1; k += WAVE) atomicAdd(bases + k, (unsigned long long)bin);
                }
            }
            r_base += __shfl(rs, WAVE - 1);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct BatchInfo {
    int n_blocks = 0;
    uint64_t file_off = 0, comp_bytes = 0, infl_bytes = 0;
    uint64_t ubase = 0;              // offset of the batch's first inflated byte in this range's uncompressed stream
    bool has_limit = false;          // the next byte range begins at or in front of this batch's end:
    long long limit_rel = 0;         //   at this offset from the batch's first inflated byte (negative: in an earlier batch)
    bool last = false;               // nothing follows (in this span)
    int span = 0;                    // span decode: which span the batch belongs to, whether it is the span's first batch and
    bool span_first = false;         //   where in its first block the span's first record starts
    uint32_t start_off = 0;
    bool span_tail = false;          // span decode: the batch ends with the span's last own block; what lies behind is only staged
                                     //   when the parse of this batch says that the span's last record goes on (span_verdict)
};

struct SpanDef {                     // a span of virtual offsets, taken apart
    uint64_t first_block = 0, end_block = 0;
    uint32_t start_off = 0, end_off = 0;
};

// what a batch leaves for the host-side worker: read names -> ids, SA text -> rows, non-ACGT records -> positions
struct HostJob {
    size_t base = 0;                 // ordinal of the batch's first record in the decoded range
    long long n = 0;
    std::vector<long long> pad, name_off, sa_off;
    std::vector<uint8_t> names, sa_text;
    std::vector<int32_t> na_list;    // (sorted) batch-local ordinals of the records with a non-ACGT code
    std::vector<long long> na_off;   // their bytes in na_raw (n + 1 offsets); a record = its bytes behind block_size
    std::vector<uint8_t> na_raw;
};

struct Carver {                      // hands the workspace out in 256-byte steps (p == 0: only the size is counted)
    uintptr_t p;
    size_t used = 0;
    void *operator()(size_t n) { used += up256(n); return (void *)(p + used - up256(n)); }
};

inline bool dev_get(void *dst, const void *src, size_t bytes) { return bytes == 0 || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; }

// The per-record scratch of the parse that a request may WRITE, built in emit.  Why that is safe:
// - k_bam_emit has finished with every array named here: the batch's host copies synchronised the stream behind it.
// - The requests are queued on the caller's stream in the order reads, coverage, read QC, binned depth, index, so each runs
//   behind the one in front.  Binned depth borrows nothing; it reads M.cig_src.
//   Reads, coverage and read QC use the same two arrays (items, item_off) in turn.  Reads also borrows out_len / out_off, which
//   nothing behind it but the index uses (and that never rides with it); it has read them back before it returns (its offsets)
//   and its k_bam_reads_emit, which reads out_off, runs in front of whatever is queued later.  Because M.name_len is `items`,
//   the reads kernels take a record's l_read_name from its bytes.
// - The index goes last because its out_key is M.cig_src, which the coverage and the depth walk read.  What every request only READS: the
//   fixed fields of M (tid .. n_cigar, seq_src), the record starts and the end positions.
// - All of it is queued in front of ev_parsed and of the next batch's k_bam_meta, which refills the arrays on the same stream.
struct GpuDecoder;
struct Borrowed {
    long long *items, *item_off;                        // reads, then coverage, then read QC (M.name_len, M.sa_len)
    long long *out_len, *out_off;                       // reads (M.pad_ops, d_cig_off)
    unsigned long long *voff, *out_voff;                // index (d_cig_off, M.sa_src)
    long long *key, *head, *head_off, *out_key;         // index (M.pad_ops, d_name_off, d_sa_off, M.cig_src)
};

inline bool launched(const char *what, std::string &err) {      // behind a request's launches
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) err = std::string(what) + " launch failed: " + hipGetErrorString(e);
    return e == hipSuccess;
}

struct CovRequest {                  // window coverage; with per_base the table of a pileup request instead of the counters
    bool active = false;
    const CovTable *T = nullptr;     // the request's segments, threshold and callback (Request::cov)
    CovSegs segs{nullptr, nullptr, nullptr, 0};          // segments and counters in the workspace (n = 0: nothing to count)
    unsigned long long *counts = nullptr;
    long long *pile_off = nullptr;   // per_base: the segments' prefix offsets and the table [positions][4]
    uint32_t *pile = nullptr;
    void carve(Carver &take) {
        if (!active) return;
        const size_t n_seg = T->size();
        int32_t *seg = (int32_t *)take(3 * n_seg * 4);
        segs = CovSegs{seg, seg + n_seg, seg + 2 * n_seg, (int)n_seg};
        counts = (unsigned long long *)take(n_seg * 8);
        if (!T->per_base) return;
        pile_off = (long long *)take((n_seg + 1) * 8);
        pile = (uint32_t *)take((size_t)T->n_pos() * 16);
    }
    const char *start(hipError_t &e) const {             // nullptr, or what failed with `e`
        if (segs.n == 0) return nullptr;
        const size_t b = T->size() * 4;
        if ((e = hipMemcpy((void *)segs.tid, T->tid.data(), b, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy((void *)segs.lo, T->lo.data(), b, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy((void *)segs.hi, T->hi.data(), b, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemset(counts, 0, 2 * b)) != hipSuccess)
            return "coverage request set-up";
        if (T->per_base && ((e = hipMemcpy(pile_off, T->seg_off.data(), (T->size() + 1) * 8, hipMemcpyHostToDevice)) != hipSuccess ||
                            (T->n_pos() > 0 && (e = hipMemset(pile, 0, (size_t)T->n_pos() * 16)) != hipSuccess)))
            return "pileup request set-up";
        return nullptr;
    }
    bool batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err) const;      // (behind GpuDecoder)
    bool finish(Decoded &D) const {
        if (!active) return true;
        if (!T->per_base) { D.cov.assign(T->size(), 0); return dev_get(D.cov.data(), counts, T->size() * 8); }
        D.pileup.assign((size_t)T->n_pos() * 4, 0);      // the table, and the counts per segment as its sums
        D.has_pileup = true;
        if (!dev_get(D.pileup.data(), pile, (size_t)T->n_pos() * 16)) return false;
        pileup_segment_sums(*T, D.pileup.data(), D.cov);
        return true;
    }
};

struct QcRequest {
    bool active = false;
    long long *rows = nullptr;                // the batch's qual_sum rows: one array for all batches (collect)
    unsigned long long *hist = nullptr;       // the device histogram of the whole decode
    long long pending_n = 0;                  // records of the batch whose rows are still on the device
    void carve(Carver &take, size_t nr) {
        if (!active) return;
        rows = (long long *)take(nr * 8);
        hist = (unsigned long long *)take(256 * 8);
    }
    const char *start(hipError_t &e) const { return active && (e = hipMemset(hist, 0, 256 * 8)) != hipSuccess ? "read-QC request set-up" : nullptr; }
    bool batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err);
    // The rows of the batch emitted last, if they are still on the device (the caller has synchronised the stream).  One array
    // for all batches: that holds only while every emit of a decode and the result call are given the SAME stream: the rows of
    // batch k-1 are complete once batch k's emit has waited for the stream that batch k-1's kernels were queued on, and batch
    // k's k_bam_qc_plan is queued only afterwards.
    bool collect(std::vector<int64_t> &v) {
        if (pending_n == 0) return true;
        const size_t base = v.size();
        v.resize(base + (size_t)pending_n);
        const bool ok = hipMemcpy(v.data() + base, rows, (size_t)pending_n * 8, hipMemcpyDeviceToHost) == hipSuccess;
        pending_n = 0;
        return ok;
    }
    bool finish(QcPartial &Q) { return !active || (collect(Q.qual_sum) && dev_get(Q.hist, hist, 256 * 8)); }
};

struct IndexRequest {
    bool active = false;
    IndexDev X{};
    uint32_t *boff[2] = {nullptr, nullptr};       // per block of the slot's batch: its file offset relative to the batch's
    BlockDesc *kept_desc[2] = {nullptr, nullptr}; // the slot's block table and offsets, kept for k_bam_index: the feeder re-stages
    uint32_t *kept_boff[2] = {nullptr, nullptr};  //   d_desc / boff for batch k + 2 while batch k is still being parsed
    int parity = 0;                               // which X.state the next batch reads
    void carve(Carver &take, size_t max_blocks, const IndexPartial &P) {      // (everything per record re-uses the batch's scratch)
        if (!active) return;
        const size_t n_ref = P.n_mapped.size();
        for (int i = 0; i < 2; ++i) {
            boff[i] = (uint32_t *)take(max_blocks * 4);
            kept_boff[i] = (uint32_t *)take(max_blocks * 4);
            kept_desc[i] = (BlockDesc *)take(max_blocks * sizeof(BlockDesc));
        }
        X.lin = (unsigned long long *)take(P.lin.size() * 8); X.lin_off = (long long *)take((n_ref + 1) * 8);
        X.n_mapped = (unsigned long long *)take(n_ref * 8); X.n_unmapped = (unsigned long long *)take(n_ref * 8);
        X.n_no_coor = (unsigned long long *)take(8); X.state = (unsigned long long *)take(16); X.unsorted = (int32_t *)take(4);
        X.n_ref = (int)n_ref;
    }
    // with nothing in front of the first record (rank 0) the first batch's end state is never read; a later rank's first
    // record is found by search and must start inside its batch (checked in coral_bamgpu_next)
    const char *start(const IndexPartial &P, hipError_t &e) const {
        const size_t n_ref = (size_t)X.n_ref;
        const bool ok = !active || ((e = hipMemset(X.lin, 0xff, P.lin.size() * 8)) == hipSuccess && (e = hipMemset(X.n_mapped, 0, n_ref * 8)) == hipSuccess &&
                                    (e = hipMemset(X.n_unmapped, 0, n_ref * 8)) == hipSuccess && (e = hipMemset(X.n_no_coor, 0, 8)) == hipSuccess &&
                                    (e = hipMemset(X.state, 0, 16)) == hipSuccess && (e = hipMemset(X.unsorted, 0, 4)) == hipSuccess &&
                                    (e = hipMemcpy(X.lin_off, P.lin_off.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice)) == hipSuccess);
        return ok ? nullptr : "index request set-up";
    }
    bool batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err);
    // false: a copy failed.  Sets P.unsorted when the device saw the order broken; it stays set: no index can be built
    bool finish(IndexPartial &P) const {
        if (!active) return true;
        const size_t n_ref = (size_t)X.n_ref;
        unsigned long long state[2] = {0, 0}, no_coor = 0;
        int32_t dev_unsorted = 0;
        if (!(dev_get(P.lin.data(), X.lin, P.lin.size() * 8) && dev_get(P.n_mapped.data(), X.n_mapped, n_ref * 8) && dev_get(P.n_unmapped.data(), X.n_unmapped, n_ref * 8) &&
              dev_get(&no_coor, X.n_no_coor, 8) && dev_get(state, X.state, 16) && dev_get(&dev_unsorted, X.unsorted, 4)))
            return false;
        if (dev_unsorted) P.unsorted = true;
        if (!P.unsorted) { P.n_no_coor = (int64_t)no_coor; P.end_voff = state[parity]; }
        return true;
    }
};

struct DepthRequest {                // binned depth: bin_off, the contig lengths and the two int64 tables in the workspace
    bool active = false;
    DepthDev X{};
    size_t n_bins = 0;
    void carve(Carver &take, const DepthPartial &P) {
        if (!active) return;
        const size_t n_ref = P.len.size();
        n_bins = (size_t)P.n_bins();
        X.bin_off = (long long *)take((n_ref + 1) * 8);
        X.len = (int32_t *)take(n_ref * 4);
        X.bases = (unsigned long long *)take(n_bins * 8);
        X.reads = (unsigned long long *)take(n_bins * 8);
        X.n_ref = (int)n_ref;
        X.bin = (uint32_t)P.bin; X.min_mapq = (uint32_t)P.min_mapq; X.exclude_flags = (uint32_t)P.exclude_flags;
        X.count_deletions = P.count_deletions ? 1 : 0;
    }
    const char *start(const DepthPartial &P, hipError_t &e) const {
        if (!active) return nullptr;
        const size_t n_ref = (size_t)X.n_ref;
        const bool ok = (e = hipMemcpy(X.bin_off, P.bin_off.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice)) == hipSuccess &&
                        (n_ref == 0 || (e = hipMemcpy(X.len, P.len.data(), n_ref * 4, hipMemcpyHostToDevice)) == hipSuccess) &&
                        (n_bins == 0 || ((e = hipMemset(X.bases, 0, n_bins * 8)) == hipSuccess && (e = hipMemset(X.reads, 0, n_bins * 8)) == hipSuccess));
        return ok ? nullptr : "binned-depth request set-up";
    }
    bool batch(GpuDecoder *G, hipStream_t stream, std::string &err) const;
    bool finish(DepthPartial &P) const {
        if (!active) return true;
        P.zero_tables();
        return dev_get(P.bases.data(), X.bases, n_bins * 8) && dev_get(P.reads.data(), X.reads, n_bins * 8);
    }
};

struct ReadsRequest {                // FASTQ text, or the own bytes (R->mode), of the selected records
    bool active = false;
    const ReadsRule *R = nullptr;    // the request (Request::reads)
    ReadsDev X{};
    uint8_t *text = nullptr;         // the batch's text: one buffer for all batches (collect)
    size_t text_cap = 0, buf_bytes = 0;
    long long pending_bytes = 0;     // text of the batch emitted last that is still on the device
    // coordinate order (R->order): the sort's double buffers of keys and ordinals, the permuted plan arrays and hipcub's
    // temporary storage - carved only for such a request
    unsigned long long *sort_key[2] = {nullptr, nullptr};
    uint32_t *sort_ord[2] = {nullptr, nullptr};
    long long *sorted_len = nullptr, *sorted_items = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    bool ordered() const { return active && R->order == READS_ORDER_COORDINATE; }
    // The output buffer is sized by a bound, not by a count: a record of l bases and a name field of n bytes (NUL included) takes
    // at least 36 + n + 1.5 l bytes of the batch (block_size, the fixed fields, the name, SEQ, QUAL) and its text 2 l + n + 5, and
    // 2 l + n + 5 <= 4/3 (36 + n + 1.5 l) = 48 + 4/3 n + 2 l.  So the text of all records of a batch fits 4/3 of the batch's bytes,
    // the carried ones included (+ 256: the division's remainder and room to spare).  In mode READS_AS_RECORDS the written bytes
    // are a part of the batch's own: one batch's capacity + 256.
    void carve(Carver &take, size_t batch_cap, size_t nr) {
        if (!active) return;
        if (ordered()) {
            for (int i = 0; i < 2; ++i) { sort_key[i] = (unsigned long long *)take(nr * 8); sort_ord[i] = (uint32_t *)take(nr * 4); }
            sorted_len = (long long *)take(nr * 8); sorted_items = (long long *)take(nr * 8);
            sort_tmp = take(sort_tmp_bytes);
        }
        buf_bytes = up256(batch_cap + COMP_SLACK);                 // (what d_infl[slot] really has: reads_window's guard)
        const size_t n_seg = R->tid.size(), n_names = (size_t)R->n_names();
        int32_t *seg = (int32_t *)take(3 * n_seg * 4);
        uint8_t *names = (uint8_t *)take(R->names.size());
        int64_t *off = (int64_t *)take((n_names + 1) * 8);
        X = ReadsDev{seg, seg + n_seg, seg + 2 * n_seg, names, off, (int)n_seg, (long long)n_names, R->exclude_flags, R->mode};
        text_cap = (R->mode == READS_AS_RECORDS ? batch_cap : batch_cap / 3 * 4) + 256;
        text = (uint8_t *)take(text_cap);
    }
    const char *start(hipError_t &e) const {
        if (!active) return nullptr;
        const size_t b = (size_t)X.n_seg * 4;
        const bool ok = (b == 0 || ((e = hipMemcpy((void *)X.tid, R->tid.data(), b, hipMemcpyHostToDevice)) == hipSuccess &&
                                    (e = hipMemcpy((void *)X.lo, R->lo.data(), b, hipMemcpyHostToDevice)) == hipSuccess &&
                                    (e = hipMemcpy((void *)X.hi, R->hi.data(), b, hipMemcpyHostToDevice)) == hipSuccess)) &&
                        (X.n_names == 0 || ((e = hipMemcpy((void *)X.names, R->names.data(), R->names.size(), hipMemcpyHostToDevice)) == hipSuccess &&
                                            (e = hipMemcpy((void *)X.name_off, R->name_off.data(), R->name_off.size() * 8, hipMemcpyHostToDevice)) == hipSuccess));
        return ok ? nullptr : "reads request set-up";
    }
    bool batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err);
    // The text of the batch emitted last, if it is still on the device (the caller has synchronised the stream).  One buffer for
    // all batches: QcRequest::collect's argument, under the same condition - every emit of a decode and the result call are
    // given the SAME stream.
    bool collect(Decoded &D) {
        if (pending_bytes == 0) return true;
        const size_t base = D.reads_text.size();
        D.reads_text.resize(base + (size_t)pending_bytes);
        const bool ok = hipMemcpy(D.reads_text.data() + base, text, (size_t)pending_bytes, hipMemcpyDeviceToHost) == hipSuccess;
        pending_bytes = 0;
        return ok;
    }
    // Coordinate order: every batch left one sorted run (D.reads_runs: the written record it begins at); more than one run goes
    // through the host's stable k-way merge, run order = batch order, and the runs are freed.
    bool finish(Decoded &D, int n_threads) {
        if (!active) return true;
        D.has_reads = true;
        if (!collect(D)) return false;
        if (!ordered() || D.reads_runs.size() < 2) return true;
        const size_t n_runs = D.reads_runs.size(), n_rec = D.reads_off.size() - 1;
        std::vector<const uint8_t *> data(n_runs, D.reads_text.data());
        std::vector<const int64_t *> off(n_runs);
        std::vector<int64_t> n(n_runs);
        for (size_t r = 0; r < n_runs; ++r) {
            off[r] = D.reads_off.data() + D.reads_runs[r];
            n[r] = (r + 1 < n_runs ? D.reads_runs[r + 1] : (int64_t)n_rec) - D.reads_runs[r];
        }
        std::vector<uint8_t> text(D.reads_text.size());
        std::vector<int64_t> merged(n_rec + 1);
        if (coral_bam_records_merge((int32_t)n_runs, data.data(), off.data(), n.data(), text.data(), merged.data(), n_threads) != CORAL_OK) return false;
        D.reads_text.swap(text);
        D.reads_off.swap(merged);
        D.reads_runs.assign(1, 0);
        return true;
    }
};

struct GpuDecoder {
    MappedFile f;
    Decoded D;
    RefIds ref_id;
    size_t hdr_bytes = 0;
    Request req;                              // what was asked for (coral_bamgpu_open_request)
    int n_threads = 1, device = 0;
    uint64_t byte_lo = 0, byte_hi = 0, first_block = 0;
    bool last_rank = true;
    std::string error;
    // capacities
    size_t infl_cap = 0, comp_cap = 0, max_blocks = 0, rec_cap = 0, nseg_cap = 0;
    uint64_t first_batch = FIRST_BATCH;
    size_t ws_bytes = 0;
    // device workspace (carved from the caller's allocation)
    uint8_t *d_comp[2] = {nullptr, nullptr}, *d_infl[2] = {nullptr, nullptr};
    BlockDesc *d_desc[2] = {nullptr, nullptr};
    uint32_t *d_crc[2] = {nullptr, nullptr};
    int32_t *d_status[2] = {nullptr, nullptr};
    long long *d_seg_first = nullptr, *d_seg_land = nullptr, *d_seg_base = nullptr, *d_result = nullptr, *d_rec_start = nullptr;
    long long *d_rec_all = nullptr;           // every record start of the batch (k_bam_starts).  d_rec_start is what everything behind
                                              // reads: the same array, or with an active record filter a second one (the kept starts)
    int32_t *d_seg_count = nullptr, *d_seg_valid = nullptr, *d_error = nullptr, *d_na_list = nullptr, *d_na_count = nullptr;
    MetaArrays M{};
    long long *d_cig_off = nullptr, *d_name_off = nullptr, *d_sa_off = nullptr;
    int32_t *d_end = nullptr, *d_qlen = nullptr;
    uint8_t *d_names = nullptr, *d_sa_text = nullptr;
    void *d_scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0, names_cap = 0, sa_cap = 0;
    // pinned staging + streams
    uint8_t *h_stage[N_STAGE] = {};
    BlockDesc *h_desc[2] = {nullptr, nullptr};      // (pinned; the blocks' trailer CRCs follow the table in the same buffer)
    hipStream_t s_copy = nullptr, s_infl = nullptr, s_crc = nullptr;
    hipEvent_t ev_stage[N_STAGE] = {};
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_infl[2] = {nullptr, nullptr}, ev_parsed[2] = {nullptr, nullptr};
    hipEvent_t ev_crc[2] = {nullptr, nullptr};          // the slot's checksum kernel has run (its own stream, beside the next inflate)
    double t_read = 0, t_alloc = 0, t_wait_staged = 0, t_wait_gpu = 0;
    // feeder
    std::thread feeder;
    std::mutex m;
    std::condition_variable cv;
    std::vector<BatchInfo> staged;            // batches whose H2D has been issued
    bool feeder_done = false, stop = false;
    int inflate_launched = 0;                 // batches whose inflate kernel has been enqueued
    int emitted = 0;                          // batches whose parse has been enqueued completely (ev_parsed recorded)
    std::string feeder_error, launch_error;
    // walk state
    int k = 0;                                // next batch to parse
    bool searching = false, finished = false;
    long long known_start = 0;                // buffer offset of the first record of batch k (CARRY_CAP-based)
    long long carry_len = 0;                  // bytes carried in front of batch k
    // the batch between next() and emit()
    BatchInfo cur;
    long long cur_n_rec = 0, cur_ops = 0, cur_name_bytes = 0, cur_sa_bytes = 0;
    bool have_cur = false;
    // host-side worker
    std::thread worker;
    std::mutex wm;
    std::condition_variable wcv;
    std::deque<std::unique_ptr<HostJob>> jobs;
    bool worker_stop = false, worker_busy = false;
    std::string worker_error;
    long long cur_carry_pos = 0;
    // the requests that ride along
    CovRequest cov;
    QcRequest qc;
    IndexRequest idx;
    DepthRequest depth;
    ReadsRequest reads;
    // span decode: the spans are decoded one after the other through the same batches
    std::vector<SpanDef> spans;
    int cur_span = 0;                         // the span the caller's thread is parsing
    std::vector<int> span_verdict;            // per span (under m): 0 = not known yet, 1 = its last record has been parsed,
                                              //   2 = the record in front of its end goes on behind its last own block
    // statistics
    double t_open = 0, seconds = 0, host_seconds = 0;
    int64_t fixups = 0, n_batches = 0, na_records = 0;
    std::chrono::steady_clock::time_point t_start;

    // work items of `slice` bytes in the batch between next() and emit(): at most one per record plus one per slice
    long long max_items(long long slice) const { return cur_n_rec + ((long long)CARRY_CAP + (long long)cur.infl_bytes) / slice + 1; }
    // exclusive sums of that batch's n + 1 per-record counts (scan inputs, work items, index run heads)
    bool scan(hipStream_t stream, long long *in, long long *out) {
        size_t tmp = scan_tmp_bytes;
        return hipcub::DeviceScan::ExclusiveSum(d_scan_tmp, tmp, in, out, (int)(cur_n_rec + 1), stream) == hipSuccess;
    }

    ~GpuDecoder() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        if (feeder.joinable()) feeder.join();
        {
            std::lock_guard<std::mutex> lk(wm);
            worker_stop = true;
        }
        wcv.notify_all();
        if (worker.joinable()) worker.join();
        // (an error may leave kernels and copies in flight: they work in the caller's workspace, which is about to be released)
        if (s_copy) (void)hipStreamSynchronize(s_copy);
        if (s_infl) (void)hipStreamSynchronize(s_infl);
        if (s_crc) (void)hipStreamSynchronize(s_crc);
        for (int i = 0; i < N_STAGE; ++i) {
            if (h_stage[i]) (void)hipHostFree(h_stage[i]);
            if (ev_stage[i]) (void)hipEventDestroy(ev_stage[i]);
        }
        for (int i = 0; i < 2; ++i) {
            if (h_desc[i]) (void)hipHostFree(h_desc[i]);
            if (ev_h2d[i]) (void)hipEventDestroy(ev_h2d[i]);
            if (ev_infl[i]) (void)hipEventDestroy(ev_infl[i]);
            if (ev_crc[i]) (void)hipEventDestroy(ev_crc[i]);
            if (ev_parsed[i]) (void)hipEventDestroy(ev_parsed[i]);
        }
        if (s_copy) (void)hipStreamDestroy(s_copy);
        if (s_infl) (void)hipStreamDestroy(s_infl);
        if (s_crc) (void)hipStreamDestroy(s_crc);
    }
};

// queued before ev_parsed so that the slot is not inflated into while the kernels read its SEQ and QUAL
bool CovRequest::batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err) const {
    const long long n = G->cur_n_rec;
    const uint8_t *buf = G->d_infl[G->k & 1];
    if (n == 0 || segs.n == 0) return true;
    hipLaunchKernelGGL(k_bam_cov_plan, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, stream, buf, n, G->M, G->d_end, segs, T->threshold,
                       (int)T->filter_all, S.items);
    if (!G->scan(stream, S.items, S.item_off)) { err = "scan of the coverage work items failed"; return false; }
    const long long items = G->max_items(COV_SLICE);
    if (T->per_base)                 // one wave per workgroup, grid-stride beyond 32 per CU
        hipLaunchKernelGGL(k_bam_pileup, dim3((unsigned)std::min<long long>(items, 8192)), dim3(WAVE), 0, stream, buf, n, G->M, segs, pile_off,
                           T->threshold, S.item_off, pile);
    else                             // 4 waves per workgroup, grid-stride beyond
        hipLaunchKernelGGL(k_bam_cov_count, dim3((unsigned)std::min<long long>((items + 3) / 4, 8192)), dim3(256), 0, stream, buf, n, G->M, segs,
                           T->threshold, S.item_off, counts);
    return launched("window coverage", err);
}

// Nothing is waited for here: the rows are fetched with the next batch's host fields (behind that emit's stream
// synchronisation, which any kernel queued here is in front of), or by coral_bamgpu_finish.
bool QcRequest::batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err) {
    const long long n = G->cur_n_rec;
    const uint8_t *buf = G->d_infl[G->k & 1];
    if (n == 0 || !active) return true;
    hipLaunchKernelGGL(k_bam_qc_plan, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, buf, G->d_rec_start, n, G->M, rows, S.items);
    if (!G->scan(stream, S.items, S.item_off)) { err = "scan of the read-QC work items failed"; return false; }
    // one wave per workgroup, grid-stride beyond 8 per CU
    hipLaunchKernelGGL(k_bam_qc, dim3((unsigned)std::min<long long>(G->max_items(QC_SLICE), 2048)), dim3(WAVE), 0, stream, buf, G->d_rec_start, n, G->M, S.item_off,
                       (unsigned long long *)rows, hist);
    if (!launched("read-QC", err)) return false;
    pending_n = n;
    return true;
}

// The reads request goes FIRST behind the batch's host copies: it waits for its own totals (16 bytes: no read-back of the batch
// lies behind these kernels, so they are a small copy of their own, as k_bam_keep_compact's count is), and in front of the other
// requests that wait is only for its plan kernel and two scans.  The text itself is not waited for (collect).
bool ReadsRequest::batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err) {
    if (!active) return true;
    if (!collect(G->D)) { err = "copy of the reads text failed"; return false; }      // (of the batch in front: its kernels have run, ours are not queued yet)
    const long long n = G->cur_n_rec;
    if (n == 0) return true;
    const uint8_t *buf = G->d_infl[G->k & 1];
    hipLaunchKernelGGL(k_bam_reads_plan, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, buf, G->d_rec_start, n, G->M, G->d_end, X,
                       S.out_len, S.items);
    const uint32_t *ord = nullptr;                   // coordinate order: sorted position -> record of the batch
    if (ordered()) {
        hipLaunchKernelGGL(k_bam_sort_keys, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, n, G->M, sort_key[0], sort_ord[0]);
        hipcub::DoubleBuffer<unsigned long long> keys(sort_key[0], sort_key[1]);
        hipcub::DoubleBuffer<uint32_t> ords(sort_ord[0], sort_ord[1]);
        size_t need = 0, tmp = sort_tmp_bytes;           // (the storage was sized for the largest batch: checked, not assumed)
        if (hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys, ords, (int)n, 0, 64, stream) != hipSuccess || need > sort_tmp_bytes ||
            hipcub::DeviceRadixSort::SortPairs(sort_tmp, tmp, keys, ords, (int)n, 0, 64, stream) != hipSuccess) {
            err = "sort of the reads keys failed";
            return false;
        }
        ord = ords.Current();
        hipLaunchKernelGGL(k_bam_sort_permute, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, n, ord, S.out_len, S.items, sorted_len,
                           sorted_items);
        if (!G->scan(stream, sorted_len, S.out_off) || !G->scan(stream, sorted_items, S.item_off)) { err = "scan of the sorted reads work items failed"; return false; }
        G->D.reads_runs.push_back((int64_t)G->D.reads_off.size() - 1);      // this batch's run begins behind what is written
    } else if (!G->scan(stream, S.out_len, S.out_off) || !G->scan(stream, S.items, S.item_off)) { err = "scan of the reads work items failed"; return false; }
    std::vector<long long> off((size_t)n + 1);
    long long items = 0;
    if (hipMemcpyAsync(off.data(), S.out_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipMemcpyAsync(&items, S.item_off + n, 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        err = std::string("reads plan failed: ") + hipGetErrorString(hipGetLastError());
        return false;
    }
    const long long bytes = off[(size_t)n];
    if (bytes < 0 || (size_t)bytes > text_cap || items < 0) { err = "reads request: the batch's text does not fit its buffer"; return false; }
    if (bytes == 0) return true;                     // no record of the batch is written: nothing more is queued
    const int64_t base = G->D.reads_off.back();
    for (long long i = 0; i < n; ++i)
        if (off[(size_t)i + 1] > off[(size_t)i]) G->D.reads_off.push_back(base + off[(size_t)i + 1]);
    // one wave per workgroup, grid-stride beyond 8 per CU
    const dim3 grid((unsigned)std::min<long long>(items, 2048));
    if (ord)
        hipLaunchKernelGGL(k_bam_reads_copy_sorted, grid, dim3(WAVE), 0, stream, buf, (long long)buf_bytes, G->d_rec_start, n, ord, S.item_off, S.out_off, text);
    else if (X.mode == READS_AS_RECORDS)
        hipLaunchKernelGGL(k_bam_reads_copy, grid, dim3(WAVE), 0, stream, buf, (long long)buf_bytes, G->d_rec_start, n, S.item_off, S.out_off, text);
    else
        hipLaunchKernelGGL(k_bam_reads_emit, grid, dim3(WAVE), 0, stream, buf, (long long)buf_bytes, G->d_rec_start, n, G->M, S.item_off, S.out_off, text);
    if (!launched("reads", err)) return false;
    pending_bytes = bytes;
    return true;
}

// reads the slot's CIGAR bytes (M.cig_src: in front of the index request, which borrows that array)
bool DepthRequest::batch(GpuDecoder *G, hipStream_t stream, std::string &err) const {
    const long long n = G->cur_n_rec;
    if (n == 0 || !active || n_bins == 0) return true;
    // one wave per workgroup, grid-stride beyond 32 per CU
    hipLaunchKernelGGL(k_bam_depth, dim3((unsigned)std::min<long long>(n, 8192)), dim3(WAVE), 0, stream, G->d_infl[G->k & 1], n, G->M, X);
    return launched("binned depth", err);
}

// the batch's part of the index; also for a batch without records: the end state it leaves is the next batch's start
bool IndexRequest::batch(GpuDecoder *G, hipStream_t stream, const Borrowed &S, std::string &err) {
    const long long n = G->cur_n_rec;
    if (!active) return true;
    hipLaunchKernelGGL(k_bam_index, dim3((unsigned)((n + 1 + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, G->d_rec_start, n, G->M, G->d_end, kept_desc[G->k & 1],
                       kept_boff[G->k & 1], G->cur.n_blocks, (unsigned long long)G->cur.file_off, (unsigned long long)G->cur.comp_bytes,
                       (long long)G->cur.infl_bytes, G->cur_carry_pos, parity, X, S.voff, S.key, S.head);
    parity ^= 1;
    long long n_heads = 0;
    if (n > 0) {
        if (!G->scan(stream, S.head, S.head_off)) { err = "scan of the index run heads failed"; return false; }
        hipLaunchKernelGGL(k_bam_index_compact, dim3((unsigned)((n + WAVE - 1) / WAVE)), dim3(WAVE), 0, stream, n, S.head, S.head_off, S.voff, S.key, S.out_voff,
                           S.out_key);
        if (hipMemcpyAsync(&n_heads, S.head_off + n, 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            err = std::string("index kernels failed: ") + hipGetErrorString(hipGetLastError());
            return false;
        }
        std::vector<long long> hk((size_t)n_heads);
        std::vector<unsigned long long> hv((size_t)n_heads);
        if (!dev_get(hk.data(), S.out_key, (size_t)n_heads * 8) || !dev_get(hv.data(), S.out_voff, (size_t)n_heads * 8)) {
            err = "copy of the index run heads failed";
            return false;
        }
        for (long long j = 0; j < n_heads; ++j) G->D.idx.add_head(hk[(size_t)j], hv[(size_t)j]);
    }
    return launched("index", err);
}

// parallel pread of [off, off + n) into dst
bool read_range(int fd, uint64_t off, size_t n, uint8_t *dst, int n_threads) {
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, n / (4u << 20) + 1));
    std::atomic<bool> bad{false};
    auto work = [&](int t) {
        size_t a = n * (size_t)t / (size_t)nt, b = n * (size_t)(t + 1) / (size_t)nt;
        while (a < b) {
            const ssize_t got = pread(fd, dst + a, b - a, (off_t)(off + a));
            if (got <= 0) { bad = true; return; }
            a += (size_t)got;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    return !bad;
}

bool launch_inflate(GpuDecoder *G, int kb, const BatchInfo &bi);

// The feeder: cuts the byte range into batches (whole BGZF blocks, <= infl_cap inflated and <= comp_cap compressed bytes),
// reads each into pinned memory, builds its block table and sends both to the device.
void feeder_main(GpuDecoder *G) {
    (void)hipSetDevice(G->device);
    uint64_t at = G->first_block;
    uint64_t ubase = 0;
    long long own_bytes = -1;                 // known once the first block of the next range has been seen
    size_t overhang_left = OVERHANG_BLOCKS;
    int kb = 0, chunk_no = 0;
    const int n_spans = G->req.span_mode ? (int)G->spans.size() : 1;
    auto fail = [&](const std::string &msg) {
        std::lock_guard<std::mutex> lk(G->m);
        G->feeder_error = msg;
        G->feeder_done = true;
        G->cv.notify_all();
    };
    std::vector<BlockDesc> desc;
    std::vector<uint32_t> crcs, boffs;
    for (int sp = 0; sp < n_spans; ++sp) {
        const SpanDef S = G->req.span_mode ? G->spans[(size_t)sp] : SpanDef();
        bool span_first = G->req.span_mode;
        if (G->req.span_mode) {
            at = S.first_block;
            ubase = 0;
            own_bytes = -1;
            overhang_left = OVERHANG_BLOCKS;
        }
        bool tail_staged = false, overhang_ok = false;
        for (;;) {
            const int slot = kb & 1;
            if (at >= G->f.size || (own_bytes >= 0 && overhang_left == 0)) break;
            if (tail_staged && !overhang_ok) {
                // the span's own blocks are on their way.  Its end is a record boundary of the index, so as a rule its last record
                // ends there too and nothing behind is read; only when the parse finds that record going on is the overhang staged
                std::unique_lock<std::mutex> lk(G->m);
                G->cv.wait(lk, [&] { return G->stop || G->span_verdict[(size_t)sp] != 0; });
                if (G->stop) return;
                if (G->span_verdict[(size_t)sp] == 1) break;
                overhang_ok = true;
            }
            {   // the slot's device buffers are free once the inflate of batch kb - 2 has run
                std::unique_lock<std::mutex> lk(G->m);
                G->cv.wait(lk, [&] { return G->stop || G->inflate_launched >= kb - 1; });
                if (G->stop) return;
            }
            if (kb >= 2 && (hipEventSynchronize(G->ev_infl[slot]) != hipSuccess || hipEventSynchronize(G->ev_crc[slot]) != hipSuccess))
                return fail("hipEventSynchronize failed in the feeder");
            // the first batches are small so that the GPU has something to inflate almost at once; then they double up to the cap
            const uint64_t infl_cap = std::min<uint64_t>(G->infl_cap, G->first_batch << std::min(kb, 20));
            const uint64_t comp_cap = std::min<uint64_t>(G->comp_cap, std::max<uint64_t>(infl_cap / 2, 1u << 20));
            BatchInfo bi;
            bi.file_off = at;
            bi.ubase = ubase;
            bi.span = sp;
            bi.span_first = span_first;
            bi.start_off = S.start_off;
            span_first = false;
            desc.clear();
            crcs.clear();
            boffs.clear();
            uint64_t comp = 0, infl = 0;          // bytes of the batch so far
            bool full = false;
            while (!full && at < G->f.size) {
                // one chunk: read -> walk its whole BGZF blocks -> send them behind what the batch already has
                const int cs = chunk_no % N_STAGE;
                if (chunk_no >= N_STAGE && hipEventSynchronize(G->ev_stage[cs]) != hipSuccess) return fail("hipEventSynchronize failed in the feeder");
                const size_t want = (size_t)std::min<uint64_t>(std::min<uint64_t>(STAGE_BYTES, comp_cap - comp), G->f.size - at);
                if (want < 28) break;
                uint8_t *data = G->h_stage[cs];
                const auto t0 = std::chrono::steady_clock::now();
                if (!read_range(G->f.fd, at, want, data, G->n_threads)) return fail("reading the BAM file failed");
                G->t_read += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                size_t p = 0;
                while (p < want) {
                    if (desc.size() >= G->max_blocks) { full = true; break; }
                    Block b;
                    if (!bgzf_header(data + p, want - p, b)) {
                        if (want - p >= 65536 + 26 || at + want >= G->f.size) return fail("not a BGZF block");
                        if (want < STAGE_BYTES) full = true;           // the block does not fit what is left of the batch
                        break;                                         // the block continues behind what was read
                    }
                    if (infl + b.isize > infl_cap) { full = true; break; }
                    if (G->req.span_mode && at + p == S.end_block && own_bytes < 0) own_bytes = (long long)(ubase + infl) + S.end_off;
                    const bool owned = G->req.span_mode ? (at + p < S.end_block || (at + p == S.end_block && S.end_off > 0)) : at + p < G->byte_hi;
                    if (!owned && G->req.span_mode && !overhang_ok && !desc.empty()) { tail_staged = true; full = true; break; }
                    // (the batch in front filled up exactly with the span's last own block: this one block alone is the tail batch
                    // the parse gives its verdict on)
                    const bool lone_tail = !owned && G->req.span_mode && !overhang_ok;
                    if (!owned) {
                        if (own_bytes < 0) own_bytes = (long long)(ubase + infl);
                        if (overhang_left == 0) { full = true; break; }
                        --overhang_left;
                    }
                    BlockDesc d;
                    d.src_off = (uint32_t)(comp + p + b.hdr);
                    d.src_len = b.csize - b.hdr - 8;
                    d.dst_off = (uint32_t)infl;
                    d.isize = b.isize;
                    desc.push_back(d);
                    crcs.push_back(rd32(data + p + b.csize - 8));
                    boffs.push_back((uint32_t)(comp + p));
                    infl += b.isize;
                    p += b.csize;
                    // (of a span every block that is read counts, its overhang included)
                    if (lone_tail) { tail_staged = true; full = true; }
                    if (owned || G->req.span_mode) { G->D.compressed_bytes += b.csize; G->D.uncompressed_bytes += b.isize; ++G->D.n_blocks; }
                }
                if (p == 0) {
                    if (desc.empty()) return fail("a BGZF block does not fit the batch buffers");
                    break;
                }
                if (hipMemcpyAsync(G->d_comp[slot] + comp, data, p, hipMemcpyHostToDevice, G->s_copy) != hipSuccess ||
                    hipEventRecord(G->ev_stage[cs], G->s_copy) != hipSuccess)
                    return fail("host-to-device copy of compressed bytes failed");
                ++chunk_no;
                comp += p;
                at += p;
                if (comp + 65536 + 26 > comp_cap) full = true;
            }
            if (desc.empty()) break;
            bi.n_blocks = (int)desc.size();
            bi.comp_bytes = comp;
            bi.infl_bytes = infl;
            if (own_bytes >= 0) {
                bi.has_limit = true;
                bi.limit_rel = own_bytes - (long long)ubase;
            }
            ubase += infl;
            bi.last = at >= G->f.size || (own_bytes >= 0 && overhang_left == 0);
            bi.span_tail = tail_staged && !overhang_ok;
            // the block table and the trailer CRCs go through their own pinned buffer (one per batch slot; host and device copies are
            // free again once the slot's inflate + checksum kernels have run: see the wait at the top of the round)
            memcpy(G->h_desc[slot], desc.data(), desc.size() * sizeof(BlockDesc));
            uint32_t *h_crc = reinterpret_cast<uint32_t *>(G->h_desc[slot] + G->max_blocks);
            memcpy(h_crc, crcs.data(), crcs.size() * 4);
            if (hipMemcpyAsync(G->d_desc[slot], G->h_desc[slot], desc.size() * sizeof(BlockDesc), hipMemcpyHostToDevice, G->s_copy) != hipSuccess ||
                hipMemcpyAsync(G->d_crc[slot], h_crc, crcs.size() * 4, hipMemcpyHostToDevice, G->s_copy) != hipSuccess ||
                (G->idx.active && (memcpy(h_crc + G->max_blocks, boffs.data(), boffs.size() * 4),
                               hipMemcpyAsync(G->idx.boff[slot], h_crc + G->max_blocks, boffs.size() * 4, hipMemcpyHostToDevice, G->s_copy) != hipSuccess)) ||
                hipEventRecord(G->ev_h2d[slot], G->s_copy) != hipSuccess)
                return fail("host-to-device copy of a block table failed");
            {
                std::lock_guard<std::mutex> lk(G->m);
                G->staged.push_back(bi);
            }
            G->cv.notify_all();
            // ... and its inflate is enqueued from here as well, as soon as the batch that used this slot's inflated buffer before
            // (kb - 2) has been parsed: the GPU never waits for the caller's thread to come round
            {
                std::unique_lock<std::mutex> lk(G->m);
                G->cv.wait(lk, [&] { return G->stop || G->emitted >= kb - 1; });
                if (G->stop) return;
            }
            if (!launch_inflate(G, kb, bi)) return fail(G->launch_error);
            ++kb;
            if (bi.last) break;
        }
    }
    {
        std::lock_guard<std::mutex> lk(G->m);
        G->feeder_done = true;
    }
    G->cv.notify_all();
}

// The host-side worker: batches in file order.  Touches only D.cigar_off, D.name_id, D.names, D.sa, D.sa_nm, D.sa_off, D.na_rec,
// D.na_pos (the caller's thread fills the per-record integer columns).
void worker_main(GpuDecoder *G) {
    Decoded &D = G->D;
    for (;;) {
        std::unique_ptr<HostJob> job;
        {
            std::unique_lock<std::mutex> lk(G->wm);
            G->wcv.wait(lk, [&] { return G->worker_stop || !G->jobs.empty(); });
            if (G->jobs.empty()) return;
            job = std::move(G->jobs.front());
            G->jobs.pop_front();
            G->worker_busy = true;
        }
        const auto t0 = std::chrono::steady_clock::now();
        std::string err;
        HostJob &J = *job;
        for (long long i = 0; i < J.n && err.empty(); ++i) {
            D.cigar_off.push_back(D.cigar_off.back() + J.pad[(size_t)i]);
            const char *s = (const char *)J.names.data() + J.name_off[(size_t)i];
            const size_t len = (size_t)(J.name_off[(size_t)i + 1] - J.name_off[(size_t)i]);
            // as the CPU pipeline: the bytes in front of the last one, cut at a NUL
            D.name_id.push_back(D.names.intern(s, len ? strnlen(s, len - 1) : 0));
            int32_t cnt = 0;
            if (J.sa_off[(size_t)i + 1] > J.sa_off[(size_t)i]) {
                const char *q = (const char *)J.sa_text.data() + J.sa_off[(size_t)i];
                const char *qe = q + (J.sa_off[(size_t)i + 1] - J.sa_off[(size_t)i]);
                while (q < qe && *q) {
                    const char *e = q;
                    while (e < qe && *e && *e != ';') ++e;
                    if (e > q) {
                        int32_t row[8], snm = 0;
                        if (!parse_sa_entry(q, e, G->ref_id, row, &snm)) { err = "malformed SA entry"; break; }
                        D.sa.insert(D.sa.end(), row, row + 8);
                        D.sa_nm.push_back(snm);
                        ++cnt;
                    }
                    q = (e < qe && *e == ';') ? e + 1 : e;
                }
            }
            D.sa_off.push_back(D.sa_off.back() + cnt);
        }
        // records with a non-ACGT code: their aligned non-ACGT positions come from the CPU pipeline's own routine
        for (size_t j = 0; j < J.na_list.size() && err.empty(); ++j) {
            Partial pt;
            if (!decode_record(J.na_raw.data() + J.na_off[j], (uint32_t)(J.na_off[j + 1] - J.na_off[j]), G->ref_id, pt, err)) break;
            for (size_t q = 0; q < pt.na_pos.size(); ++q) {
                D.na_rec.push_back((int64_t)J.base + J.na_list[j]);
                D.na_pos.push_back(pt.na_pos[q]);
            }
        }
        {
            std::lock_guard<std::mutex> lk(G->wm);
            G->host_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (!err.empty() && G->worker_error.empty()) G->worker_error = err;
            G->worker_busy = false;
        }
        G->wcv.notify_all();
    }
}

// Lays the device workspace out (ws == nullptr: only its size is computed, the pointers stay meaningless).
bool carve(GpuDecoder *G, void *ws, size_t bytes) {
    Carver take{(uintptr_t)ws};
    for (int i = 0; i < 2; ++i) {
        G->d_comp[i] = (uint8_t *)take(G->comp_cap + COMP_SLACK);
        G->d_infl[i] = (uint8_t *)take((size_t)CARRY_CAP + G->infl_cap + COMP_SLACK);
        G->d_desc[i] = (BlockDesc *)take(G->max_blocks * sizeof(BlockDesc));
        G->d_crc[i] = (uint32_t *)take(G->max_blocks * 4);
        G->d_status[i] = (int32_t *)take(G->max_blocks * 4);
    }
    const size_t ns = G->nseg_cap, nr = G->rec_cap + 1;
    G->d_seg_first = (long long *)take(ns * 8);
    G->d_seg_land = (long long *)take(ns * 8);
    G->d_seg_base = (long long *)take(ns * 8);
    G->d_seg_count = (int32_t *)take(ns * 4);
    G->d_seg_valid = (int32_t *)take(ns * 4);
    G->d_result = (long long *)take(64);
    G->d_error = (int32_t *)take(16);
    G->d_na_count = (int32_t *)take(16);
    G->d_rec_start = G->d_rec_all = (long long *)take(nr * 8);
    if (G->req.keep.active()) G->d_rec_start = (long long *)take(nr * 8);      // the kept starts (k_bam_keep_compact)
    G->M.tid = (int32_t *)take(nr * 4); G->M.pos = (int32_t *)take(nr * 4); G->M.flag = (int32_t *)take(nr * 4);
    G->M.mapq = (int32_t *)take(nr * 4); G->M.l_seq = (int32_t *)take(nr * 4); G->M.nm = (int32_t *)take(nr * 4);
    G->M.n_cigar = (int32_t *)take(nr * 4);
    G->M.cig_src = (long long *)take(nr * 8); G->M.seq_src = (long long *)take(nr * 8); G->M.sa_src = (long long *)take(nr * 8);
    G->M.pad_ops = (long long *)take(nr * 8); G->M.name_len = (long long *)take(nr * 8); G->M.sa_len = (long long *)take(nr * 8);
    G->d_cig_off = (long long *)take(nr * 8); G->d_name_off = (long long *)take(nr * 8); G->d_sa_off = (long long *)take(nr * 8);
    G->d_end = (int32_t *)take(nr * 4); G->d_qlen = (int32_t *)take(nr * 4);
    G->d_na_list = (int32_t *)take(nr * 4);
    G->d_scan_tmp = take(G->scan_tmp_bytes);
    // read names and SA text of one batch can never exceed its inflated bytes (+ what was carried)
    G->names_cap = G->sa_cap = (size_t)CARRY_CAP + G->infl_cap;
    G->d_names = (uint8_t *)take(G->names_cap);
    G->d_sa_text = (uint8_t *)take(G->sa_cap);
    G->idx.carve(take, G->max_blocks, G->D.idx);
    G->qc.carve(take, nr);
    G->cov.carve(take);
    G->depth.carve(take, G->D.depth);
    G->reads.carve(take, (size_t)CARRY_CAP + G->infl_cap, nr);
    if (ws && take.used > bytes) return false;
    G->ws_bytes = take.used;
    return true;
}

#define HIP_LAUNCH_OK(call, what)                                                           \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            G->launch_error = std::string(what) + ": " + hipGetErrorString(e_);             \
            return false;                                                                   \
        }                                                                                   \
    } while (0)

bool launch_inflate(GpuDecoder *G, int kb, const BatchInfo &bi) {
    const int slot = kb & 1;
    HIP_LAUNCH_OK(hipStreamWaitEvent(G->s_infl, G->ev_h2d[slot], 0), "hipStreamWaitEvent");
    if (kb >= 2) HIP_LAUNCH_OK(hipStreamWaitEvent(G->s_infl, G->ev_parsed[slot], 0), "hipStreamWaitEvent");     // the buffer's previous batch has been parsed
    if (G->idx.active) {    // (behind ev_parsed of batch kb - 2, whose k_bam_index read the copies; in front of ev_infl, which this batch's parse waits for)
        HIP_LAUNCH_OK(hipMemcpyAsync(G->idx.kept_desc[slot], G->d_desc[slot], (size_t)bi.n_blocks * sizeof(BlockDesc), hipMemcpyDeviceToDevice, G->s_infl), "hipMemcpyAsync");
        HIP_LAUNCH_OK(hipMemcpyAsync(G->idx.kept_boff[slot], G->idx.boff[slot], (size_t)bi.n_blocks * 4, hipMemcpyDeviceToDevice, G->s_infl), "hipMemcpyAsync");
    }
    const int grid = (bi.n_blocks + INFL_WAVES - 1) / INFL_WAVES;
    hipLaunchKernelGGL(k_bgzf_inflate<0>, dim3(grid), dim3(INFL_WAVES * WAVE), 0, G->s_infl, G->d_comp[slot], G->d_desc[slot], bi.n_blocks,
                       G->d_infl[slot] + CARRY_CAP, G->d_status[slot]);
    HIP_LAUNCH_OK(hipGetLastError(), "k_bgzf_inflate");
    HIP_LAUNCH_OK(hipEventRecord(G->ev_infl[slot], G->s_infl), "hipEventRecord");
    // checksums of the inflated blocks (as htslib's bgzf_read_block): a mismatch becomes the block's status.  On a stream of its own,
    // behind this batch's inflate and beside the next one's (the inflate is bound by scalar issue, the checksum by memory and
    // LDS: they overlap well).  The batch slot's block table, CRCs and status words are free again when ev_crc fires: the
    // feeder waits for it before it re-stages the slot, the caller before it reads the status words.
    HIP_LAUNCH_OK(hipStreamWaitEvent(G->s_crc, G->ev_infl[slot], 0), "hipStreamWaitEvent");
    hipLaunchKernelGGL(k_bgzf_crc, dim3((unsigned)bi.n_blocks), dim3(WAVE), 0, G->s_crc, G->d_infl[slot] + CARRY_CAP, G->d_desc[slot], G->d_crc[slot],
                       bi.n_blocks, G->d_status[slot]);
    HIP_LAUNCH_OK(hipGetLastError(), "k_bgzf_crc");
    HIP_LAUNCH_OK(hipEventRecord(G->ev_crc[slot], G->s_crc), "hipEventRecord");
    {
        std::lock_guard<std::mutex> lk(G->m);
        G->inflate_launched = kb + 1;
    }
    G->cv.notify_all();
    return true;
}

// wait until batch kb has been staged; false = there is no such batch (or the feeder failed: G->error set)
bool wait_staged(GpuDecoder *G, int kb, BatchInfo *bi) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(G->m);
    G->cv.wait(lk, [&] { return (int)G->staged.size() > kb || G->feeder_done; });
    G->t_wait_staged += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!G->feeder_error.empty()) { G->error = G->feeder_error; return false; }
    if ((int)G->staged.size() <= kb) return false;
    *bi = G->staged[(size_t)kb];
    return true;
}

const char *rec_error_text(int e) {
    switch (e) {
        case REC_ERR_SHORT: return "record shorter than its fixed fields";
        case REC_ERR_FIELDS: return "record fields overrun the record";
        case REC_ERR_TAG_B: return "truncated B tag";
        case REC_ERR_TAG_TYPE: return "unknown tag type";
        case REC_ERR_TAG_OVERRUN: return "tag overruns the record";
    }
    return "malformed record";
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int coral_bamgpu_open_request(const char *path, int32_t n_threads, int64_t batch_bytes, const coral_bam_request_t *req, void **handle,
                                         int64_t *workspace_bytes) {
    return coral_bamgpu_open_request_ordered(path, n_threads, batch_bytes, req, READS_ORDER_FILE, handle, workspace_bytes);
}

extern "C" int coral_bamgpu_open_request_ordered(const char *path, int32_t n_threads, int64_t batch_bytes, const coral_bam_request_t *req,
                                                 int32_t reads_order, void **handle, int64_t *workspace_bytes) {
    if (!path || !handle || !workspace_bytes) return CORAL_ERR_ARG;
    std::unique_ptr<GpuDecoder> G(new GpuDecoder());
    G->t_start = std::chrono::steady_clock::now();
    std::string err;
    if (!parse_request(req, G->req, err) || !set_reads_order(G->req, reads_order, err)) { set_error(err); return CORAL_ERR_ARG; }
    const Request &R = G->req;
    const int32_t rank = R.rank, world = R.world;
    if (!G->f.open(path, G->error) || !read_bam_header(G->f, G->D, G->ref_id, &G->hdr_bytes)) {
        set_error(G->error.empty() ? G->D.error : G->error);
        return CORAL_ERR_FORMAT;
    }
    if (!spans_inside_file(R, G->f.size, err)) { set_error(err); return CORAL_ERR_ARG; }
    G->n_threads = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads);
    G->last_rank = rank == world - 1;
    G->byte_lo = rank == 0 ? 0 : G->f.size / (uint64_t)world * (uint64_t)rank;
    G->byte_hi = G->last_rank ? G->f.size : G->f.size / (uint64_t)world * (uint64_t)(rank + 1);
    G->first_block = 0;
    if (rank > 0 && !find_block(G->f, G->byte_lo, &G->first_block)) G->first_block = G->f.size;
    if (G->first_block >= G->byte_hi) G->first_block = G->f.size;          // no block starts in this range: nothing to do
    G->searching = rank > 0;
    if (R.span_mode) {                         // the records that start inside the spans, nothing else: only the spans' BGZF blocks
        uint64_t span_bytes = 0;               // (and what their last records straddle into) are read, uploaded and inflated
        G->last_rank = false;
        for (const Span &sp : R.spans) {
            SpanDef S;
            S.first_block = sp.beg >> 16; S.start_off = (uint32_t)(sp.beg & 0xffff);
            S.end_block = sp.end >> 16; S.end_off = (uint32_t)(sp.end & 0xffff);
            span_bytes = std::max(span_bytes, S.end_block - S.first_block + 65536 + (uint64_t)OVERHANG_BLOCKS * 65536 / 4);
            G->spans.push_back(S);
        }
        G->span_verdict.assign(G->spans.size(), 0);
        G->first_block = G->byte_lo = 0;
        G->byte_hi = span_bytes;
        if (G->spans.empty()) G->first_block = G->f.size;
    }
    G->cov.active = R.has_cov;
    G->cov.T = &G->req.cov;
    if ((G->idx.active = R.want_index)) G->D.idx.init(G->D.ref_lens);
    if ((G->qc.active = R.want_qc)) G->D.qc.init();
    G->reads.active = R.reads.on;
    G->reads.R = &G->req.reads;
    if (R.depth_bin > 0) {                     // the rule that needs the header: at most 2^28 bins (refused here, nothing allocated)
        if (!G->D.depth.init(R.depth_bin, R.depth_min_mapq, R.depth_exclude_flags, R.depth_count_deletions, G->D.ref_lens, err)) { set_error(err); return CORAL_ERR_ARG; }
        G->depth.active = true;
    }
    // batch size: at most `batch_bytes` inflated, no more than the range can need.  Default 2.52 GiB = 6 x 6 912 BGZF blocks of
    // 65 280 bytes (htslib's block size): the inflate kernel keeps 27 one-wave workgroups per CU x 256 CUs resident, blocks of
    // equal size finish in rounds, and a batch that is a whole number of rounds has no part-filled last round; bigger batches
    // also mean fewer of them (1 GiB batches: 1.31 s for the 2 M-read file, 2.4 GiB ones: 1.13 s with the same kernel).  Offsets
    // inside a batch are 32-bit: CARRY_CAP + the batch must stay below 4 GiB.
    const uint64_t range = G->byte_hi > G->first_block ? G->byte_hi - G->first_block : 0;
    uint64_t cap = batch_bytes > 0 ? (uint64_t)batch_bytes : 6ull * 6912ull * 65280ull;
    if (cap > (3ull << 30) + (512ull << 20)) cap = (3ull << 30) + (512ull << 20);
    cap = std::min<uint64_t>(cap, std::max<uint64_t>(16ull << 20, (range * 6 + (64ull << 20) + 0xffff) & ~0xffffull));
    G->infl_cap = (size_t)std::max<uint64_t>(cap, 1ull << 20);
    G->comp_cap = std::max<size_t>(G->infl_cap / 2, 1u << 20);
    G->max_blocks = G->comp_cap / 28 < (1u << 22) ? std::max<size_t>(G->comp_cap / 28, 64) : (1u << 22);   // a block is >= 28 bytes
    if (G->max_blocks > G->infl_cap / 256 + 65536) G->max_blocks = G->infl_cap / 256 + 65536;
    G->rec_cap = ((size_t)CARRY_CAP + G->infl_cap) / 36 + 2;
    G->nseg_cap = ((size_t)CARRY_CAP + G->infl_cap) / (size_t)SEG_BYTES + 4;
    size_t tmp = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (long long *)nullptr, (long long *)nullptr, (int)std::min<size_t>(G->rec_cap + 1, 0x7fffffff));
    G->scan_tmp_bytes = tmp + 256;
    if (G->reads.ordered()) {                  // the sort's temporary storage, queried once for the largest batch, as the scan's is
        hipcub::DoubleBuffer<unsigned long long> keys(nullptr, nullptr);
        hipcub::DoubleBuffer<uint32_t> ords(nullptr, nullptr);
        size_t sort_tmp = 0;
        if (hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, keys, ords, (int)std::min<size_t>(G->rec_cap + 1, 0x7fffffff), 0, 64) != hipSuccess) {
            set_error("coral_bamgpu_open_request_ordered: the size of the sort's temporary storage could not be queried");
            return CORAL_ERR_HIP;
        }
        G->reads.sort_tmp_bytes = sort_tmp + 256;
    }
    carve(G.get(), nullptr, 0);
    if (const char *fb = getenv("CORAL_BAMGPU_FIRST_BATCH")) G->first_batch = std::max<uint64_t>(1u << 20, strtoull(fb, nullptr, 10));      // tuning
    G->known_start = CARRY_CAP + (long long)(rank == 0 ? G->hdr_bytes : 0);
    *workspace_bytes = (int64_t)G->ws_bytes;
    *handle = G.release();
    return CORAL_OK;
}

extern "C" int coral_bamgpu_open(const char *path, int32_t n_threads, int32_t rank, int32_t world, int64_t batch_bytes, void **handle,
                                 int64_t *workspace_bytes) {
    const coral_bam_request_t q = range_request(rank, world);
    return coral_bamgpu_open_request(path, n_threads, batch_bytes, &q, handle, workspace_bytes);
}

// Once every batch has been emitted: waits for `stream_` and leaves what was requested in the host-side result
// (coral_bamgpu_host -> coral_bam_coverage_result, coral_bam_index_sizes / _fill, coral_bam_qc_sizes / _fill,
// coral_bam_depth_sizes / _fill, coral_bam_reads_sizes / _fill).
extern "C" int coral_bamgpu_finish(void *handle, void *stream_) {
    GpuDecoder *G = (GpuDecoder *)handle;
    if (!G) return CORAL_ERR_ARG;
    if (!G->finished || G->have_cur) { set_error("coral_bamgpu_finish: the decode is not finished"); return CORAL_ERR_ARG; }
    if (!G->cov.active && !G->qc.active && !G->idx.active && !G->depth.active && !G->reads.active) return CORAL_OK;
    if (hipStreamSynchronize((hipStream_t)stream_) != hipSuccess || !G->cov.finish(G->D) || !G->idx.finish(G->D.idx) || !G->qc.finish(G->D.qc) ||
        !G->depth.finish(G->D.depth) || !G->reads.finish(G->D, G->n_threads)) {
        set_error("coral_bamgpu_finish: copy of the requested results failed");
        return CORAL_ERR_HIP;
    }
    if (G->D.idx.unsorted) { set_error("the records are not in coordinate order: no index can be built"); return CORAL_ERR_FORMAT; }
    return CORAL_OK;
}

extern "C" int coral_bamgpu_start(void *handle, void *workspace, int64_t workspace_bytes) {
    GpuDecoder *G = (GpuDecoder *)handle;
    if (!G || !workspace || workspace_bytes < (int64_t)G->ws_bytes || (((uintptr_t)workspace) & 255)) return CORAL_ERR_ARG;
    auto bad = [&](const char *what, hipError_t e) {
        set_error(std::string(what) + ": " + hipGetErrorString(e));
        return CORAL_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipGetDevice(&G->device)) != hipSuccess) return bad("hipGetDevice", e);
    carve(G, workspace, (size_t)workspace_bytes);
    const auto t_alloc0 = std::chrono::steady_clock::now();
    for (int i = 0; i < N_STAGE; ++i) {
        if ((e = hipHostMalloc((void **)&G->h_stage[i], STAGE_BYTES, hipHostMallocDefault)) != hipSuccess) return bad("hipHostMalloc", e);
        if ((e = hipEventCreateWithFlags(&G->ev_stage[i], hipEventDisableTiming)) != hipSuccess) return bad("hipEventCreate", e);
    }
    for (int i = 0; i < 2; ++i) {
        if ((e = hipHostMalloc((void **)&G->h_desc[i], up256(G->max_blocks * (sizeof(BlockDesc) + 8)), hipHostMallocDefault)) != hipSuccess) return bad("hipHostMalloc", e);
        if ((e = hipEventCreateWithFlags(&G->ev_h2d[i], hipEventDisableTiming)) != hipSuccess) return bad("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&G->ev_infl[i], hipEventDisableTiming)) != hipSuccess) return bad("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&G->ev_crc[i], hipEventDisableTiming)) != hipSuccess) return bad("hipEventCreate", e);
        if ((e = hipEventCreateWithFlags(&G->ev_parsed[i], hipEventDisableTiming)) != hipSuccess) return bad("hipEventCreate", e);
    }
    if ((e = hipStreamCreateWithFlags(&G->s_copy, hipStreamNonBlocking)) != hipSuccess) return bad("hipStreamCreate", e);
    {   // the inflate stream gets the LOWEST priority: when a batch's inflate ends, the parse kernels of that batch (caller's
        // stream) and the next batch's inflate become runnable at the same moment; an inflate launch fills every CU with waves
        // that run for milliseconds, and the record-start search behind it took 26 ms instead of 1.2 ms (rocprofv3 timeline)
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
        if ((e = hipStreamCreateWithPriority(&G->s_infl, hipStreamNonBlocking, least)) != hipSuccess) return bad("hipStreamCreate", e);
    }
    if ((e = hipStreamCreateWithFlags(&G->s_crc, hipStreamNonBlocking)) != hipSuccess) return bad("hipStreamCreate", e);
    G->t_alloc = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_alloc0).count();
    const char *what;
    if ((what = G->idx.start(G->D.idx, e)) || (what = G->qc.start(e)) || (what = G->cov.start(e)) || (what = G->depth.start(G->D.depth, e)) || (what = G->reads.start(e))) return bad(what, e);
    G->feeder = std::thread(feeder_main, G);
    G->worker = std::thread(worker_main, G);
    return CORAL_OK;
}

// Parse the next batch up to the sizes of what it contributes.  out: [0] records, [1] padded CIGAR ops, [2] 1 = a batch was
// parsed (call coral_bamgpu_emit next), 0 = the file is done.
extern "C" int coral_bamgpu_next(void *handle, int64_t out[4], void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GpuDecoder *G = (GpuDecoder *)handle;
    if (!G || !out) return CORAL_ERR_ARG;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (G->have_cur) { set_error("coral_bamgpu_next: the previous batch has not been emitted"); return CORAL_ERR_ARG; }
    auto fail = [&](int code) {
        set_error(G->error);
        return code;
    };
    if (G->finished) return CORAL_OK;
    BatchInfo bi;
    for (;;) {
        if (!wait_staged(G, G->k, &bi)) {
            if (!G->error.empty()) return fail(CORAL_ERR_FORMAT);
            if (G->carry_len > 0 && !G->searching) { G->error = G->last_rank ? "truncated record at the end of the file" : "a record straddles further than the supported overhang"; return fail(CORAL_ERR_FORMAT); }
            G->finished = true;
            return CORAL_OK;
        }
        {   // the feeder enqueues the inflate of a batch right after staging it
            const int kw = G->k;
            std::unique_lock<std::mutex> lk(G->m);
            G->cv.wait(lk, [&] { return G->inflate_launched > kw || !G->feeder_error.empty(); });
            if (G->inflate_launched <= kw) { G->error = G->feeder_error; return fail(CORAL_ERR_HIP); }
        }
        if (!G->req.span_mode || bi.span >= G->cur_span) break;
        // a batch of overhang blocks behind a span whose last record has been seen already: nothing to parse, the slot is free
        // again once its inflate has run
        const int sl = G->k & 1;
        if (hipStreamWaitEvent(stream, G->ev_infl[sl], 0) != hipSuccess || hipEventRecord(G->ev_parsed[sl], stream) != hipSuccess) {
            G->error = "hipEventRecord failed";
            return fail(CORAL_ERR_HIP);
        }
        {
            std::lock_guard<std::mutex> lk(G->m);
            ++G->emitted;
        }
        G->cv.notify_all();
        ++G->k;
    }
    if (G->req.span_mode) {
        if (bi.span > G->cur_span) {             // the span in front ran out of blocks without reaching its end
            if (G->carry_len > 0) { G->error = "a record straddles further than the supported overhang"; return fail(CORAL_ERR_FORMAT); }
            G->cur_span = bi.span;
        }
        if (bi.span_first) {                     // the span's first record: at a known place, nothing carried, nothing searched
            G->known_start = CARRY_CAP + (long long)bi.start_off;
            G->carry_len = 0;
            G->searching = false;
        }
    }
    const int kb = G->k, slot = kb & 1;
    uint8_t *buf = G->d_infl[slot];
    // this batch's inflate must be complete before the parse kernels read its bytes
    if (hipStreamWaitEvent(stream, G->ev_infl[slot], 0) != hipSuccess) { G->error = "hipStreamWaitEvent failed"; return fail(CORAL_ERR_HIP); }
    const long long data_end = CARRY_CAP + (long long)bi.infl_bytes;
    const long long begin = G->searching ? (long long)CARRY_CAP - G->carry_len : std::min(G->known_start, data_end);
    const long long limit = (G->last_rank || !bi.has_limit) ? (1ll << 62) : (long long)CARRY_CAP + bi.limit_rel;
    const int seg0 = (int)(begin / SEG_BYTES);
    const int n_seg = (int)((data_end + SEG_BYTES - 1) / SEG_BYTES) - seg0;
    const int n_ref = (int)G->D.ref_names.size();
    long long res[6] = {0, 0, 0, 0, 0, 0};
    if (n_seg > 0) {
        hipLaunchKernelGGL(k_bam_find, dim3(n_seg), dim3(WAVE), 0, stream, buf, begin, data_end, limit, n_ref, seg0, n_seg, G->d_seg_first,
                           G->d_seg_land, G->d_seg_count, G->d_seg_valid);
        hipLaunchKernelGGL(k_bam_verify, dim3(1), dim3(WAVE), 0, stream, buf, G->searching ? -1ll : G->known_start, begin, data_end, limit, seg0, n_seg,
                           G->d_seg_first, G->d_seg_land, G->d_seg_count, G->d_seg_valid, G->d_seg_base, G->d_result);
    }
    int32_t status_bad = 0;
    if (n_seg > 0) {
        const auto t_gpu0 = std::chrono::steady_clock::now();
        const bool synced = hipMemcpyAsync(res, G->d_result, sizeof(res), hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
        G->t_wait_gpu += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_gpu0).count();
        if (!synced) {
            G->error = std::string("record walk failed: ") + hipGetErrorString(hipGetLastError());
            return fail(CORAL_ERR_HIP);
        }
    } else {
        res[1] = G->known_start;
        if (hipStreamSynchronize(stream) != hipSuccess) { G->error = "hipStreamSynchronize failed"; return fail(CORAL_ERR_HIP); }
    }
    {   // every block of the batch must have inflated cleanly and have the checksum of its trailer
        if (hipEventSynchronize(G->ev_crc[slot]) != hipSuccess) { G->error = "hipEventSynchronize failed"; return fail(CORAL_ERR_HIP); }
        std::vector<int32_t> st((size_t)bi.n_blocks);
        if (hipMemcpy(st.data(), G->d_status[slot], st.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { G->error = "hipMemcpy failed"; return fail(CORAL_ERR_HIP); }
        for (int32_t s : st) if (s != 0) { status_bad = s; break; }
        if (status_bad == ERR_CRC) { G->error = "CRC32 of an inflated BGZF block differs from the one in its trailer"; return fail(CORAL_ERR_FORMAT); }
        if (status_bad) { G->error = "inflate failed (corrupt BGZF block), code " + std::to_string(status_bad); return fail(CORAL_ERR_FORMAT); }
    }
    if (res[3] == 1) { G->error = "record shorter than its fixed fields"; return fail(CORAL_ERR_FORMAT); }
    bool still_searching = false;
    if (res[3] == 2) {
        // no confirmed record start in what this byte range has seen so far (the chained check needs three records in a row): keep
        // the bytes and look again with the next batch behind them, as the host pipeline does; at the end of the range it simply
        // has no record of its own (it lies inside one record of the previous range)
        if (data_end - begin > CARRY_CAP) { G->error = "no record start found in 64 MiB at the beginning of the byte range"; return fail(CORAL_ERR_FORMAT); }
        res[0] = 0;
        res[1] = bi.last ? data_end : begin;
        res[2] = 0;
        still_searching = !bi.last;
    }
    long long n_rec = res[0];
    const long long carry_pos = res[1];
    if (G->idx.active && G->searching && n_rec > 0 && res[5] < CARRY_CAP) {
        // (a byte range that found no record start in its first batch and finds one in the bytes kept from it)
        G->error = "index request: the first record of the byte range does not start in the batch it was found in";
        return fail(CORAL_ERR_FORMAT);
    }
    G->cur_carry_pos = carry_pos < data_end ? carry_pos : data_end;
    G->fixups += res[4];
    if (n_rec > (long long)G->rec_cap) { G->error = "more records in a batch than its workspace holds"; return fail(CORAL_ERR_FORMAT); }
    G->searching = still_searching;
    G->cur = bi;
    G->cur_n_rec = n_rec;
    G->cur_ops = G->cur_name_bytes = G->cur_sa_bytes = 0;
    if (n_rec > 0) {
        hipLaunchKernelGGL(k_bam_starts, dim3((n_seg + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, buf, seg0, n_seg, G->d_seg_first, G->d_seg_count, G->d_seg_valid,
                           G->d_seg_base, G->d_rec_all);
        (void)hipMemsetAsync(G->d_error, 0, 4, stream);
    }
    if (n_rec > 0 && G->req.keep.active()) {
        // The record filter: from here on the batch's records are the kept ones.  Everything above (carry_pos, done, the span
        // verdicts: byte positions of the walk) has not seen and does not see the kept count.  The flags and their offsets borrow
        // two arrays k_bam_meta and the scans behind it refill (M.pad_ops, d_cig_off); the kept count comes back on its own
        // (8 bytes + the error word): k_bam_meta's launch and the three scans are sized by it.
        long long *keep = G->M.pad_ops, *keep_off = G->d_cig_off;
        const unsigned grid = (unsigned)((n_rec + 1 + WAVE - 1) / WAVE);
        hipLaunchKernelGGL(k_bam_keep, dim3(grid), dim3(WAVE), 0, stream, buf, G->d_rec_all, n_rec, G->req.keep, keep, G->d_error);
        (void)G->scan(stream, keep, keep_off);                   // (over cur_n_rec + 1 = every record of the walk + the extra slot)
        hipLaunchKernelGGL(k_bam_keep_compact, dim3(grid), dim3(WAVE), 0, stream, G->d_rec_all, n_rec, keep, keep_off, G->d_rec_start);
        long long n_kept = 0;
        int32_t rec_err = 0;
        if (hipMemcpyAsync(&n_kept, keep_off + n_rec, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(&rec_err, G->d_error, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            G->error = std::string("record filter failed: ") + hipGetErrorString(hipGetLastError());
            return fail(CORAL_ERR_HIP);
        }
        if (rec_err) { G->error = rec_error_text(rec_err); return fail(CORAL_ERR_FORMAT); }
        if (n_kept < 0 || n_kept > n_rec) { G->error = "record filter: the kept count is out of range"; return fail(CORAL_ERR_HIP); }
        n_rec = n_kept;
        G->cur_n_rec = n_rec;
    }
    if (n_rec > 0) {
        const long long waves = n_rec + 1;
        hipLaunchKernelGGL(k_bam_meta, dim3((unsigned)waves), dim3(WAVE), 0, stream, buf, G->d_rec_start, n_rec, G->M, G->d_error);
        (void)G->scan(stream, G->M.pad_ops, G->d_cig_off);
        (void)G->scan(stream, G->M.name_len, G->d_name_off);
        (void)G->scan(stream, G->M.sa_len, G->d_sa_off);
        long long totals[3] = {0, 0, 0};
        int32_t rec_err = 0;
        if (hipMemcpyAsync(&totals[0], G->d_cig_off + n_rec, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(&totals[1], G->d_name_off + n_rec, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(&totals[2], G->d_sa_off + n_rec, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(&rec_err, G->d_error, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            G->error = std::string("record parse failed: ") + hipGetErrorString(hipGetLastError());
            return fail(CORAL_ERR_HIP);
        }
        if (rec_err) { G->error = rec_error_text(rec_err); return fail(CORAL_ERR_FORMAT); }
        G->cur_ops = totals[0];
        G->cur_name_bytes = totals[1];
        G->cur_sa_bytes = totals[2];
    }
    // what the next batch starts with
    const bool done = res[2] != 0;
    // (a span decode goes on with the next span)
    auto verdict = [&](int v) {
        if (!G->req.span_mode) return;
        {
            std::lock_guard<std::mutex> lk(G->m);
            if (G->span_verdict[(size_t)bi.span] == 0) G->span_verdict[(size_t)bi.span] = v;
        }
        G->cv.notify_all();
    };
    auto range_done = [&]() {
        G->carry_len = 0;
        verdict(1);
        if (G->req.span_mode && G->cur_span + 1 < (int)G->spans.size()) ++G->cur_span; else G->finished = true;
    };
    if (done) {
        range_done();
    } else if (carry_pos < data_end) {
        G->carry_len = data_end - carry_pos;
        if (G->carry_len > CARRY_CAP) { G->error = "a record larger than 64 MiB straddles two batches"; return fail(CORAL_ERR_FORMAT); }
        G->known_start = CARRY_CAP - G->carry_len;
    } else {
        G->carry_len = 0;
        G->known_start = CARRY_CAP + (carry_pos - data_end);
    }
    if (bi.last && !done) {
        if (G->carry_len > 0) { G->error = G->last_rank ? "truncated record at the end of the file" : "a record straddles further than the supported overhang"; return fail(CORAL_ERR_FORMAT); }
        range_done();
    }
    if (bi.span_tail && !done) verdict(2);       // the feeder stages what lies behind the span's own blocks
    G->have_cur = true;
    ++G->n_batches;
    out[0] = n_rec;
    out[1] = G->cur_ops;
    out[2] = 1;
    return CORAL_OK;
}

// Write the batch's CIGAR ops (padded SoA, `cigar_dst` device pointer with room for out[1] of coral_bamgpu_next words) and,
// if wanted, the batch-local op offsets (`cigar_off_dst`, device, n_rec + 1 int64; may be NULL — the offsets over the whole
// file are part of the host-side result), and take the batch's host-side fields in.
extern "C" int coral_bamgpu_emit(void *handle, uint32_t *cigar_dst, int64_t *cigar_off_dst, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GpuDecoder *G = (GpuDecoder *)handle;
    if (!G || !G->have_cur) return CORAL_ERR_ARG;
    auto fail = [&](int code, const std::string &msg) {
        set_error(msg);
        return code;
    };
    const int kb = G->k, slot = kb & 1;
    uint8_t *buf = G->d_infl[slot];
    const long long n = G->cur_n_rec;
    Decoded &D = G->D;
    if (n > 0) {
        if (G->cur_ops > 0 && !cigar_dst) return CORAL_ERR_ARG;
        (void)hipMemsetAsync(G->d_na_count, 0, 4, stream);
        hipLaunchKernelGGL(k_bam_emit, dim3((unsigned)n), dim3(WAVE), 0, stream, buf, G->d_rec_start, n, G->M, G->d_cig_off, G->d_name_off,
                           G->d_sa_off, cigar_dst, G->d_end, G->d_qlen, G->d_names, G->d_sa_text, G->d_na_list, G->d_na_count);
        if (cigar_off_dst && hipMemcpyAsync(cigar_off_dst, G->d_cig_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return fail(CORAL_ERR_HIP, "device copy of the op offsets failed");
    }
    // the head of a straddling record moves in front of the next batch's bytes (same stream: after the kernels above)
    if (G->carry_len > 0 && !G->finished) {
        const long long data_end = CARRY_CAP + (long long)G->cur.infl_bytes;
        if (hipMemcpyAsync(G->d_infl[slot ^ 1] + CARRY_CAP - G->carry_len, buf + data_end - G->carry_len, (size_t)G->carry_len, hipMemcpyDeviceToDevice,
                           stream) != hipSuccess)
            return fail(CORAL_ERR_HIP, "device copy of the carried bytes failed");
    }
    if (n > 0) {
        std::unique_ptr<HostJob> job(new HostJob());
        HostJob &J = *job;
        const size_t base = D.tid.size();
        J.base = base;
        J.n = n;
        auto grow = [&](std::vector<int32_t> &v) { v.resize(base + (size_t)n); return v.data() + base; };
        int32_t *tid = grow(D.tid), *pos = grow(D.pos), *end = grow(D.end), *flag = grow(D.flag), *mapq = grow(D.mapq), *qlen = grow(D.qlen),
                *has_seq = grow(D.has_seq), *nm = grow(D.nm), *n_cigar = grow(D.n_cigar);
        J.pad.resize((size_t)n);
        J.name_off.resize((size_t)n + 1);
        J.sa_off.resize((size_t)n + 1);
        J.names.resize((size_t)G->cur_name_bytes);
        J.sa_text.resize((size_t)G->cur_sa_bytes);
        int32_t na_count = 0;
        auto get = [&](void *dst, const void *src, size_t bytes) { return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess; };
        const size_t n4 = (size_t)n * 4;
        const auto t_gpu0 = std::chrono::steady_clock::now();
        bool ok = get(tid, G->M.tid, n4) && get(pos, G->M.pos, n4) && get(end, G->d_end, n4) && get(flag, G->M.flag, n4) && get(mapq, G->M.mapq, n4) &&
                  get(qlen, G->d_qlen, n4) && get(has_seq, G->M.l_seq, n4) && get(nm, G->M.nm, n4) && get(n_cigar, G->M.n_cigar, n4) &&
                  get(J.pad.data(), G->M.pad_ops, (size_t)n * 8) && get(J.name_off.data(), G->d_name_off, (size_t)(n + 1) * 8) &&
                  get(J.sa_off.data(), G->d_sa_off, (size_t)(n + 1) * 8) && get(J.names.data(), G->d_names, J.names.size()) &&
                  get(J.sa_text.data(), G->d_sa_text, J.sa_text.size()) && get(&na_count, G->d_na_count, 4);
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) return fail(CORAL_ERR_HIP, std::string("copy of the batch's host fields failed: ") + hipGetErrorString(hipGetLastError()));
        G->t_wait_gpu += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_gpu0).count();
        if (!G->qc.collect(D.qc.qual_sum)) return fail(CORAL_ERR_HIP, "copy of the read-QC rows failed");      // (of the batch in front)
        for (long long i = 0; i < n; ++i) has_seq[i] = has_seq[i] > 0 ? 1 : 0;       // (arrived as l_seq)
        if (G->idx.active) {                              // the batch's first record against the last one of the batch in front (inside a batch: k_bam_index)
            D.idx.note_order(IndexPartial::sort_word(tid[0], pos[0]), IndexPartial::sort_word(tid[n - 1], pos[n - 1]));
            D.idx.n_rec += n;
        }
        if (na_count > 0) {
            // the records with a non-ACGT code, whole, in one gather + one copy (the offset arrays of the scans are free by now)
            J.na_list.resize((size_t)na_count);
            std::vector<long long> starts((size_t)n);
            if (hipMemcpy(J.na_list.data(), G->d_na_list, (size_t)na_count * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(starts.data(), G->d_rec_start, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(CORAL_ERR_HIP, "copy of the non-ACGT list failed");
            std::sort(J.na_list.begin(), J.na_list.end());
            // a record ends where the next one starts - unless a record filter dropped that one: then its block_size says where
            std::vector<uint32_t> own_size;
            if (G->req.keep.active()) {
                own_size.resize((size_t)na_count);
                for (int32_t j = 0; j < na_count; ++j)
                    if (hipMemcpy(&own_size[(size_t)j], buf + starts[(size_t)J.na_list[(size_t)j]], 4, hipMemcpyDeviceToHost) != hipSuccess)
                        return fail(CORAL_ERR_HIP, "copy of the non-ACGT list failed");
            }
            std::vector<long long> src((size_t)na_count), dst((size_t)na_count), len((size_t)na_count);
            J.na_off.assign((size_t)na_count + 1, 0);
            for (int32_t j = 0; j < na_count; ++j) {
                const int32_t li = J.na_list[(size_t)j];
                const long long rec_end = !own_size.empty() ? starts[(size_t)li] + 4 + (long long)own_size[(size_t)j]
                                          : li + 1 < n ? starts[(size_t)li + 1] : G->cur_carry_pos;
                src[(size_t)j] = starts[(size_t)li] + 4;
                len[(size_t)j] = rec_end - starts[(size_t)li] - 4;
                dst[(size_t)j] = J.na_off[(size_t)j];
                J.na_off[(size_t)j + 1] = J.na_off[(size_t)j] + len[(size_t)j];
            }
            const long long total = J.na_off[(size_t)na_count];
            J.na_raw.resize((size_t)total);
            if ((size_t)total > G->names_cap) return fail(CORAL_ERR_FORMAT, "records with non-ACGT bases exceed the batch workspace");
            if (hipMemcpy(G->d_cig_off, src.data(), (size_t)na_count * 8, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(G->d_name_off, dst.data(), (size_t)na_count * 8, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(G->d_sa_off, len.data(), (size_t)na_count * 8, hipMemcpyHostToDevice) != hipSuccess)
                return fail(CORAL_ERR_HIP, "upload of the non-ACGT gather list failed");
            hipLaunchKernelGGL(k_bam_gather, dim3((unsigned)na_count), dim3(WAVE), 0, stream, buf, G->d_cig_off, G->d_name_off, G->d_sa_off, (int)na_count,
                               G->d_names);
            if (hipMemcpyAsync(J.na_raw.data(), G->d_names, (size_t)total, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
                return fail(CORAL_ERR_HIP, "copy of the records with non-ACGT bases failed");
            G->na_records += na_count;
        }
        {
            std::lock_guard<std::mutex> lk(G->wm);
            G->jobs.push_back(std::move(job));
        }
        G->wcv.notify_all();
    } else if (hipStreamSynchronize(stream) != hipSuccess) {
        return fail(CORAL_ERR_HIP, "hipStreamSynchronize failed");
    }
    const Borrowed S{G->M.name_len, G->M.sa_len, G->M.pad_ops, G->d_cig_off, (unsigned long long *)G->d_cig_off, (unsigned long long *)G->M.sa_src, G->M.pad_ops, G->d_name_off, G->d_sa_off, G->M.cig_src};
    std::string err;
    if (!G->reads.batch(G, stream, S, err) || !G->cov.batch(G, stream, S, err) || !G->qc.batch(G, stream, S, err) || !G->depth.batch(G, stream, err) || !G->idx.batch(G, stream, S, err))
        return fail(CORAL_ERR_HIP, err);
    // this buffer may be inflated into again (batch k + 2) once everything above has run
    if (hipEventRecord(G->ev_parsed[slot], stream) != hipSuccess) return fail(CORAL_ERR_HIP, "hipEventRecord failed");
    {
        std::lock_guard<std::mutex> lk(G->m);
        ++G->emitted;
    }
    G->cv.notify_all();
    G->have_cur = false;
    ++G->k;
    if (G->finished) D.seconds = G->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - G->t_start).count();
    return CORAL_OK;
}

// The host-side half of the result as a handle for coral_bam_decode_sizes / coral_bam_decode_fill / coral_bam_decode_stats
// (cigar: pass NULL to coral_bam_decode_fill — the ops are on the device).  Owned by the GPU decoder: do not close it.
extern "C" int coral_bamgpu_host(void *handle, void **decoded) {
    GpuDecoder *G = (GpuDecoder *)handle;
    if (!G || !decoded) return CORAL_ERR_ARG;
    {   // the worker must have taken every batch in
        std::unique_lock<std::mutex> lk(G->wm);
        G->wcv.wait(lk, [&] { return G->jobs.empty() && !G->worker_busy; });
        if (!G->worker_error.empty()) {
            set_error(G->worker_error);
            return CORAL_ERR_FORMAT;
        }
    }
    G->D.seconds = G->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - G->t_start).count();
    *decoded = &G->D;
    return CORAL_OK;
}

// stats: [0] batches, [1] segments whose speculative start was replaced by the exact walk, [2] records fetched for the
// non-ACGT list, [3] batch capacity (inflated bytes); seconds: [0] total, [1] host-side field handling (worker thread),
// [2] file reads of the feeder, [3] pinned buffers / streams set-up, [4] caller waiting for the feeder, [5] caller waiting for the GPU
extern "C" int coral_bamgpu_stats(void *handle, int64_t stats[4], double seconds[6]) {
    GpuDecoder *G = (GpuDecoder *)handle;
    if (!G || !stats || !seconds) return CORAL_ERR_ARG;
    stats[0] = G->n_batches; stats[1] = G->fixups; stats[2] = G->na_records; stats[3] = (int64_t)G->infl_cap;
    seconds[0] = G->seconds; seconds[1] = G->host_seconds; seconds[2] = G->t_read; seconds[3] = G->t_alloc; seconds[4] = G->t_wait_staged;
    seconds[5] = G->t_wait_gpu;
    return CORAL_OK;
}

extern "C" int coral_bamgpu_close(void *handle) {
    delete (GpuDecoder *)handle;
    return CORAL_OK;
}

// One BGZF-style inflate launch on caller-provided buffers (tests; tools/bench_inflate.py): `desc` = n_blocks x 4 uint32
// (src_off, src_len, dst_off, isize) on the device, `comp` readable COMP_SLACK bytes beyond its last stream.
extern "C" int coral_bgzf_inflate(const uint8_t *comp, const uint32_t *desc, int32_t n_blocks, uint8_t *out, int32_t *status, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_blocks < 0 || (n_blocks > 0 && (!comp || !desc || !out || !status))) return CORAL_ERR_ARG;
    if (n_blocks == 0) return CORAL_OK;
    const dim3 grid((n_blocks + INFL_WAVES - 1) / INFL_WAVES), block(INFL_WAVES * WAVE);
#define CORAL_INFL_LAUNCH(M) hipLaunchKernelGGL(k_bgzf_inflate<M>, grid, block, 0, stream, comp, (const BlockDesc *)desc, n_blocks, out, status)
#ifdef CORAL_EXPERIMENTS
    // timing experiments (tools/bench_inflate.py with a -DCORAL_EXPERIMENTS build): variants that skip parts of the work and
    // produce wrong output by design; not compiled into the product library
    const char *ab = getenv("CORAL_INFLATE_ABLATE");
    switch (ab ? atoi(ab) : 0) {
        case 0: CORAL_INFL_LAUNCH(0); break;
        case 1: CORAL_INFL_LAUNCH(1); break;
        case 2: CORAL_INFL_LAUNCH(2); break;
        case 4: CORAL_INFL_LAUNCH(4); break;
        case 12: CORAL_INFL_LAUNCH(12); break;
        case 13: CORAL_INFL_LAUNCH(13); break;
        default: set_error("CORAL_INFLATE_ABLATE: unknown mode"); return CORAL_ERR_ARG;
    }
#else
    CORAL_INFL_LAUNCH(0);
#endif
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string("k_bgzf_inflate: ") + hipGetErrorString(e)); return CORAL_ERR_HIP; }
    return CORAL_OK;
}
