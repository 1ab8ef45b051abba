"""Cost of bam.import_sam (coral_samgpu_import: k_sam_lines, k_sam_size, a scan, k_sam_encode and the record sink) against the
host's rule book on one thread (coral_sam_encode).

The input is SAM text rendered from the bench's BAM shape: `--reads` reads of the 'cfg3' configuration (20 kb reads, real QUAL,
NM and SA tags; default 3 000 reads, about 125 MB of text - a slice that is rendered in seconds; the size is in the result),
written with bam.write_bam, read back as record bytes on the host and turned into text here.  Per run of `runs`:
  text_GBps        text bytes over the wall time of import_sam, end to end (read, upload, encode, deflate, write)
  size_kernel_s    k_sam_size, from events, summed over the batches; it reads the text once
  encode_kernel_s  k_sam_encode, from events; it reads the text of the written lines and writes the record bytes
and once, as the comparison, the host core's single-thread rate on the same text.  One JSON line; the kernels' GB/s are DERIVED
from the measured times and the bytes named above.
    python tools/bench_sam_import.py [runs] [--reads N] [--batch_bytes N] [--sam PATH]"""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from coral_amd import bam, synth

ap = argparse.ArgumentParser()
ap.add_argument("runs", nargs="?", type=int, default=5)
ap.add_argument("--reads", type=int, default=3000)
ap.add_argument("--batch_bytes", type=int, default=0)
ap.add_argument("--sam", default="", help="SAM text to use instead of the rendered one")
ap.add_argument("--no-host", action="store_true", help="skip the host core's run")
args = ap.parse_args()

_TAG_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_SEQ = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
_OPS = "MIDNSHP=X"


def tags_text(raw, p, end):
    out = []
    while p < end:
        key, ty = raw[p:p + 2].decode(), chr(raw[p + 2])
        p += 3
        if ty == "A":
            out.append("%s:A:%s" % (key, chr(raw[p])))
            p += 1
        elif ty in _TAG_INT:
            out.append("%s:i:%d" % (key, struct.unpack_from(_TAG_INT[ty], raw, p)[0]))
            p += struct.calcsize(_TAG_INT[ty])
        elif ty == "f":
            out.append("%s:f:%r" % (key, float(np.float32(struct.unpack_from("<f", raw, p)[0]))))
            p += 4
        elif ty in "ZH":
            z = raw.index(b"\0", p)
            out.append("%s:%s:%s" % (key, ty, raw[p:z].decode("latin-1")))
            p = z + 1
        else:
            raise ValueError("tag type %r is not rendered here" % ty)
    return out


def render(path):
    """The BAM file `path` as SAM text (bytes)."""
    header = bam.bam_header_bytes(path)
    names = bam.bam_reference_names(path)
    rec = bam.extract_records(path, device="cpu", index=False)
    raw = rec.data.tobytes()
    pieces = [header[8:8 + struct.unpack_from("<i", header, 4)[0]]]
    for a, b in zip(rec.offsets[:-1].tolist(), rec.offsets[1:].tolist()):
        tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", raw, a + 4)
        p = a + 36
        name = raw[p:p + l_name - 1]
        p += l_name
        ops = np.frombuffer(raw, dtype="<u4", count=n_cig, offset=p)
        p += 4 * n_cig
        packed = np.frombuffer(raw, dtype=np.uint8, count=(l_seq + 1) // 2, offset=p)
        p += (l_seq + 1) // 2
        codes = np.empty(2 * len(packed), dtype=np.uint8)
        codes[0::2], codes[1::2] = packed >> 4, packed & 15
        qual = np.frombuffer(raw, dtype=np.uint8, count=l_seq, offset=p)
        p += l_seq
        cigar = "".join("%d%s" % (n, _OPS[op]) for op, n in zip((ops & 15).tolist(), (ops >> 4).tolist())) or "*"
        fields = [name, b"%d" % flag, names[tid].encode() if tid >= 0 else b"*", b"%d" % (pos + 1), b"%d" % mapq, cigar.encode(),
                  b"*" if ntid < 0 else b"=" if ntid == tid else names[ntid].encode(), b"%d" % (npos + 1), b"%d" % tlen,
                  _SEQ[codes[:l_seq]].tobytes() if l_seq else b"*", (qual + 33).astype(np.uint8).tobytes() if l_seq and qual[0] != 0xff else b"*"]
        pieces.append(b"\t".join(fields + [t.encode("latin-1") for t in tags_text(raw, p, b)]) + b"\n")
    return b"".join(pieces)


d = tempfile.mkdtemp(prefix="coral_sam_import_")
sam = args.sam or os.path.join(d, "cfg3_%d.sam" % args.reads)
if not os.path.exists(sam):
    t0 = time.perf_counter()
    rec = synth.generate(synth.scaled_config("cfg3", args.reads), "cpu")
    src = os.path.join(d, "src.bam")
    bam.write_bam(rec, src, seed=1, with_qual=True, fast_seq=True, long_cigar_as_cg=False)
    text = render(src)
    with open(sam, "wb") as fp:
        fp.write(text)
    os.remove(src)
    del text
    print("SAM text written: %.1f MB in %.1f s" % (os.path.getsize(sam) / 1e6, time.perf_counter() - t0), file=sys.stderr, flush=True)

out = os.path.join(d, "imported.bam")
runs = []
bam.import_sam(sam, out, device="cuda:0", batch_bytes=args.batch_bytes)          # (warm-up: the library, the allocator, the page cache)
for _ in range(args.runs):
    t0 = time.perf_counter()
    st = bam.import_sam(sam, out, device="cuda:0", batch_bytes=args.batch_bytes)
    wall = time.perf_counter() - t0
    runs.append(dict(bam.LAST_IMPORT, wall_s=wall, text_GBps=st.text_bytes / wall / 1e9))
med = lambda k: statistics.median(r[k] for r in runs)
res = {"tool": "bench_sam_import", "reads": args.reads if not args.sam else None, "sam_MB": round(os.path.getsize(sam) / 1e6, 1), "lines": st.lines, "records": st.records,
       "text_bytes": st.text_bytes, "record_bytes": st.bytes, "file_bytes": st.file_bytes, "batches": st.batches, "runs": args.runs,
       "workspace_MB": round(runs[-1]["workspace_bytes"] / 2 ** 20, 1), "float_fixups": runs[-1]["float_fixups"],
       "median": {"wall_s": round(med("wall_s"), 4), "text_GBps": round(med("text_GBps"), 3), "feeder_wait_s": round(med("feeder_wait_seconds"), 4),
                  "size_kernel_s": round(med("size_kernel_seconds"), 5), "encode_kernel_s": round(med("encode_kernel_seconds"), 5)}}
res["derived"] = {"size_kernel_GBps": round(st.text_bytes / med("size_kernel_seconds") / 1e9, 1),
                  "encode_kernel_GBps": round((st.text_bytes + st.bytes) / med("encode_kernel_seconds") / 1e9, 1)}
if not args.no_host:
    with open(sam, "rb") as fp:
        text = fp.read()
    H = bam._sam_header(text)
    t0 = time.perf_counter()
    data = bam.sam_encode(text[H.text_bytes:], H)[0]
    host_s = time.perf_counter() - t0
    assert len(data) == st.bytes
    res["host_core_one_thread"] = {"seconds": round(host_s, 3), "text_GBps": round(st.text_bytes / host_s / 1e9, 3)}
print(json.dumps(res))
import shutil
shutil.rmtree(d, ignore_errors=True)
