"""What the modes that stream a text file through a native session share (a reference FASTA: `kmers`: kmers.py, `composition`:
composition.py; the reads' FASTQ: `qc --fastq` and `filter`: fastq.py): the file's pieces, the GPU side of a session and the timed
loop over a ``*_feed`` entry point.  The native counterpart is coral_stream_gpu.h."""
from __future__ import annotations

import os
import time

import numpy as np

from . import _lib


def check(rc, what):
    if rc != 0:
        raise _lib.CoralHipError("%s failed (%d): %s" % (what, rc, _lib.lib().coral_bam_last_error().decode()))


def pieces(fasta, chunk_bytes):
    """The stream's pieces as (array or bytes, length), and the seconds spent reading them (a one-entry list, filled as it goes)."""
    spent = [0.0]

    def gen(fp):
        buf = np.empty(chunk_bytes, dtype=np.uint8)
        into = getattr(fp, "readinto", None)
        while True:
            t0 = time.perf_counter()
            if into is not None:
                n = into(memoryview(buf))
                piece = buf
            else:
                piece = fp.read(chunk_bytes)
                n = len(piece)
            spent[0] += time.perf_counter() - t0
            if not n:
                return
            yield piece, n

    def opened():
        if hasattr(fasta, "read"):
            yield from gen(fasta)
            return
        path = os.fspath(fasta)
        if path.endswith(".gz"):                                  # inflated by Python's gzip on the host: slow, not the hot path
            import gzip
            with gzip.open(path, "rb") as fp:
                yield from gen(fp)
        else:
            with open(path, "rb", buffering=0) as fp:
                yield from gen(fp)
    return opened(), spent


def stream_size(fasta):
    """The bytes still to come from ``fasta`` (None: not known without reading) and a function that starts it over."""
    if hasattr(fasta, "read"):
        try:
            at = fasta.tell()
            end = fasta.seek(0, os.SEEK_END)
            fasta.seek(at)
            return end - at, lambda: fasta.seek(at)
        except (OSError, AttributeError, ValueError):
            return None, None
    path = os.fspath(fasta)
    return (None if path.endswith(".gz") else os.path.getsize(path)), lambda: None


def gpu_side(dev, ws_bytes, what):
    """The GPU side of a session on the torch device ``dev``, once the caller's tables are allocated: a workspace of ``ws_bytes``
    (what ``what``, a ``*_workspace_bytes``, gave) and the current stream, synchronised -> (workspace tensor, stream)."""
    import torch
    torch.cuda.set_device(dev)
    if ws_bytes < 0:
        raise _lib.CoralHipError("%s failed (%d)" % (what, ws_bytes))
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    stream.synchronize()                                         # (the blocks may be recycled ones)
    return ws, stream


def feed_all(feed, handle, fasta, chunk_bytes):
    """Every piece of ``fasta`` through the ``*_feed`` entry point ``feed`` -> the seconds spent reading and in ``feed``."""
    it, read_s = pieces(fasta, int(chunk_bytes))
    feed_s = 0.0
    for piece, n in it:
        t0 = time.perf_counter()
        rc = feed(handle, piece.ctypes.data if isinstance(piece, np.ndarray) else piece, n)
        feed_s += time.perf_counter() - t0
        check(rc, feed.__name__)
    return read_s[0], feed_s
