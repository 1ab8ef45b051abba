"""The one driver of the GPU BAM decoder (csrc/coral_bamgpu.hip): the sink descriptor its open call is given, and the
call sequence on the handle - open, workspace, start, next / emit per batch, finish, host, close."""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

# where a decode writes its reads request's result while it runs, instead of keeping it on the host
TextFile = collections.namedtuple("TextFile", "path")                         # FASTQ text (want_reads 1), batch by batch
BamFile = collections.namedtuple("BamFile", "path header chunk_blocks")       # records (want_reads 2) as a BAM file behind `header` (inflated bytes)
Runs = collections.namedtuple("Runs", "spill_path chunk_blocks")              # records as sorted runs, for coral_bamgpu_merge_runs


def open_handle(L, path, n_threads, batch_bytes, req, sink=None):
    """coral_bamgpu_open_request with the coral_bam_sink_t that ``sink`` (None, TextFile, BamFile, Runs) stands for -> (rc, handle,
    workspace_bytes); no GPU work.  The arguments go through as they are (a None path or header as NULL), and a refusal is
    returned, not raised: coral_bam_last_error() has its text.  A Runs sink puts ``req`` in coordinate order (the library's runs
    sink takes no other).  ``req`` must outlive the handle."""
    h, ws_bytes = C.c_void_p(), C.c_int64(0)
    fs = lambda p: None if p is None else os.fsencode(p)
    if sink is None:
        to = None
    elif isinstance(sink, TextFile):
        to = _lib.coral_bam_sink_t(_lib.SINK_TEXT, fs(sink.path))
    elif isinstance(sink, BamFile):
        head = np.frombuffer(bytes(b"" if sink.header is None else sink.header), dtype=np.uint8)       # (alive until the return; the library copies it)
        to = _lib.coral_bam_sink_t(_lib.SINK_BAM, fs(sink.path), head.ctypes.data if len(head) else None, len(head), int(sink.chunk_blocks))
    elif isinstance(sink, Runs):
        req.reads_order = 1                                      # (runs are sorted runs: what the sink means, said where the library reads it)
        to = _lib.coral_bam_sink_t(_lib.SINK_RUNS, fs(sink.spill_path), chunk_blocks=int(sink.chunk_blocks))
    else:
        raise TypeError("sink must be None, a TextFile, a BamFile or a Runs, got %r" % (sink,))
    rc = L.coral_bamgpu_open_request(path.encode(), n_threads, batch_bytes, C.byref(req), to, C.byref(h), C.byref(ws_bytes))
    return rc, h, int(ws_bytes.value)


class DecodeSession:
    """One GPU decode of ``path`` for the request ``req``, as a context manager over its handle::

        with DecodeSession(path, req, device=dev, n_threads=n, batch_bytes=b, sink=sink) as s:
            s.start()
            s.run(keep=True)        # or, step by step:  while s.next() is not None: s.emit()
            dh = s.finish()         # the host handle of the coral_bam_*_result / _sizes / _fill calls

    The rules every decode obeys, which this class alone carries out:

    1. The workspace may be a recycled block of torch's caching allocator, which is ordered only against the stream it was
       allocated on, while the decoder's threads and streams write it from ``start`` on.  So the current stream is drained once
       before ``start``, and again before a second workspace (``workspace``: the merge's) is handed out.
    2. coral_bamgpu_close drains the decoder's streams - a byte range may still be inflating batches of its overhang.  Only
       after it are the workspace tensors and the CIGAR pieces released: the session holds them until ``close``.
    3. The handle is closed exactly once, on every way out (``close`` is idempotent and runs in ``__exit__``).
    4. The request struct owns the numpy arrays its pointers name; the session keeps it for as long as the handle lives.

    A refused open raises _lib.CoralHipError and leaves nothing to close; so does every later step that fails, with the library's
    text (``error_names``: a dict code -> name that is put beside the code).  Attributes: L, h, dev, ws_bytes, and from ``start``
    on stream (the current stream's handle), pieces and words (each batch's CIGAR words, int32 on the device, and their count; with ``keep``
    False only the last batch's) and batches (batches emitted), from ``finish`` on dh."""

    def __init__(self, path, req, device="cuda:0", n_threads=1, batch_bytes=0, sink=None, L=None, error_names=None):
        self.L = _lib.lib() if L is None else L
        self.path, self.req, self.dev, self.n_threads, self.error_names = path, req, torch.device(device), int(n_threads), error_names
        self.h, self.stream, self.dh, self.pieces, self.words, self.batches, self._held = None, None, None, [], [], 0, []
        rc, h, self.ws_bytes = open_handle(self.L, path, self.n_threads, batch_bytes, req, sink)
        if rc != 0:
            raise self.fail("coral_bamgpu_open_request", rc)
        self.h = h

    # ---- the two device operations ------------------------------------------------------------------------------------------
    def _alloc(self, n: int, dtype=torch.uint8):
        return torch.empty(n, dtype=dtype, device=self.dev)

    def _drain(self):
        """Make the device current (the library works on the current one) and wait for what its current stream has queued ->
        that stream's handle."""
        torch.cuda.set_device(self.dev)
        stream = torch.cuda.current_stream(self.dev)
        stream.synchronize()
        return stream.cuda_stream

    # ---- the sequence ---------------------------------------------------------------------------------------------------------
    def fail(self, what: str, rc: int) -> _lib.CoralHipError:
        code = "%d" % rc if self.error_names is None else "%d, %s" % (rc, self.error_names.get(rc, "?"))
        return _lib.CoralHipError("%s(%s) failed (%s): %s" % (what, self.path, code, self.L.coral_bam_last_error().decode()))

    def _check(self, what: str, rc: int):
        if rc != 0:
            raise self.fail(what, rc)

    def workspace(self, nbytes: int) -> int:
        """A device block of ``nbytes`` that lives until ``close`` -> its 256-aligned base, handed out behind a drain (rule 1)."""
        self._held.append(self._alloc(int(nbytes) + 256))
        self.stream = self._drain()
        return (self._held[-1].data_ptr() + 255) & ~255

    def start(self):
        self._check("coral_bamgpu_start", self.L.coral_bamgpu_start(self.h, self.workspace(self.ws_bytes), self.ws_bytes))

    def next(self):
        """Parse the next batch -> (records, CIGAR words) - ``emit`` is due -, or None behind the last one."""
        out = (C.c_int64 * 4)()
        self._check("coral_bamgpu_next", self.L.coral_bamgpu_next(self.h, out, self.stream))
        self._words = int(out[1])
        return (int(out[0]), self._words) if out[2] else None

    def emit(self, keep: bool = True):
        """Take the parsed batch in -> its CIGAR words, a device tensor of the session's (``keep`` False: until the next ``emit``)."""
        if not keep:
            self.pieces.clear()
            self.words.clear()
        self.pieces.append(self._alloc(max(self._words, 1), torch.int32))
        self.words.append(self._words)
        self._check("coral_bamgpu_emit", self.L.coral_bamgpu_emit(self.h, self.pieces[-1].data_ptr(), None, self.stream))
        self.batches += 1
        return self.pieces[-1][:self._words]

    def run(self, keep: bool = True):
        """Every batch: the loop over ``next`` and ``emit``."""
        while self.next() is not None:
            self.emit(keep)

    def finish(self):
        self._check("coral_bamgpu_finish", self.L.coral_bamgpu_finish(self.h, self.stream))
        dh = C.c_void_p()
        self._check("coral_bamgpu_host", self.L.coral_bamgpu_host(self.h, C.byref(dh)))
        self.dh = dh
        return dh

    def cigar(self):
        """The kept pieces as one tensor: the CIGAR words of the whole decode, in record order."""
        pieces = [p[:n] for p, n in zip(self.pieces, self.words) if n]
        return torch.cat(pieces) if len(pieces) > 1 else (pieces[0] if pieces else torch.zeros(0, dtype=torch.int32, device=self.dev))

    def stats(self) -> dict:
        """coral_bam_decode_stats and coral_bamgpu_stats of a finished decode, under bam.LAST_DECODE's names."""
        st, secs, gst, gsecs = (C.c_int64 * 3)(), C.c_double(0.0), (C.c_int64 * 4)(), (C.c_double * 6)()
        self.L.coral_bam_decode_stats(self.dh, st, C.byref(secs))
        self.L.coral_bamgpu_stats(self.h, gst, gsecs)
        return dict(seconds=float(gsecs[0]), compressed_bytes=int(st[0]), uncompressed_bytes=int(st[1]), blocks=int(st[2]),
                    threads=self.n_threads, where="gpu", batches=int(gst[0]), rewalked_segments=int(gst[1]),
                    nonacgt_records_fetched=int(gst[2]), batch_bytes=int(gst[3]), host_seconds=float(gsecs[1]), read_seconds=float(gsecs[2]),
                    setup_seconds=float(gsecs[3]), waited_for_file_seconds=float(gsecs[4]), waited_for_gpu_seconds=float(gsecs[5]),
                    workspace_bytes=self.ws_bytes)

    def sink_stats(self):
        """What went to the sink's file: (records, their bytes, the file's bytes, its BGZF members)."""
        sst = (C.c_int64 * 4)()
        _lib.check(self.L.coral_bamgpu_sink_stats(self.h, sst), "coral_bamgpu_sink_stats")
        return tuple(int(v) for v in sst)

    def close(self):
        if self.h is not None:
            h, self.h = self.h, None
            rc = self.L.coral_bamgpu_close(h)
            self.pieces, self._held = [], []                     # (rule 2: not before)
            self._check("coral_bamgpu_close", rc)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
