"""coral_amd/decode_session.py without a GPU: the coral_bam_sink_t that open_handle hands to coral_bamgpu_open_request for each kind
of sink, against the library itself (an open does no GPU work) and against a stub that records what it was given, and the order in
which a DecodeSession calls the library and the device, against that stub.  The session's two device operations (_alloc, _drain)
are overridden and nothing else; what the session references is observed through weak references, never through its private
attributes."""
import ctypes as C
import gc
import os
import weakref

import pytest
import torch

from coral_amd import _lib, bam, synth
from coral_amd.decode_session import BamFile, DecodeSession, Runs, TextFile, open_handle
from tests.bamfile import M
from tests.decode_support import CORAL_ERR_ARG, CORAL_OK

CORAL_ERR_HIP = -2
NEEDS_A_DEVICE = ("no sink, coordinate order", "runs")
RECORDS, FASTQ, SORTED = (0, None, None, 2), (0, None, None, 1), (0, None, None, 2, 1)


# ---- which sink ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_session")
    path = str(d / "small.bam")
    bam.write_bam(synth.records_from_alignments([dict(tid=0, pos=100 + 10 * k, cigar=[(M, 50)], name="r%d" % k) for k in range(5)]), path)
    return dict(dir=d, path=path, header=bam.bam_header_bytes(path))


def direct(L, path, request, fields, order=None, n_threads=1, batch_bytes=1 << 20):
    """coral_bamgpu_open_request called as include/coral_hip.h declares it, with the coral_bam_sink_t of ``fields`` = (kind, path,
    header, header_bytes, chunk_blocks), or NULL for None, and ``order`` (None: as ``request`` has it) in the request's reads_order
    -> (rc, handle granted, ws_bytes, message); closed."""
    req, h, ws = _lib.bam_request(**request), C.c_void_p(), C.c_int64(0)
    if order is not None:
        req.reads_order = order
    to = None if fields is None else _lib.coral_bam_sink_t(*fields)
    rc = L.coral_bamgpu_open_request(path.encode(), n_threads, batch_bytes, C.byref(req), to, C.byref(h), C.byref(ws))
    message = L.coral_bam_last_error().decode()
    if h.value is not None:
        L.coral_bamgpu_close(h)
    return rc, h.value is not None, int(ws.value), message


def through_open_handle(L, path, request, sink, n_threads=1, batch_bytes=1 << 20):
    req = _lib.bam_request(**request)
    rc, h, ws = open_handle(L, path, n_threads, batch_bytes, req, sink)
    message = L.coral_bam_last_error().decode()
    if h.value is not None:
        L.coral_bamgpu_close(h)
    return rc, h.value is not None, ws, message


def cases(small, sub):
    """name -> (request, sink, the sink struct's fields: kind, path, header, header_bytes, chunk_blocks, the request's reads_order
    in the call); every sink's file in the directory ``sub``"""
    out = lambda name: str(sub / name)
    head = small["header"]
    head_ptr = C.cast(C.c_char_p(head), C.c_void_p)
    return {
        "no sink": (dict(), None, None, 0),
        "no sink, coordinate order": (dict(reads=SORTED), None, None, 1),
        "text file": (dict(reads=FASTQ), TextFile(out("x.fastq")), (_lib.SINK_TEXT, os.fsencode(out("x.fastq")), None, 0, 0), 0),
        "BAM file": (dict(reads=RECORDS), BamFile(out("x.bam"), head, 3), (_lib.SINK_BAM, os.fsencode(out("x.bam")), head_ptr, len(head), 3), 0),
        "runs": (dict(reads=RECORDS), Runs(out("x.runs.tmp"), 3), (_lib.SINK_RUNS, os.fsencode(out("x.runs.tmp")), None, 0, 3), 1),      # (the sink asks for the order)
    }


def test_open_handle_grants_what_the_entry_point_grants(small, tmp_path):
    """(reads_order = 1 sizes hipcub's sort at open: without a device the library answers CORAL_ERR_HIP, to the direct call and to
    open_handle alike - the same request in file order would have been granted; with a device they are granted like the others.)"""
    L, sizes = _lib.lib(), {}
    for name, (request, sink, fields, order) in cases(small, tmp_path).items():
        want = direct(L, small["path"], request, fields, order)
        got = through_open_handle(L, small["path"], request, sink)
        if want[0] == CORAL_ERR_HIP and not torch.cuda.is_available():
            assert name in NEEDS_A_DEVICE and "sort" in want[3], (name, want)
        else:
            assert want[:2] == (CORAL_OK, True) and want[2] > 0, (name, want)
            sizes[name] = got[2]
        assert got == want, name
    # they carve differently: a call that described another sink would not have returned this size
    assert sizes["no sink"] < sizes["BAM file"] and len(set(sizes.values())) == len(sizes) >= 3, sizes


def test_open_handle_refuses_what_the_entry_point_refuses(small, tmp_path):
    L, c = _lib.lib(), cases(small, tmp_path)
    path = small["path"]
    text, bam_file, runs = c["text file"][2], c["BAM file"][2], c["runs"][2]
    bad = {                                                      # the case's request or sink with one thing wrong -> a word of the message
        "no sink": (dict(rank=2, world=2), None, None, 0, "rank"),
        "no sink, coordinate order": (dict(reads=FASTQ + (1,)), None, None, 1, "reads_order"),       # (in file order it is granted)
        "text file": (dict(reads=RECORDS), c["text file"][1], text, 0, "want_reads"),
        "BAM file": (dict(reads=RECORDS), c["BAM file"][1]._replace(header=None), bam_file[:2] + (None, 0, 3), 0, "header"),
        "runs": (dict(reads=RECORDS), c["runs"][1]._replace(chunk_blocks=16385), runs[:4] + (16385,), 1, "chunk_blocks"),
        "runs, no path": (dict(reads=RECORDS), Runs(None, 3), (_lib.SINK_RUNS, None, None, 0, 3), 1, "path"),
    }
    for name, (request, sink, fields, order, word) in bad.items():
        want = direct(L, path, request, fields, order)
        got = through_open_handle(L, path, request, sink)
        assert want[:3] == (CORAL_ERR_ARG, False, 0) and word in want[3], (name, want)
        assert got == want, name
    with pytest.raises(TypeError):
        open_handle(L, path, 1, 0, _lib.bam_request(), (str(tmp_path / "x"), None, 0))       # (the tuple of before is not a sink)


def test_the_one_open_call_refuses_before_any_device_call(small, tmp_path):
    """The rules of reads_order and of the sink kinds, on both pipelines where both have them; nothing is created, no handle is given."""
    L, path = _lib.lib(), small["path"]
    out = os.fsencode(str(tmp_path / "never"))
    head = C.cast(C.c_char_p(small["header"]), C.c_void_p)
    assert direct(L, path, dict(reads=RECORDS), (7, out, head, len(small["header"]), 0))[:3] == (CORAL_ERR_ARG, False, 0)       # an unknown kind
    assert direct(L, path, dict(reads=RECORDS), (-1, out, None, 0, 0))[:3] == (CORAL_ERR_ARG, False, 0)
    for request in (dict(reads=RECORDS + (2,)), dict(reads=FASTQ + (1,)), dict()):          # reads_order = 2; = 1 without want_reads = 2
        req, h = _lib.bam_request(**request), C.c_void_p()
        if not request:
            req.reads_order = 1
        assert L.coral_bam_decode_request(path.encode(), 1, C.byref(req), C.byref(h)) == CORAL_ERR_ARG and h.value is None, request
        assert "reads_order" in L.coral_bam_last_error().decode(), request
        ws = C.c_int64(0)
        assert L.coral_bamgpu_open_request(path.encode(), 1, 0, C.byref(req), None, C.byref(h), C.byref(ws)) == CORAL_ERR_ARG and h.value is None, request
        assert "reads_order" in L.coral_bam_last_error().decode() and ws.value == 0, request
    got = direct(L, path, dict(reads=SORTED), (_lib.SINK_BAM, out, head, len(small["header"]), 0))       # a BAM file is written in file order
    assert got[:3] == (CORAL_ERR_ARG, False, 0) and "reads_order must be 0" in got[3], got
    got = direct(L, path, dict(reads=RECORDS), (_lib.SINK_RUNS, out, None, 0, 0))                          # runs are sorted
    assert got[:3] == (CORAL_ERR_ARG, False, 0) and "reads_order must be 1" in got[3], got
    assert not os.path.exists(out)
    # the host kind reads none of the other fields: garbage there opens like NULL
    plain = direct(L, path, dict(reads=RECORDS), None)
    assert plain[:2] == (CORAL_OK, True) and direct(L, path, dict(reads=RECORDS), (_lib.SINK_HOST, b"/no/such/dir/x", 0x10, -5, 99999)) == plain
    assert not os.path.exists(out)


def test_open_handle_fills_the_sink_struct(small, tmp_path):
    """What the one call is given: the fs-encoded path, the header's bytes and length, chunk_blocks, and the order in the request."""
    head = small["header"]
    for name, (request, sink, fields, order) in cases(small, tmp_path).items():
        stub = StubLib()
        rc, h, ws = open_handle(stub, small["path"], 2, 1 << 20, _lib.bam_request(**request), sink)
        assert (rc, h.value, ws) == (CORAL_OK, 0x1000, WS_BYTES) and stub.opened[:3] == (small["path"].encode(), 2, 1 << 20), name
        assert stub.opened[3] == order, name
        if fields is None:
            assert stub.opened[4] is None, name
        else:
            kind, path, header, header_bytes, chunk_blocks = stub.opened[4]
            assert (kind, path, header_bytes, chunk_blocks) == (fields[0], fields[1], fields[3], fields[4]), name
            assert header == (head if fields[2] is not None else None), name


# ---- the call order -----------------------------------------------------------------------------------------------------------
WS_BYTES, STREAM, WORDS = 1000, 0x77, (40, 0, 7)                 # (the second batch has no CIGAR word: its piece is still one)


class StubLib:
    """Stands in for the library: every call is logged by its short name and answers CORAL_OK, but for the ``fail_at`` = (name,
    k)-th one.  The device operations of `Recorded` log here too, and leave weak references to what they allocated."""

    def __init__(self, fail_at=None):
        self.fail_at, self.log, self.emitted = fail_at, [], 0
        self.blocks, self.pieces, self.live_pieces = [], [], []

    def rc(self, name):
        self.log.append(name)
        self.live_pieces.append(sum(r() is not None for r in self.pieces))
        return -3 if self.fail_at == (name, self.log.count(name)) else CORAL_OK

    def coral_bam_last_error(self):
        return b"the stub says no"

    def coral_bamgpu_open_request(self, path, n_threads, batch_bytes, req, sink, h, ws_bytes):
        rc = self.rc("open")
        to = None if sink is None else (sink.kind, sink.path, None if not sink.header else C.string_at(sink.header, sink.header_bytes), sink.header_bytes, sink.chunk_blocks)
        self.opened = (path, n_threads, batch_bytes, req._obj.reads_order, to)
        if rc == CORAL_OK:
            h._obj.value, ws_bytes._obj.value = 0x1000, WS_BYTES
        return rc

    def coral_bamgpu_start(self, h, base, nbytes):
        assert h.value == 0x1000 and nbytes == WS_BYTES and base % 256 == 0
        ws = self.blocks[0]()
        assert ws.data_ptr() <= base and base + nbytes <= ws.data_ptr() + ws.numel()
        return self.rc("start")

    def coral_bamgpu_next(self, h, out, stream):
        assert stream == STREAM
        rc = self.rc("next")
        if rc == CORAL_OK and self.emitted < len(WORDS):
            out[0], out[1], out[2] = 5, WORDS[self.emitted], 1
        return rc

    def coral_bamgpu_emit(self, h, piece, cigar_off, stream):
        assert stream == STREAM and cigar_off is None and piece == self.pieces[-1]().data_ptr() and self.pieces[-1]().numel() >= max(WORDS[self.emitted], 1)
        self.emitted += 1
        return self.rc("emit")

    def coral_bamgpu_finish(self, h, stream):
        assert stream == STREAM
        return self.rc("finish")

    def coral_bamgpu_host(self, h, dh):
        dh._obj.value = 0x2000
        return self.rc("host")

    def coral_bamgpu_close(self, h):
        assert h.value == 0x1000
        assert all(r() is not None for r in self.blocks), "a workspace was released before close"
        return self.rc("close")


class Recorded(DecodeSession):
    def _alloc(self, n, dtype=torch.uint8):
        t = torch.empty(n, dtype=dtype)
        if dtype == torch.uint8:
            self.L.log.append("alloc")
            self.L.blocks.append(weakref.ref(t))
        else:
            assert dtype == torch.int32
            self.L.pieces.append(weakref.ref(t))
        return t

    def _drain(self):
        self.L.log.append("drain")
        return STREAM


def session(stub, **kw):
    return Recorded("x.bam", _lib.bam_request(), device="cpu", n_threads=2, L=stub, **kw)


def whole_decode(stub, keep=True, body=None):
    with session(stub) as s:
        s.start()
        s.run(keep=keep)
        dh = s.finish()
        assert dh.value == 0x2000 and s.dh is dh and s.batches == len(WORDS)
        if body is not None:
            body(s)
    return s


NORMAL = ["open", "alloc", "drain", "start"] + ["next", "emit"] * 3 + ["next", "finish", "host", "close"]


def test_the_normal_path():
    stub = StubLib()

    def body(s):
        stub.log.append("body")
        assert s.words == list(WORDS) and [p.numel() for p in s.pieces] == [max(w, 1) for w in WORDS] and s.cigar().numel() == sum(WORDS)
    s = whole_decode(stub, body=body)
    assert stub.log == NORMAL[:-1] + ["body", "close"]
    s.close()                                                    # idempotent
    assert stub.log.count("close") == 1
    gc.collect()
    assert all(r() is None for r in stub.blocks + stub.pieces)   # released - behind close, as the stub's close has checked
    assert s.req is not None                                     # the request outlives the handle


@pytest.mark.parametrize("fail_at", [("start", 1), ("next", 2), ("emit", 1), ("emit", 3), ("finish", 1), ("host", 1)])
def test_a_failing_step_closes_once_and_last(fail_at):
    stub = StubLib(fail_at)
    with pytest.raises(_lib.CoralHipError, match=r"coral_bamgpu_%s\(x\.bam\) failed \(-3\): the stub says no" % fail_at[0]):
        whole_decode(stub)
    at = [k for k, name in enumerate(NORMAL) if name == fail_at[0]][fail_at[1] - 1]
    assert stub.log == NORMAL[:at + 1] + ["close"]


def test_an_exception_in_the_body_closes_once_and_last():
    stub = StubLib()

    def body(s):
        raise KeyError("the caller's own")
    with pytest.raises(KeyError):
        whole_decode(stub, body=body)
    assert stub.log == NORMAL
    stub = StubLib()
    with pytest.raises(KeyError):                                # before `start`: nothing but the handle
        with session(stub):
            raise KeyError("early")
    assert stub.log == ["open", "close"]


def test_a_refused_open_leaves_nothing_to_close():
    stub = StubLib(("open", 1))
    with pytest.raises(_lib.CoralHipError, match=r"coral_bamgpu_open_request\(x\.bam\) failed \(-3\): the stub says no"):
        session(stub)
    assert stub.log == ["open"]
    with pytest.raises(_lib.CoralHipError, match=r"failed \(-3, CORAL_ERR_CAPACITY\): the stub"):
        session(StubLib(("open", 1)), error_names={-3: "CORAL_ERR_CAPACITY"})


@pytest.mark.parametrize("keep", [True, False])
def test_pieces_kept_or_not(keep):
    stub = StubLib()
    live_in_body = []
    s = whole_decode(stub, keep=keep, body=lambda s: live_in_body.append(sum(r() is not None for r in stub.pieces)))
    assert len(stub.pieces) == len(WORDS)
    if keep:
        assert live_in_body == [len(WORDS)] and stub.live_pieces[-1] == len(WORDS)           # all of them, still at close
        assert stub.live_pieces == [0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 3, 3]                       # (open, start, next, emit, ...)
    else:
        assert live_in_body == [1] and max(stub.live_pieces) == 1                             # at no call more than the current one
    del s


def test_a_second_workspace_is_drained_and_lives_until_close():
    stub = StubLib()

    def body(s):
        before = len(stub.log)
        base = s.workspace(500)
        assert stub.log[before:] == ["alloc", "drain"] and s.stream == STREAM
        ws2 = stub.blocks[1]()
        assert base % 256 == 0 and ws2.data_ptr() <= base and base + 500 <= ws2.data_ptr() + ws2.numel()
    whole_decode(stub, body=body)
    assert len(stub.blocks) == 2 and stub.log[-1] == "close"     # (whose stub checked that both blocks were still there)
    gc.collect()
    assert all(r() is None for r in stub.blocks)
