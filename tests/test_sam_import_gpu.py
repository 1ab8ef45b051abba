"""bam.import_sam on the GPU (coral_samgpu_import: k_sam_lines, k_sam_size, k_sam_encode, k_sam_fixup and the record sink): the
device build of coral_sam_core.h against the host build of the same rules (coral_sam_encode, which tests/test_sam_core.py checks
against a plain-Python restatement), on the case table of tests/sam_cases.py; the file's layout; batch boundaries; launch
geometry; the float fix-ups; refusals; and the pipeline import -> sort --stream --index."""
import gzip
import os

import numpy as np
import pytest
import torch  # noqa: F401

from coral_amd import CoRAL, _lib, bam, synth
from tests import sam_cases as sc
from tests.bamfile import many_ops, parse, read_bam_bgzf

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
SMALL = 1 << 20                                        # batch_bytes of the tests: the longest line of the case table fits
CORAL_ERR_CAPACITY, CORAL_ERR_FORMAT = -3, -4


def host_stream(text, keep=None):
    """The inflated stream by the host's rule book: header + records."""
    H = bam._sam_header(text)                           # (only the leading '@' lines count)
    data, n_lines, written, dropped = bam.sam_encode(text[H.text_bytes:], H, keep, H.n_lines + 1)
    return H.bam.tobytes(), data.tobytes(), (n_lines, written, dropped)


def run_gpu(tmp_path, name, text, keep=None, **kw):
    sam, out = str(tmp_path / (name + ".sam")), str(tmp_path / (name + ".bam"))
    with open(sam, "wb") as fp:
        fp.write(text)
    kw.setdefault("batch_bytes", SMALL)
    st = bam.import_sam(sam, out, record_filter=keep, device=GPU, **kw)
    with open(out, "rb") as fp:
        raw = fp.read()
    return st, raw, out


@pytest.fixture(scope="module")
def table():
    return sc.cases()


def test_device_bytes_equal_the_host_cores_on_the_case_table(tmp_path, table):
    for name, (text, keep) in table.items():
        head, data, counts = host_stream(text, keep)
        st, raw, out = run_gpu(tmp_path, name, text, keep)
        assert gzip.decompress(raw) == head + data, name
        assert (st.lines, st.records, st.dropped, st.bytes, st.file_bytes) == counts + (len(data), len(raw)), name
    assert bam.LAST_IMPORT["workspace_bytes"] > 0


def test_the_file_is_the_gpu_writers_of_header_and_host_records(tmp_path, table):
    """Every part cut at 0xff00 bytes, the header ending a block, the EOF block last: coral_bgzf_write_gpu of the two parts."""
    for name in ("cigar", "seq", "header_only", "filter_all"):
        text, keep = table[name]
        head, data, _ = host_stream(text, keep)
        st, raw, _ = run_gpu(tmp_path, name, text, keep)
        want = str(tmp_path / (name + "_want.bam"))
        bam.RecordBytes(np.frombuffer(data, dtype=np.uint8), np.array([0, len(data)], dtype=np.int64), header=head).write(want, device=GPU)
        with open(want, "rb") as fp:
            assert fp.read() == raw, name
        assert st.members == (len(head) + 0xfeff) // 0xff00 + (len(data) + 0xfeff) // 0xff00 + 1
    assert len(host_stream(*table["cigar"])[1]) > 2 * 0xff00


def boundary_text():
    """60 lines of different lengths, the lines 20..23 of mapping quality 0."""
    lines = [sc.line("b%d" % k, mapq=0 if 20 <= k < 24 else 60, seq="ACGT" * (20 + k), qual=sc.quals(4 * (20 + k), k), cigar="%dM" % (4 * (20 + k)),
                     tags=["NM:i:%d" % k, "de:f:0.0%d" % k]) for k in range(60)]
    return sc.text_of(lines), [len(ln) + 1 for ln in lines]


def test_the_bytes_do_not_depend_on_the_batches(tmp_path):
    text, lens = boundary_text()
    keep = bam.RecordFilter(min_mapq=25)
    st0, raw0, _ = run_gpu(tmp_path, "whole", text, keep)
    assert (st0.batches, st0.records, st0.dropped) == (1, 56, 4)
    assert gzip.decompress(raw0) == b"".join(host_stream(text, keep)[:2])
    ends = np.cumsum(lens)
    longest = max(lens)
    sizes = {"at": int(ends[6]), "before": int(ends[6]) - 1, "after": int(ends[6]) + 1, "alone": longest, "two": 2 * longest + 3}
    for name, b in sizes.items():
        st, raw, _ = run_gpu(tmp_path, name, text, keep, batch_bytes=b)
        assert raw == raw0 and st.batches > 1 and st[:7] == st0[:7], name
    # the lines 20..23 alone in a batch, between two batches that write: equal lengths make the batches line up
    same = sc.text_of([sc.line("e%02d" % k, mapq=10 if 4 <= k < 8 else 60, seq="ACGTACGT", qual="IIIIIIII") for k in range(12)])
    width = (len(same) - len(sc.HEADER)) // 12
    st1, raw1, _ = run_gpu(tmp_path, "same_whole", same, keep)
    st2, raw2, _ = run_gpu(tmp_path, "same_split", same, keep, batch_bytes=4 * width)
    assert raw1 == raw2 and (st2.batches, st2.records, st2.dropped) == (3, 8, 4)
    big = sc.cases()["cigar"]
    _, raw3, _ = run_gpu(tmp_path, "chunk_default", big[0])
    st4, raw4, _ = run_gpu(tmp_path, "chunk_one", big[0], chunk_blocks=1)
    assert raw3 == raw4 and st4.members > 4


def test_launch_geometry(tmp_path):
    short = lambda k: sc.line("s%d" % k, seq="ACG", qual="III", tags=["NM:i:%d" % (k % 300)])
    texts = {"n%d" % n: sc.text_of([short(k) for k in range(n)]) for n in (0, 1, 63, 64, 65, 2 * 2048 + 1)}
    mixed = [short(k) for k in range(70)]
    mixed.insert(3, sc.line("ops65536", cigar="1M1I" * 32768, seq="AC" * 32768, qual="*"))
    mixed.insert(40, sc.line("seq200k", seq="ACGTN" * 40000, qual=sc.quals(200000, 5), cigar="200000M"))
    texts["mixed"] = sc.text_of(mixed)
    for name, text in texts.items():
        head, data, counts = host_stream(text)
        st, raw, _ = run_gpu(tmp_path, name, text)
        assert gzip.decompress(raw) == head + data and (st.lines, st.records) == counts[:2], name


def test_float_fixups_zero_one_and_many(tmp_path):
    exact, left = "0.0123", "0.30000001192092896"          # 17 digits: outside the device's exact path, converted by the host
    plain = lambda k: sc.line("p%d" % k, tags=["de:f:" + exact])
    for name, lines, n_fix in (("zero", [plain(k) for k in range(10)], 0),
                               ("one", [plain(k) for k in range(5)] + [sc.line("x", tags=["de:f:" + left])] + [plain(k) for k in range(5)], 1),
                               ("first_and_last", [sc.line("a", tags=["de:f:" + left])] + [plain(k) for k in range(70)] + [sc.line("z", tags=["XF:B:f,1," + left])], 2),
                               ("many", [sc.line("m%d" % k, tags=["de:f:1.%017d" % (k * 7919), "XF:B:f," + ",".join([left, exact] * 3)]) for k in range(200)], 800)):
        text = sc.text_of(lines, last_newline=name != "first_and_last")
        head, data, _ = host_stream(text)
        st, raw, _ = run_gpu(tmp_path, name, text)
        assert gzip.decompress(raw) == head + data, name
        assert bam.LAST_IMPORT["float_fixups"] == n_fix, name


def test_refusals_match_the_host_and_leave_the_process_usable(tmp_path, table):
    for name, text, line_no, field in sc.refusals():
        with pytest.raises(_lib.CoralHipError) as host:
            host_stream(text)
        with pytest.raises(_lib.CoralHipError) as dev:
            run_gpu(tmp_path, name, text, batch_bytes=1 << 16)
        assert host.value.code == dev.value.code == CORAL_ERR_FORMAT, name
        assert ("SAM line %d: " % line_no) in str(dev.value) and str(host.value).split(": ", 1)[1] == str(dev.value).split(": ", 1)[1], (name, str(dev.value))
        assert not os.path.exists(str(tmp_path / (name + ".bam"))), name
    good = sc.line("good", seq="ACGT", qual="IIII", cigar="4M")
    # bad lines in two batches: the lowest; and a batch of lines too short for the device's arrays, named by the host's pass
    for name, text, line_no, b in (("two_batches", sc.text_of([good] * 30 + [sc.line("b1", mapq=256)] + [good] * 30 + [sc.line("b2", flag="x")]), sc.N_HEADER_LINES + 31, 512),
                                   ("tiny_lines", sc.text_of([good] * 3 + ["a"] * 1000), sc.N_HEADER_LINES + 4, 4096)):
        with pytest.raises(_lib.CoralHipError, match="SAM line %d: " % line_no) as dev:
            run_gpu(tmp_path, name, text, batch_bytes=b)
        assert dev.value.code == CORAL_ERR_FORMAT and not os.path.exists(str(tmp_path / (name + ".bam")))
    with pytest.raises(_lib.CoralHipError, match="does not fit a batch") as dev:
        run_gpu(tmp_path, "too_long", sc.text_of([good, sc.line("long", seq="A" * 5000, qual="*"), good]), batch_bytes=4096)
    assert dev.value.code == CORAL_ERR_CAPACITY and not os.path.exists(str(tmp_path / "too_long.bam"))
    text, keep = table["tags"]
    st, raw, _ = run_gpu(tmp_path, "afterwards", text, keep)
    assert gzip.decompress(raw) == b"".join(host_stream(text, keep)[:2])


def test_import_then_sort_stream_equals_sort_of_the_written_file(tmp_path):
    """The reference's preparation script as commands of ours: SAM text in the mapper's (name) order -> import -> sort --stream
    --index, against sort_bam of write_bam's file of the same records in that order."""
    from tests.test_sam_core import sam_text_of
    M, I, D, S = 0, 1, 2, 4
    alns = [dict(tid=(k * 7) % 24, pos=(k * 7919) % 100_000, cigar=[(S, k % 5), (M, 50 + k), (I, k % 3), (D, 4), (M, 30)] if k % 11 else many_ops(70 + k), name="read%03d" % k,
                 flag=(0, 16, 2048, 256)[k % 4], mapq=(60, 3, 40)[k % 3], nm=k % 200) for k in range(300)]
    rec = synth.records_from_alignments(alns)
    src, sam, imported = str(tmp_path / "name_order.bam"), str(tmp_path / "mapped.sam"), str(tmp_path / "mapped.bam")
    bam.write_bam(rec, src, with_qual=True, nm_type="C")
    text, raw = sam_text_of(src)
    with open(sam, "wb") as fp:
        fp.write(text)
    CoRAL.main(["import", "--sam", sam, "--output", imported, "--device", GPU])
    back = read_bam_bgzf(imported)
    assert [r["name"] for r in back.recs] == [a["name"] for a in alns] and back.n_bytes == len(raw)
    assert gzip.decompress(open(imported, "rb").read()) == raw
    got, want = str(tmp_path / "sorted.bam"), str(tmp_path / "want.bam")
    CoRAL.main(["sort", "--lr_bam", imported, "--output", got, "--stream", "--index", "--device", GPU, "--filter_min_mapq", "25"])
    bam.sort_bam(src, want, index=True, record_filter=bam.RecordFilter(min_mapq=25), device=GPU, write_device=GPU)
    for ext in ("", ".bai"):
        with open(got + ext, "rb") as a, open(want + ext, "rb") as b:
            assert a.read() == b.read(), ext
    n = len(parse(gzip.decompress(open(got, "rb").read())).recs)
    assert n == sum(1 for a in alns if a["mapq"] >= 25) > 0
