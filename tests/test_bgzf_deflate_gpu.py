"""BGZF blocks made on the GPU (coral_amd/csrc/coral_bamgpu_deflate.h: k_bgzf_deflate, k_bgzf_pack; coral_bgzf_deflate,
coral_bgzf_pack, coral_bgzf_write_gpu; bam.RecordBytes.write(device=...), bam.sort_bam(write_device=...), bam.bgzf_compress).

The kernel's members are compared byte for byte with the host build of the same core (tests/native/deflate_host.cpp, which
tests/test_deflate_core.py checks against zlib) and inflated with zlib themselves; the files are read back with gzip, the
plain-Python reader and both decoders."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest
import torch

from coral_amd import CoRAL, _lib, bam
from tests import deflate_cases as dc
from tests.decode_support import CORAL_ERR_ARG, CORAL_OK, assert_same_records
from tests.test_deflate_core import host_deflate_library
from tests.test_extract_records import REGIONS, blocks_of, case, gunzip  # noqa: F401  (`case`: the module's file fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOT = 65536
GRID_CAP = 2048                                  # workgroups of a k_bgzf_deflate launch (DEFL_GRID_CAP)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return host_deflate_library(tmp_path_factory.mktemp("deflate_host"))


def on_device(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a writable copy)


def device_deflate(blocks, misalign=(1, 3, 7, 13), scratch_bytes=None, expect=CORAL_OK):
    """One coral_bgzf_deflate launch over `blocks`: block k starts misalign[k % 4] mod 16 bytes into the source buffer.  Returns
    (members, slots tensor, member_bytes tensor)."""
    L = _lib.lib()
    n = len(blocks)
    desc, at, buf = np.zeros((max(n, 1), 4), dtype=np.uint32), 0, bytearray()
    for k, b in enumerate(blocks):
        at = (len(buf) + 15) // 16 * 16 + misalign[k % len(misalign)]
        buf += bytes(at - len(buf)) + b
        desc[k] = (at, len(b), k * SLOT, 0)
    src = on_device(np.frombuffer(bytes(buf) + bytes(16), dtype=np.uint8))
    t_desc = on_device(desc.view(np.int32))
    slots = torch.zeros(max(n, 1) * SLOT, dtype=torch.uint8, device=DEV)
    member = torch.full((max(n, 1),), -1, dtype=torch.int32, device=DEV)
    need = int(L.coral_bgzf_deflate_scratch_bytes(n))
    scratch = torch.empty(max(need if scratch_bytes is None else scratch_bytes, 1), dtype=torch.uint8, device=DEV)
    rc = L.coral_bgzf_deflate(src.data_ptr(), t_desc.data_ptr(), n, slots.data_ptr(), member.data_ptr(), scratch.data_ptr(),
                              need if scratch_bytes is None else scratch_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.coral_bam_last_error().decode())
    if rc != CORAL_OK:
        return None, slots, member
    sizes, raw = member.cpu().numpy(), slots.cpu().numpy()
    return [raw[k * SLOT:k * SLOT + sizes[k]].tobytes() for k in range(n)], slots, member


def test_every_case_in_one_launch_equals_the_host_core(host):
    cases = dc.cases()
    members, slots, _ = device_deflate([c for _, c in cases])
    for (name, data), member in zip(cases, members):
        assert member == host(data)[0], name
        dc.check_member(member, data)
    raw = slots.cpu().numpy()
    for k, member in enumerate(members):                       # behind a member only the zero padding of its last word
        assert not raw[k * SLOT + len(member):(k + 1) * SLOT].any(), cases[k][0]
    # other alignments of the same blocks, and another launch: the same bytes
    again, _, _ = device_deflate([c for _, c in cases][::-1], misalign=(0, 15, 8, 2))
    assert again[::-1] == members


def test_more_blocks_than_the_grid_and_the_pack(host):
    rng = np.random.default_rng(3)
    n = GRID_CAP + 1500
    blocks = [bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 100)) if k % 7 else bytes([k % 251]) * (k % 97) for k in range(n)]
    members, slots, member = device_deflate(blocks)
    want = {}
    for k in (0, 1, 7, 96, 97, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, n - 1):
        want[k] = host(blocks[k])[0]
        assert members[k] == want[k], k
    for b, m in zip(blocks, members):
        dc.check_member(m, b)
    # k_bgzf_pack: the slots gathered into the concatenation of the members
    L = _lib.lib()
    packed = torch.zeros(n * SLOT // 8, dtype=torch.uint8, device=DEV)
    off = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    tmp = torch.empty(int(L.coral_bgzf_pack_scratch_bytes(n)), dtype=torch.uint8, device=DEV)
    assert sum(len(m) for m in members) + 16 <= packed.numel()
    rc = L.coral_bgzf_pack(slots.data_ptr(), member.data_ptr(), n, packed.data_ptr(), off.data_ptr(), tmp.data_ptr(), tmp.numel(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == CORAL_OK, L.coral_bam_last_error().decode()
    joined = b"".join(members)
    assert off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(m) for m in members])]).tolist()
    assert packed.cpu().numpy()[:len(joined)].tobytes() == joined and not packed.cpu().numpy()[len(joined):].any()
    assert gzip.decompress(joined + dc.EOF_BLOCK) == b"".join(blocks)


def test_no_blocks_and_refused_arguments(host):
    L = _lib.lib()
    assert L.coral_bgzf_deflate(None, None, 0, None, None, None, 0, None) == CORAL_OK
    assert L.coral_bgzf_deflate_scratch_bytes(0) == 0 and L.coral_bgzf_deflate_scratch_bytes(1) == 4 * 0xff00
    assert L.coral_bgzf_deflate_scratch_bytes(10 ** 6) == GRID_CAP * 4 * 0xff00
    assert L.coral_bgzf_deflate(None, None, 1, None, None, None, 0, None) == CORAL_ERR_ARG
    assert L.coral_bgzf_deflate(None, None, -1, None, None, None, 0, None) == CORAL_ERR_ARG
    device_deflate([b"abc"], scratch_bytes=4 * 0xff00 - 1, expect=CORAL_ERR_ARG)
    assert "scratch" in L.coral_bam_last_error().decode()
    # src_len > 0xff00: refused before anything is launched (the descriptor is patched behind the helper's back)
    src = on_device(np.zeros(0xff01 + 16, dtype=np.uint8))
    desc = on_device(np.array([[0, 0xff01, 0, 0]], dtype=np.uint32).view(np.int32))
    slots, member = torch.zeros(SLOT, dtype=torch.uint8, device=DEV), torch.full((1,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(4 * 0xff00, dtype=torch.uint8, device=DEV)
    rc = L.coral_bgzf_deflate(src.data_ptr(), desc.data_ptr(), 1, slots.data_ptr(), member.data_ptr(), scratch.data_ptr(), scratch.numel(), None)
    torch.cuda.synchronize()
    assert rc == CORAL_ERR_ARG and "0xff00" in L.coral_bam_last_error().decode() and int(member[0]) == -1 and not slots.any()
    members, _, _ = device_deflate([bytes(0xff00)])
    assert members[0] == host(bytes(0xff00))[0]


def test_bgzf_compress(host):
    assert bam.bgzf_compress(b"", device=DEV) == dc.EOF_BLOCK
    rng = np.random.default_rng(9)
    data = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 3 * 0xff00 + 17))
    got = bam.bgzf_compress(data, device=DEV)
    cuts = [data[at:at + 0xff00] for at in range(0, len(data), 0xff00)]
    assert got == b"".join(host(c)[0] for c in cuts) + dc.EOF_BLOCK and gzip.decompress(got) == data
    assert bam.bgzf_compress(np.frombuffer(data, dtype=np.uint8), device=DEV) == got
    with pytest.raises(ValueError):
        bam.bgzf_compress(b"x", device="cpu")


def isizes(path):
    return [n for _, n in blocks_of(path)[1]]


def test_the_written_file(case, host, tmp_path):  # noqa: F811
    L = _lib.lib()
    got = bam.extract_records(case["path"], device="cpu", n_threads=2, index=False)
    payload = case["header"] + got.data.tobytes()
    on_host, out, small = (str(tmp_path / n) for n in ("host.bam", "gpu.bam", "gpu_small.bam"))
    got.write(on_host)
    assert got.write(out, device=DEV) == out and not os.path.exists(out + ".bai")
    assert gunzip(out) == payload == gunzip(on_host)
    assert isizes(out) == isizes(on_host) and len(isizes(out)) > 10           # the same cuts: the header ends a block here too
    with open(out, "rb") as fp:
        raw = fp.read()
    assert raw[-28:] == dc.EOF_BLOCK
    # the file is the host core's members of the same cuts, whatever the chunk size: one block per chunk, and 1 024
    cuts = [case["header"][at:at + 0xff00] for at in range(0, len(case["header"]), 0xff00)]
    cuts += [got.data[at:at + 0xff00].tobytes() for at in range(0, len(got.data), 0xff00)]
    assert raw == b"".join(host(c)[0] for c in cuts) + dc.EOF_BLOCK
    least = int(L.coral_bgzf_write_gpu_workspace_min_bytes())
    assert 0 < least < int(L.coral_bgzf_write_gpu_workspace_bytes()) // 512
    got.write(small, device=DEV, workspace_bytes=least)
    with open(small, "rb") as fp:
        assert fp.read() == raw
    with pytest.raises(_lib.CoralHipError, match="workspace"):
        got.write(small, device=DEV, workspace_bytes=least - 1)
    # both decoders read it back: the source's records
    want = bam.load_bam(case["path"], device="cpu")
    for dev in ("cpu", DEV):
        assert_same_records(bam.load_bam(out, device=dev), want)
    assert want.n == got.n


def test_the_written_index_and_the_view_mode(case, tmp_path):  # noqa: F811
    got = bam.extract_records(case["path"], device=DEV, n_threads=2, index=False)
    on_host, out = str(tmp_path / "host.bam"), str(tmp_path / "gpu.bam")
    got.write(on_host, index=True)
    got.write(out, index=True, device=DEV)
    assert os.path.exists(out + ".bai")
    a, b = bam.load_bam(out, device=DEV, regions=REGIONS), bam.load_bam(on_host, device=DEV, regions=REGIONS)
    assert a.n == b.n > 0
    assert_same_records(a, b)
    x, y = bam.extract_records(out, REGIONS, device="cpu"), bam.extract_records(on_host, REGIONS, device="cpu")
    assert x.n == y.n > 0 and np.array_equal(x.data, y.data)
    viewed = str(tmp_path / "view.bam")
    CoRAL.main(["view", "--lr_bam", case["path"], "--output", viewed, "--gpu_compress", "--index"])
    with open(viewed, "rb") as fa, open(out, "rb") as fb:
        assert fa.read() == fb.read()
    with open(viewed + ".bai", "rb") as fa, open(out + ".bai", "rb") as fb:
        assert fa.read() == fb.read()


def test_sort_bam_on_the_device(case, tmp_path):  # noqa: F811
    on_host, out, moded = (str(tmp_path / n) for n in ("host.bam", "gpu.bam", "mode.bam"))
    kw = dict(record_filter=bam.RecordFilter(min_mapq=1), device=DEV, n_threads=2)
    bam.sort_bam(case["path"], on_host, **kw)
    assert bam.sort_bam(case["path"], out, write_device=DEV, **kw) == out
    assert gunzip(out) == gunzip(on_host) and isizes(out) == isizes(on_host) and len(gunzip(out)) > 100_000
    with open(out + ".bai", "rb") as fa, open(on_host + ".bai", "rb") as fb:
        assert len(fa.read()) == len(fb.read())                # (virtual offsets differ: other compressed bytes)
    CoRAL.main(["sort", "--lr_bam", case["path"], "--output", moded, "--filter_min_mapq", "1", "--gpu_compress", "--index"])
    with open(moded, "rb") as fa, open(out, "rb") as fb:
        assert fa.read() == fb.read()


def test_python_and_c_argument_rules(case, tmp_path):  # noqa: F811
    L = _lib.lib()
    got = bam.extract_records(case["path"], REGIONS, device="cpu", index=False)
    for level in (0, 2, 9):
        with pytest.raises(ValueError, match="level"):
            got.write(str(tmp_path / "x.bam"), level=level, device=DEV)
    with pytest.raises(ValueError, match="level"):
        bam.sort_bam(case["path"], str(tmp_path / "x.bam"), level=6, write_device=DEV)
    assert not os.path.exists(str(tmp_path / "x.bam"))
    path = os.fsencode(str(tmp_path / "y.bam"))
    data = np.arange(100, dtype=np.uint8)
    parts, sizes = (C.c_void_p * 1)(data.ctypes.data), (C.c_int64 * 1)(100)
    ws = torch.empty(int(L.coral_bgzf_write_gpu_workspace_min_bytes()), dtype=torch.uint8, device=DEV)
    args = (ws.data_ptr(), ws.numel(), None)
    assert L.coral_bgzf_write_gpu(None, parts, sizes, 1, *args) == CORAL_ERR_ARG
    assert L.coral_bgzf_write_gpu(path, parts, sizes, -1, *args) == CORAL_ERR_ARG and "n_parts" in L.coral_bam_last_error().decode()
    assert L.coral_bgzf_write_gpu(path, None, None, 1, *args) == CORAL_ERR_ARG
    assert L.coral_bgzf_write_gpu(path, parts, (C.c_int64 * 1)(-5), 1, *args) == CORAL_ERR_ARG
    assert L.coral_bgzf_write_gpu(path, parts, sizes, 1, None, 0, None) == CORAL_ERR_ARG
    assert L.coral_bgzf_write_gpu(os.fsencode(str(tmp_path / "no_dir" / "y.bam")), parts, sizes, 1, *args) == CORAL_ERR_ARG
    assert not os.path.exists(path)
    assert L.coral_bgzf_write_gpu(path, parts, sizes, 1, *args) == CORAL_OK and gunzip(path.decode()) == data.tobytes()
    two = (C.c_void_p * 3)(data.ctypes.data, None, data.ctypes.data)
    assert L.coral_bgzf_write_gpu(path, two, (C.c_int64 * 3)(60, 0, 100), 3, *args) == CORAL_OK
    assert isizes(path.decode()) == [60, 100, 0]                               # an empty part makes no block
    assert L.coral_bgzf_write_gpu(path, None, None, 0, *args) == CORAL_OK
    with open(path, "rb") as fp:
        assert fp.read() == dc.EOF_BLOCK
