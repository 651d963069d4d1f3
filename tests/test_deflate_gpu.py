"""BGZF blocks deflated on the GPU (xm_bgzf_deflate_dev, xm_bgzf_compress: include/xenomapper_bgzf.h) -- every payload of
tests/deflate_shapes.py in one launch, at every alignment, with poisoned guard bytes between the slots: zlib inflates every stream
to its payload, the streams are byte for byte those of the host build of the same source (tests/deflate_core_host.cpp), the
project's own GPU decoder and CRC kernel take them back; launches with more blocks than chains, with one block, with none;
blocks the call declines; and the host-buffer call that frames the streams as BGZF members."""
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import deflate_shapes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(H.REPO, "tools"))
POISON = 0xEE
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def work():
    import torch
    from xenomapper_amd import _ffi
    n = _ffi.bgzf_deflate_work_bytes()
    assert 261376 <= n <= 256 << 20
    return torch.empty(n, dtype=torch.uint8, device="cuda:0")


def layout(payloads, capacity=None, odd_slot=()):
    """payload k at an address k mod 16 in the input, slots 16-byte aligned with GUARD bytes between them -> (input bytes,
    descriptors, bytes of the slot buffer).  capacity: per block, default n + 5; odd_slot: blocks whose slot begins one byte late."""
    from xenomapper_amd import _ffi
    blocks = np.zeros(len(payloads), dtype=_ffi.BGZF_BLOCK)
    at, slot = 0, GUARD
    for k, p in enumerate(payloads):
        at += (k - at) % 16
        cap = len(p) + 5 if capacity is None else capacity[k]
        blocks[k] = (slot + (1 if k in odd_slot else 0), at, cap, len(p))
        at += len(p)
        slot = (slot + cap + 1 + GUARD + 15) & ~15
    inp = np.full(at + 16, 0x5A, dtype=np.uint8)
    for k, p in enumerate(payloads):
        o = int(blocks["out_off"][k])
        inp[o:o + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8) if not isinstance(p, np.ndarray) else p
    return inp, blocks, slot


def gpu_deflate(ctx, work, inp, blocks, comp_bytes):
    """-> (slot buffer, clen, status, input afterwards, descriptors afterwards), all host arrays"""
    import torch
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(inp).to(dev)
    d_blocks = torch.from_numpy(blocks.view(np.uint8).copy()).to(dev)
    comp = torch.full((comp_bytes,), POISON, dtype=torch.uint8, device=dev)
    clen = torch.full((max(len(blocks), 1),), -1, dtype=torch.int32, device=dev)
    status = torch.full((max(len(blocks), 1),), -1, dtype=torch.int32, device=dev)
    ctx.bgzf_deflate_dev(d_in, d_blocks, comp, clen, status, work)
    torch.cuda.synchronize()
    return (comp.cpu().numpy(), clen.cpu().numpy()[:len(blocks)], status.cpu().numpy()[:len(blocks)], d_in.cpu().numpy(),
            d_blocks.cpu().numpy().view(blocks.dtype))


def outside_slots_is_poison(comp, blocks, written):
    """every byte of the slot buffer that lies in no block's [cdata_off, cdata_off + written[k]) still holds the poison"""
    mark = np.zeros(comp.shape[0] + 1, dtype=np.int32)
    np.add.at(mark, blocks["cdata_off"].astype(np.int64), 1)
    np.add.at(mark, blocks["cdata_off"].astype(np.int64) + np.asarray(written, dtype=np.int64), -1)
    inside = np.cumsum(mark[:-1]) > 0
    return bool((comp[~inside] == POISON).all())


def inflates_to(stream, payload):
    d = zlib.decompressobj(-15)
    return d.decompress(bytes(stream)) == bytes(payload) and d.eof and not d.unused_data


@pytest.fixture(scope="module")
def shapes():
    return S.all_shapes()


@pytest.fixture(scope="module")
def launch(ctx, work, shapes):
    """every shape x kind in ONE launch"""
    payloads = [p for _, p in shapes]
    inp, blocks, comp_bytes = layout(payloads)
    assert inp.shape[0] < 32 << 20 and len(set(int(o) % 16 for o in blocks["out_off"])) == 16
    comp, clen, status, inp_after, blocks_after = gpu_deflate(ctx, work, inp, blocks, comp_bytes)
    return dict(inp=inp, blocks=blocks, comp=comp, clen=clen, status=status, inp_after=inp_after, blocks_after=blocks_after)


def stream_of(launch, k):
    o = int(launch["blocks"]["cdata_off"][k])
    return launch["comp"][o:o + int(launch["clen"][k])]


def test_every_shape_and_kind_in_one_launch(launch, shapes):
    from xenomapper_amd import _ffi
    L = launch
    assert len(shapes) > 1500
    assert (L["status"] == 0).all(), [(shapes[k][0], _ffi.bgzf_strerror(s)) for k, s in enumerate(L["status"]) if s][:5]
    sizes = L["blocks"]["isize"].astype(np.int64)
    assert (L["clen"] > 0).all() and (L["clen"] <= sizes + 5).all()
    for k, (name, p) in enumerate(shapes):
        assert inflates_to(stream_of(L, k), p.tobytes()), name
        if name.startswith("random/"):
            assert L["clen"][k] == len(p) + 5, name                        # incompressible: the stored form
    assert outside_slots_is_poison(L["comp"], L["blocks"], sizes + 5)       # guards between the slots, in front and behind
    assert np.array_equal(L["inp_after"], L["inp"]) and np.array_equal(L["blocks_after"], L["blocks"])


def test_device_bytes_equal_the_host_build(launch, shapes, tmp_path):
    """R3 of xm_deflate_core.h: the output is a function of the payload's bytes alone -- the wave of 64 lanes on the device and the
    64 lanes emulated in turn on the host (plain g++, no sanitizer) write the same streams"""
    exe, blocks, emit = str(tmp_path / "deflate_core_host"), str(tmp_path / "blocks.bin"), str(tmp_path / "streams.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(H.REPO, "tests", "deflate_core_host.cpp"),
                           "-o", exe, "-lz"])
    S.write_blocks(blocks, [p for _, p in shapes])
    proc = subprocess.run([exe, "--blocks", blocks, "--emit", emit], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout + proc.stderr)[-2000:]
    host = S.read_streams(emit)
    assert len(host) == len(shapes)
    differ = [shapes[k][0] for k in range(len(shapes)) if stream_of(launch, k).tobytes() != host[k]]
    assert not differ, differ[:10]


def test_round_trip_through_the_gpu_decoder_and_crc(ctx, launch, shapes):
    """the descriptors with cdata_len = clen are what xm_bgzf_inflate_dev and xm_bgzf_crc32_dev take"""
    import torch
    from xenomapper_amd import _ffi
    dev = torch.device("cuda:0")
    L = launch
    blocks = L["blocks"].copy()
    blocks["cdata_len"] = L["clen"]
    comp = torch.zeros(L["comp"].shape[0] + _ffi.BGZF_COMP_PAD, dtype=torch.uint8, device=dev)
    comp[:L["comp"].shape[0]] = torch.from_numpy(L["comp"]).to(dev)
    d_blocks = torch.from_numpy(blocks.view(np.uint8)).to(dev)
    out = torch.full((L["inp"].shape[0],), POISON, dtype=torch.uint8, device=dev)
    status = torch.full((len(blocks),), -1, dtype=torch.int32, device=dev)
    crc = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx.bgzf_inflate_dev(comp, d_blocks, out, status, cnt)
    ctx.bgzf_crc32_dev(out, d_blocks, crc)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    got, got_crc = out.cpu().numpy(), crc.cpu().numpy().view(np.uint32)
    for k, (name, p) in enumerate(shapes):
        o = int(blocks["out_off"][k])
        assert np.array_equal(got[o:o + len(p)], p), name
        assert int(got_crc[k]) == zlib.crc32(p.tobytes()), name


@pytest.fixture(scope="module")
def fixture_bytes():
    return np.frombuffer(gzip.decompress(open(S.BAM_FIXTURES[0], "rb").read()), dtype=np.uint8)


def test_more_blocks_than_chains_one_block_and_none(ctx, work, fixture_bytes):
    """15000 blocks of 1 - 3 KB (30 MB): every chain of the launch comes back for work many times; then a launch of one block, and
    one of none (XM_OK without a launch: nothing is touched)"""
    import torch
    rng = np.random.default_rng(5)
    sizes = rng.integers(1024, 3073, 15000)
    starts = rng.integers(0, fixture_bytes.shape[0] - 3072, 15000)
    payloads = [fixture_bytes[int(s):int(s) + int(n)] for s, n in zip(starts, sizes)]
    inp, blocks, comp_bytes = layout(payloads)
    assert inp.shape[0] < 32 << 20
    comp, clen, status, inp_after, _ = gpu_deflate(ctx, work, inp, blocks, comp_bytes)
    assert (status == 0).all() and (clen <= sizes + 5).all() and np.array_equal(inp_after, inp)
    for k, p in enumerate(payloads):
        o = int(blocks["cdata_off"][k])
        assert inflates_to(comp[o:o + int(clen[k])], p.tobytes()), k
    assert outside_slots_is_poison(comp, blocks, sizes + 5)
    assert int(clen.sum()) < 0.7 * int(sizes.sum())                         # (BAM bytes: matches were found)
    # exactly one block
    inp, blocks, comp_bytes = layout([fixture_bytes[:50000]])
    comp, clen, status, _, _ = gpu_deflate(ctx, work, inp, blocks, comp_bytes)
    assert status[0] == 0 and inflates_to(comp[GUARD:GUARD + int(clen[0])], fixture_bytes[:50000].tobytes())
    assert outside_slots_is_poison(comp, blocks, [50005])
    # none
    dev = torch.device("cuda:0")
    some = torch.full((64,), POISON, dtype=torch.uint8, device=dev)
    empty = torch.zeros(0, dtype=torch.uint8, device=dev)
    ctx.bgzf_deflate_dev(some, empty, some, some, some, work)
    torch.cuda.synchronize()
    assert (some.cpu().numpy() == POISON).all()


def test_declined_blocks_are_named_and_leave_their_slot_alone(ctx, work, fixture_bytes):
    """plain argument checks: a payload longer than a block may hold, a slot smaller than n + 5, a slot that is not 16-byte
    aligned -- each a status of its own, clen 0 and a slot that is still poison, while the neighbours are encoded"""
    from xenomapper_amd import _ffi
    good = [fixture_bytes[10000 * k:10000 * k + 9000 + k] for k in range(7)]
    payloads = [good[0], fixture_bytes[:65281], good[1], good[2], good[3], good[4], good[5], good[6]]
    capacity = [len(p) + 5 for p in payloads]
    capacity[3] = len(payloads[3]) + 4
    inp, blocks, comp_bytes = layout(payloads, capacity=capacity, odd_slot=(5,))
    comp, clen, status, inp_after, _ = gpu_deflate(ctx, work, inp, blocks, comp_bytes)
    want = {1: "more payload bytes", 3: "smaller than the payload + 5", 5: "not 16-byte aligned"}
    written = []
    for k, p in enumerate(payloads):
        o = int(blocks["cdata_off"][k])
        if k in want:
            assert status[k] != 0 and clen[k] == 0 and want[k] in _ffi.bgzf_strerror(status[k]), k
            written.append(0)
        else:
            assert status[k] == 0 and inflates_to(comp[o:o + int(clen[k])], p.tobytes()), k
            written.append(len(p) + 5)
    assert len(set(int(status[k]) for k in want)) == 3
    assert outside_slots_is_poison(comp, blocks, written)
    assert np.array_equal(inp_after, inp)


def tiled_fixture(fixture_bytes, n):
    return np.tile(fixture_bytes, n // fixture_bytes.shape[0] + 1)[:n].copy()


@pytest.mark.parametrize("payload", [0, 64, 1000])
def test_compress_frames_complete_bgzf_members(ctx, fixture_bytes, payload):
    from xenomapper_amd import _ffi
    from xenomapper_amd import xenomapper as xm
    assert _ffi.BGZF_EOF == xm.BGZF_EOF
    P = payload or 65280
    rng = np.random.default_rng(payload)
    for n in (0, 1, 65279, 65280, 65281, 200000, 16 << 20):
        data = tiled_fixture(fixture_bytes, n)
        if n == 200000:
            data[100000:150000] = rng.integers(0, 256, 50000, dtype=np.uint8)       # some members in the stored form
        pinned = _ffi.pinned_bytes()
        got = ctx.bgzf_compress(data, payload)
        assert _ffi.pinned_bytes() == pinned
        assert got.shape[0] <= _ffi.bgzf_compress_bound(n, P)
        assert gzip.decompress(got.tobytes() + _ffi.BGZF_EOF) == data.tobytes(), n
        blocks, crc, nxt, total = _ffi.bgzf_index(got) if n else (np.zeros(0, dtype=_ffi.BGZF_BLOCK), None, 0, 0)
        assert nxt == got.shape[0] and total == n and len(blocks) == (n + P - 1) // P
        if n:
            assert (blocks["isize"][:-1] == P).all() and int(blocks["isize"][-1]) == n - P * (len(blocks) - 1)
        if n == 0:
            assert got.shape[0] == 0


def test_compress_refuses_a_short_buffer_and_beats_the_bound_on_bam_bytes(ctx, fixture_bytes):
    import ctypes
    from xenomapper_amd import _ffi
    from xenomapper_amd import xenomapper as xm
    data = tiled_fixture(fixture_bytes, 200000)
    bound = _ffi.bgzf_compress_bound(200000, 65280)
    out = np.full(bound + 8, POISON, dtype=np.uint8)
    got = ctypes.c_uint64(7)
    L = _ffi.lib()
    rc = L.xm_bgzf_compress(ctx._h, data.ctypes.data_as(ctypes.c_void_p), 200000, 0, out.ctypes.data_as(ctypes.c_void_p), bound - 1,
                            ctypes.byref(got))
    assert rc == -1 and (out == POISON).all()
    rc = L.xm_bgzf_compress(ctx._h, data.ctypes.data_as(ctypes.c_void_p), 200000, 63, out.ctypes.data_as(ctypes.c_void_p), bound + 8,
                            ctypes.byref(got))
    assert rc == -1 and (out == POISON).all()
    rc = L.xm_bgzf_compress(ctx._h, data.ctypes.data_as(ctypes.c_void_p), 200000, 0, out.ctypes.data_as(ctypes.c_void_p), bound,
                            ctypes.byref(got))
    assert rc == 0 and 0 < got.value <= bound and (out[bound:] == POISON).all()
    # the two paired-end fixtures whole: shorter than zlib level 1 in the same members x 1.15
    for path in S.BAM_FIXTURES[:2]:
        raw = gzip.decompress(open(path, "rb").read())
        ours, level1 = ctx.bgzf_compress(raw).shape[0], len(xm._bgzf_frame(raw, level=1))
        print("%s: %d bytes, encoder %d, zlib level 1 %d, x %.4f" % (os.path.basename(path), len(raw), ours, level1, ours / level1))
        assert ours < 1.15 * level1
