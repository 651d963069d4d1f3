"""The hand-made DEFLATE corpus (tests/deflate_asm.py) through xm_bgzf_inflate_dev: every stream as a BGZF member, the corpus
twice in one launch (two orders, so every stream meets two output and two input alignments), members with one defect each
between the valid ones.  Valid members: status 0, zlib's bytes, the CRC-32 kernel equal to zlib.crc32.  Invalid members: exactly
the status that names the defect -- the same the host build of the decoder's source gives -- and nothing written outside their
own output.  Then every stream with one flipped bit: the kernel's verdict is zlib's.  The wide token loop, long_token() and the
lane-per-symbol table builder exist on the device only: this is the test that holds their copies of RFC 1951's arithmetic."""
import zlib

import numpy as np
import pytest

from tests import deflate_asm as A
from tests import helpers as H

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xEE, 64


def image_of(entries):
    """entries: [(stream, ISIZE, CRC field)] -> (the members back to back, their descriptors, bytes of output)"""
    from xenomapper_amd import _ffi
    image = np.frombuffer(b"".join(A.bgzf_member(*e) for e in entries), dtype=np.uint8)
    blocks, _crc, nxt, _total = _ffi.bgzf_index(image)
    assert nxt == image.shape[0] and len(blocks) == len(entries)
    assert [int(b["cdata_len"]) for b in blocks] == [len(e[0]) for e in entries]
    at = GUARD
    for k in range(len(blocks)):                                              # gaps of 0 .. 15 bytes between the outputs: they stay poison
        at += (k * 5) % 16
        blocks["out_off"][k] = at
        at += int(blocks["isize"][k])
    return image, blocks, at + GUARD


def inflate(image, blocks, out_bytes):
    """-> (the output buffer, poison where nothing was written; status per member; the CRC-32 kernel's word per member)"""
    import torch
    from xenomapper_amd import _ffi
    dev = torch.device("cuda:0")
    with _ffi.Context(0) as ctx:
        comp = torch.zeros(image.shape[0] + _ffi.BGZF_COMP_PAD, dtype=torch.uint8, device=dev)
        comp[:image.shape[0]] = torch.from_numpy(image.copy()).to(dev)
        d_blocks = torch.from_numpy(blocks.view(np.uint8)).to(dev)
        out = torch.full((out_bytes,), POISON, dtype=torch.uint8, device=dev)
        status = torch.full((len(blocks),), -1, dtype=torch.int32, device=dev)
        crc = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
        ctx.bgzf_inflate_dev(comp, d_blocks, out, status, torch.zeros(1, dtype=torch.int32, device=dev))
        ctx.bgzf_crc32_dev(out, d_blocks, crc)
        torch.cuda.synchronize()
        return out.cpu().numpy(), status.cpu().numpy(), crc.cpu().numpy().view(np.uint32)


def test_hand_made_streams_valid_and_invalid_in_one_launch(tmp_path):
    from xenomapper_amd import _ffi
    valid, invalid = A.valid_corpus(), A.invalid_corpus()
    # the two orders: an invalid member behind every second valid one (other neighbours the second time); a valid member ends each
    entries = []
    for order, phase, bad in ((valid, 1, list(invalid)), (valid[::-1], 0, invalid[7:] + invalid[:7])):
        for k, v in enumerate(order):
            entries.append(v)
            if bad and k % 2 == phase and k + 1 < len(order):
                entries.append(bad.pop(0))
        assert not bad and isinstance(entries[-1], A.Valid)
    # an invalid member carries a zero CRC field (deflate_asm's convention: a reader that runs past the end of its stream meets zeros)
    image, blocks, out_bytes = image_of([(e.stream, len(e.expected), zlib.crc32(e.expected)) if isinstance(e, A.Valid) else
                                         (e.stream, e.isize, 0) for e in entries])
    assert len({int(o) % 16 for o in blocks["out_off"]}) == 16 and len({int(c) % 128 for c in blocks["cdata_off"]}) >= 16
    for e in valid + invalid:                                                 # every stream at two alignments of its output or its input
        mine = [k for k, x in enumerate(entries) if x is e]
        assert len(mine) == 2 and len({(int(blocks["out_off"][k]) % 16, int(blocks["cdata_off"][k]) % 128) for k in mine}) == 2, e.name
    # what the host build says of the invalid streams (no sanitizer here: tests/test_inflate_streams_cpu.py runs it with them)
    exe = A.build_host_decoder(H.REPO, str(tmp_path / "inflate_core_host"), sanitize=False)
    host, _ = A.run_host_decoder(exe, [(v.stream, v.isize, 0, 0) for v in invalid], str(tmp_path))
    host_status = {v.name: r[0] for v, r in zip(invalid, host)}

    got, status, crc = inflate(image, blocks, out_bytes)

    want = np.full(out_bytes, POISON, dtype=np.uint8)
    own = np.zeros(out_bytes, dtype=bool)                                     # bytes an invalid member may have written
    wrong = []
    for k, e in enumerate(entries):
        o, n = int(blocks["out_off"][k]), int(blocks["isize"][k])
        if isinstance(e, A.Valid):
            assert zlib.decompress(e.stream, -15) == e.expected, e.name            # the reference's bytes are the interpreter's
            want[o:o + n] = np.frombuffer(e.expected, dtype=np.uint8)
            if status[k] != 0:
                wrong.append((k, e.name, "status %d: %s" % (status[k], _ffi.bgzf_strerror(status[k]))))
            elif not np.array_equal(got[o:o + n], want[o:o + n]):
                wrong.append((k, e.name, "byte %d of %d differs" % (int(np.nonzero(got[o:o + n] != want[o:o + n])[0][0]), n)))
            elif int(crc[k]) != zlib.crc32(e.expected):
                wrong.append((k, e.name, "crc"))
        else:
            own[o:o + n] = True
            if status[k] != e.status or status[k] != host_status[e.name]:
                wrong.append((k, e.name, "status %d, the corpus says %d, the host build %d" % (status[k], e.status, host_status[e.name])))
    assert not wrong, wrong[:12]
    assert _ffi.bgzf_strerror(A.ERR_INCOMPLETE).startswith("incomplete")
    # outside an invalid member's own output every byte is poison or a neighbour's right byte; the guards at both ends are poison
    outside = ~own
    assert np.array_equal(got[outside], want[outside]), np.nonzero((got != want) & outside)[0][:8]
    assert (got[:GUARD] == POISON).all() and (got[-GUARD:] == POISON).all()


def test_single_bit_damage_the_kernels_verdict_is_zlibs():
    """One flipped bit in every stream of the corpus, twenty times (deflate_asm.damaged_corpus): the kernel accepts a member exactly
    when zlib reaches the end of its stream, and then the bytes and the CRC-32 are zlib's; a refused member has written nothing
    outside its own output.  No status is named here: where a flip leaves two defects the wide loop may meet the other one first."""
    damaged = A.damaged_corpus()
    if not damaged[-1].accepted:                                              # a sound member ends the image
        damaged.append(next(d for d in damaged if d.accepted))
    image, blocks, out_bytes = image_of([(d.stream, d.isize, 0) for d in damaged])
    got, status, crc = inflate(image, blocks, out_bytes)
    want = np.full(out_bytes, POISON, dtype=np.uint8)
    own = np.zeros(out_bytes, dtype=bool)
    wrong = []
    for k, d in enumerate(damaged):
        o, n = int(blocks["out_off"][k]), int(blocks["isize"][k])
        if d.accepted:
            want[o:o + n] = np.frombuffer(d.expected, dtype=np.uint8)
            if status[k] != 0 or not np.array_equal(got[o:o + n], want[o:o + n]) or int(crc[k]) != zlib.crc32(d.expected):
                wrong.append((d.name, int(status[k]), "zlib accepts"))
        else:
            own[o:o + n] = True
            if status[k] == 0:
                wrong.append((d.name, 0, "zlib refuses"))
    assert not wrong, wrong[:12]
    assert np.array_equal(got[~own], want[~own]), np.nonzero((got != want) & ~own)[0][:8]
    assert (got[:GUARD] == POISON).all() and (got[-GUARD:] == POISON).all()
