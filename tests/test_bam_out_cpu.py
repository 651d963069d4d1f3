"""BAM outputs (output_format="bam"), the host's share, without a GPU: the refusals that come before the device is touched, the
BAM headers process_headers writes (text and binary reference list, `unresolved` with both inputs' lists), and the host framer.
The reader is the oracle's (oracle/bam_oracle.py)."""
import gzip
import io
import os
import struct

import pytest

from tests import helpers as H
from oracle import bam_oracle

DATA = os.path.join(H.REPO, "tests", "golden", "ref_data")
HUMAN = os.path.join(DATA, "paired_end_testdata_human.bam")
MOUSE = os.path.join(DATA, "paired_end_testdata_mouse.bam")
# the 28-byte BGZF end-of-file marker (SAM specification 4.1.2), written out here so that the tests do not take it from the code
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
KEYS = ("primary_specific", "secondary_specific", "primary_multi", "secondary_multi", "unassigned", "unresolved")


def split_header(raw):
    """(text, [(name, length)], bytes of the header) of an inflated BAM image (SAM specification 4.2)."""
    assert raw[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        name = raw[at + 4:at + 4 + l_name]
        assert name[-1:] == b"\0"
        refs.append((name[:-1], struct.unpack_from("<i", raw, at + 4 + l_name)[0]))
        at += 8 + l_name
    return raw[8:8 + l_text], refs, at


def renamed_copy(src, dst, prefix=b"m_"):
    """The BAM file `src` with every reference renamed, in the header text's @SQ lines and in the binary list (the records keep
    their reference ids): an input whose names do not clash with the other species' file."""
    import sys
    sys.path.insert(0, os.path.join(H.REPO, "tools"))
    import bench_bam
    raw = gzip.decompress(open(src, "rb").read())
    text, refs, at = split_header(raw)
    lines = [(l.replace(b"\tSN:", b"\tSN:" + prefix) if l[:3] == b"@SQ" else l) for l in text.split(b"\n")]
    text = b"\n".join(lines)
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        head += struct.pack("<i", len(prefix + name) + 1) + prefix + name + b"\0" + struct.pack("<i", length)
    with open(dst, "wb") as fh:
        fh.write(bench_bam.bgzf_blocks(head) + bench_bam.record_aligned_blocks(raw[at:]) + bench_bam.BGZF_EOF)
    return dst


def members(image):
    """[(member bytes, BSIZE)] of a BGZF image, every member's fixed header checked."""
    out, at = [], 0
    while at < len(image):
        assert image[at:at + 4] == b"\x1f\x8b\x08\x04" and image[at + 10:at + 16] == b"\x06\x00BC\x02\x00"
        bsize, = struct.unpack_from("<H", image, at + 16)
        out.append((image[at:at + bsize + 1], bsize))
        at += bsize + 1
    assert at == len(image)
    return out


def sam_route_headers(paths):
    from xenomapper_amd import xenomapper as xm
    sinks = {k: io.StringIO() for k in KEYS}
    with open(paths[0], "rb") as f1, open(paths[1], "rb") as f2:
        xm.process_headers(f1, f2, bam=True, **sinks)
    return {k: v.getvalue() for k, v in sinks.items()}


def bam_route_headers(paths, keys=KEYS):
    from xenomapper_amd import xenomapper as xm
    sinks = {k: io.BytesIO() for k in keys}
    with open(paths[0], "rb") as f1, open(paths[1], "rb") as f2:
        xm.process_headers(f1, f2, bam=True, output_format="bam", **sinks)
    return {k: v.getvalue() for k, v in sinks.items()}


def test_refusals_before_the_device_is_touched_leave_the_sinks_empty(tmp_path):
    from xenomapper_amd import xenomapper as xm
    sam = [os.path.join(DATA, "paired_end_testdata_%s.sam" % t) for t in ("human", "mouse")]
    sinks = [io.BytesIO() for _ in range(6)]
    with pytest.raises(ValueError):                                  # SAM inputs
        xm.classify_sam_files(sam[0], sam[1], *sinks, paired=True, output_format="bam")
    assert not any(s.getvalue() for s in sinks)
    shared = io.BytesIO()
    sinks = [io.BytesIO(), io.BytesIO(), shared, shared, None, None]
    with pytest.raises(ValueError):                                  # two bins, one sink
        xm.classify_sam_files(HUMAN, MOUSE, *sinks, paired=True, bam=True, output_format="bam")
    assert not any(s.getvalue() for s in sinks if s)
    sinks = [io.BytesIO(), io.StringIO()] + [None] * 4
    with pytest.raises(TypeError):                                   # a sink that takes text only
        xm.classify_sam_files(HUMAN, MOUSE, *sinks, paired=True, bam=True, output_format="bam")
    assert not any(s.getvalue() for s in sinks if s)
    with open(HUMAN, "rb") as f1, open(MOUSE, "rb") as f2:           # the same sinks are refused by process_headers
        with pytest.raises(TypeError):
            xm.process_headers(f1, f2, sinks[0], sinks[1], bam=True, output_format="bam")
        with pytest.raises(ValueError):
            xm.process_headers(f1, f2, shared, shared, bam=True, output_format="bam")
    assert not any(s.getvalue() for s in sinks if s) and not shared.getvalue()
    with open(sam[0]) as f1, open(sam[1]) as f2:
        with pytest.raises(ValueError):
            xm.process_headers(f1, f2, io.BytesIO(), output_format="bam")


def test_headers_hold_the_sam_route_text_and_the_inputs_reference_lists():
    from xenomapper_amd import xenomapper as xm
    keys = KEYS[:5]                                                  # (`unresolved`: the tests below)
    want = sam_route_headers((HUMAN, MOUSE))
    got = bam_route_headers((HUMAN, MOUSE), keys)
    lists = [split_header(gzip.decompress(open(p, "rb").read()))[1] for p in (HUMAN, MOUSE)]
    plan = {key: which for key, which, _comment in xm._HEADER_PLAN}
    for key in keys:
        header, lines = bam_oracle.bam_to_sam(got[key] + EOF)
        assert header == want[key] and lines == []
        text, refs, end = split_header(gzip.decompress(got[key]))
        assert text.decode("ascii") == want[key]
        assert refs == lists[plan[key]] and len(refs) > 0
        assert end == len(gzip.decompress(got[key]))


def test_unresolved_with_names_in_both_inputs_is_refused_before_anything_is_written():
    from xenomapper_amd import xenomapper as xm
    lists = [split_header(gzip.decompress(open(p, "rb").read()))[1] for p in (HUMAN, MOUSE)]
    clash = [name for name, _l in lists[1] if name in set(n for n, _l in lists[0])]
    sinks = {k: io.BytesIO() for k in KEYS}
    with open(HUMAN, "rb") as f1, open(MOUSE, "rb") as f2:
        if clash:
            with pytest.raises(ValueError) as err:
                xm.process_headers(f1, f2, bam=True, output_format="bam", **sinks)
            assert clash[0].decode("ascii") in str(err.value)
            assert not any(s.getvalue() for s in sinks.values())
        else:
            xm.process_headers(f1, f2, bam=True, output_format="bam", **sinks)
            assert all(s.getvalue() for s in sinks.values())


def test_unresolved_gets_both_reference_lists_and_file_2s_sq_lines_behind_file_1s(tmp_path):
    mouse = renamed_copy(MOUSE, str(tmp_path / "mouse_renamed.bam"))
    lists = [split_header(gzip.decompress(open(p, "rb").read()))[1] for p in (HUMAN, mouse)]
    assert all(name.startswith(b"m_") for name, _l in lists[1])
    want = sam_route_headers((HUMAN, mouse))
    got = bam_route_headers((HUMAN, mouse))
    text, refs, _end = split_header(gzip.decompress(got["unresolved"]))
    assert refs == lists[0] + lists[1]
    # the text: file 1's, with file 2's @SQ lines behind file 1's last @SQ line
    mine = want["unresolved"].split("\n")
    sq2 = [l for l in want["secondary_specific"].split("\n") if l[:3] == "@SQ"]
    last = max(k for k, l in enumerate(mine) if l[:3] == "@SQ")
    assert text.decode("ascii") == "\n".join(mine[:last + 1] + sq2 + mine[last + 1:])
    # text and list agree, in order
    assert [l.split("\t")[1][3:].encode() for l in text.decode("ascii").split("\n") if l[:3] == "@SQ"] == [n for n, _l in refs]
    header, lines = bam_oracle.bam_to_sam(got["unresolved"] + EOF)
    assert header == text.decode("ascii") and lines == []
    # the other sinks are what they are without `unresolved`
    for key in KEYS[:5]:
        assert split_header(gzip.decompress(got[key]))[0].decode("ascii") == want[key]


def test_host_framer():
    import zlib
    from xenomapper_amd import xenomapper as xm
    assert xm._bgzf_frame(b"") == b""
    rng = __import__("numpy").random.default_rng(5)
    for payload in (b"x", bytes(rng.integers(0, 256, size=65280, dtype="uint8")), bytes(rng.integers(0, 256, size=200000, dtype="uint8")),
                    b"@SQ\tSN:chr1\tLN:1000\n" * 10000):
        for level in (1, 6):
            image = xm._bgzf_frame(payload, level)
            assert gzip.decompress(image) == payload
            parts = members(image)
            assert len(parts) == (len(payload) + 65279) // 65280
            for part, bsize in parts:
                assert len(part) <= 65536 and bsize == len(part) - 1
                isize, = struct.unpack_from("<I", part, len(part) - 4)
                assert 0 < isize <= 65280
                assert struct.unpack_from("<I", part, len(part) - 8)[0] == zlib.crc32(zlib.decompress(part[18:-8], -15))
    assert xm.BGZF_EOF == EOF and len(EOF) == 28 and gzip.decompress(EOF) == b""
    # a header of 200 KB splits into members, and reads back
    refs = [(b"contig%05d" % k, 1000 + k) for k in range(9000)]
    text = "".join("@SQ\tSN:contig%05d\tLN:%d\n" % (k, 1000 + k) for k in range(9000))
    raw = xm._bam_header_bytes(text, refs)
    assert len(raw) > 200000
    image = xm._bgzf_frame(raw)
    assert len(members(image)) == (len(raw) + 65279) // 65280 > 3
    assert split_header(gzip.decompress(image)) == (text.encode(), refs, len(raw))


def test_host_assembler_takes_the_units_records_in_order():
    """_bam_records_of on a hand-made window: the order within a unit (records i - 1 and i, file 1 before file 2 in `unresolved`),
    which file a bin reads, and the reference shift of file 2's records in `unresolved` only."""
    import numpy as np
    from xenomapper_amd import xenomapper as xm

    def rec(ref, nxt, fill, extra):
        body = struct.pack("<ii", ref, 7) + bytes([fill]) * 12 + struct.pack("<i", nxt) + bytes([fill]) * (8 + extra)
        return struct.pack("<I", len(body)) + body
    recs = [[rec(k, -1 if k % 2 else k, 0x10 + k, k) for k in range(6)], [rec(k, k, 0x40 + k, 2 * k) for k in range(6)]]
    raws = [np.frombuffer(b"".join(r), dtype=np.uint8) for r in recs]
    offs = [np.cumsum([0] + [len(x) for x in r[:-1]]).astype(np.uint32) for r in recs]
    seg = np.array([1, 5], dtype=np.uint32)
    assert bytes(xm._bam_records_of(seg, True, 0, raws, offs, 7)) == recs[0][0] + recs[0][1] + recs[0][4] + recs[0][5]
    assert bytes(xm._bam_records_of(seg, True, 3, raws, offs, 7)) == recs[1][0] + recs[1][1] + recs[1][4] + recs[1][5]
    assert bytes(xm._bam_records_of(seg, False, 2, raws, offs, 7)) == recs[0][1] + recs[0][5]
    assert bytes(xm._bam_records_of(seg[:0], True, 4, raws, offs, 7)) == b""
    shifted = [rec(k + 7, k + 7, 0x40 + k, 2 * k) for k in range(6)]
    assert bytes(xm._bam_records_of(seg, True, 4, raws, offs, 7)) == (recs[0][0] + recs[0][1] + shifted[0] + shifted[1] +
                                                                      recs[0][4] + recs[0][5] + shifted[4] + shifted[5])
    none = [rec(-1, -1, 0x40, 0)]
    got = xm._bam_records_of(np.array([0]), False, 4, [raws[0], np.frombuffer(none[0], dtype=np.uint8)], [offs[0], np.array([0], dtype=np.uint32)], 7)
    assert bytes(got) == recs[0][0] + none[0]                        # fields below 0 stay


def test_the_header_reader_takes_members_with_further_gzip_subfields(tmp_path):
    """A BGZF member may carry other gzip subfields beside BC (RFC 1952 2.3.1.1; SAM specification 4.1): the reference list is read
    through them, and a BytesIO handle (no descriptor to map) gives the same headers as the file."""
    from xenomapper_amd import xenomapper as xm
    image, out, at = open(HUMAN, "rb").read(), bytearray(), 0
    extra = b"XY\x03\x00abc"
    while at < len(image):
        size = struct.unpack_from("<H", image, at + 16)[0] + 1
        member = image[at:at + size]
        out += member[:10] + struct.pack("<H", 6 + len(extra)) + extra + b"BC\x02\x00" + struct.pack("<H", size + len(extra) - 1) + member[18:]
        at += size
    assert gzip.decompress(bytes(out)) == gzip.decompress(image)
    path = str(tmp_path / "subfields.bam")
    open(path, "wb").write(out)
    want_refs = split_header(gzip.decompress(image))[1]
    got = []
    for handle in (open(path, "rb"), io.BytesIO(bytes(out))):
        sink = io.BytesIO()
        with handle, open(MOUSE, "rb") as f2:
            xm.process_headers(handle, f2, bam=True, output_format="bam", primary_specific=sink)
        assert split_header(gzip.decompress(sink.getvalue()))[1] == want_refs
        got.append(sink.getvalue())
    assert got[0] == got[1]
