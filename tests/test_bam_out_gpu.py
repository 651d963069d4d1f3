"""BAM outputs for BAM inputs (output_format="bam"): the wanted records gathered and BGZF-framed ON THE GPU
(xm_bamdev_fetch_bins_bam: members of stored DEFLATE blocks, CRC-32s made on the device), first through the C ABI against the
records the unit lists select, then through the file path against the SAM-text run of the same call, read back with the oracle's
BAM reader (oracle/bam_oracle.py), and the routes that assemble on the host instead."""
import gzip
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import helpers as H
from tests.test_bam_gpu import run_whole_files
from tests.test_bam_out_cpu import EOF, HUMAN, KEYS, MOUSE, renamed_copy, split_header

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(H.REPO, "tools"))


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import xenomapper as xm
    return xm.default_context()


def files_of_bin(b):
    return (0, 1) if b == 4 else ((1,) if b in (1, 3) else (0,))


def expected_bin(b, seg, paired, raws, offs, shift=0):
    """The records of bin b's units, in the order the reference prints their lines (xenomapper.py:332-350, :423-448, :521-550)."""
    out = bytearray()
    for i in seg:
        for f in files_of_bin(b):
            for r in ((int(i) - 1, int(i)) if paired else (int(i),)):
                at = int(offs[f][r])
                size, = struct.unpack_from("<I", raws[f], at)
                rec = bytearray(raws[f][at:at + 4 + size])
                if shift and b == 4 and f == 1:
                    for field in (4, 24):
                        v, = struct.unpack_from("<i", rec, field)
                        if v >= 0:
                            struct.pack_into("<i", rec, field, v + shift)
                out += rec
    return bytes(out)


def check_members(image, payload_size):
    """Every member of a framed range: fixed header, BSIZE, one stored block (01 LEN NLEN), CRC-32 and ISIZE; all but the last hold
    exactly payload_size record bytes.  -> the payload."""
    at, out, sizes = 0, [], []
    while at < len(image):
        assert image[at:at + 16] == b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00", at
        bsize, = struct.unpack_from("<H", image, at + 16)
        final, ln, nln = struct.unpack_from("<BHH", image, at + 18)
        assert final == 1 and ln ^ nln == 0xFFFF and bsize + 1 == ln + 31
        body = image[at + 23:at + 23 + ln]
        crc, isize = struct.unpack_from("<II", image, at + 23 + ln)
        assert isize == ln and 0 < ln <= payload_size and crc == zlib.crc32(body)
        out.append(body)
        sizes.append(ln)
        at += bsize + 1
    assert at == len(image) and all(s == payload_size for s in sizes[:-1])
    return b"".join(out)


@pytest.mark.parametrize("mode", ["liberal", "conservative", "single"])
def test_c_abi_records_of_every_bin_framed_on_the_device(ctx, mode):
    from xenomapper_amd import _ffi
    images = [open(p, "rb").read() for p in (HUMAN, MOUSE)]
    paired = mode != "single"
    dev = _ffi.BamDev(ctx)
    try:
        blk, readers = run_whole_files(dev, images, 0, paired, skip_repeated=not paired)
        for r in readers:
            r.close()
        n = blk.n
        assert n > 200 and not blk.unaligned and not blk.n_exceptions
        raws = [bytes(_ffi._host_view(blk.raw_addr[f], blk.raw_len[f], np.uint8)) for f in (0, 1)]
        offs = [_ffi._host_view(blk.rec_off_addr[f], n, np.uint32).copy() for f in (0, 1)]
        sizes = [struct.unpack_from("<I", raws[0], int(o))[0] + 4 for o in offs[0]]
        assert min(sizes) < 256 < max(sizes)                         # at payload 256 records span two members, at 64 several
        code, idx, off, counts = dev.classify(0, {"liberal": _ffi.MODE_PE_LIBERAL, "conservative": _ffi.MODE_PE_CONSERVATIVE,
                                                  "single": _ffi.MODE_SE}[mode], n, -2**31)
        idx, off = idx.copy(), [int(v) for v in off]
        assert sum(1 for b in range(6) if off[b + 1] > off[b]) >= 2
        plain = {}
        for payload in (64, 256, 4096, 0):
            for mask, shift in ((0b111111, 0), (0b111111, 7), (0b010110, 0), (0, 0)):
                status, stream, boff = dev.fetch_bins_bam(0, n, paired, mask, payload, shift)
                assert status == 0
                dev.raw_wait(0)
                stream = bytes(stream)
                assert boff[0] == 0 and boff[6] == boff[7] == len(stream)
                for b in range(6):
                    piece = stream[boff[b]:boff[b + 1]]
                    if not (mask >> b) & 1 or off[b + 1] == off[b]:
                        assert piece == b""
                        continue
                    want = expected_bin(b, idx[off[b]:off[b + 1]], paired, raws, offs, shift)
                    assert gzip.decompress(piece) == want
                    assert check_members(piece, payload or 65280) == want
                    if mask == 0b111111 and shift == 0:
                        plain[(payload, b)] = want
                    elif mask == 0b111111:
                        # the shift changes exactly the two fields of file 2's records in bin 4 that are >= 0, nothing else
                        assert (want == plain[(payload, b)]) == (b != 4)
                        assert want == expected_bin(b, idx[off[b]:off[b + 1]], paired, raws, offs, 7)
        if off[5] > off[4]:
            assert plain[(0, 4)] != expected_bin(4, idx[off[4]:off[5]], paired, raws, offs, 7)
        with pytest.raises(ValueError):
            dev.fetch_bins_bam(0, n, paired, 0b111111, 63, 0)
        with pytest.raises(ValueError):
            dev.fetch_bins_bam(0, n, paired, 0b111111, 65281, 0)
    finally:
        dev.close()


# ---- the file path ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiled(tmp_path_factory):
    """The fixtures tiled 40 times (many windows of 1 MB, carried tails, halo records): human, mouse with its references renamed
    (no name in both inputs, so `unresolved` can be BAM), the same with blocks that cut records, and human with renamed references."""
    import bench_bam
    d = tmp_path_factory.mktemp("bam_out")
    mouse = renamed_copy(MOUSE, str(d / "mouse_renamed.bam"))
    human2 = renamed_copy(HUMAN, str(d / "human_renamed.bam"))
    out = {}
    for key, src, aligned in (("human", HUMAN, True), ("mouse", mouse, True), ("human_cut", HUMAN, False), ("mouse_cut", mouse, False),
                              ("human_renamed", human2, True)):
        out[key] = str(d / ("%s_x40.bam" % key))
        bench_bam.tiled_bam(src, out[key], 40, aligned=aligned)
    return out


def small_windows(monkeypatch, xm):
    """Windows of 1 MB: the engine asks the GPU BAM front end for max(FILE_WINDOW_BYTES, BAM_GPU_WINDOW_BYTES) of each file, so both
    are lowered (as tests/test_bam_gpu.py does where it counts windows); the tiled inputs then take many windows."""
    monkeypatch.setattr(xm, "BAM_GPU_WINDOW_BYTES", 1 << 20)
    monkeypatch.setattr(xm, "FILE_WINDOW_BYTES", 1 << 20)


def run_both(paths, paired=True, conservative=False, tag="AS", keys=KEYS):
    """The same call with SAM-text outputs and with BAM outputs -> ((counts, {key: header + text}), (counts, {key: image}, profile))."""
    from xenomapper_amd import xenomapper as xm
    tag_func = {"AS": xm.get_tag, "NM": xm.get_cigarbased_AS_tag}[tag]
    res = []
    for fmt in ("sam", "bam"):
        sinks = {k: (io.StringIO() if fmt == "sam" else io.BytesIO()) for k in keys}
        kw = {"output_format": "bam"} if fmt == "bam" else {}
        with open(paths[0], "rb") as f1, open(paths[1], "rb") as f2:
            xm.process_headers(f1, f2, bam=True, **kw, **sinks)
        heads = {k: len(v.getvalue()) for k, v in sinks.items()}
        counts = xm.classify_sam_files(paths[0], paths[1], paired=paired, conservative=conservative, bam=True, tag_func=tag_func, **kw, **sinks)
        res.append((dict(counts), {k: v.getvalue() for k, v in sinks.items()}, dict(xm.LAST_FILE_PROFILE), heads))
    return res


def compare(sam, bam, device=True):
    from oracle import bam_oracle
    assert bam[0] == sam[0] and sum(sam[0].values()) > 0
    prof = bam[2]
    for key, image in bam[1].items():
        assert image.endswith(EOF)
        header, lines = bam_oracle.bam_to_sam(image)
        want = sam[1][key]
        want_header = want[:sam[3][key]]
        if key == "unresolved":
            # the one output with records of both inputs: file 1's text with file 2's @SQ lines behind file 1's last @SQ line
            mine = want_header.split("\n")
            sq2 = [l for l in sam[1]["secondary_specific"][:sam[3]["secondary_specific"]].split("\n") if l[:3] == "@SQ"]
            last = max(k for k, l in enumerate(mine) if l[:3] == "@SQ")
            want_header = "\n".join(mine[:last + 1] + sq2 + mine[last + 1:])
        assert header == want_header
        assert "".join(l + "\n" for l in lines) == want[sam[3][key]:], key
        # size: stored blocks cost 31 bytes per 65280 of records, and a short last member per (window, bin)
        raw = gzip.decompress(image)
        records = len(raw) - split_header(raw)[2]
        assert len(image) <= records * (1 + 31 / 65280) + 31 * prof["bam_windows"] + bam[3][key] + 28, key
    if device:
        assert prof.get("bam_windows_device_bam_bins", 0) > 0, prof
    assert not prof.get("bam_windows_device_text", 0) and not prof.get("bam_print", 0), prof


@pytest.mark.parametrize("case", ["liberal", "conservative", "cigar_scores", "single"])
def test_file_path_bam_outputs_hold_the_lines_of_the_sam_run(tiled, monkeypatch, case):
    from xenomapper_amd import xenomapper as xm
    small_windows(monkeypatch, xm)
    sam, bam = run_both([tiled["human"], tiled["mouse"]], paired=case != "single", conservative=case == "conservative",
                        tag="NM" if case == "cigar_scores" else "AS")
    compare(sam, bam)
    assert bam[2]["bam_windows"] > 4
    if case == "liberal":
        # file 2's records print under file 2's names in `unresolved`, file 1's under file 1's
        from oracle import bam_oracle
        _header, lines = bam_oracle.bam_to_sam(bam[1]["unresolved"])
        rnames = set(l.split("\t")[2] for l in lines)
        assert any(r.startswith("m_") for r in rnames) and any(not r.startswith("m_") and r != "*" for r in rnames)


def test_raw_windows_are_assembled_on_the_host(tiled, monkeypatch):
    """Blocks that cut records: the device reports the windows as unaligned, the host walks them, the text rules classify them,
    and the records come from the whole windows."""
    from xenomapper_amd import xenomapper as xm
    small_windows(monkeypatch, xm)
    for paired in (True, False):                                     # (single-end: the skipping walk, pair k is not record k)
        sam, bam = run_both([tiled["human_cut"], tiled["mouse_cut"]], paired=paired)
        compare(sam, bam, device=False)
        assert bam[2].get("bam_windows_raw", 0) > 0


def test_packed_records_are_assembled_on_the_host(tiled, monkeypatch):
    from xenomapper_amd import xenomapper as xm
    small_windows(monkeypatch, xm)
    monkeypatch.setenv("XENOMAPPER_GPU_BAM_BINS", "0")
    sam, bam = run_both([tiled["human"], tiled["mouse"]])
    compare(sam, bam, device=False)
    assert bam[2].get("bam_windows_host_bam", 0) > 0 and not bam[2].get("bam_windows_device_bam_bins", 0)


def test_all_unresolved_same_records_on_both_sides(tiled, monkeypatch):
    """The same records on both sides (file 2 with renamed references): every pair is unresolved, every record of both files is
    wanted -- whether the framed stream fits the slot's buffers (device) or not (status 2, the packed records), the lines are equal."""
    from xenomapper_amd import xenomapper as xm
    small_windows(monkeypatch, xm)
    xm.release_buffers()                                             # a fresh front end: the process-wide one keeps the largest
    try:                                                             # buffers any earlier run asked for
        sam, bam = run_both([tiled["human"], tiled["human_renamed"]])
    finally:
        xm.release_buffers()
    compare(sam, bam, device=False)
    assert len(bam[1]["unresolved"]) > 40 * 100000 and bam[2].get("bam_windows_device_bam_bins", 0) + bam[2].get("bam_windows_host_bam", 0) > 0
    assert all(len(bam[1][k]) == bam[3][k] + 28 for k in KEYS[:4])   # header and marker only


def test_without_the_gpu_bam_front_end_bam_outputs_are_refused(monkeypatch):
    from xenomapper_amd import xenomapper as xm
    monkeypatch.setenv("XENOMAPPER_GPU_BAM", "0")
    sinks = [io.BytesIO() for _ in range(5)]
    with pytest.raises(RuntimeError, match="BAM outputs need"):
        xm.classify_sam_files(HUMAN, MOUSE, *sinks, paired=True, bam=True, output_format="bam")
    assert not any(s.getvalue() for s in sinks)
    with pytest.raises(RuntimeError, match="BAM outputs need"):      # a min_score the device path does not take
        monkeypatch.delenv("XENOMAPPER_GPU_BAM")
        xm.classify_sam_files(HUMAN, MOUSE, *sinks, paired=True, bam=True, output_format="bam", min_score=float("nan"))
    assert not any(s.getvalue() for s in sinks)


def test_command_line_writes_what_the_api_call_writes(tiled, tmp_path):
    from xenomapper_amd import xenomapper as xm
    paths = [tiled["human"], tiled["mouse"]]
    sinks = {k: io.BytesIO() for k in KEYS}
    with open(paths[0], "rb") as f1, open(paths[1], "rb") as f2:
        xm.process_headers(f1, f2, bam=True, output_format="bam", **sinks)
    xm.classify_sam_files(paths[0], paths[1], paired=True, bam=True, output_format="bam", **sinks)
    outs = {k: str(tmp_path / (k + ".bam")) for k in KEYS}
    cmd = [sys.executable, "-m", "xenomapper_amd.xenomapper", "--primary_bam", paths[0], "--secondary_bam", paths[1], "--paired", "--bam_outputs"]
    for k in KEYS:
        cmd += ["--" + k, outs[k]]
    proc = subprocess.run(cmd, cwd=H.REPO, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    for k in KEYS:
        assert open(outs[k], "rb").read() == sinks[k].getvalue(), k
    # SAM inputs with the flag: the usage error
    sam = os.path.join(H.REPO, "tests", "golden", "ref_data", "paired_end_testdata_human.sam")
    proc = subprocess.run([sys.executable, "-m", "xenomapper_amd.xenomapper", "--primary_sam", sam, "--secondary_sam", sam, "--bam_outputs"],
                          cwd=H.REPO, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 2 and "--bam_outputs needs" in proc.stderr
