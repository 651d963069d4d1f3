"""Compressed BAM outputs (xm_bamdev_fetch_bins_bamz; output_format="bam", bam_compress=True; --bam_outputs --bam_compress): the
wanted records gathered, DEFLATED and BGZF-framed on the GPU.  Through the C ABI every bin's range is walked member by member (header,
BSIZE, zlib inflates the stream to ISIZE bytes with the trailer's CRC-32, all members but the last hold the payload asked for), holds
the records the unit lists select, and equals, byte for byte, what xm_bgzf_compress makes of those records -- the encoder is a
function of the payload bytes alone, so that pins the layout, the scan of the members' places and the pack kernel.  Through the file
path the outputs read back (oracle/bam_oracle.py) as the lines of the SAM run, are never longer than the stored route's, and come
out the same through the host assembler."""
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import bam_shapes as S
from tests import helpers as H
from tests.test_bam_gpu import run_whole_files
from tests.test_bam_out_cpu import EOF, HUMAN, KEYS, MOUSE
from tests.test_bam_out_gpu import compare, expected_bin, small_windows, tiled  # noqa: F401  (tiled: a fixture)
from tests.test_bam_shapes_gpu import Window

pytestmark = pytest.mark.gpu

ALL = 0b111111
HEAD16 = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
# bamz_place_kernel (xm_bamdev.hip) scans the members' lengths in one workgroup of 256 threads: up to 256 members a thread has one
# member and the scan is the LDS scan alone; beyond that a thread walks several members from its base
PLACE_TILE = 256


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import xenomapper as xm
    return xm.default_context()


def walk_members(image, payload_size):
    """Every member of a bin's range: the fixed 16 header bytes, BSIZE + 1 steps exactly to the next member and to the range's end, no
    member beyond 65280 + 5 + 26 bytes, the raw-DEFLATE stream inflates to ISIZE bytes with the trailer's CRC-32; all members but the
    last hold exactly payload_size bytes.  -> (the payload, [(member start, stream length)])"""
    at, out, where = 0, [], []
    while at < len(image):
        assert image[at:at + 16] == HEAD16, at
        size = struct.unpack_from("<H", image, at + 16)[0] + 1
        assert 26 < size <= 65280 + 5 + 26 and at + size <= len(image), (at, size)
        stream = image[at + 18:at + size - 8]
        crc, isize = struct.unpack_from("<II", image, at + size - 8)
        d = zlib.decompressobj(-15)
        body = d.decompress(stream)
        assert d.eof and not d.unused_data and len(body) == isize and zlib.crc32(body) == crc, at
        assert 0 < isize <= payload_size and len(stream) <= isize + 5, at
        out.append(body)
        where.append((at, len(stream)))
        at += size
    assert at == len(image) and all(len(b) == payload_size for b in out[:-1])
    return b"".join(out), where


class Checker(object):
    """The per-bin checks of one classified window, and what the runs covered."""

    def __init__(self, ctx, dev, n, paired, idx, off, raws, offs):
        self.ctx, self.dev, self.n, self.paired, self.idx, self.off, self.raws, self.offs = ctx, dev, n, paired, idx, off, raws, offs
        self.want, self.packed = {}, {}
        self.length_residues, self.start_residues, self.most_members = set(), set(), 0

    def expected(self, b, shift):
        key = (b, shift if b == 4 else 0)
        if key not in self.want:
            self.want[key] = expected_bin(b, self.idx[self.off[b]:self.off[b + 1]], self.paired, self.raws, self.offs, key[1])
        return self.want[key]

    def compressed(self, b, shift, payload):
        """xm_bgzf_compress on the bin's records: the reference every bin's bytes are compared with (made once per bin and payload)"""
        key = (b, shift if b == 4 else 0, payload)
        if key not in self.packed:
            self.packed[key] = self.ctx.bgzf_compress(self.expected(b, shift), payload).tobytes()
        return self.packed[key]

    def run(self, payload, mask, shift):
        status, stream, boff = self.dev.fetch_bins_bamz(0, self.n, self.paired, mask, payload, shift)
        assert status == 0
        self.dev.raw_wait(0)
        stream = bytes(stream)
        assert boff[0] == 0 and boff[6] == boff[7] == len(stream)
        members = 0
        for b in range(6):
            piece = stream[boff[b]:boff[b + 1]]
            if not (mask >> b) & 1 or self.off[b + 1] == self.off[b]:
                assert piece == b"", b
                continue
            want = self.expected(b, shift)
            got, where = walk_members(piece, payload or 65280)
            assert got == want, (payload, mask, shift, b)
            assert piece == self.compressed(b, shift, payload), (payload, mask, shift, b)
            members += len(where)
            self.length_residues |= set(n % 16 for _at, n in where)
            self.start_residues |= set((boff[b] + at) % 16 for at, _n in where)
        self.most_members = max(self.most_members, members)
        return len(stream)


MODES = ("liberal", "conservative", "single")
COVERED = {}                                                         # mode -> what its runs covered (c_abi_runs, once per mode)


def c_abi_runs(ctx, mode):
    """The two paired-end fixtures as one window, every payload x (mask, shift), every check per bin -> the mode's Checker."""
    if mode in COVERED:
        return COVERED[mode]
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
        # a fetch before classify is refused, as the stored call is
        with pytest.raises(ValueError, match="xm_bamdev_fetch_bins_bam"):
            dev.fetch_bins_bam(0, n, paired, ALL, 0, 0)
        with pytest.raises(ValueError, match="xm_bamdev_fetch_bins_bamz"):
            dev.fetch_bins_bamz(0, n, paired, ALL, 0, 0)
        raws = [bytes(_ffi._host_view(blk.raw_addr[f], blk.raw_len[f], np.uint8)) for f in (0, 1)]
        offs = [_ffi._host_view(blk.rec_off_addr[f], n, np.uint32).copy() for f in (0, 1)]
        code, idx, off, counts = dev.classify(0, {"liberal": _ffi.MODE_PE_LIBERAL, "conservative": _ffi.MODE_PE_CONSERVATIVE,
                                                  "single": _ffi.MODE_SE}[mode], n, -2**31)
        idx, off = idx.copy(), [int(v) for v in off]
        assert sum(1 for b in range(6) if off[b + 1] > off[b]) >= 2
        chk = Checker(ctx, dev, n, paired, idx, off, raws, offs)
        sizes = {}
        for payload in (64, 256, 4096, 0):
            for mask, shift in ((ALL, 0), (ALL, 7), (0b010110, 0), (0, 0)):
                sizes[(payload, mask, shift)] = chk.run(payload, mask, shift)
            assert sizes[(payload, 0, 0)] == 0
        if off[5] > off[4]:
            assert chk.expected(4, 0) != chk.expected(4, 7)               # (the shift is seen in `unresolved`)
        assert chk.most_members > PLACE_TILE, chk.most_members           # payload 64, every bin: the scan's threads walk several members
        # the last member of a bin exactly full, one byte long, one byte short of full: for one bin of L payload bytes the smallest
        # payloads P in 64 .. 65280 (several members: P < L) with L % P == 0, == 1 and == P - 1
        ran = None
        for b in sorted(range(6), key=lambda b: -(off[b + 1] - off[b])):
            if off[b + 1] == off[b]:
                continue
            L = len(chk.expected(b, 0))
            found = [next((P for P in range(64, min(L, 65281)) if L % P == r % P), None) for r in (0, 1, -1)]
            if None in found:
                continue
            for P, r in zip(found, (0, 1, -1)):
                assert L % P == r % P and L > P
                chk.run(P, ALL, 0)
                piece_members = (L + P - 1) // P
                assert piece_members >= 2 and L - P * (piece_members - 1) == (P, 1, P - 1)[(0, 1, -1).index(r)]
            ran = (b, L, found)
            break
        assert ran is not None, "no bin of the fixtures has the three payloads"
        # the declined payloads
        with pytest.raises(ValueError):
            dev.fetch_bins_bamz(0, n, paired, ALL, 63, 0)
        with pytest.raises(ValueError):
            dev.fetch_bins_bamz(0, n, paired, ALL, 65281, 0)
        # the stored call on the same slot still frames stored blocks, of the same payloads
        status, stream, boff = dev.fetch_bins_bam(0, n, paired, ALL, 4096, 0)
        assert status == 0
        dev.raw_wait(0)
        stream = bytes(stream)
        assert len(stream) > sizes[(4096, ALL, 0)]
        for b in range(6):
            if off[b + 1] > off[b]:
                assert walk_members(stream[boff[b]:boff[b + 1]], 4096)[0] == chk.expected(b, 0)
        COVERED[mode] = chk
        return chk
    finally:
        dev.close()


@pytest.mark.parametrize("mode", MODES)
def test_c_abi_every_bin_deflated_and_framed_on_the_device(ctx, mode):
    c_abi_runs(ctx, mode)


def test_c_abi_runs_reach_every_alignment_of_a_member(ctx):
    """Over the runs of the three modes (made here for a mode whose test has not run): the members' stream lengths hit every residue
    mod 16 (the pack kernel's whole 16-byte pieces and its tail), and so do the places the scan gives them (its unaligned stores)."""
    runs = [c_abi_runs(ctx, mode) for mode in MODES]
    lengths = set().union(*[chk.length_residues for chk in runs])
    starts = set().union(*[chk.start_residues for chk in runs])
    assert lengths == set(range(16)), sorted(lengths)
    assert starts == set(range(16)), sorted(starts)


@pytest.mark.parametrize("paired", [True, False])
def test_c_abi_records_of_38_bytes_to_63_kb(ctx, paired):
    """The `spread` window of tests/bam_shapes.py: records shorter than a lane's piece and records that fill a member, gathered
    without frames (record_fill_kernel<false>) and deflated."""
    win = Window(ctx, S.shape_records(paired, "spread"), paired)
    try:
        n = win.n
        assert n == len(win.recs[0]) >= S.MIN_RECORDS and not win.blk.unaligned and not win.blk.n_exceptions
        sizes = sorted(set(len(r) for r in win.recs[0]))
        assert sizes[0] == 38 and sizes[-1] > 63000
        idx, off = win.classify("liberal" if paired else "single")
        assert sum(1 for b in range(6) if off[b + 1] > off[b]) >= 5
        chk = Checker(ctx, win.dev, n, paired, idx, off, win.raws, win.offs)
        for payload in (256, 0):
            for shift in (0, 7):
                chk.run(payload, ALL, shift)
        if off[5] > off[4]:
            assert chk.expected(4, 0) != chk.expected(4, 7)
    finally:
        win.close()


# ---- the file path ----------------------------------------------------------------------------------------------------------

def run_one(paths, fmt, paired, conservative, tag, compress=False):
    """One call of the file path -> (counts, {key: what the sink holds}, profile, {key: bytes of the header}), as run_both's entries."""
    from xenomapper_amd import xenomapper as xm
    tag_func = {"AS": xm.get_tag, "NM": xm.get_cigarbased_AS_tag}[tag]
    sinks = {k: (io.StringIO() if fmt == "sam" else io.BytesIO()) for k in KEYS}
    kw = {"output_format": "bam"} if fmt == "bam" else {}
    with open(paths[0], "rb") as f1, open(paths[1], "rb") as f2:
        xm.process_headers(f1, f2, bam=True, **kw, **sinks)
    heads = {k: len(v.getvalue()) for k, v in sinks.items()}
    if compress:
        kw["bam_compress"] = True
    counts = xm.classify_sam_files(paths[0], paths[1], paired=paired, conservative=conservative, bam=True, tag_func=tag_func, **kw, **sinks)
    return dict(counts), {k: v.getvalue() for k, v in sinks.items()}, dict(xm.LAST_FILE_PROFILE), heads


@pytest.mark.parametrize("case", ["liberal", "cigar_scores", "single"])
def test_file_path_compressed_outputs_hold_the_lines_of_the_sam_run(tiled, monkeypatch, case):  # noqa: F811
    from xenomapper_amd import xenomapper as xm
    small_windows(monkeypatch, xm)
    paths = [tiled["human"], tiled["mouse"]]
    how = dict(paired=case != "single", conservative=False, tag="NM" if case == "cigar_scores" else "AS")
    sam = run_one(paths, "sam", **how)
    stored = run_one(paths, "bam", **how)
    bamz = run_one(paths, "bam", compress=True, **how)
    # counts, the end-of-file marker, header and lines as the SAM run's; nothing printed
    compare(sam, bamz, device=False)
    prof = bamz[2]
    assert prof["bam_windows"] > 4 and prof.get("bam_windows_device_bamz_bins", 0) > 0, prof
    assert not prof.get("bam_windows_device_bam_bins", 0) and not prof.get("bam_windows_device_text", 0) and not prof.get("bam_print", 0), prof
    assert stored[2].get("bam_windows_device_bam_bins", 0) > 0 and not stored[2].get("bam_windows_device_bamz_bins", 0)
    # never longer than the stored route's output of the same call, and smaller in all
    for key in KEYS:
        assert len(bamz[1][key]) <= len(stored[1][key]), key
    assert sum(len(v) for v in bamz[1].values()) < sum(len(v) for v in stored[1].values())
    # the same lines through the host assembler
    monkeypatch.setenv("XENOMAPPER_GPU_BAM_BINS", "0")
    host = run_one(paths, "bam", compress=True, **how)
    compare(sam, host, device=False)
    assert host[2].get("bam_windows_host_bam", 0) > 0 and not host[2].get("bam_windows_device_bamz_bins", 0), host[2]


def test_command_line_writes_what_the_api_call_writes(tiled, tmp_path):  # noqa: F811
    from xenomapper_amd import xenomapper as xm
    paths = [tiled["human"], tiled["mouse"]]
    sinks = {k: io.BytesIO() for k in KEYS}
    with open(paths[0], "rb") as f1, open(paths[1], "rb") as f2:
        xm.process_headers(f1, f2, bam=True, output_format="bam", **sinks)
    xm.classify_sam_files(paths[0], paths[1], paired=True, bam=True, output_format="bam", bam_compress=True, **sinks)
    assert xm.LAST_FILE_PROFILE.get("bam_windows_device_bamz_bins", 0) > 0
    outs = {k: str(tmp_path / (k + ".bam")) for k in KEYS}
    cmd = [sys.executable, "-m", "xenomapper_amd.xenomapper", "--primary_bam", paths[0], "--secondary_bam", paths[1], "--paired", "--bam_outputs",
           "--bam_compress"]
    for k in KEYS:
        cmd += ["--" + k, outs[k]]
    proc = subprocess.run(cmd, cwd=H.REPO, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    for k in KEYS:
        image = open(outs[k], "rb").read()
        assert image == sinks[k].getvalue() and image.endswith(EOF), k
    # ... and not what it writes without the flag
    plain = {k: io.BytesIO() for k in KEYS}
    with open(paths[0], "rb") as f1, open(paths[1], "rb") as f2:
        xm.process_headers(f1, f2, bam=True, output_format="bam", **plain)
    xm.classify_sam_files(paths[0], paths[1], paired=True, bam=True, output_format="bam", **plain)
    assert sum(len(v.getvalue()) for v in sinks.values()) < sum(len(v.getvalue()) for v in plain.values())
