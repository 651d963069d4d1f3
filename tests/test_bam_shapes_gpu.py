"""The device SAM printer (xm_bamdev.hip: sam_line / WriteChars / fmt_g_f32, launched by text_fill_kernel and line_fill_kernel) and
the BAM framer (record_fill_kernel / record_to_frames / bam_frame_kernel) on the images of tests/bam_shapes.py, through the C ABI as
tests/test_bam_gpu.py and tests/test_bam_out_gpu.py go through it: every trip boundary of every loop, records of 38 bytes and of
63 KB in one wave.  Every comparison is byte for byte, against oracle/bam_oracle.py's line of the raw record (floating-point values:
printf("%g"), a NaN with its sign); every fetch must return status 0 -- a declined window cannot pass as a comparison skipped."""
import functools
import gzip
import struct

import numpy as np
import pytest

from oracle import bam_oracle
from tests import bam_shapes as S
from tests.test_bam_out_gpu import check_members, expected_bin, files_of_bin
from tests.test_bam_gpu import run_whole_files

pytestmark = pytest.mark.gpu

ABSENT = -2**31
ALL = 0b111111


@pytest.fixture(scope="module")
def ctx():
    from xenomapper_amd import xenomapper as xm
    return xm.default_context()


@functools.lru_cache(maxsize=None)
def line_of(rec):
    """The expected SAM line of one record (with its block_size word), as bytes without the newline."""
    return S.expected_line(rec[4:], bam_oracle.record_to_line(rec[4:], S.REFS)).encode("latin-1")


def shape_of(rec):
    p = S.parse(rec[4:])
    out = {key: p[key] for key in ("size", "l_seq", "ref", "pos", "mapq", "flag", "next_ref", "next_pos", "tlen")}
    out.update(l_read_name=len(p["name_field"]), nul_at=p["name_field"].index(b"\0"), n_cigar=p["cigar"].shape[0],
               qual0=p["qual"][0] if p["qual"] else None, top_bit_qual=bool(p["qual"]) and max(p["qual"]) >= 128,
               fields=[(t[0], t[1], t[2], len(t[3])) for t in p["fields"]][:6])
    return out


def first_difference(got, parts):
    """got: bytes; parts: [(label, record, expected bytes)] that should lie back to back in it -> None, or a description of the first
    part that differs: the record's shape and the offset of the first differing byte inside its line."""
    at = 0
    for label, rec, want in parts:
        mine = got[at:at + len(want)]
        if mine != want:
            j = next((k for k in range(min(len(mine), len(want))) if mine[k] != want[k]), min(len(mine), len(want)))
            return "%r: byte %d of %d: got %r, want %r; record %r" % (label, j, len(want), mine[max(0, j - 16):j + 24], want[max(0, j - 16):j + 24],
                                                                       shape_of(rec))
        at += len(want)
    if at != len(got):
        return "%d bytes behind the last expected line" % (len(got) - at)
    return None


class Window(object):
    """Two record lists inflated and stripped on the device as one window of slot 0, room reserved for their text, the reference
    names set; raws / offs / recs: the inflated windows on the host, the record tables, and the records cut out of them."""

    def __init__(self, ctx, files, paired):
        from xenomapper_amd import _ffi
        self.ffi, self.paired = _ffi, paired
        images = [S.image_of(r) for r in files]
        raw_len = max(sum(len(r) for r in recs) for recs in files) + 4096
        self.dev = dev = _ffi.BamDev(ctx)
        try:
            # a B:f array prints as about three times its bytes, a B:c array as up to five: nothing may be declined for its size
            dev.reserve(0, raw_len + (1 << 16), 6 * raw_len, 4096, 1 << 16)
            self.blk, readers = run_whole_files(dev, images, 0, paired)
            for r in readers:
                r.close()
            n = self.n = self.blk.n
            self.raws = [bytes(_ffi._host_view(self.blk.raw_addr[f], self.blk.raw_len[f], np.uint8)) for f in (0, 1)]
            self.offs = [_ffi._host_view(self.blk.rec_off_addr[f], n, np.uint32).copy() for f in (0, 1)]
            self.recs = [[self.raws[f][int(o):int(o) + 4 + struct.unpack_from("<I", self.raws[f], int(o))[0]] for o in self.offs[f]] for f in (0, 1)]
            for f in (0, 1):
                dev.set_refs(f, [name.encode() for name in S.REFS])
        except BaseException:
            dev.close()
            raise

    def classify(self, mode):
        _ffi = self.ffi
        _code, idx, off, _counts = self.dev.classify(0, {"liberal": _ffi.MODE_PE_LIBERAL, "conservative": _ffi.MODE_PE_CONSERVATIVE,
                                                         "single": _ffi.MODE_SE}[mode], self.n, ABSENT)
        return idx.copy(), [int(v) for v in off]

    def wanted(self, idx, off, mask):
        """Per file: which records a sink of `mask` takes (tests/test_bam_gpu.py, test_only_the_records_a_sink_takes_come_back)."""
        want = [np.zeros(self.n, dtype=bool), np.zeros(self.n, dtype=bool)]
        for b in range(6):
            if (mask >> b) & 1:
                seg = idx[off[b]:off[b + 1]].astype(np.int64)
                for f in files_of_bin(b):
                    want[f][seg] = True
                    if self.paired:
                        want[f][seg - 1] = True
        return want

    def bin_parts(self, b, seg):
        """The lines of bin b's units in the order of expected_bin (tests/test_bam_out_gpu.py), lines in place of records."""
        parts = []
        for i in seg:
            for f in files_of_bin(b):
                for r in ((int(i) - 1, int(i)) if self.paired else (int(i),)):
                    parts.append(((b, f, r), self.recs[f][r], line_of(self.recs[f][r]) + b"\n"))
        return parts

    def close(self):
        self.dev.close()


def check_text(win, mask, idx, off):
    """xm_bamdev_fetch_text: per file the wanted records' lines back to back in input order, the line table, the total."""
    status, text, loff, llen = win.dev.fetch_text(0, win.n, win.paired, mask)
    assert status == 0
    win.dev.raw_wait(0)
    want = win.wanted(idx, off, mask)
    for f in (0, 1):
        got = bytes(text[f])
        lo, ll = loff[f].copy(), llen[f].copy()
        parts = [((f, i), win.recs[f][i], line_of(win.recs[f][i]) + b"\n") for i in np.flatnonzero(want[f]).tolist()]
        total = sum(len(p[2]) for p in parts)
        assert first_difference(got[:total], parts) is None
        assert len(got) == max(total, 1)                              # (nothing counted behind the last line)
        at = 0
        for i in range(win.n):
            if not want[f][i]:
                assert lo[i] == 0 and ll[i] == 0, (f, i)
                continue
            size = len(line_of(win.recs[f][i]))
            assert (int(lo[i]), int(ll[i])) == (at, size) and got[at + size] == 0x0A, (f, i, shape_of(win.recs[f][i]))
            at += size + 1
        assert at == total


def check_bins(win, mask, idx, off):
    """xm_bamdev_fetch_bins: the six texts back to back."""
    status, text, boff = win.dev.fetch_bins(0, win.n, win.paired, mask)
    assert status == 0
    win.dev.raw_wait(0)
    text = bytes(text)
    assert boff[0] == 0 and boff[6] == boff[7] == len(text)
    for b in range(6):
        piece = text[boff[b]:boff[b + 1]]
        if not (mask >> b) & 1 or off[b + 1] == off[b]:
            assert piece == b"", b
            continue
        assert first_difference(piece, win.bin_parts(b, idx[off[b]:off[b + 1]])) is None


@pytest.mark.parametrize("paired", [True, False])
def test_stripper_columns_at_every_shape(ctx, paired):
    """The record chain and parse_record over 40 KB of bases and 10 000 CIGAR words: AS and XS of every record as its own fields
    hold them, the unit mask as the names say, nothing flagged."""
    files = S.shape_records(paired, "spread")
    win = Window(ctx, files, paired)
    try:
        blk, n = win.blk, len(files[0])
        assert not blk.bad_block and not blk.unaligned and blk.n_exceptions == 0 and blk.mismatch_at == -1
        assert blk.n == n and blk.n_rec == (n, n)
        assert win.recs[0] == list(files[0]) and win.recs[1] == list(files[1])
        cols = win.dev.columns(0, n)
        for f in (0, 1):
            sc = [S.scores_of(S.parse(r[4:])["fields"]) for r in files[f]]
            for j in (0, 1):
                want = np.array([ABSENT if v[j] is None else v[j] for v in sc], dtype=np.int32)
                bad = np.flatnonzero(cols[2 * f + j] != want)
                assert bad.shape[0] == 0, (f, "AS XS".split()[j], int(bad[0]), int(cols[2 * f + j][bad[0]]), int(want[bad[0]]), shape_of(files[f][int(bad[0])]))
        names = [S.parse(r[4:])["name_field"].split(b"\0")[0] for r in files[0]]
        bits = np.unpackbits(cols[4].view(np.uint8), bitorder="little")[:n]
        assert bits.tolist() == [(1 if k > 0 and names[k] == names[k - 1] else 0) if paired else 1 for k in range(n)]
    finally:
        win.close()


@pytest.mark.parametrize("paired", [True, False])
def test_text_printed_per_file_equals_the_oracle(ctx, paired):
    win = Window(ctx, S.shape_records(paired, "all_unresolved"), paired)
    try:
        assert win.n == len(win.recs[0]) >= S.MIN_RECORDS and not win.blk.unaligned
        idx, off = win.classify("liberal" if paired else "single")
        want = win.wanted(idx, off, ALL)
        assert want[0].all() and want[1].sum() > 0.9 * win.n           # (file 2's records without a score: `unassigned` prints file 1's)
        check_text(win, ALL, idx, off)
    finally:
        win.close()


@pytest.mark.parametrize("mode", ["liberal", "conservative", "single"])
@pytest.mark.parametrize("scores", ["spread", "all_unresolved"])
def test_six_outputs_gathered_on_the_device_equal_the_oracle(ctx, scores, mode):
    paired = mode != "single"
    win = Window(ctx, S.shape_records(paired, scores), paired)
    try:
        assert win.n == len(win.recs[0]) >= S.MIN_RECORDS and not win.blk.unaligned
        idx, off = win.classify(mode)
        filled = sum(1 for b in range(6) if off[b + 1] > off[b])
        assert filled >= (5 if scores == "spread" and mode != "conservative" else 1), off
        for mask in (ALL, 0b010110, 0):
            check_bins(win, mask, idx, off)
    finally:
        win.close()


def test_floats_printed_on_the_device(ctx):
    """fmt_g_f32 as hipcc compiles it for gfx950, on all patterns of the float image, through both printing kernels."""
    files = S.float_records(False)
    win = Window(ctx, files, False)
    try:
        assert win.n == len(files[0]) and win.recs[0] == list(files[0]) and win.recs[1] == list(files[1])
        idx, off = win.classify("single")
        assert off[5] - off[4] == win.n                               # every record of both files is printed
        status, text, _loff, _llen = win.dev.fetch_text(0, win.n, False, ALL)
        assert status == 0
        win.dev.raw_wait(0)
        texts = [bytes(text[0]), bytes(text[1])]
        status, stream, boff = win.dev.fetch_bins(0, win.n, False, ALL)
        assert status == 0
        win.dev.raw_wait(0)
        stream = bytes(stream)
        assert boff[4] == 0 and boff[5] == len(stream)
        seen = 0
        bad = []
        for route, lines in (("fetch_text 1", texts[0].split(b"\n")), ("fetch_text 2", texts[1].split(b"\n")), ("fetch_bins", stream.split(b"\n"))):
            assert lines.pop() == b""
            order = [(f, int(i)) for i in idx[off[4]:off[5]] for f in (0, 1)] if route == "fetch_bins" else [(int(route[-1]) - 1, i) for i in range(win.n)]
            assert len(lines) == len(order)
            for (f, i), line in zip(order, lines):
                rec = win.recs[f][i]
                got, want = line.split(b"\t"), line_of(rec).split(b"\t")
                assert len(got) == len(want) and got[:11] == want[:11], (route, f, i)
                for (tag, t, sub, value), a, b in zip(S.parse(rec[4:])["fields"], got[11:], want[11:]):
                    if t == "B" and sub == "f":
                        a, b = a.split(b","), b.split(b",")
                        bits = np.frombuffer(value, dtype="<u4")
                        assert len(a) == len(b) == bits.shape[0] + 1 and a[0] == b[0], (route, f, i)
                        bad += [(route, hex(int(v)), x, y) for v, x, y in zip(bits, a[1:], b[1:]) if x != y]
                        seen += bits.shape[0]
                    elif t == "f" and a != b:
                        bad.append((route, hex(struct.unpack("<I", value)[0]), a, b))
                    else:
                        assert a == b, (route, f, i, tag)
        assert not bad, (len(bad), bad[:12])
        assert seen == 4 * win.n * S.FLOATS_PER_RECORD >= 4 * S.float_patterns().shape[0]   # each file's values through both kernels
    finally:
        win.close()


def seam_residues(sizes, payload):
    """How many bytes a member has left where a record's 16-byte piece crosses its end (record_to_frames' byte path at a seam):
    the set of those counts (1 .. 15) over records of `sizes` lying back to back."""
    out, r = set(), 0
    for size in sizes:
        for k in range(0, size, 16):
            left = payload - (r + k) % payload
            if left < min(16, size - k):
                out.add(left)
        r += size
    return out


@pytest.mark.parametrize("paired", [True, False])
def test_bam_frames_at_every_record_size(ctx, paired):
    """Records of 38 bytes .. 63 KB copied into BGZF members of every payload size: shorter than a lane's piece, exactly P, P - 1
    and P + 1 bytes, many trips of a lane, a 16-byte piece across a member seam at every residue."""
    win = Window(ctx, S.shape_records(paired, "spread"), paired)
    try:
        n = win.n
        assert n == len(win.recs[0]) >= S.MIN_RECORDS and not win.blk.unaligned and not win.blk.n_exceptions
        sizes = sorted(set(len(r) for r in win.recs[0]))
        assert sizes[0] == 38 and {63, 64, 65, 255, 256, 257, 4095, 4096, 4097} <= set(sizes) and sizes[-1] > 63000
        # a payload that is some filler record's size, and the two next to it
        mid = next(s for s in sizes if s > 280 and s - 1 not in sizes and s + 1 not in sizes)
        idx, off = win.classify("liberal" if paired else "single")
        assert sum(1 for b in range(6) if off[b + 1] > off[b]) >= 5
        residues = {64: set(), 256: set()}
        plain = {}
        for payload in (64, 256, 4096, 0, mid - 1, mid, mid + 1):
            for shift in (0, 7):
                status, stream, boff = win.dev.fetch_bins_bam(0, n, paired, ALL, payload, shift)
                assert status == 0
                win.dev.raw_wait(0)
                stream = bytes(stream)
                assert boff[0] == 0 and boff[6] == boff[7] == len(stream)
                for b in range(6):
                    piece = stream[boff[b]:boff[b + 1]]
                    if off[b + 1] == off[b]:
                        assert piece == b""
                        continue
                    seg = idx[off[b]:off[b + 1]]
                    want = expected_bin(b, seg, paired, win.raws, win.offs, shift)
                    got = check_members(piece, payload or 65280)
                    if got != want:
                        at = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
                        parts, r = win.bin_parts(b, seg), 0
                        for label, rec, _line in parts:
                            if r + len(rec) > at:
                                pytest.fail("payload %d shift %d bin %d: byte %d of record %r (its payload bytes %d ..): %r" %
                                            (payload, shift, b, at - r, label, r, shape_of(rec)))
                            r += len(rec)
                        pytest.fail("payload %d shift %d bin %d: %d bytes, %d expected" % (payload, shift, b, len(got), len(want)))
                    assert gzip.decompress(piece) == want
                    if shift == 0:
                        plain[(payload, b)] = want
                        if payload in residues:
                            residues[payload] |= seam_residues([len(rec) for _label, rec, _line in win.bin_parts(b, seg)], payload)
                    else:
                        # the shift moves refID / next_refID of file 2's records in `unresolved` where they name a reference (>= 0);
                        # -1 and -2 stay, and so does every other bin
                        assert (want == plain[(payload, b)]) == (b != 4)
        for payload in (64, 256):
            assert residues[payload] == set(range(1, 16)), (payload, sorted(residues[payload]))
        # the unresolved bin holds file 2's records with negative and with shifted reference ids
        refs2 = [struct.unpack_from("<i", win.recs[1][r], 4)[0] for i in idx[off[4]:off[5]] for r in ((int(i) - 1, int(i)) if paired else (int(i),))]
        assert min(refs2) < 0 <= max(refs2)
    finally:
        win.close()


def test_classify_of_no_records_counts_as_classified_and_the_gathers_return_nothing(ctx):
    """xm_bamdev_classify with n_records == 0 returns empty results without running the fused pass and MARKS the slot classified
    (xm_bamdev_run cleared the mark), so xm_bamdev_fetch_bins and xm_bamdev_fetch_bins_bam of no records are accepted and return
    status 0 with an empty stream.  (xm_strip_classify leaves the slot unclassified in the same case, and its fetch is refused:
    tests/test_strip_shapes_gpu.py.)  Without any classify since the run the same fetch is refused with XM_ERR_INVALID_ARG."""
    win = Window(ctx, S.shape_records(False, "spread"), False)
    try:
        assert win.n > 0
        with pytest.raises(ValueError, match="xm_bamdev_fetch_bins"):
            win.dev.fetch_bins(0, 0, False, ALL)
        code, idx, off, counts = win.dev.classify(0, win.ffi.MODE_SE, 0, ABSENT)
        assert code.shape[0] == 0 and idx.shape[0] == 0 and not off.any() and not counts.any()
        for fetch in (win.dev.fetch_bins, win.dev.fetch_bins_bam):
            status, stream, boff = fetch(0, 0, False, ALL)
            assert status == 0 and boff == [0] * 8 and stream.shape[0] == 0
    finally:
        win.close()
