"""The SAM gather on the device (xm_strip_fetch_bins: sam_unit_size_kernel, the size scan of xm_gather.h, bin_start_kernel,
sam_line_copy_kernel, out_copy_kernel) on the images of tests/sam_shapes.py, through the C ABI: every line length from 1 to 1100
bytes and two lines longer than a chunk next to each other in one wave, all terminators, lines of different lengths in the two
files, every sink mask, both slots, windows with a halo record, the skipping walk, declined windows, unit counts on the scan's tile
boundaries and a window of 4.2 M units.  Every comparison is byte for byte with tests/sam_shapes.py's expected_bins (pinned to the
oracle by tests/test_sam_shapes_cpu.py) on unit lists that equal the C oracle's; every fetch that is expected to succeed must return
status 0 -- a declined window cannot pass as a comparison skipped -- and every check counts the lines and bytes it compared."""
import numpy as np
import pytest

from tests import helpers as H
from tests import sam_shapes as S
from tests.test_strip_gpu import compare, strip

pytestmark = pytest.mark.gpu

ABSENT = -2**31
MASKS = [S.ALL, 0b010110, 0] + [1 << b for b in range(6)]
MODES = {"liberal": (1, True), "conservative": (2, True), "single": (0, False)}


@pytest.fixture(scope="module")
def rig():
    from xenomapper_amd import _ffi, _host
    from xenomapper_amd.xenomapper import default_context
    ctx = default_context()
    s = _ffi.Stripper(ctx)
    p = _host.Parser(4)
    yield ctx, s, p
    s.close()
    p.close()


def oracle_units(want, mode, score_mode, n=None):
    """The C oracle's unit lists on the host stripper's columns (first n records) -> (idx, off)."""
    n = want.n if n is None else n
    cols = [c[:n].copy() for c in want.cols]
    if score_mode == 2:
        for f in (0, 1):
            nm, coff, ops = want.csr[f]
            cols[2 * f], bad = H.c_cigar_scores(nm[:n].copy(), coff[:n + 1].copy(), ops.copy())
            assert bad == 0
    code, _counts = H.c_classify(mode, *cols, want.unit_bits.copy(), ABSENT)
    idx, off = H.c_compact(mode, code)
    return idx.copy(), [int(v) for v in off]


def record_lines(got, b1, b2):
    """The line of every record of the block in each window -> ([lines 1, lines 2], offsets), from the block's line table, which
    compare() has just found equal to the HOST stripper's."""
    out = []
    for f, text in enumerate((b1, b2)):
        out.append([text[o:o + n] for o, n in zip(got.line_off[f].tolist(), got.line_len[f].tolist())])
    return out, [got.line_off[0].copy(), got.line_off[1].copy()]


def first_difference(got, parts, line_off):
    """got: bytes; parts: [((bin, file, record), printed line)] that should lie back to back in it -> None, or which line differs:
    bin, file and record, the line's length, where it lies in its window and in the stream modulo 8, and the first differing byte."""
    at = 0
    for (b, f, r), want in parts:
        mine = got[at:at + len(want)]
        if mine != want:
            j = next((k for k in range(min(len(mine), len(want))) if mine[k] != want[k]), min(len(mine), len(want)))
            return ("bin %d, file %d, record %d: line of %d bytes, source offset %% 8 = %d, destination offset %% 8 = %d: byte %d: got %r, "
                    "want %r" % (b, f + 1, r, len(want) - 1, int(line_off[f][r]) % 8, at % 8, j, mine[max(0, j - 12):j + 20], want[max(0, j - 12):j + 20]))
        at += len(want)
    if at != len(got):
        return "%d bytes behind the last expected line" % (len(got) - at)
    return None


def out_capacity(s, slot):
    """Bytes of the slot's output stream as include/xenomapper_strip.h words it: both windows' text and a little more (status 2
    beyond that).  Only compared with sizes here, never used as an address bound."""
    cap = (s._cap[slot][0] + S.CHUNK - 1) // S.CHUNK * S.CHUNK
    return 2 * cap + 4096


def check_gather(s, slot, n, paired, mask, lines, line_off, idx, off, guard=False):
    """One xm_strip_fetch_bins of the slot's classified block against expected_bins -> (bin texts, lines compared, bytes compared).
    guard (a mask that leaves bins out): nothing may be written behind the stream but the copy's rounding to 16 bytes.  The stream
    of ALL sinks is fetched first and the bytes it returned -- memory the ABI has just handed out, no more -- are painted; what the
    shorter stream of `mask` leaves of the paint must still be there."""
    painted = None
    if guard:
        status, painted, ball = s.fetch_bins(slot, n, paired, S.ALL)
        assert status == 0
        s.out_wait(slot)
        painted[:] = 0xEE
    status, text, boff = s.fetch_bins(slot, n, paired, mask)
    assert status == 0, (status, mask)
    s.out_wait(slot)
    if guard:
        assert boff[7] <= ball[7] and (boff[7] == 0 or text.ctypes.data == painted.ctypes.data)
        assert (painted[(boff[7] + 15) // 16 * 16:] == 0xEE).all()
    got = bytes(text)
    assert boff[0] == 0 and boff[6] == boff[7] == len(got) and all(boff[b] <= boff[b + 1] for b in range(7)), boff
    want = S.expected_bins(lines[0], lines[1], idx, off, paired, mask)
    pieces = [got[boff[b]:boff[b + 1]] for b in range(6)]
    for b in range(6):
        if not (mask >> b) & 1 or off[b + 1] == off[b]:
            assert pieces[b] == b"" == want[b], (b, boff)                # a bin without a sink or without units: an empty piece
        if pieces[b] != want[b]:
            pytest.fail(first_difference(pieces[b], S.bin_parts(lines[0], lines[1], idx, off, paired, mask, b), line_off))
    # what was compared: every line of every unit of the bins the mask takes (a printed line ends with its only '\n')
    n_lines = sum((off[b + 1] - off[b]) * (2 if paired else 1) * len(S.files_of_bin(b)) for b in range(6) if (mask >> b) & 1)
    n_bytes = sum(len(t) for t in want)
    assert got.count(b"\n") == n_lines and len(got) == n_bytes
    return pieces, n_lines, n_bytes


def run_block(rig, slot, b1, b2, mode, score_mode, eof=(True, True), keep_halo=False, skip=False, max_records=1 << 16, n=None):
    """Strip (checked against the host stripper), classify (checked against the C oracle) -> (got, lines, line_off, idx, off)."""
    _ctx, s, p = rig
    m, paired = MODES[mode]
    got, want = compare(s, p, b1, b2, eof[0], eof[1], score_mode, paired, keep_halo, max_records, slot=slot, skip=skip)
    assert want is not None and not got.overflow and not got.n_exceptions
    n = got.n if n is None else n
    _code, idx, off, _counts = s.classify(slot, m, n, ABSENT)
    idx, off = idx.copy(), [int(v) for v in off]
    want_idx, want_off = oracle_units(want, m, score_mode, n)
    assert off == want_off and np.array_equal(idx, want_idx)
    lines, line_off = record_lines(got, b1, b2)
    return got, lines, line_off, idx, off


@pytest.mark.parametrize("newline", S.NEWLINES, ids=["lf", "crlf", "cr", "mixed"])
@pytest.mark.parametrize("scores", S.SCORE_LAYOUTS)
def test_every_line_length_terminator_mode_mask_and_slot(rig, scores, newline):
    _ctx, s, _p = rig
    for score_mode, mode in enumerate(("liberal", "conservative", "single")):
        paired = MODES[mode][1]
        b1, b2 = S.shape_text(paired, scores, newline)
        whole = [S.split_lines(b)[0] for b in (b1, b2)]
        for slot in (0, 1):
            got, lines, line_off, idx, off = run_block(rig, slot, b1, b2, mode, score_mode)
            assert got.n == S.N_RECORDS and got.ended and lines == whole and off[7] == S.N_RECORDS // (2 if paired else 1)
            total_lines = 0
            for mask in MASKS:
                _pieces, n_lines, n_bytes = check_gather(s, slot, got.n, paired, mask, lines, line_off, idx, off, guard=mask != S.ALL)
                total_lines += n_lines
                if mask == S.ALL:                                        # every unit printed: its line(s) of one file, or of both
                    assert n_lines >= S.N_RECORDS and n_bytes > min(len(b1), len(b2)) // 2
            assert total_lines >= 2 * S.N_RECORDS


@pytest.mark.parametrize("mode", ["liberal", "conservative"])
def test_windows_with_a_halo_record_add_up_to_the_whole_file(rig, mode):
    """The image cut into windows by `consumed` as the file path cuts it, keep_halo on: record 0 of a later window is the record in
    front of it, and where the cut fell between two mates the window's first unit has that halo record as its first mate."""
    _ctx, s, _p = rig
    m, paired = MODES[mode]
    b1, b2 = S.shape_text(True, "spread", "mixed")
    _got, lines, line_off, idx, off = run_block(rig, 0, b1, b2, mode, 0)
    want = S.expected_bins(lines[0], lines[1], idx, off, True, S.ALL)
    for window in (300_000, 333_333):
        pos, blocks, halo_units, texts, units = [0, 0], 0, 0, [[] for _ in range(6)], 0
        while True:
            w1, w2 = b1[pos[0]:pos[0] + window], b2[pos[1]:pos[1] + window]
            eof = (pos[0] + window >= len(b1), pos[1] + window >= len(b2))
            got, wl, wo, widx, woff = run_block(rig, blocks & 1, w1, w2, mode, 0, eof=eof, keep_halo=True)
            halo_units += int(blocks > 0 and 1 in widx.tolist())
            pieces, n_lines, _n_bytes = check_gather(s, blocks & 1, got.n, True, S.ALL, wl, wo, widx, woff)
            assert n_lines >= 2 * woff[7]
            units += woff[7]
            for b in range(6):
                texts[b].append(pieces[b])
            blocks += 1
            if got.ended:
                break
            assert got.consumed[0] > 0
            pos[0] += got.consumed[0]
            pos[1] += got.consumed[1]
        assert blocks >= 3 and units == S.N_RECORDS // 2
        assert [b"".join(t) for t in texts] == want
        if window == 333_333:
            assert halo_units >= 1
    # fewer records than the block holds: classify and fetch the same n
    for n in (S.N_RECORDS - 601, 257):
        got, lines, line_off, idx, off = run_block(rig, 1, b1, b2, mode, 0, n=n)
        assert got.n == S.N_RECORDS and off[7] == n // 2
        for mask in (S.ALL, 0b010110):
            _pieces, n_lines, _n_bytes = check_gather(s, 1, n, True, mask, lines, line_off, idx, off)
        assert n_lines > 0


def repeated_text(seed=5):
    """The single-end image with runs of one to four lines per name, of different lengths in the two files: the first line of a run
    is the image's, the further ones carry the name and fields of their own."""
    rng = np.random.default_rng(seed)
    texts, firsts = [], []
    b = S.shape_text(False, "spread", "\n")
    for f in (0, 1):
        lines = S.split_lines(b[f])[0]
        reps = rng.integers(0, 4, size=len(lines))
        out = []
        for r, line in enumerate(lines):
            out.append(line)
            name = line.split(b"\t")[0]
            for k in range(int(reps[r])):
                out.append(name + b"\tdup%d\tof\t%d" % (k, r) + b"\tx" * int(rng.integers(0, 12)))
        texts.append(b"\n".join(out) + b"\n")
        firsts.append((lines, reps))
    assert (firsts[0][1] != firsts[1][1]).mean() > 0.5
    return texts[0], texts[1], firsts[0][0], firsts[1][0]


def test_skipping_walk_gathers_the_lines_the_runs_start_with(rig):
    _ctx, s, _p = rig
    b1, b2, first1, first2 = repeated_text()
    for slot in (0, 1):
        got, lines, line_off, idx, off = run_block(rig, slot, b1, b2, "single", 0, skip=True)
        assert got.n == S.N_RECORDS and got.ended and got.n_lines[0] != got.n_lines[1] and min(got.n_lines) > 2 * S.N_RECORDS
        assert lines == [first1, first2]
        for mask in (S.ALL, 0b010110, 0b100000):
            _pieces, n_lines, _n_bytes = check_gather(s, slot, got.n, False, mask, lines, line_off, idx, off)
            assert n_lines > 0


@pytest.mark.parametrize("mode", ["liberal", "conservative", "single"])
def test_a_wanted_odd_line_declines_the_window_and_no_other_does(rig, mode):
    """Status 3 exactly when the mask takes a bin that prints a line which is not '\t'.join(fields) -- also when that line is the
    unit's first mate, and not when it is the line of the file that the bin does not print."""
    _ctx, s, _p = rig
    m, paired = MODES[mode]
    b1, b2, odd = S.odd_lines(paired)
    odd = {at for at, _form in odd}
    got, lines, line_off, idx, off = run_block(rig, 0, b1, b2, mode, 0)
    assert got.n == S.N_RECORDS
    seen, compared = {0: 0, 3: 0}, 0
    for mask in MASKS + [0b000011, 0b111100, 0b111101, 0b111110, 0b101101]:
        wanted_odd = [label for b in range(6) for label, _text in S.bin_parts(lines[0], lines[1], idx, off, paired, mask, b) if label[1:] in odd]
        if wanted_odd:
            status, text, boff = s.fetch_bins(0, got.n, paired, mask)
            assert status == 3 and text is None, (mask, wanted_odd[:4])
        else:
            _pieces, n_lines, _n_bytes = check_gather(s, 0, got.n, paired, mask, lines, line_off, idx, off)
            compared += n_lines
        seen[3 if wanted_odd else 0] += 1
        # the bins of ODD_UNITS and nothing else decide
        assert bool(wanted_odd) == bool(mask & 0b000011), mask
        if paired and mask == 0b000001:                                  # bin 0: only FIRST mates (records i - 1) are odd
            assert wanted_odd and all(r % 2 == 0 for _b, _f, r in wanted_odd)
        if paired and mask == 0b000010:
            assert wanted_odd and all(r % 2 == 1 for _b, _f, r in wanted_odd)
    # what was compared is what the masks that take neither bin of ODD_UNITS hold: the units of bins 2 - 5, each once as a single
    # bit and once under 0b111100 (liberal mode leaves few of them: the better mate decides)
    per = 2 if paired else 1
    held = sum((off[b + 1] - off[b]) * per * len(S.files_of_bin(b)) for b in range(2, 6))
    assert seen[0] >= 6 and seen[3] >= 6 and compared == 2 * held > 0


def test_more_text_than_the_stream_holds_is_declined_and_less_is_not():
    """One repeated name and equal scores: every record closes a unit with the one in front, every unit is `unresolved` and prints four
    lines -- four times the window, twice what the output stream of a stripper reserved for just this window holds: status 2.
    With primary_specific as the only sink nothing is printed and the window fits; so do the first records alone."""
    from xenomapper_amd import _ffi, _host
    from xenomapper_amd.xenomapper import default_context
    line = b"samename\t%d\tchr1\t%d\t30\t50M\t=\t%d\t0\t" + b"ACGT" * 12 + b"AC\t" + b"F" * 50 + b"\tAS:i:-5\tXS:i:-9\n"
    text = b"".join(line % (99 if k % 2 == 0 else 147, 100 + k, 300 + k) for k in range(400))
    assert 48_000 < len(text) < S.CHUNK
    s, p = _ffi.Stripper(default_context()), _host.Parser(2)
    try:
        rig = (None, s, p)
        got, lines, line_off, idx, off = run_block(rig, 0, text, text, "liberal", 0, max_records=1024)
        assert got.n == 400 and off[4] == 0 and off[5] == off[7] == 399
        want = S.expected_bins(lines[0], lines[1], idx, off, True, S.ALL)
        assert sum(len(t) for t in want) > out_capacity(s, 0) == 2 * S.CHUNK + 4096
        for mask in (S.ALL, 0b010000):
            status, text_out, _boff = s.fetch_bins(0, got.n, True, mask)
            assert status == 2 and text_out is None
        _pieces, n_lines, n_bytes = check_gather(s, 0, got.n, True, 0b000001, lines, line_off, idx, off)
        assert (n_lines, n_bytes) == (0, 0)
        # the first 200 records: 199 overlapping units, every line but the outer two printed twice from each file
        got, lines, line_off, idx, off = run_block(rig, 0, text, text, "liberal", 0, max_records=1024, n=200)
        _pieces, n_lines, n_bytes = check_gather(s, 0, 200, True, S.ALL, lines, line_off, idx, off)
        assert n_lines == 4 * 199 and 3 * len(text) // 2 < n_bytes <= out_capacity(s, 0)
    finally:
        s.close()
        p.close()


_STATE_TAGS = {0: (b"\tAS:i:0", b""), 1: (b"", b"\tAS:i:0"), 2: (b"\tAS:i:-5\tXS:i:-5", b""), 3: (b"", b"\tAS:i:-5\tXS:i:-5"),
               4: (b"\tAS:i:-3", b"\tAS:i:-3\tXS:i:-8"), 5: (b"", b"\tXS:i:-1")}


def binned_records(n, bins, seed):
    """n single-end records whose states are drawn from `bins`, lines of 36 .. 110 bytes, different in the two files."""
    rng = np.random.default_rng(seed)
    state = np.asarray(bins)[rng.integers(0, len(bins), size=n)]
    state[:len(bins)] = bins[:n]                                         # (each of them at least once, n permitting)
    out = [[], []]
    for k in range(n):
        for f in (0, 1):
            seq = b"ACGT" * 10
            cut = int(rng.integers(1, 38))
            out[f].append(b"q%d\t0\tchr%d\t%d\t30\t%dM\t*\t0\t0\t%s\t%s%s" % (k, f + 1, 100 + k, cut, seq[:cut], b"F" * cut, _STATE_TAGS[int(state[k])][f]))
    return b"\n".join(out[0]) + b"\n", b"\r\n".join(out[1]) + b"\r\n", state[:n]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_unit_counts_on_the_scan_boundaries_and_bins_that_are_empty_or_unwanted(rig, n):
    """The size scan's tiles (4096 units) and the copy kernel's blocks (256 lines) at their boundaries; bins without units in the
    middle and at the end; a bin WITH units but without a sink between two bins with sinks: its units have size 0 and take the next
    unit's place, so the bin's piece is empty and the next bin starts where the one in front ended."""
    _ctx, s, _p = rig
    for bins, masks in (((0, 1, 2, 3, 4, 5), (S.ALL, 0b111101, 0b101101, 0b010110, 0b011111, 0b100000)),
                        ((0, 4), (S.ALL, 0b010000, 0b000001)),              # bins 1 - 3 and 5 are empty
                        ((1, 3, 5), (S.ALL, 0b100010, 0b001000))):          # bins 0, 2 and 4 are empty
        b1, b2, state = binned_records(n, bins, n)
        slot = n & 1
        got, lines, line_off, idx, off = run_block(rig, slot, b1, b2, "single", 0)
        assert got.n == n == off[7]
        assert [off[b + 1] - off[b] for b in range(6)] == [int((state == b).sum()) for b in range(6)]
        for mask in masks:
            _pieces, n_lines, _n_bytes = check_gather(s, slot, n, False, mask, lines, line_off, idx, off, guard=mask != S.ALL)
            assert n_lines == sum(int((state == b).sum()) * len(S.files_of_bin(b)) for b in range(6) if (mask >> b) & 1)


def test_a_window_of_more_units_than_one_part_per_thread_of_the_scan():
    """4.2 M single-end records of 6 - 8 bytes: the size scan has 1026 parts, two per thread of part_scan_kernel.  No line has a
    score, every unit is `unassigned`, and that bin's text is file 1 itself."""
    from xenomapper_amd import _ffi
    from xenomapper_amd.xenomapper import default_context
    n = 4_200_000
    b1, b2 = S.tiny_lines(n)
    assert (n + 4095) // 4096 > 1024
    s = _ffi.Stripper(default_context())
    try:
        got = strip(s, 0, b1, b2, True, True, 0, False, False, n + 16)
        assert got.n == n and got.ended and got.n_lines == (n, n) and not got.n_exceptions and not got.overflow
        assert np.array_equal(got.line_len[0][:6], [6, 7, 8, 6, 7, 8]) and int(got.line_len[0].sum()) == len(b1) - n
        assert int(got.line_off[0][-1]) == len(b1) - 9 and int(got.line_off[1][-1]) == len(b2) - 11
        _code, idx, off, counts = s.classify(0, _ffi.MODE_SE, n, ABSENT)
        assert [int(v) for v in off] == [0, 0, 0, 0, 0, 0, n, n] and np.array_equal(idx, np.arange(n, dtype=np.uint32))
        assert int(counts.sum()) == n
        for mask in (S.ALL, 0b100000):
            status, text, boff = s.fetch_bins(0, n, False, mask)
            assert status == 0
            s.out_wait(0)
            assert boff == [0, 0, 0, 0, 0, 0, len(b1), len(b1)]
            assert text.shape[0] == len(b1) and np.array_equal(text, np.frombuffer(b1, dtype=np.uint8))
        status, text, boff = s.fetch_bins(0, n, False, 0b011111)             # no sink takes the one bin that has units
        assert status == 0 and boff == [0] * 8 and text.shape[0] == 0
    finally:
        s.close()


def test_classify_of_no_records_leaves_the_slot_unclassified(rig):
    """xm_strip_classify with n_records == 0 returns empty results without running the fused pass and WITHOUT marking the slot
    classified (xm_strip_run cleared the mark), so xm_strip_fetch_bins on the slot is refused with XM_ERR_INVALID_ARG, whatever
    n_records it is given.  (xm_bamdev_classify marks the slot in the same case: tests/test_bam_shapes_gpu.py.)  A classify of the
    block's records afterwards makes the same fetch succeed, and a fetch of no records then returns an empty stream."""
    _ctx, s, p = rig
    b1, b2, _state = binned_records(5, (0, 4), 5)
    for slot in (0, 1):
        got, want = compare(s, p, b1, b2, True, True, 0, False, False, 1 << 16, slot=slot)
        assert want is not None and got.n == 5
        code, idx, off, counts = s.classify(slot, MODES["single"][0], 0, ABSENT)
        assert code.shape[0] == 0 and idx.shape[0] == 0 and not off.any() and not counts.any()
        for n in (0, 5):
            with pytest.raises(ValueError, match="xm_strip_fetch_bins"):
                s.fetch_bins(slot, n, False, S.ALL)
        _code, idx, off, _counts = s.classify(slot, MODES["single"][0], 5, ABSENT)
        assert int(off[7]) == 5
        status, text, boff = s.fetch_bins(slot, 5, False, S.ALL)
        assert status == 0 and boff[7] > 0
        s.out_wait(slot)
        status, text, boff = s.fetch_bins(slot, 0, False, S.ALL)
        assert status == 0 and boff == [0] * 8 and text.shape[0] == 0
