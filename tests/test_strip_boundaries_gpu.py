"""The stripper's kernels S1 - S8 (xm_strip.hip) where they have never run: terminators on every position of mark_kernel's 16-byte
groups, 1 KiB steps, 16 KiB wave quarters and 64 KiB chunks, "\r\n" across each of them, waves and chunks without a terminator,
windows that end on and next to those boundaries or with a '\r'; windows of 600 000 lines, where the striding kernels (2048
workgroups of 256) take a second trip and the scans more than one item per thread; and windows uploaded piece by piece
(xm_strip_upload) with pieces that end on, before and behind a chunk boundary and between a '\r' and its '\n'.  Everything is compared
field by field with the host stripper through compare() of tests/test_strip_gpu.py; the gather on the large windows with
expected_bins of tests/sam_shapes.py."""
import numpy as np
import pytest

from tests import sam_shapes as S
from tests.test_strip_gpu import compare
from tests.test_strip_shapes_gpu import ABSENT, MODES, check_gather, oracle_units, record_lines

pytestmark = pytest.mark.gpu

VARIANTS = sorted(S.BOUNDARY_VARIANTS)
TRIP = 2048 * 256                                     # lines (records) of one trip of the striding kernels


@pytest.fixture(scope="module")
def rig():
    from xenomapper_amd import _ffi, _host
    from xenomapper_amd.xenomapper import default_context
    ctx = default_context()
    s = _ffi.Stripper(ctx)
    p = _host.Parser(8)
    yield ctx, s, p
    s.close()
    p.close()


@pytest.mark.parametrize("first", VARIANTS)
def test_terminators_on_every_boundary_and_windows_that_end_there(rig, first):
    """Every pair of boundary texts, each as a window that ends its file and as one that does not.  A trailing '\r' of a window that
    goes on is no terminator yet (its '\n' may follow): the line in front of it stays unconsumed; at the end of the file it is one."""
    _ctx, s, p = rig
    b1 = S.boundary_text(first)
    lines1 = len(S.split_lines(b1)[0])
    runs = 0
    for second in VARIANTS:
        b2 = S.boundary_text(second)
        lines2 = len(S.split_lines(b2)[0])
        for eof1 in (True, False):
            for eof2 in (True, False):
                got, want = compare(s, p, b1, b2, eof1, eof2, 0, False, False, 1 << 16, slot=runs & 1)
                assert want is not None and got.mismatch_at < 0
                # the lines of a window: every terminated one, the last one too where the file ends; a last '\r' does not
                # terminate where the window goes on
                for f, (text, n_lines, eof) in enumerate(((b1, lines1, eof1), (b2, lines2, eof2))):
                    open_end = not eof and text[-1:] != b"\n"
                    assert got.n_lines[f] == n_lines - (1 if open_end else 0), (first, second, f, eof)
                assert got.n > 3000
                if first == second and eof1 and eof2:
                    assert got.ended and got.consumed == (len(b1), len(b2))
                if first == second and not eof1 and not eof2 and b1[-1:] == b"\r":
                    assert got.consumed[0] == got.consumed[1] < len(b1) - 1
                runs += 1
    assert runs == 4 * len(VARIANTS)


COMBOS = [(0, False, False, False), (0, True, False, False), (0, False, True, True), (0, True, True, False),
          (1, False, False, False), (1, True, False, False), (1, False, True, True), (1, True, True, False),
          (2, False, False, False), (2, True, False, False), (2, False, True, True), (2, True, True, False)]


@pytest.mark.parametrize("score_mode,paired,skip,repeats", COMBOS)
def test_windows_of_more_lines_than_one_trip(rig, score_mode, paired, skip, repeats):
    """600 000 records of 41 bytes per window: parse_kernel, pair_kernel and cig_write_kernel stride a second time, the skipping
    walk's start_count / start_fill too and start_scan_kernel takes three counts per thread, chunk_scan_kernel two.  Scores, CIGARs
    and the flagged values differ along the file, so a second trip that repeated the first one's answers would show."""
    ctx, s, p = rig
    n = 600_000
    b1, b2 = S.many_lines(n, paired, repeats)
    got, want = compare(s, p, b1, b2, True, True, score_mode, paired, paired, n + 16, skip=skip)
    assert want is not None and not got.overflow
    assert got.n_lines == (n, n) and n > TRIP and len(b1) > 16 << 20 and len(b2) > 16 << 20
    if not skip:
        assert got.n == n
    elif repeats:
        assert got.n > 262_144                                  # runs of one to three lines
    else:
        assert got.n == (n // 2 if paired else n)               # mates share a name: the skipping walk yields one of them
    if not skip:                                                # (many_lines: an AS, XS, ZS and NM among the values that are no integers)
        assert any(k > TRIP for k, _c, _kind in got.exc), "no flagged value behind the first trip"
    mode = "liberal" if paired else "single"
    m = MODES[mode][0]
    code, idx, off, counts = s.classify(0, m, got.n, ABSENT)
    if score_mode == 2:
        h = ctx.classify_compact_cigar(m, want.csr[0][0], want.csr[0][1], want.csr[0][2], want.cols[1],
                                       want.csr[1][0], want.csr[1][1], want.csr[1][2], want.cols[3], want.unit_bits, ABSENT)
    else:
        h = ctx.classify_compact(m, *want.cols, want.unit_bits, ABSENT)
    assert np.array_equal(code, h[0]) and np.array_equal(idx, h[1]) and np.array_equal(off, h[2]) and np.array_equal(counts, h[3])
    idx, off = idx.copy(), [int(v) for v in off]
    want_idx, want_off = oracle_units(want, m, score_mode)
    assert off == want_off and np.array_equal(idx, want_idx)
    # every record a unit; two mates a unit; after the skipping walk no name follows itself, so no record closes a pair
    assert off[7] == (got.n if not paired else 0 if skip else n // 2)
    # the gather on the same block (the score mode decides the bins, and with them the layout of the size scan)
    lines, line_off = record_lines(got, b1, b2)
    _pieces, n_lines, n_bytes = check_gather(s, 0, got.n, paired, S.ALL, lines, line_off, idx, off)
    assert n_lines >= off[7] * (2 if paired else 1) and n_bytes == 41 * n_lines
    assert n_lines > 262_144 or (paired and skip)


def staged_run(s, slot, texts, steps, eof, score_mode, paired, keep_halo, max_records):
    """The windows `texts` staged and announced as `steps` say -- (file, offset, bytes, announce) in order; a step's bytes are copied
    into the staging buffer immediately before its upload -- then whatever is left staged, and xm_strip_run.  The staging buffers
    are filled with '\n' beforehand: a mark beyond the announced bytes would count terminators that are not there."""
    s.reserve(slot, max(len(t) for t in texts) + 4 * S.CHUNK, max_records)
    stage = [s.staging(slot, f) for f in (0, 1)]
    raw = [np.frombuffer(t, dtype=np.uint8) for t in texts]
    done = [0, 0]
    for f in (0, 1):
        stage[f][:] = 0x0A
    for f, at, n, announce in steps:
        assert at == done[f] and at + n <= len(texts[f])
        stage[f][at:at + n] = raw[f][at:at + n]
        if announce:
            s.upload(slot, f, at, n)
        done[f] = at + n
    for f in (0, 1):
        stage[f][done[f]:len(texts[f])] = raw[f][done[f]:]
    return s.run(slot, len(texts[0]), eof[0], len(texts[1]), eof[1], score_mode, paired, False, keep_halo, max_records)


def tables_of(s, slot, blk):
    n = blk.n
    out = {"n": n, "consumed": blk.consumed, "consumed_lines": blk.consumed_lines, "n_lines": blk.n_lines,
           "walk": (blk.ended, blk.starved, blk.mismatch_at, blk.non_ascii, blk.overflow, blk.n_exceptions)}
    for f in (0, 1):
        out["off%d" % f], out["len%d" % f] = blk.line_off[f].copy(), blk.line_len[f].copy()
        out["norm%d" % f], out["flags%d" % f] = blk.norm_len[f].copy(), blk.line_flags[f].copy()
    for k, c in enumerate(s.columns(slot, n)):
        out["col%d" % k] = c
    return out


def same_tables(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key
    return True


def pieces(total, size, start=0):
    out, at = [], start
    while at < total:
        out.append((at, min(size, total - at)))
        at += out[-1][1]
    return out


def piece_plans(texts):
    """name -> steps of staged_run.  Sizes around the chunk; single bytes across a chunk boundary; a piece that ends between a '\r' and
    its '\n' (file 1's first "\r\n" behind its first chunk); one file announced and the other not; both announced in part; a window
    abandoned after two pieces -- of other text -- and begun again from offset 0."""
    plans = {}
    lens = [len(t) for t in texts]
    for name, size in (("chunk", S.CHUNK), ("chunk-1", S.CHUNK - 1), ("chunk+1", S.CHUNK + 1), ("3chunks+5", 3 * S.CHUNK + 5)):
        plans[name] = [(f, at, n, True) for f in (0, 1) for at, n in pieces(lens[f], size)]
    single = [(0, 2 * S.CHUNK - 3)] + [(2 * S.CHUNK - 3 + k, 1) for k in range(7)]
    plans["single_bytes"] = [(f, at, n, True) for f in (0, 1) for at, n in single + pieces(lens[f], 5 * S.CHUNK // 2, 2 * S.CHUNK + 4)]
    cut = texts[0].index(b"\r\n", S.CHUNK) + 1
    plans["between_cr_and_lf"] = [(0, 0, cut, True)] + [(0, at, n, True) for at, n in pieces(lens[0], S.CHUNK + 7, cut)] + \
        [(1, at, n, True) for at, n in pieces(lens[1], 2 * S.CHUNK)]
    plans["first_file_only"] = [(0, at, n, True) for at, n in pieces(lens[0], S.CHUNK + 1)]
    plans["both_in_part"] = [(f, at, n, at < lens[f] // 2) for f in (0, 1) for at, n in pieces(lens[f], S.CHUNK - 1)]
    return plans


def _piece_texts(which):
    if which == "boundary":
        return (S.boundary_text("cr_first_of_chunk"), S.boundary_text("crlf_across_end")), False, 1 << 16
    return S.shape_text(True, "spread", "mixed"), True, 1 << 16


@pytest.mark.parametrize("which", ["boundary", "spread"])
def test_windows_uploaded_piece_by_piece_equal_the_one_shot_run(rig, which):
    _ctx, s, p = rig
    texts, paired, max_records = _piece_texts(which)
    assert b"\r\n" in texts[0][S.CHUNK:]
    plans = piece_plans(texts)
    assert len(plans) == 8
    for eof in ((True, True), (False, False)):
        got, want = compare(s, p, texts[0], texts[1], eof[0], eof[1], 0, paired, paired, max_records, slot=0)
        assert want is not None and got.n > 1000
        ref = tables_of(s, 0, got)
        for k, (name, steps) in enumerate(sorted(plans.items())):
            slot = k & 1
            blk = staged_run(s, slot, texts, steps, eof, 0, paired, paired, max_records)
            assert same_tables(tables_of(s, slot, blk), ref), name
        # a window abandoned after two pieces of OTHER text, then begun again from offset 0.  (staged_run overwrites the staging
        # buffer while the abandoned pieces' S1 launches may still be reading it: nothing of theirs is kept -- the new window's
        # launches follow them on the slot's stream and mark every chunk again -- so the test does not wait for them, and the
        # product does not need it to.)
        other = [t[::-1].replace(b"\n", b"\r").replace(b"\t", b"\n") for t in texts]
        for slot in (0, 1):
            s.reserve(slot, max(len(t) for t in texts) + 4 * S.CHUNK, max_records)
            for f in (0, 1):
                stage = s.staging(slot, f)
                for at, n in pieces(3 * S.CHUNK + 11, 3 * S.CHUNK // 2 + 6)[:2]:
                    stage[at:at + n] = np.frombuffer(other[f][at:at + n], dtype=np.uint8)
                    s.upload(slot, f, at, n)
            blk = staged_run(s, slot, texts, plans["chunk+1"], eof, 0, paired, paired, max_records)
            assert same_tables(tables_of(s, slot, blk), ref), "abandoned"
