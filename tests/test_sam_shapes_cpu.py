"""The images of tests/sam_shapes.py on the CPU: they hold every line length, alignment and terminator position they promise, and
expected_bins -- the plain-Python statement of include/xenomapper_strip.h's output rule that tests/test_strip_shapes_gpu.py compares
the device gather with -- equals the text-level oracle's six outputs and the host writer's (xmh_emit) on them, fed with the C
oracle's unit lists.  No GPU: this proves the inputs and the expectation of the GPU tests before a GPU sees them."""
import io

import numpy as np
import pytest

from tests import helpers as H
from tests import sam_shapes as S
from tests.helpers import ORACLE

LAYOUTS = [(paired, scores, newline) for paired in (True, False) for scores in S.SCORE_LAYOUTS for newline in S.NEWLINES]
MODES = {"pe": (True, False), "pe_conservative": (True, True), "se": (False, False)}
SCORERS = [ORACLE.tag_score, ORACLE.tag_score_zs, ORACLE.cigar_score]
ABSENT = -2**31


@pytest.fixture(scope="module")
def parser():
    from xenomapper_amd import _host
    p = _host.Parser(4)
    yield p
    p.close()


def host_units(parser, b1, b2, mode, score_mode):
    """The host parser's block of the two whole files and the C oracle's unit lists on its columns -> (block, idx, off)."""
    paired = mode != "se"
    r1, r2 = np.frombuffer(b1, dtype=np.uint8), np.frombuffer(b2, dtype=np.uint8)
    blk = parser.parse(r1, 0, len(r1), True, r2, 0, len(r2), True, score_mode, paired, False, False, 1 << 20)
    assert not blk.exc
    cols = [c.copy() for c in blk.cols]
    if score_mode == 2:
        for f in (0, 1):
            cols[2 * f], bad = H.c_cigar_scores(*blk.csr[f])
            assert bad == 0
    code, _counts = H.c_classify(H.MODES[mode], *cols, blk.unit_bits.copy(), ABSENT)
    idx, off = H.c_compact(H.MODES[mode], code)
    return blk, idx.copy(), [int(v) for v in off]


def oracle_texts(b1, b2, mode, score_mode):
    outs = [io.StringIO() for _ in range(6)]
    pairs = ORACLE.read_pairs(io.StringIO(b1.decode("ascii"), newline=None), io.StringIO(b2.decode("ascii"), newline=None), False)
    if mode == "se":
        ORACLE.run_single_end(pairs, outs, H.NEG, SCORERS[score_mode])
    else:
        ORACLE.run_paired_end(pairs, outs, H.NEG, SCORERS[score_mode], conservative=mode == "pe_conservative")
    return [o.getvalue().encode("ascii") for o in outs]


@pytest.mark.parametrize("paired,scores,newline", LAYOUTS)
def test_images_hold_every_length_and_every_alignment_of_both_sides(paired, scores, newline):
    b1, b2 = S.shape_text(paired, scores, newline)
    tables, shorts = [], []
    for f, text in enumerate((b1, b2)):
        lines, starts, terminated = S.split_lines(text)
        assert len(lines) == S.N_RECORDS >= S.MIN_RECORDS and terminated == (f == 1)          # file 1's last line has no terminator
        sizes = np.array([len(l) for l in lines])
        assert set(range(1, S.MAX_PLAIN + 1)) <= set(sizes.tolist()) and set(S.LONG_LINES) <= set(sizes.tolist())
        assert sizes.max() > 3 * S.CHUNK and sorted(sizes.tolist())[-2] > S.CHUNK
        assert np.unique((starts % 8) * 8 + sizes % 8).shape[0] == 64                         # every (offset % 8, length % 8)
        assert all(l == S.printed(l)[:-1] for l in lines)                                     # every line is '\t'.join(fields)
        assert sum(1 for l in lines if len(l.split()) < 12) >= S.SHORT_BELOW - 1
        short = {r for r, l in enumerate(lines) if len(l) < S.SHORT_BELOW}
        shorts.append(short)
        if newline == "mixed":
            assert {kind for _p, kind in S.terminators_of(text)} == {"lf", "cr", "crlf"}
        tables.append((lines, sizes))
    names = [[l.split()[0] for l in t[0]] for t in tables]
    assert names[0] == names[1]
    if paired:
        assert all(names[0][r] == names[0][r + 1] for r in range(0, S.N_RECORDS, 2))
        assert all(names[0][r] != names[0][r + 1] for r in range(1, S.N_RECORDS - 1, 2))
    # the same record has different lengths in the two files, and so different offsets
    assert (tables[0][1] != tables[1][1]).mean() > 0.9
    assert shorts[0] == shorts[1] if scores == "all_unresolved" else not shorts[0] & shorts[1]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("scores", S.SCORE_LAYOUTS)
def test_bins_filled_and_every_destination_alignment(parser, mode, scores):
    paired = MODES[mode][0]
    b1, b2 = S.shape_text(paired, scores, "\n")
    lines = [S.split_lines(b)[0] for b in (b1, b2)]
    _blk, idx, off = host_units(parser, b1, b2, mode, 0)
    filled = sum(1 for b in range(6) if off[b + 1] > off[b])
    if scores == "all_unresolved":
        # exactly: a unit is outside `unresolved` only where a record has no score in either file (a line too short for its tags):
        # single-end and conservative mode leave such a unit unassigned, liberal mode takes the mate's state -- every unit unresolved
        per = 2 if paired else 1
        bare = {r // per for r in range(S.N_RECORDS) if len(lines[0][r].split()) < 12 and len(lines[1][r].split()) < 12}
        assert len(bare) == S.SHORT_BELOW - 1
        outside = {int(i) // per for b in (0, 1, 2, 3, 5) for i in idx[off[b]:off[b + 1]]}
        assert outside == (set() if mode == "pe" else bare) and off[5] - off[4] == off[7] - len(outside)
        assert set((idx[off[5]:off[6]] // per).tolist()) == outside
        return
    if mode != "pe_conservative":
        assert filled >= 5
    at, residues = 0, set()
    for b in range(6):
        for _label, text in S.bin_parts(lines[0], lines[1], idx, off, paired, S.ALL, b):
            residues.add(at % 8)
            at += len(text)
    assert residues == set(range(8))


@pytest.mark.parametrize("variant", sorted(S.BOUNDARY_VARIANTS))
def test_boundary_text_hits_every_listed_position(variant):
    text = S.boundary_text(variant)
    total, end = S.BOUNDARY_VARIANTS[variant]
    assert len(text) == total
    need = S.required_boundary_positions()
    assert len(need) == 3 * 16 + 3 * 7
    assert S.boundary_positions(text) & need == need
    lines, starts, terminated = S.split_lines(text)
    assert terminated == (end != "none") and all(l[:1] == b"r" and l.split()[0] == b"r" for l in lines)
    sizes = sorted(len(l) for l in lines)
    assert S.CHUNK < sizes[-2] < 2 * S.CHUNK < sizes[-1]
    terms = np.array([p for p, _k in S.terminators_of(text)])
    for c in (8, 10, 11):                                            # whole chunks without a terminator
        assert not ((terms >= c * S.CHUNK) & (terms < (c + 1) * S.CHUNK)).any()
    assert text[-1:] == {"lf": b"\n", "cr": b"\r", "crlf": b"\n"}.get(end, text[-1:])
    if end == "crlf":
        assert text[-2:] == b"\r\n" and (total - 1) % S.CHUNK == 0


def test_boundary_variants_end_where_they_should():
    lengths = {name: v[0] for name, v in S.BOUNDARY_VARIANTS.items()}
    assert lengths["x16"] % 16 == 0 and lengths["x16"] % S.CHUNK
    assert lengths["chunk"] % S.CHUNK == 0 and lengths["chunk-1"] % S.CHUNK == S.CHUNK - 1 and lengths["chunk+1"] % S.CHUNK == 1
    assert sum(1 for v in S.BOUNDARY_VARIANTS.values() if v[1] == "cr") >= 3


def test_large_windows_are_what_their_tests_count_on():
    b1, b2 = S.many_lines(600_000, False, False)
    assert len(b1) == len(b2) == 600_000 * 41 > 16 << 20 and b1.count(b"\n") == 600_000
    first = b1[:41].split(b"\t")
    assert len(first) == 12 and b1[41 * 524_293:41 * 524_294].rstrip(b"\n").endswith(b"x")
    r1, r2 = S.many_lines(600_000, False, True)
    names = [np.frombuffer(r, dtype=np.uint8).reshape(-1, 41)[:, :8] for r in (r1, r2)]
    runs = [int((n[1:] != n[:-1]).any(axis=1).sum()) + 1 for n in names]
    assert min(runs) > 262_144 and runs[0] != runs[1]
    t1, t2 = S.tiny_lines(4_200_000)
    assert 33 << 20 > len(t1) == 4_200_000 * 8 and t1.count(b"\n") == t2.count(b"\n") == 4_200_000
    assert t1[:24] == b"a00000\nb000000\nc0000000\n" and t2[:30] == b"a00000\tq\nb000000\tq\nc0000000\tq\n"


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("scores,newline,score_mode", [("spread", "\n", 0), ("spread", "mixed", 1), ("spread", "\r\n", 2),
                                                       ("all_unresolved", "\r", 0), ("all_unresolved", "mixed", 2)])
def test_expected_bins_equal_the_oracle_and_the_host_writer(parser, mode, scores, newline, score_mode):
    paired = MODES[mode][0]
    b1, b2 = S.shape_text(paired, scores, newline)
    _check_expectation(parser, b1, b2, mode, score_mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_expected_bins_rejoin_odd_lines_like_the_oracle(parser, mode):
    paired = MODES[mode][0]
    b1, b2, odd = S.odd_lines(paired)
    lines = [S.split_lines(b)[0] for b in (b1, b2)]
    assert {form for _at, form in odd} == set(S.ODD_FORMS)
    for (f, r), _form in odd:
        assert S.printed(lines[f][r])[:-1] != lines[f][r]
    assert sum(1 for f in (0, 1) for l in lines[f] if S.printed(l)[:-1] != l) == len(odd)
    _blk, idx, off = host_units(parser, b1, b2, mode, 0)
    # the odd lines sit where ODD_UNITS says: in units of that bin, and in the paired modes as the FIRST mate (record i - 1) of
    # every such unit of bin 0 and as the second mate of every such unit of bin 1 -- so mask 0b000001 is declined for first mates alone
    per = 2 if paired else 1
    for first, b, f, mate in S.ODD_UNITS:
        members = set(idx[off[b]:off[b + 1]].tolist())
        mine = [r for (g, r), _form in odd if g == f and first * per <= r < (first + 30) * per]
        assert len(mine) == 10 and all((r | 1 if paired else r) in members for r in mine)
        assert not paired or {r & 1 for r in mine} == {mate}
    printed_odd = {b: [(g, r) for (g, r), _form in odd if g in S.files_of_bin(b) and (r | 1 if paired else r) in set(idx[off[b]:off[b + 1]].tolist())]
                   for b in range(6)}
    assert [len(printed_odd[b]) for b in range(6)] == [10, 10, 0, 0, 0, 0]
    if paired:
        assert all(r % 2 == 0 for _g, r in printed_odd[0]) and all(r % 2 == 1 for _g, r in printed_odd[1])
    _check_expectation(parser, b1, b2, mode, 0)


def _check_expectation(parser, b1, b2, mode, score_mode):
    paired = MODES[mode][0]
    lines = [S.split_lines(b)[0] for b in (b1, b2)]
    blk, idx, off = host_units(parser, b1, b2, mode, score_mode)
    assert blk.n == S.N_RECORDS and blk.ended and off[7] == (S.N_RECORDS // 2 if paired else S.N_RECORDS)
    want = oracle_texts(b1, b2, mode, score_mode)
    got = S.expected_bins(lines[0], lines[1], idx, off, paired, S.ALL)
    assert got == want
    assert sum(len(t) for t in got) > len(b1) // 2
    for b in range(6):
        assert bytes(parser.emit(paired, b, idx[off[b]:off[b + 1]])) == got[b], b
    for mask in (0, 0b010110, 0b000001, 0b100000):
        masked = S.expected_bins(lines[0], lines[1], idx, off, paired, mask)
        assert masked == [want[b] if (mask >> b) & 1 else b"" for b in range(6)]
