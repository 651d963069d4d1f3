"""The images of tests/bam_shapes.py on the CPU: the host decoder's SAM text (xm_bam.cpp: format_record) equals the oracle's
restatement of the BAM layout (oracle/bam_oracle.py) at every shape -- which its Hypothesis fuzz reaches only by luck --, floating-
point fields equal printf("%g") value by value, and the builder really holds every value its sweeps list.  No GPU: this proves the
inputs of tests/test_bam_shapes_gpu.py valid before a GPU sees them."""
import struct

import numpy as np
import pytest

from oracle import bam_oracle
from tests import bam_shapes as S
from tests import helpers as H
from tests.test_bam_gpu import host_text

LAYOUTS = [(True, "spread"), (False, "spread"), (True, "all_unresolved"), (False, "all_unresolved")]


def _diff(got, want, recs):
    """The first record whose line differs: its number, its shape and the first differing byte."""
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            at = next((j for j in range(min(len(g), len(w))) if g[j] != w[j]), min(len(g), len(w)))
            p = S.parse(recs[k][4:])
            shape = {key: p[key] for key in ("size", "l_seq", "ref", "pos", "mapq", "flag", "next_ref", "next_pos", "tlen")}
            shape.update(l_read_name=len(p["name_field"]), n_cigar=p["cigar"].shape[0], fields=[(t[0], t[1], t[2], len(t[3])) for t in p["fields"]][:8])
            return "record %d: byte %d of the line: got %r, want %r; %r" % (k, at, g[max(0, at - 20):at + 20], w[max(0, at - 20):at + 20], shape)
    return None


@pytest.mark.parametrize("paired,scores", LAYOUTS)
def test_host_printer_equals_the_oracle_at_every_shape(paired, scores):
    for recs in S.shape_records(paired, scores):
        image = S.image_of(recs)
        _header, lines = bam_oracle.bam_to_sam(image)
        assert len(lines) == len(recs) >= S.MIN_RECORDS
        got = host_text(image).split(b"\n")
        assert got.pop() == b""
        assert _diff(got, [l.encode("latin-1") for l in lines], recs) is None


def test_host_printer_prints_floats_as_printf_g():
    """Every value of the float image: Python's '%g' (byte-identical to glibc's for everything but a NaN), a NaN as `nan` or `-nan` by
    its sign bit (xm_fmtg.h; what snprintf prints).  The rest of every line: the oracle's."""
    seen = []
    for recs in S.float_records(False):
        image = S.image_of(recs)
        _header, lines = bam_oracle.bam_to_sam(image)
        got = host_text(image).split(b"\n")[:-1]
        assert len(got) == len(lines) == len(recs)
        for rec, line, mine in zip(recs, lines, got):
            mine = mine.decode("latin-1").split("\t")
            want = S.expected_line(rec[4:], line).split("\t")
            assert len(mine) == len(want)
            for a, b, field in zip(mine, want, [None] * 11 + S.parse(rec[4:])["fields"]):
                if field is not None and field[1:3] == ("B", "f"):
                    a, b = a.split(","), b.split(",")
                    bits = np.frombuffer(field[3], dtype="<u4")
                    bad = [(hex(int(v)), x, y) for v, x, y in zip(bits, a[1:], b[1:]) if x != y]
                    assert not bad and a[0] == b[0] and len(a) == len(b) == bits.shape[0] + 1, bad[:8]
                    seen.append(bits)
                else:
                    assert a == b
    pats = S.float_patterns()
    assert 75000 < pats.shape[0] and np.isin(pats, np.concatenate(seen)).all()
    # what the patterns have to hold
    ex, fr = (pats >> 23) & 0xFF, pats & 0x7FFFFF
    for sign in (0, 1):
        for e in range(256):
            mine = fr[(ex == e) & ((pats >> 31) == sign)]
            assert np.isin(np.arange(8), mine).all() and np.isin(0x7FFFFF - np.arange(8), mine).all() and np.unique(mine).shape[0] >= 24
    values = pats.view("<f4")
    for v in range(999980, 1000021):
        assert np.isin(np.array([v, v + 0.5, v + 0.25], dtype="<f4"), values).all()
    assert sum(1 for v in pats if S.g_text(v) == "nan") >= 8 and sum(1 for v in pats if S.g_text(v) == "-nan") >= 8
    assert {S.g_text(v) for v in (0, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x007FFFFF)} == \
        {"0", "-0", "inf", "-inf", "1.4013e-45", "1.17549e-38"}


@pytest.mark.parametrize("paired", [True, False])
def test_the_builder_holds_every_listed_shape(paired):
    for f, recs in enumerate(S.shape_records(paired, "spread")):
        assert len(recs) >= S.MIN_RECORDS and len(recs) % 64 and len(recs) % 256
        ps = [S.parse(r[4:]) for r in recs]
        sizes = [p["size"] for p in ps]
        assert sizes == [len(r) for r in recs] and max(sizes) <= S.MAX_RECORD and min(sizes) == 38
        assert set(S.SIZES) <= set(sizes) and any(63000 <= s <= 64000 for s in sizes)
        assert sum(p["l_seq"] for p in ps) < 3_000_000
        # neighbours of very different sizes in one wave
        waves = [sizes[at:at + 64] for at in range(0, len(sizes), 64)]
        assert sum(1 for w in waves if min(w) < 80 and max(w) > 20000) >= 3
        # l_seq: every value with ordinary, top-bit and 0xFF-first qualities; all 16 codes inside a 128-letter trip, top-bit bytes
        # inside a 64-byte trip
        for l_seq in S.L_SEQ + [S.L_SEQ_LARGE]:
            mine = [p for p in ps if p["l_seq"] == l_seq]
            if l_seq:
                assert any(p["qual"][0] == 0xFF for p in mine), l_seq
                assert any(p["qual"][0] != 0xFF and max(p["qual"]) >= 128 for p in mine) or l_seq < 4, l_seq
                assert any(max(p["qual"]) < 94 for p in mine), l_seq
            else:
                assert len(mine) >= 3
        assert all(q <= 222 and not 94 <= q < 128 for p in ps if p["l_seq"] and p["qual"][0] != 0xFF for q in p["qual"])
        long_ones = [p for p in ps if p["l_seq"] >= 128 and p["qual"][0] != 0xFF]
        def codes_of(p):
            trip = np.frombuffer(p["seq"][:64], dtype=np.uint8)
            return set((trip >> 4).tolist()) | set((trip & 15).tolist())
        assert any(codes_of(p) == set(range(16)) for p in long_ones)
        assert any(max(p["qual"][:64]) >= 128 for p in long_ones)
        # names
        printed = [p["name_field"].split(b"\0")[0] for p in ps]
        for n in S.NAME_LEN:
            assert any(len(p["name_field"]) == n + 1 and len(nm) == n for p, nm in zip(ps, printed)), n
        for z in S.NUL_AT:
            assert any(len(p["name_field"]) == 100 and len(nm) == z and 0 not in p["name_field"][z + 1:99] for p, nm in zip(ps, printed)), z
        assert all(p["name_field"][-1] == 0 for p in ps)
        white = set(b"\t\n\v\f\r \x1c\x1d\x1e\x1f\x85\xa0")
        assert not any(white & set(nm) for nm in printed)
        if paired:
            assert all(printed[k] == printed[k + 1] for k in range(0, len(ps), 2))
            assert all(printed[k] != printed[k + 1] for k in range(1, len(ps) - 1, 2))
        else:
            assert len(set(printed)) == len(printed)
        # CIGAR
        assert set(S.N_CIGAR) <= {p["cigar"].shape[0] for p in ps}
        words = np.concatenate([p["cigar"] for p in ps])
        assert set((words & 15).tolist()) == set(range(16)) and set(S.CIGAR_LEN) <= set((words >> 4).tolist())
        assert not any(p["cigar"].shape[0] and int(p["cigar"][0]) & 15 == 4 and int(p["cigar"][0]) >> 4 == p["l_seq"] for p in ps)
        # fixed fields
        assert set(S.POS) <= {p["pos"] for p in ps} and set(S.POS) <= {p["next_pos"] for p in ps}
        assert set(S.TLEN) <= {p["tlen"] for p in ps} and set(S.FLAG) <= {p["flag"] for p in ps} and set(S.MAPQ) <= {p["mapq"] for p in ps}
        assert {(a, b) for a in S.REF_IDS for b in S.REF_IDS} <= {(p["ref"], p["next_ref"]) for p in ps}
        # optional fields
        fields = [x for p in ps for x in p["fields"]]
        for t in S.INT_TYPES:
            have = {struct.unpack(S.FMT[t], v)[0] for _tag, ft, _sub, v in fields if ft == t}
            assert set(S.int_values(t)) <= have, t
            assert {-1, 9, 10, 99, 100}.issubset(have) or t in "CSI"
        assert {b"!", b"~"} <= {v for _tag, ft, _sub, v in fields if ft == "A"}
        for t in "ZH":
            assert set(S.STRING_LEN) <= {len(v) for _tag, ft, _sub, v in fields if ft == t}, t
        for sub in "cCsSiIf":
            width = struct.calcsize(S.FMT[sub])
            assert set(S.B_COUNT) <= {len(v) // width for _tag, ft, fs, v in fields if ft == "B" and fs == sub}, sub
        assert any(len(p["fields"]) >= 40 and len({x[1] for x in p["fields"]}) >= 10 for p in ps)
        assert any(not p["fields"] and p["l_seq"] for p in ps)
        for t in "CSI":
            assert any(p["fields"] and p["fields"][-1][1] == t for p in ps), t
        assert not any(white & set(v) for _tag, ft, _sub, v in fields if ft in "AZ")
        assert all(S.scores_of(p["fields"])[0] is None or -2**31 < S.scores_of(p["fields"])[0] < 2**31 for p in ps)
    # the two files: the same names in the same order, other records
    one, two = S.shape_records(paired, "spread")
    assert [S.parse(r[4:])["name_field"].split(b"\0")[0] for r in one] == [S.parse(r[4:])["name_field"].split(b"\0")[0] for r in two]
    assert sum(1 for a, b in zip(one, two) if a != b) > len(one) * 0.9


@pytest.mark.parametrize("paired", [True, False])
def test_score_layouts(paired):
    """`spread`: at least five of the six bins have units; `all_unresolved`: every unit with a score is unresolved."""
    for scores in S.SCORE_LAYOUTS:
        files = S.shape_records(paired, scores)
        cols = []
        for recs in files:
            sc = [S.scores_of(S.parse(r[4:])["fields"]) for r in recs]
            cols += [np.array([-2**31 if v[j] is None else v[j] for v in sc], dtype=np.int32) for j in (0, 1)]
        names = [S.parse(r[4:])["name_field"].split(b"\0")[0] for r in files[0]]
        flags = np.array([(k > 0 and names[k] == names[k - 1]) if paired else True for k in range(len(names))], dtype=np.uint8)
        bits = np.packbits(np.concatenate([flags, np.zeros((-len(flags)) % 64, np.uint8)]), bitorder="little").view(np.uint64)
        mode = H.MODES["pe"] if paired else H.MODES["se"]
        code, _counts = H.c_classify(mode, *cols, bits, -2**31)
        _idx, off = H.c_compact(mode, code)
        filled = [int(off[b + 1]) > int(off[b]) for b in range(6)]
        if scores == "spread":
            assert sum(filled) >= 5, off
        else:
            assert filled[4] and not any(filled[:4]) and int(off[5]) - int(off[4]) > 0.8 * int(off[7]), off
