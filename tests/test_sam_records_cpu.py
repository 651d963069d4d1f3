"""SAM lines as BAM alignment records on the host (xmh_sam_encode, built on xenomapper_amd/csrc/xm_samrec.h) against the plain-Python
model of tests/sam_records.py, which is itself pinned to the reference's fixture pairs; every device-eligible record printed back by
oracle/bam_oracle.py; the host-only forms; every error form with its line and reason.  The device side: test_sam_records_gpu.py."""
import gzip
import os
import struct

import numpy as np
import pytest

from tests import helpers as H
from tests import sam_records as R

GOLD = os.path.join(H.REPO, "tests", "golden")
FIXTURES = [os.path.join(GOLD, "ref_data", "paired_end_testdata_%s" % s) for s in ("human", "mouse")]


def bam_parts(path):
    """(reference names, the inflated record section) of a BAM file"""
    raw = gzip.decompress(open(path, "rb").read())
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    names = []
    for _ in range(n_ref):
        ln, = struct.unpack_from("<i", raw, p)
        names.append(raw[p + 4:p + 4 + ln - 1])
        p += 8 + ln
    return names, raw[p:]


def sam_lines(path):
    return [ln for ln in open(path, "rb").read().split(b"\n") if ln and not ln.startswith(b"@")]


def native(lines, names, **kw):
    from xenomapper_amd import _host
    text = b"\n".join(lines)
    off = np.cumsum([0] + [len(ln) + 1 for ln in lines[:-1]]) if lines else np.zeros(0)
    return _host.sam_encode(text, off, [len(ln) for ln in lines], names, **kw)


@pytest.fixture(scope="module")
def cat():
    return R.catalogue()


@pytest.mark.parametrize("base", FIXTURES)
def test_model_and_host_encoder_reproduce_the_fixture_record_sections(base):
    names, section = bam_parts(base + ".bam")
    lines = sam_lines(base + ".sam")
    assert len(lines) == 476 and len(section) in (124136, 121309)
    model = b"".join(R.encode(ln, names) for ln in lines)
    assert model == section
    for device_forms in (False, True):
        blob, sizes, bad, reason = native(lines, names, device_forms=device_forms)
        assert bad is None and reason == 0 and blob == section
        assert [int(s) for s in sizes] == [len(r) + 4 for r in R.split_records(section)]


def test_catalogue_host_encoder_equals_the_model(cat):
    assert len(cat) > 200
    encoded = declined = 0
    for name, line, dev, host in cat:
        for device_forms, expect in ((False, host), (True, dev)):
            rec, why = R.try_encode(line, R.REFS, host=not device_forms)
            assert why == expect, (name, device_forms, why)
            blob, sizes, bad, reason = native([line], R.REFS, device_forms=device_forms)
            if expect:
                assert (bad, reason, blob, len(sizes)) == (0, expect, b"", 0), name
                declined += 1
            else:
                assert bad is None and blob == rec and int(sizes[0]) == len(rec), name
                encoded += 1
    assert encoded > 300 and declined > 80
    assert {dev for _, _, dev, _ in cat} >= {R.FIELDS, R.QNAME, R.FLAG, R.RNAME, R.POS, R.MAPQ, R.CIGAR, R.RNEXT, R.PNEXT, R.TLEN, R.QUAL,
                                            R.AUX, R.AUX_RANGE, R.HOST_FLOAT, R.HOST_LONG_CIGAR, R.HOST_SEQ_CODE, R.HOST_NUMBER}


def test_every_device_eligible_record_prints_back_as_its_line(cat):
    from oracle import bam_oracle
    names = [r.decode() for r in R.REFS]
    lines = [e[1] for e in cat if R.printable(e)]
    assert len(lines) > 150
    blob, sizes, bad, _ = native(lines, R.REFS, device_forms=True)
    assert bad is None
    records = R.split_records(blob)
    assert len(records) == len(lines)
    for rec, line in zip(records, lines):
        assert bam_oracle.record_to_line(rec, names).encode("latin-1") == line
    # with the two RNEXT spellings whose record is another spelling's
    by_name = {e[0]: e[1] for e in cat}
    for name, printed in (("rnext_same_name", b"="), ("rnext_eq_star", b"*")):
        rec = R.encode(by_name[name], R.REFS, host=False)
        back = bam_oracle.record_to_line(rec[4:], names).encode("latin-1").split(b"\t")
        want = by_name[name].split(b"\t")
        assert back[6] == printed and back[:6] + back[7:] == want[:6] + want[7:]


def test_bins_at_pos_zero_and_unmapped():
    rec = R.encode(R.make(pos=0, pnext=0, cigar=b"*"), R.REFS)             # (with a CIGAR across 0: no level holds both ends, bin 0)
    assert struct.unpack_from("<H", rec, 4 + 10)[0] == 4680
    a = R.encode(R.make(pos=(1 << 14) - 8, flag=0, l_seq=10), R.REFS)
    b = R.encode(R.make(pos=(1 << 14) - 8, flag=4, l_seq=10), R.REFS)
    assert struct.unpack_from("<H", a, 14)[0] == 585 and struct.unpack_from("<H", b, 14)[0] == 4681


def test_long_cigar_fixture_goes_through_the_cg_form():
    from oracle import bam_oracle
    lines = sam_lines(os.path.join(GOLD, "long_cigar_cg.sam"))
    assert len(lines) == 4
    names, _ = bam_parts(os.path.join(GOLD, "long_cigar_cg.bam"))
    blob, sizes, bad, reason = native(lines, names)
    assert bad is None and len(sizes) == 4
    records = R.split_records(blob)
    assert blob == b"".join(R.encode(ln, names) for ln in lines)
    assert [bam_oracle.record_to_line(r, [n.decode() for n in names]).encode("latin-1") for r in records] == lines
    n_ops = [ln.split(b"\t")[5] for ln in lines]
    n_ops = [sum(1 for c in f if not 48 <= c <= 57) for f in n_ops]
    assert sorted(n > 65535 for n in n_ops) == [False, False, True, True] and 65535 in n_ops
    for rec, n in zip(records, n_ops):
        stored, = struct.unpack_from("<H", rec, 12)
        if n > 65535:
            assert stored == 2 and b"CGBI" + struct.pack("<I", n) in rec
        else:
            assert stored == n and b"CGBI" not in rec
    # the device declines exactly the two long ones
    for ln, n in zip(lines, n_ops):
        _, _, bad, reason = native([ln], names, device_forms=True)
        assert (bad, reason) == ((0, R.HOST_LONG_CIGAR) if n > 65535 else (None, 0))


@pytest.mark.parametrize("text", ["1.5", "-3", "0", "1e10", "3.4028235e38", "1e-45", "0.1", "-0.0", "16777217", "inf", "nan"])
def test_float_values_are_strtof(text):
    want = struct.pack("<f", float(text))
    for field, at in ((b"XF:f:" + text.encode(), 3), (b"XF:B:f," + text.encode() + b",2", 8)):
        blob, _, bad, _ = native([R.make(aux=[field])], R.REFS)
        assert bad is None
        plain, _, _, _ = native([R.make()], R.REFS)
        assert blob[len(plain) + at:len(plain) + at + 4] == want, (text, field)


def test_an_error_yields_its_line_and_reason_and_nothing_behind_it(cat):
    good = [e[1] for e in cat if e[3] == 0 and len(e[1]) < 2000][:5]
    front = b"".join(R.encode(ln, R.REFS) for ln in good[:3])
    seen = 0
    for name, line, dev, host in cat:
        if not host:
            continue
        blob, sizes, bad, reason = native(good[:3] + [line] + good[3:], R.REFS)
        assert (bad, reason, blob, len(sizes)) == (3, host, front, 3), name
        seen += 1
    assert seen > 50


def test_refs_with_a_duplicate_name_are_refused():
    with pytest.raises(ValueError):
        native([R.make()], [b"chr1", b"chr2", b"chr1"])


def test_ref_shift_moves_only_ids_that_name_a_reference():
    lines = [R.make(rname=R.REFS[3], rnext=b"*"), R.make(rname=b"*", rnext=b"*", pos=0, pnext=0), R.make(rname=R.REFS[7], rnext=R.REFS[9])]
    blob, _, bad, _ = native(lines, R.REFS, ref_shift=5000)
    assert bad is None and blob == b"".join(R.encode(ln, R.REFS, ref_shift=5000) for ln in lines)
    ids = [(struct.unpack_from("<i", r, 0)[0], struct.unpack_from("<i", r, 20)[0]) for r in R.split_records(blob)]
    assert ids == [(5003, -1), (-1, -1), (5007, 5009)]
