"""SAM inputs, BAM outputs (output_format="bam", encode_sam=True), the host's share, without a GPU: the reference list made from the
@SQ lines, the BAM headers process_headers writes from SAM headers, the host encoder of a bin's text (_sam_records_of) against the
Python model (tests/sam_records.py), the refusals that come before a sink or the device is touched, and the command line's usage
errors.  The reader is the oracle's (oracle/bam_oracle.py)."""
import gzip
import io
import os
import struct
import subprocess
import sys

import pytest

from oracle import bam_oracle
from tests import helpers as H
from tests import sam_records as R
from tests.test_bam_out_cpu import EOF, KEYS, split_header

DATA = os.path.join(H.REPO, "tests", "golden", "ref_data")
SAM = [os.path.join(DATA, "paired_end_testdata_%s.sam" % t) for t in ("human", "mouse")]
BAM = [os.path.join(DATA, "paired_end_testdata_%s.bam" % t) for t in ("human", "mouse")]


def header_lines(path):
    return [l for l in open(path).read().split("\n") if l[:1] == "@"]


def prefixed_copy(src, dst, prefix="m_"):
    """The SAM file `src` with every reference renamed: the @SQ lines' SN, and RNAME / RNEXT where they name one."""
    out = []
    for line in open(src).read().split("\n"):
        if line[:3] == "@SQ":
            line = line.replace("\tSN:", "\tSN:" + prefix)
        elif line and line[0] != "@":
            f = line.split("\t")
            for k in (2, 6):
                if f[k] not in ("*", "="):
                    f[k] = prefix + f[k]
            line = "\t".join(f)
        out.append(line)
    open(dst, "w").write("\n".join(out))
    return dst


def sam_route_headers(paths, keys=KEYS):
    from xenomapper_amd import xenomapper as xm
    sinks = {k: io.StringIO() for k in keys}
    with open(paths[0]) as f1, open(paths[1]) as f2:
        xm.process_headers(f1, f2, **sinks)
    return {k: v.getvalue() for k, v in sinks.items()}


def encoded_headers(paths, keys=KEYS):
    from xenomapper_amd import xenomapper as xm
    sinks = {k: io.BytesIO() for k in keys}
    with open(paths[0]) as f1, open(paths[1]) as f2:
        xm.process_headers(f1, f2, output_format="bam", encode_sam=True, **sinks)
    return {k: v.getvalue() for k, v in sinks.items()}


def test_sq_parser_on_the_fixture_headers_equals_the_bam_twins_reference_lists():
    from xenomapper_amd import xenomapper as xm
    counts = []
    for sam, bam in zip(SAM, BAM):
        want = split_header(gzip.decompress(open(bam, "rb").read()))[1]
        assert xm._sam_header_refs(header_lines(sam)) == want
        counts.append(len(want))
    assert counts == [25, 22]


def test_headers_hold_the_sam_route_text_and_the_list_of_the_sq_lines():
    from xenomapper_amd import xenomapper as xm
    keys = KEYS[:5]                                                  # (`unresolved`: the tests below)
    want = sam_route_headers(SAM, keys)
    got = encoded_headers(SAM, keys)
    lists = [split_header(gzip.decompress(open(p, "rb").read()))[1] for p in BAM]
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
    lists = [xm._sam_header_refs(header_lines(p)) for p in SAM]
    clash = [name for name, _l in lists[1] if name in set(n for n, _l in lists[0])]
    assert clash and clash[0] == b"1"
    sinks = {k: io.BytesIO() for k in KEYS}
    with open(SAM[0]) as f1, open(SAM[1]) as f2:
        with pytest.raises(ValueError) as err:
            xm.process_headers(f1, f2, output_format="bam", encode_sam=True, **sinks)
    assert repr(clash[0].decode("ascii")) in str(err.value)
    assert not any(s.getvalue() for s in sinks.values())


def test_unresolved_gets_both_lists_and_the_merged_text(tmp_path):
    from xenomapper_amd import xenomapper as xm
    mouse = prefixed_copy(SAM[1], str(tmp_path / "mouse_renamed.sam"))
    lists = [xm._sam_header_refs(header_lines(p)) for p in (SAM[0], mouse)]
    assert all(name.startswith(b"m_") for name, _l in lists[1]) and len(lists[1]) == 22
    want = sam_route_headers((SAM[0], mouse))
    got = encoded_headers((SAM[0], mouse))
    text, refs, _end = split_header(gzip.decompress(got["unresolved"]))
    assert refs == lists[0] + lists[1]
    mine = want["unresolved"].split("\n")
    sq2 = [l for l in want["secondary_specific"].split("\n") if l[:3] == "@SQ"]
    last = max(k for k, l in enumerate(mine) if l[:3] == "@SQ")
    assert text.decode("ascii") == "\n".join(mine[:last + 1] + sq2 + mine[last + 1:])
    header, lines = bam_oracle.bam_to_sam(got["unresolved"] + EOF)
    assert header == text.decode("ascii") and lines == []
    for key in KEYS[:5]:
        assert split_header(gzip.decompress(got[key]))[0].decode("ascii") == want[key]


def test_sq_edge_lines():
    from xenomapper_amd.xenomapper import _sam_header_refs as refs
    assert refs(["@HD\tVN:1.0", "@SQ\tLN:10\tSN:a", "@SQ\tAS:hg19\tSN:b\tM5:0123\tLN:2147483647\tSP:x", "@PG\tID:p"]) == [(b"a", 10), (b"b", 2 ** 31 - 1)]
    assert refs(["@HD\tVN:1.0", "@PG\tID:SN:x\tLN:5", "@CO\t@SQ\tSN:c\tLN:1"]) == []
    assert refs([]) == []
    assert refs([b"@SQ\tSN:a\tLN:1\n"]) == [(b"a", 1)]                # (bytes, and a terminator, as they stand in a file)
    for bad, word in ((["@SQ\tSN:a"], "LN"), (["@SQ\tLN:5"], "SN"), (["@SQ\tSN:a\tLN:0"], "LN"), (["@SQ\tSN:a\tLN:2147483648"], "LN"),
                      (["@SQ\tSN:a\tLN:-3"], "LN"), (["@SQ\tSN:a\tLN:1x"], "LN"), (["@SQ\tSN:a\tLN:7", "@SQ\tSN:b\tLN:7", "@SQ\tLN:9\tSN:a"], "twice")):
        with pytest.raises(ValueError) as err:
            refs(bad)
        assert word in str(err.value) and repr(bad[-1]) in str(err.value), (bad, str(err.value))


NAMES = ([b"chr1", b"chr2", b"chr3"], [b"m1", b"m2"])


def line(q, rname, rnext=b"=", **kw):
    return R.make(qname=q, rname=rname, rnext=rnext, **kw)


def model(lines_and_files, b, ref_shift):
    return b"".join(R.encode(l, NAMES[f], ref_shift=ref_shift if (f == 1 and b == 4) else 0) for l, f in lines_and_files)


def test_host_encoder_of_a_bins_text_against_the_model():
    from xenomapper_amd import xenomapper as xm
    one = [line(b"a", b"chr2", l_seq=7), line(b"b", b"*", b"*", pos=0, pnext=0), line(b"c", b"chr3", b"chr1", l_seq=33, aux=(b"XF:f:1.5",))]
    two = [line(b"a", b"m2", l_seq=9), line(b"b", b"m1", b"m2"), line(b"c", b"*", b"*", pos=0, pnext=0, l_seq=5)]
    compared = 0
    for b, lines, f in ((0, one, 0), (2, one, 0), (5, one, 0), (1, two, 1), (3, two, 1)):
        text = b"".join(l + b"\n" for l in lines)
        for paired in (False, True):                                 # (outside bin 4 a unit's lines are one file's: paired plays no part)
            got = xm._sam_records_of(text, b, paired, NAMES, 3)
            assert got == model([(l, f) for l in lines], b, 3) and len(R.split_records(got)) == 3
            compared += 3
    # bin 4, single: per unit file 1's line, then file 2's
    order = [(one[0], 0), (two[0], 1), (one[1], 0), (two[1], 1), (one[2], 0), (two[2], 1)]
    got = xm._sam_records_of(b"".join(l + b"\n" for l, _f in order), 4, False, NAMES, 3)
    assert got == model(order, 4, 3)
    ids = [(struct.unpack_from("<i", x, 0)[0], struct.unpack_from("<i", x, 20)[0]) for x in R.split_records(got)]
    # ref_shift moves only file 2's ids, and only those that name a reference
    assert ids == [(1, 1), (4, 4), (-1, -1), (3, 4), (2, 0), (-1, -1)]
    compared += 6
    # bin 4, paired: per unit file 1's two lines, then file 2's two
    order = [(one[0], 0), (one[2], 0), (two[0], 1), (two[1], 1), (one[1], 0), (one[0], 0), (two[2], 1), (two[0], 1)]
    got = xm._sam_records_of(b"".join(l + b"\n" for l, _f in order), 4, True, NAMES, 3)
    assert got == model(order, 4, 3) and len(R.split_records(got)) == 8
    assert got != xm._sam_records_of(b"".join(l + b"\n" for l, _f in order), 4, True, NAMES, 0)
    compared += 8
    # a numpy view as Parser.emit returns it, and no text at all
    import numpy as np
    text = b"".join(l + b"\n" for l in one)
    assert xm._sam_records_of(np.frombuffer(text, dtype=np.uint8), 0, True, NAMES, 0) == model([(l, 0) for l in one], 0, 0)
    assert xm._sam_records_of(b"", 4, True, NAMES, 3) == b""
    assert compared == 44


def test_a_line_the_encoder_refuses_raises_with_file_qname_and_reason():
    from xenomapper_amd import xenomapper as xm
    good = line(b"fine", b"chr1")
    cases = ((line(b"lost", b"chr9"), "XMH_ENC_RNAME", "'chr9'"), (line(b"lost", b"chr1", b"chrZ"), "XMH_ENC_RNEXT", "'chrZ'"),
             (b"\t".join(good.replace(b"fine", b"lost").split(b"\t")[:9]), "XMH_ENC_FIELDS", "lost"),
             (line(b"lost", b"chr1", aux=(b"XZ:q:1",)), "XMH_ENC_AUX", "lost"))
    for bad, reason, word in cases:
        for b, f in ((0, 0), (1, 1)):
            names = (NAMES[0], NAMES[0])
            with pytest.raises(ValueError) as err:
                xm._sam_records_of(good + b"\n" + bad + b"\n", b, False, names, 0, ("first.sam", "second.sam"))
            text = str(err.value)
            assert ("first.sam", "second.sam")[f] in text and "'lost'" in text and reason in text and word in text, text
    # bin 4: the line of file 2 is looked up in file 2's names
    with pytest.raises(ValueError) as err:
        xm._sam_records_of(good + b"\n" + line(b"lost", b"chr1") + b"\n", 4, False, NAMES, 3)
    assert "file 2" in str(err.value) and "XMH_ENC_RNAME" in str(err.value)


def test_refusals_leave_the_sinks_empty():
    from xenomapper_amd import xenomapper as xm

    def both(sinks, exc, sam=True, **kw):
        with pytest.raises(exc):
            xm.classify_sam_files(*(SAM if sam else BAM), *sinks, paired=True, **kw)
        with open((SAM if sam else BAM)[0], "r" if sam else "rb") as f1, open((SAM if sam else BAM)[1], "r" if sam else "rb") as f2:
            with pytest.raises(exc):
                xm.process_headers(f1, f2, *sinks, **kw)
        assert not any(s.getvalue() for s in sinks if s)
    both([io.BytesIO() for _ in range(6)], ValueError, sam=False, bam=True, output_format="bam", encode_sam=True)
    both([io.BytesIO() for _ in range(6)], ValueError, output_format="sam", encode_sam=True)
    both([io.StringIO() for _ in range(6)], ValueError, encode_sam=True)
    shared = io.BytesIO()
    both([io.BytesIO(), io.BytesIO(), shared, shared, None, None], ValueError, output_format="bam", encode_sam=True)
    both([io.BytesIO(), io.StringIO(), None, None, None, None], TypeError, output_format="bam", encode_sam=True)
    # and without the keyword every call is refused as it was
    sinks = [io.BytesIO() for _ in range(6)]
    with pytest.raises(ValueError):
        xm.classify_sam_files(SAM[0], SAM[1], *sinks, paired=True, output_format="bam")
    assert not any(s.getvalue() for s in sinks)


def cli(*args):
    env = dict(os.environ, PYTHONPATH=H.REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", "from xenomapper_amd.xenomapper import main; main()"] + list(args), env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, cwd=H.REPO)


def test_command_line_usage_errors(tmp_path):
    out = str(tmp_path / "ps.bam")
    r = cli("--primary_sam", SAM[0], "--secondary_sam", SAM[1], "--encode_sam", "--primary_specific", out)
    assert r.returncode == 2 and "--encode_sam needs --bam_outputs" in r.stderr
    r = cli("--primary_bam", BAM[0], "--secondary_bam", BAM[1], "--bam_outputs", "--encode_sam", "--primary_specific", out)
    assert r.returncode == 2 and "--encode_sam needs" in r.stderr
    r = cli("--primary_sam", SAM[0], "--secondary_sam", SAM[1], "--primary_bam", BAM[0], "--secondary_bam", BAM[1], "--bam_outputs",
            "--encode_sam", "--primary_specific", out)
    assert r.returncode == 2 and "--encode_sam needs" in r.stderr
    r = cli("--primary_sam", SAM[0], "--secondary_sam", SAM[1], "--bam_outputs", "--primary_specific", out)
    assert r.returncode == 2 and "--bam_outputs needs --primary_bam and --secondary_bam" in r.stderr and "--encode_sam" in r.stderr
    assert os.path.getsize(out) == 0
    r = cli("--help")
    assert r.returncode == 0 and "encode_sam" not in r.stdout and "bam_outputs" not in r.stdout and "bam_compress" not in r.stdout
