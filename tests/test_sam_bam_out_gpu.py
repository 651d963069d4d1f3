"""SAM inputs, BAM outputs through the file path (process_headers / classify_sam_files with output_format="bam", encode_sam=True;
--bam_outputs --encode_sam): the lines encoded as BAM records on the GPU (xm_strip_fetch_bins_bam, with bam_compress
xm_strip_fetch_bins_bamz), the windows the device declines encoded by the host.  The outputs are read back by the oracle's reader
(oracle/bam_oracle.py) and must hold the header and the lines of the text run of the same call."""
import gzip
import io
import os
import subprocess
import sys

import pytest

from oracle import bam_oracle
from tests import helpers as H
from tests import sam_records as R
from tests.test_bam_out_cpu import EOF, KEYS
from tests.test_sam_bam_out_cpu import SAM, prefixed_copy

pytestmark = pytest.mark.gpu

TILES = 40
CASES = {"liberal": dict(paired=True), "conservative": dict(paired=True, conservative=True), "cigar_scores": dict(paired=True, tag="NM"),
         "single": dict(paired=False)}


def split_sam(path):
    lines = open(path).read().split("\n")
    return [l for l in lines if l[:1] == "@"], [l for l in lines if l and l[0] != "@"]


def write_sam(path, header, body):
    open(path, "w").write("\n".join(header + body) + "\n")
    return path


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """The two fixture .sam files with their bodies tiled 40 times (about 6 MB each: more than 4 windows of 1 MB with carried tails);
    the mouse file's references carry an m_ prefix, so that `unresolved` has a dictionary.  `odd`: the same with three unit pairs
    spliced in, far enough apart to fall into three windows, whose first line in either file the device does not encode (in either:
    whichever bin the unit goes to, one of the two is wanted)."""
    d = tmp_path_factory.mktemp("sam_bam_out")
    mouse = prefixed_copy(SAM[1], str(d / "mouse_renamed.sam"))
    (h1, b1), (h2, b2) = split_sam(SAM[0]), split_sam(mouse)
    assert len(b1) == len(b2) == 476
    # what keeps the plain inputs on the device route and inside the encoder's one documented departure (RNEXT '=' where it equals RNAME)
    for body in (b1, b2):
        for l in body:
            f = l.split("\t")
            assert f[6] != f[2] or f[2] == "*", l
            assert not any(x[2:5] == ":f:" or x[2:7] == ":B:f," for x in f[11:]) and " " not in l, l
    plain = [write_sam(str(d / "human_x40.sam"), h1, b1 * TILES), write_sam(str(d / "mouse_x40.sam"), h2, b2 * TILES)]
    assert all(os.path.getsize(p) > 5_000_000 for p in plain)
    # the first unit pair of the fixtures under three new names; the first line of each file in a form that is the host's
    assert b1[0].split("\t")[0] == b1[1].split("\t")[0] == b2[0].split("\t")[0] == b2[1].split("\t")[0]

    def unit(body, name, change=None):
        out = ["\t".join([name] + l.split("\t")[1:]) for l in body[:2]]
        if change:
            out[0] = change(out[0])
        return out

    def lower(l):
        f = l.split("\t")
        f[9] = f[9][:3] + f[9][3].lower() + f[9][4:]
        return "\t".join(f)
    changes = (("odd_float", lambda l: l + "\tXF:f:1.5"), ("odd_tabs", lambda l: l.replace("\t", "\t\t", 1)), ("odd_lower", lower))
    o1, o2 = [], []
    for t in range(TILES):
        for k, (name, change) in enumerate(changes):
            if t == 5 + 12 * k:
                o1 += unit(b1, name, change)
                o2 += unit(b2, name, change)
        o1 += b1
        o2 += b2
    odd = [write_sam(str(d / "human_odd.sam"), h1, o1), write_sam(str(d / "mouse_odd.sam"), h2, o2)]
    return {"plain": plain, "odd": odd, "lower_lines": tuple(lower(unit(b, "odd_lower")[0]) for b in (b1, b2)), "dir": d,
            "parts": ((h1, b1), (h2, b2))}


def small_windows(monkeypatch):
    from xenomapper_amd import xenomapper as xm
    monkeypatch.setattr(xm, "FILE_WINDOW_BYTES", 1 << 20)


def run_one(paths, fmt, paired=True, conservative=False, tag="AS", compress=False):
    """One call of the file path -> (counts, {key: what the sink holds}, profile, {key: bytes of the header})."""
    from xenomapper_amd import xenomapper as xm
    tag_func = {"AS": xm.get_tag, "NM": xm.get_cigarbased_AS_tag}[tag]
    sinks = {k: (io.StringIO() if fmt == "sam" else io.BytesIO()) for k in KEYS}
    kw = {"output_format": "bam", "encode_sam": True} if fmt == "bam" else {}
    with open(paths[0]) as f1, open(paths[1]) as f2:
        xm.process_headers(f1, f2, **kw, **sinks)
    heads = {k: len(v.getvalue()) for k, v in sinks.items()}
    if compress:
        kw["bam_compress"] = True
    counts = xm.classify_sam_files(paths[0], paths[1], paired=paired, conservative=conservative, tag_func=tag_func, **kw, **sinks)
    return dict(counts), {k: v.getvalue() for k, v in sinks.items()}, dict(xm.LAST_FILE_PROFILE), heads


def compare(sam, bam, through_model=()):
    """counts, the end-of-file marker, header and lines of every output as the text run's -> lines compared.  through_model: the
    lines (text) that are compared as the oracle's print of the Python model's record (BAM cannot keep the case of a SEQ letter)."""
    assert bam[0] == sam[0] and sum(sam[0].values()) > 0
    n_lines = 0
    for key, image in bam[1].items():
        assert image.endswith(EOF), key
        header, lines = bam_oracle.bam_to_sam(image)
        want = sam[1][key]
        want_header = want[:sam[3][key]]
        if key == "unresolved":                                      # file 1's text with file 2's @SQ lines behind file 1's last @SQ line
            mine = want_header.split("\n")
            sq2 = [l for l in sam[1]["secondary_specific"][:sam[3]["secondary_specific"]].split("\n") if l[:3] == "@SQ"]
            last = max(k for k, l in enumerate(mine) if l[:3] == "@SQ")
            want_header = "\n".join(mine[:last + 1] + sq2 + mine[last + 1:])
        assert header == want_header, key
        want_lines = want[sam[3][key]:].split("\n")[:-1]
        if through_model:
            names = [l.split("\t")[1][3:] for l in header.split("\n") if l[:3] == "@SQ"]
            for k, l in enumerate(want_lines):
                if l in through_model:
                    rec = R.encode(l.encode(), [n.encode() for n in names])
                    want_lines[k] = bam_oracle.record_to_line(rec[4:], names)
                    assert want_lines[k] != l and want_lines[k].upper() == l.upper()
        assert lines == want_lines, key
        n_lines += len(lines)
    assert n_lines > 0
    return n_lines


@pytest.mark.parametrize("case", list(CASES))
def test_bam_outputs_hold_the_header_and_lines_of_the_text_run(inputs, monkeypatch, case):
    small_windows(monkeypatch)
    sam = run_one(inputs["plain"], "sam", **CASES[case])
    bam = run_one(inputs["plain"], "bam", **CASES[case])
    n = compare(sam, bam)
    prof = bam[2]
    assert n > 400 * TILES // 2 and prof["sam_windows"] > 4, (n, prof)
    assert prof.get("sam_windows_device_bam_bins", 0) > 0 and not prof.get("sam_windows_device_bamz_bins", 0), prof
    if case != "cigar_scores":                                       # every window with records came from the device, none from the host
        assert prof["sam_windows_device_bam_bins"] >= prof["sam_windows"] - 1 and not prof.get("sam_windows_host_bam", 0), prof
    assert prof["bam_out_bytes"] == sum(len(v) - bam[3][k] - len(EOF) for k, v in bam[1].items())


@pytest.mark.parametrize("case", ["liberal", "single"])
def test_compressed_outputs_hold_the_same_lines_and_are_no_longer(inputs, monkeypatch, case):
    small_windows(monkeypatch)
    sam = run_one(inputs["plain"], "sam", **CASES[case])
    stored = run_one(inputs["plain"], "bam", **CASES[case])
    bamz = run_one(inputs["plain"], "bam", compress=True, **CASES[case])
    compare(sam, bamz)
    prof = bamz[2]
    assert prof.get("sam_windows_device_bamz_bins", 0) > 0 and not prof.get("sam_windows_device_bam_bins", 0), prof
    for key in KEYS:
        assert len(bamz[1][key]) <= len(stored[1][key]), key
        assert gzip.decompress(bamz[1][key]) == gzip.decompress(stored[1][key]), key
    assert sum(len(v) for v in bamz[1].values()) < sum(len(v) for v in stored[1].values())


@pytest.mark.parametrize("compress", [False, True])
def test_windows_the_device_declines_are_encoded_by_the_host(inputs, monkeypatch, compress):
    small_windows(monkeypatch)
    sam = run_one(inputs["odd"], "sam")
    bam = run_one(inputs["odd"], "bam", compress=compress)
    assert any(line + "\n" in text for text in sam[1].values() for line in inputs["lower_lines"])
    assert any("XF:f:1.5\n" in text for text in sam[1].values()) and any("odd_tabs\t" in text for text in sam[1].values())
    compare(sam, bam, through_model=inputs["lower_lines"])
    prof = bam[2]
    device = "sam_windows_device_bamz_bins" if compress else "sam_windows_device_bam_bins"
    assert prof.get("sam_windows_host_bam", 0) == 3 and prof["sam_windows"] - 4 <= prof.get(device, 0) <= prof["sam_windows"] - 3, prof


@pytest.mark.parametrize("knob", ["XENOMAPPER_GPU_SAM_BINS", "XENOMAPPER_GPU_STRIP"])
def test_environment_knobs_give_the_device_runs_payloads(inputs, monkeypatch, knob):
    small_windows(monkeypatch)
    device = run_one(inputs["plain"], "bam")
    assert device[2].get("sam_windows_device_bam_bins", 0) > 0
    monkeypatch.setenv(knob, "0")
    host = run_one(inputs["plain"], "bam")
    assert host[0] == device[0]
    assert not host[2].get("sam_windows_device_bam_bins", 0) and host[2].get("sam_windows_host_bam", 0) > 4, host[2]
    for key in KEYS:
        assert host[1][key].endswith(EOF) and gzip.decompress(host[1][key]) == gzip.decompress(device[1][key]), key


def test_an_rname_that_is_not_in_the_header_raises_and_leaves_no_marker(inputs, monkeypatch):
    from xenomapper_amd import xenomapper as xm
    small_windows(monkeypatch)
    (h1, b1), (h2, b2) = inputs["parts"]
    # (every mapped line of one tile: whichever bins its units go to, one of them is wanted)
    lost = ["\t".join(f[:2] + ["nowhere"] + f[3:]) if f[2] != "*" else "\t".join(f) for f in (l.split("\t") for l in b1)]
    assert lost != b1
    body = b1 * 3 + lost + b1 * 3
    paths = [write_sam(str(inputs["dir"] / "human_lost.sam"), h1, body), write_sam(str(inputs["dir"] / "mouse_lost.sam"), h2, b2 * 7)]
    sinks = {key: io.BytesIO() for key in KEYS}
    with open(paths[0]) as f1, open(paths[1]) as f2:
        xm.process_headers(f1, f2, output_format="bam", encode_sam=True, **sinks)
    with pytest.raises(ValueError) as err:
        xm.classify_sam_files(paths[0], paths[1], paired=True, output_format="bam", encode_sam=True, **sinks)
    text = str(err.value)
    assert "'nowhere'" in text and "XMH_ENC_RNAME" in text and paths[0] in text, text
    assert any(repr(l.split("\t")[0]) in text for l in b1), text
    assert all(v.getvalue() and not v.getvalue().endswith(EOF) for v in sinks.values())


@pytest.mark.parametrize("compress", [False, True])
def test_command_line_writes_what_the_two_api_calls_write(inputs, tmp_path, compress):
    from xenomapper_amd import xenomapper as xm
    paths = inputs["plain"]
    sinks = {k: io.BytesIO() for k in KEYS}
    with open(paths[0]) as f1, open(paths[1]) as f2:
        xm.process_headers(f1, f2, output_format="bam", encode_sam=True, **sinks)
    xm.classify_sam_files(paths[0], paths[1], paired=True, output_format="bam", encode_sam=True, bam_compress=compress, **sinks)
    assert xm.LAST_FILE_PROFILE.get("sam_windows_device_bamz_bins" if compress else "sam_windows_device_bam_bins", 0) > 0
    outs = {k: str(tmp_path / (k + ".bam")) for k in KEYS}
    cmd = [sys.executable, "-m", "xenomapper_amd.xenomapper", "--primary_sam", paths[0], "--secondary_sam", paths[1], "--paired", "--bam_outputs",
           "--encode_sam"] + (["--bam_compress"] if compress else [])
    for k in KEYS:
        cmd += ["--" + k, outs[k]]
    proc = subprocess.run(cmd, cwd=H.REPO, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    for k in KEYS:
        image = open(outs[k], "rb").read()
        assert image == sinks[k].getvalue() and image.endswith(EOF), k
