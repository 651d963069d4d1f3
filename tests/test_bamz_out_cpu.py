"""Compressed BAM outputs (output_format="bam", bam_compress=True; --bam_outputs --bam_compress), what is decided without a GPU:
the refusal that comes before the device or a sink is touched, the command line's usage error, and the help text, which stays the
reference's byte for byte."""
import hashlib
import io
import os
import subprocess
import sys

import pytest

from tests import helpers as H
from tests.test_bam_out_cpu import DATA, HUMAN, MOUSE


def test_bam_compress_without_bam_outputs_is_refused_and_leaves_the_sinks_empty():
    from xenomapper_amd import xenomapper as xm
    sam = [os.path.join(DATA, "paired_end_testdata_%s.sam" % t) for t in ("human", "mouse")]
    sinks = [io.StringIO() for _ in range(6)]
    with pytest.raises(ValueError, match="bam_compress"):            # SAM inputs, SAM outputs
        xm.classify_sam_files(sam[0], sam[1], *sinks, paired=True, output_format="sam", bam_compress=True)
    assert not any(s.getvalue() for s in sinks)
    with pytest.raises(ValueError, match="bam_compress"):            # the default output_format is "sam"
        xm.classify_sam_files(sam[0], sam[1], *sinks, paired=True, bam_compress=True)
    assert not any(s.getvalue() for s in sinks)
    sinks = [io.BytesIO() for _ in range(6)]
    with pytest.raises(ValueError, match="bam_compress"):            # BAM inputs, SAM outputs
        xm.classify_sam_files(HUMAN, MOUSE, *sinks, paired=True, bam=True, output_format="sam", bam_compress=True)
    assert not any(s.getvalue() for s in sinks)
    with pytest.raises(ValueError, match="output_format"):           # (an unknown format is still named first)
        xm.classify_sam_files(HUMAN, MOUSE, *sinks, paired=True, bam=True, output_format="cram", bam_compress=True)
    assert not any(s.getvalue() for s in sinks)


def test_command_line_takes_the_flag_only_with_bam_outputs(capsys):
    from xenomapper_amd import xenomapper as xm
    with pytest.raises(SystemExit) as exc:
        xm.command_line_interface(["--primary_bam", HUMAN, "--secondary_bam", MOUSE, "--bam_compress"])
    assert exc.value.code == 2
    err = capsys.readouterr().err
    assert "--bam_compress needs --bam_outputs" in err and err.startswith("usage: xenomapper")
    ns = xm.command_line_interface(["--primary_bam", HUMAN, "--secondary_bam", MOUSE, "--bam_outputs", "--bam_compress"])
    for handle in (ns.primary_bam, ns.secondary_bam):
        handle.close()
    assert ns.bam_outputs and ns.bam_compress
    ns = xm.command_line_interface(["--primary_bam", HUMAN, "--secondary_bam", MOUSE, "--bam_outputs"])
    for handle in (ns.primary_bam, ns.secondary_bam):
        handle.close()
    assert ns.bam_outputs and not ns.bam_compress                    # off unless asked for
    # as a child process, with SAM inputs: the parser's error, exit status 2, nothing on stdout
    sam = os.path.join(DATA, "paired_end_testdata_human.sam")
    proc = subprocess.run([sys.executable, "-m", "xenomapper_amd.xenomapper", "--primary_sam", sam, "--secondary_sam", sam, "--bam_compress"],
                          cwd=H.REPO, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 2 and "--bam_compress needs --bam_outputs" in proc.stderr and proc.stdout == ""


def test_help_is_the_reference_text_with_the_flag_in_the_parser(capsys, monkeypatch):
    """--help prints what the reference's command line prints (the text behind the error line of G9's `no_inputs_is_a_usage_error`,
    recorded from the reference), although the parser knows --bam_compress."""
    from xenomapper_amd import xenomapper as xm
    case = {c["name"]: c for c in H.golden("g9_cli.json")["cases"]}["no_inputs_is_a_usage_error"]
    monkeypatch.setenv("COLUMNS", "80")
    with pytest.raises(SystemExit) as exc:
        xm.command_line_interface(["--help"])
    assert exc.value.code == 0
    text = capsys.readouterr().out
    assert "bam_compress" not in text and "bam_outputs" not in text
    with pytest.raises(SystemExit):
        xm.main([])
    usage = capsys.readouterr().out
    assert (hashlib.sha224(usage.encode("latin-1")).hexdigest(), len(usage)) == (case["stdout"]["sha224"], case["stdout"]["len"])
    assert usage.endswith(text) and len(usage) - len(text) == len("ERROR: You must provide --primary_sam and --secondary_sam\n"
                                                                  " or --primary_bam and --secondary_bam\n\n")
    # the flag is in the parser all the same
    with pytest.raises(SystemExit) as exc:
        xm.command_line_interface(["--bam_compress"])
    assert exc.value.code == 1                                       # (no inputs: the usage error, not "unrecognized arguments")
    capsys.readouterr()
