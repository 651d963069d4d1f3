"""single_end_mappability_from_sam(on_device=True) against on_device=False, byte for byte: the E. coli fixture at three window
sizes, texts with a window the device declines, the error of a SAM that is not name sorted, the command line, and the buffers
given back."""
import hashlib
import io
import os

import pytest

from tests import helpers as H
from tests import mapp_shapes as S

pytestmark = pytest.mark.gpu

ECOLI = os.path.join(H.GOLDEN, "ref_data", "test_from_EcoliK12DH10B_150reads.sam")     # 3462 lines, two segments, no line the grammar declines
ECOLI_SHA224 = "e8e8557a16c05aaa436c2c0fe616450d82a955e0f6de8eb3d190cdf4"              # tests/test_mappability.py; the same with and without sizes
G10 = {c["name"]: c for c in H.golden("g10_mappability_cli.json")["cases"]}


def wiggle(path, on_device, sizes={}):
    from xenomapper_amd import mappability as mp
    out = io.StringIO()
    with open(path, encoding="utf-8") as fh:
        mp.single_end_mappability_from_sam(fh, outfile=out, chromosome_sizes=dict(sizes), on_device=on_device)
        assert fh.read() == ""                                        # both routes leave the handle at its end
    return out.getvalue()


@pytest.mark.parametrize("window_kb", (None, 64, 1))
@pytest.mark.parametrize("sizes", ({"Chromosome": 2752, "A_Repeat": 991}, {}), ids=("sizes", "no_sizes"))
def test_ecoli_fixture_at_three_window_sizes(window_kb, sizes, monkeypatch):
    from xenomapper_amd import mappability as mp
    if window_kb is None:
        monkeypatch.delenv("XENOMAPPER_MAPP_WINDOW_KB", raising=False)
    else:
        monkeypatch.setenv("XENOMAPPER_MAPP_WINDOW_KB", str(window_kb))
    text = wiggle(ECOLI, True, sizes)
    assert hashlib.sha224(text.encode("latin-1")).hexdigest() == ECOLI_SHA224
    run = mp.last_run
    assert run["windows_host"] == 0 and run["reasons"] == {} and run["lines"] == 3462
    with open(ECOLI, "rb") as fh:
        body = sum(len(x) for x in fh if not x.startswith(b"@"))      # (the header is consumed on the host)
    assert run["windows_device"] >= (1 if window_kb is None else body // (window_kb << 10))
    assert run["ms_kernels"] > 0


def one_chromosome_with_a_blank_separated_line():
    lines = S.reads("c", range(1, 121)).splitlines(True)
    lines[60] = lines[60].replace("\t", " ")                          # str.split() takes it; the device declines the window
    return "".join(lines)


def test_a_declined_window_between_device_windows_of_one_segment(tmp_path, monkeypatch):
    from xenomapper_amd import mappability as mp
    text = one_chromosome_with_a_blank_separated_line()
    path = tmp_path / "reads.sam"
    path.write_text(text)
    monkeypatch.setenv("XENOMAPPER_MAPP_WINDOW_KB", "1")
    windows, raised = S.chain(S.Shape("blank", text.encode(), 1024, S.BIG, S.BIG, False, False))
    status = [w.want.status for w in windows]
    assert raised is None and status.count(S.DECLINED) == 1 and S.OK in status[:status.index(S.DECLINED)] and S.OK in status[status.index(S.DECLINED) + 1:]
    assert all(not s.starts for w in windows[1:] for s in w.want.segments)          # one segment all the way
    got = wiggle(str(path), True)
    assert got == wiggle(str(path), False) == "fixedStep\tchrom=c\tstart=1\tstep=1\n" + "1\n" * 120
    assert (mp.last_run["windows_host"], mp.last_run["windows_device"]) == (1, len(windows) - 1)
    assert mp.last_run["reasons"] == {"separator": 1} and mp.last_run["lines"] == 120


@pytest.mark.parametrize("name", ("unsettled_x_windows_130", "key_70_bytes_windows", "byte_0c_second_window", "near_origins", "gap_100000",
                                  "pos_underscore", "last_line_open"))
def test_catalogue_texts_through_the_file_route(name, tmp_path, monkeypatch):
    """Texts of the catalogue as files, at the window size the file route can be given (1 KiB) and at the default."""
    shape = S.BY_NAME[name]
    path = tmp_path / "reads.sam"
    path.write_bytes(shape.text)
    want = wiggle(str(path), False)
    for window_kb in ("1", None):
        if window_kb:
            monkeypatch.setenv("XENOMAPPER_MAPP_WINDOW_KB", window_kb)
        else:
            monkeypatch.delenv("XENOMAPPER_MAPP_WINDOW_KB", raising=False)
        assert wiggle(str(path), True) == want


def test_a_sam_that_is_not_name_sorted_raises_the_hosts_error(tmp_path, monkeypatch):
    from xenomapper_amd import mappability as mp
    text = S.reads("c", range(1, 80)) + S.reads("c", (40, 41))
    path = tmp_path / "reads.sam"
    path.write_text(text)
    errors = []
    for on_device, window_kb in ((False, None), (True, "1"), (True, None)):
        if window_kb:
            monkeypatch.setenv("XENOMAPPER_MAPP_WINDOW_KB", window_kb)
        else:
            monkeypatch.delenv("XENOMAPPER_MAPP_WINDOW_KB", raising=False)
        with pytest.raises(ValueError) as exc:
            wiggle(str(path), on_device)
        errors.append(str(exc.value))
    assert errors[0] == errors[1] == errors[2] and "Name: c_40 Expected: c_80" in errors[0]
    assert mp.last_run["reasons"] == {"not_sequential": 1}


def test_command_line_on_device(monkeypatch, capsys):
    from xenomapper_amd import mappability as mp
    case = G10["single_end_wiggle"]
    argv = [a.replace("{D}", os.path.join(H.GOLDEN, "ref_data")) for a in case["argv"]] + ["--on_device"]
    monkeypatch.setattr("sys.argv", ["xenomappability"] + argv)
    monkeypatch.delenv("XENOMAPPER_MAPP_WINDOW_KB", raising=False)
    mp.main()
    out = capsys.readouterr().out
    assert (hashlib.sha224(out.encode("latin-1")).hexdigest(), len(out)) == (case["stdout"]["sha224"], case["stdout"]["len"])
    assert mp.last_run["windows_device"] == 1 and mp.last_run["windows_host"] == 0


def test_release_buffers_gives_the_page_locked_memory_back(monkeypatch):
    from xenomapper_amd import _ffi, mappability as mp, xenomapper as xm
    xm.release_buffers()
    base = _ffi.pinned_bytes()["allocated"]
    monkeypatch.setenv("XENOMAPPER_MAPP_WINDOW_KB", "256")
    wiggle(ECOLI, True)
    assert _ffi.pinned_bytes()["allocated"] >= base + (256 << 10) and mp._front_end is not None
    assert xm.release_buffers()["allocated"] == base and mp._front_end is None
    assert hashlib.sha224(wiggle(ECOLI, True).encode("latin-1")).hexdigest() == ECOLI_SHA224       # a fresh front end, the same answer
    assert xm.release_buffers()["allocated"] == base
