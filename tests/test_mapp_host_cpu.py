"""CPU-only checks of the single-end mappability step's GPU route: what on_device=True refuses, and the C ABI of
include/xenomapper_mappability.h (plain C99, exported, bound in _ffi under its own tuple)."""
import ctypes
import io
import os
import re
import subprocess

import pytest

from tests import helpers as H
from tests import mapp_shapes as S


def _declared():
    text = open(os.path.join(H.REPO, "include", "xenomapper_mappability.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(xmm?_[a-z0-9_]+)\s*\(", text)))


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_on_device_needs_a_regular_file(tmp_path):
    from xenomapper_amd import mappability as mp
    with pytest.raises(ValueError, match="regular file"):
        mp.single_end_mappability_from_sam(io.StringIO(S.reads("c", (1, 2))), outfile=io.StringIO(), on_device=True)
    path = tmp_path / "reads.sam"
    path.write_text(S.reads("c", (1, 2)))
    with open(path, encoding="utf-16") as fh, pytest.raises(ValueError, match="encoding"):
        mp.single_end_mappability_from_sam(fh, outfile=io.StringIO(), on_device=True)
    with open(path, "rb") as fh, pytest.raises(ValueError, match="text-mode"):
        mp.single_end_mappability_from_sam(fh, outfile=io.StringIO(), on_device=True)


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU behaviour")
def test_on_device_has_no_fallback_without_a_device(tmp_path):
    from xenomapper_amd import mappability as mp
    path = tmp_path / "reads.sam"
    path.write_text(S.reads("c", (1, 2)))
    out = io.StringIO()
    with open(path) as fh, pytest.raises(RuntimeError, match="gfx950"):
        mp.single_end_mappability_from_sam(fh, outfile=out, on_device=True)
    assert out.getvalue() == ""
    with open(path) as fh:                                            # and without the keyword nothing has changed
        mp.single_end_mappability_from_sam(fh, outfile=out)
    assert out.getvalue() == "fixedStep\tchrom=c\tstart=1\tstep=1\n1\n1\n"


def test_command_line_takes_on_device_with_the_sam_step_only(monkeypatch, capsys):
    from xenomapper_amd import mappability as mp
    sam = os.path.join(H.GOLDEN, "ref_data", "test_from_EcoliK12DH10B_150reads.sam")
    for argv in (["--on_device"], ["--on_device", "--mapped_test_data", sam, "--fasta", sam],
                 ["--on_device", "--mapped_test_data", sam, "--sam_for_sizes", sam]):
        monkeypatch.setattr("sys.argv", ["xenomappability"] + argv)
        with pytest.raises(SystemExit) as exc:
            mp.command_line_interface()
        assert exc.value.code == 2 and "--on_device goes with --mapped_test_data" in capsys.readouterr().err
    monkeypatch.setattr("sys.argv", ["xenomappability", "--mapped_test_data", sam, "--on_device"])
    args = mp.command_line_interface()
    assert args.on_device and args.mapped_test_data.name == sam
    args.mapped_test_data.close()


def test_header_is_plain_c_and_the_library_exports_it(tmp_path):
    from xenomapper_amd import _ffi, build
    names = _declared()
    assert len(names) == 8 and "xmm_abi_version" in names and "xm_mapp_run" in names
    src = tmp_path / "use_mapp.c"
    src.write_text('#include "xenomapper_mappability.h"\n'
                   "typedef void (*fn)(void);\n"
                   "static const fn table[] = {" + ", ".join("(fn)%s" % n for n in names) + "};\n"
                   "int main(void) { xm_mapp_block b; xm_mapp_segment s; b.status = XMM_OK_WINDOW; s.starts = 0;\n"
                   "  return (XMM_ABI_VERSION == xmm_abi_version() && table[0] && sizeof s == 48 && XMM_MAX_WINDOW == 0xFFFF0000ull &&\n"
                   "          XMM_R_NOT_SEQUENTIAL == 6 && XMM_TOO_MANY_VALUES == 3 && b.status == 0 && s.starts == 0) ? 0 : 1; }\n")
    inc = os.path.join(H.REPO, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "c99.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "cxx.o")])
    build.build_hip()
    exe, libdir = tmp_path / "use_mapp", os.path.dirname(_ffi.LIB_PATH)
    subprocess.check_call(["gcc", str(tmp_path / "c99.o"), "-o", str(exe), "-L", libdir, "-l:libxenomapper_hip.so",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib"])
    assert subprocess.call([str(exe)]) == 0
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n
    assert sorted(_ffi.EXPORTED_MAPP) == names
    assert not set(_ffi.EXPORTED_MAPP) & set(_ffi.EXPORTED)
    assert _ffi.lib().xmm_abi_version() == 1
    assert ctypes.sizeof(_ffi._MappBlock) == 80 and _ffi.MAPP_SEGMENT.itemsize == 48
